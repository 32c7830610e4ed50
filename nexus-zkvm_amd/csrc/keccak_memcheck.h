// The main-trace columns of the reference's PermutationMemoryCheck component for one row (prover/src/extensions/keccak/memory_check/
// trace.rs:32-123): the 200 input-state bytes, the 200 bytes of keccak-f[1600] of them, and for each of the 200 byte accesses the
// address, the previous and the next timestamp as 16-bit limbs with their carry flags.  ONE text with two readers, like keccak_round.h,
// which the includer takes in first: keccak_memcheck.hip compiles it for the device, tests/native/keccak_memcheck_host.cpp as plain C++
// under the sanitizers.  Plain NX_HD functions templated on the store (S::put, S::word: keccak_round.h) and on the timestamp source:
//   T::ts4(j, w)   w gets the row's timestamps 4 j .. 4 j + 3 (zeros on a padding row)
// Besides put and word a store has S::here(): the same store, taken anew at the head of every stretch of straight-line stores (each batch
// of the loop below, the input bytes, the output bytes).  The device's store makes the lane's offset a value of that basic block there
// (keccak_store.h), the host's returns itself.
// addr + i and ts + 1 are taken modulo 2^32.
constexpr u32 KM_STATE = 200, KM_MAIN_COLS = 2001, KM_PRE_COLS = 1;
constexpr u32 KM_IN = 0, KM_OUT = KM_STATE, KM_ADDR = 2 * KM_STATE, KM_PREV_TS = 4 * KM_STATE, KM_NEXT_TS = 6 * KM_STATE, KM_ADDR_CARRY = 8 * KM_STATE,
              KM_TS_CARRY = 9 * KM_STATE, KM_IS_PADDING = 10 * KM_STATE;
// the accesses are walked in batches of KM_BATCH timestamp quads: the loads of a batch are issued together, ahead of its stores (a store
// through a pointer from the table may alias anything, so no load moves up across one by itself), and the batches are a loop that is NOT
// unrolled, whose counter is the same in every lane: the column index stays wave-uniform and the text stays a fifth as long
constexpr u32 KM_QUADS = KM_STATE / 4, KM_BATCH = 10;
static_assert(KM_QUADS % KM_BATCH == 0 && KM_IS_PADDING + 1 == KM_MAIN_COLS && KM_STATE == 8 * KR_LANES, "the layout of trace.rs:34");

// addresses, timestamps and carries: main columns 400 .. 1999.  live: 0 on a padding row (every column 0), else all ones.
template <class S, class T> NX_HD void km_fill_accesses(const S& main, const T& ts, u32 addr, u32 live) {
#pragma unroll 1
    for (u32 q0 = 0; q0 < KM_QUADS; q0 += KM_BATCH) {
        const S st = main.here();
        u32 w[KM_BATCH][4];
#pragma unroll
        for (u32 q = 0; q < KM_BATCH; q++) ts.ts4(q0 + q, w[q]);
#pragma unroll
        for (u32 q = 0; q < KM_BATCH; q++)
#pragma unroll
            for (u32 k = 0; k < 4; k++) {
                const u32 i = 4 * (q0 + q) + k, a = addr + i, t = w[q][k], t1 = t + 1;
                st.word(KM_ADDR + 2 * i, a & 0xFFFFu & live);
                st.word(KM_ADDR + 2 * i + 1, (a >> 16) & live);
                st.word(KM_PREV_TS + 2 * i, t & 0xFFFFu & live);
                st.word(KM_PREV_TS + 2 * i + 1, (t >> 16) & live);
                st.word(KM_NEXT_TS + 2 * i, t1 & 0xFFFFu & live);
                st.word(KM_NEXT_TS + 2 * i + 1, (t1 >> 16) & live);
                st.word(KM_ADDR_CARRY + i, ((a & 0xFFFFu) == 0xFFFFu ? 1u : 0u) & live);
                st.word(KM_TS_CARRY + i, ((t & 0xFFFFu) == 0xFFFFu ? 1u : 0u) & live);
            }
    }
}

// One trace row.  a: the instance's input state (zero on a padding row); on return keccak-f[1600] of it (unchanged on a padding row:
// trace.rs:41 writes the real rows only, so out_state is 0 there and not the permutation of the zero state).  The 24 rounds are a loop
// that is not unrolled: its round constant has the loop counter as index, one scalar load for all lanes.
// pre (has_pre): is_last.
template <class SM, class SP, class T> NX_HD void km_fill_row(const SM& main, const SP& pre, bool has_pre, u64 (&a)[KR_LANES], u32 addr, const T& ts, bool padding,
                                                                bool last_row) {
    km_fill_accesses(main, ts, addr, padding ? 0u : ~0u);
    const SM in = main.here();
#pragma unroll
    for (u32 l = 0; l < KR_LANES; l++) in.put(KM_IN + 8 * l, a[l]);
#pragma unroll 1
    for (u32 k = 0; k < KR_MAX_ROUNDS; k++) {
        const u64 rc = kr_rc(k);
        if (!padding) kr_round(KrNoStore(), a, rc);
    }
    const SM out = main.here();
#pragma unroll
    for (u32 l = 0; l < KR_LANES; l++) out.put(KM_OUT + 8 * l, a[l]);
    out.word(KM_IS_PADDING, padding ? 1u : 0u);
    if (has_pre) pre.here().word(0, last_row ? 1u : 0u);
}
