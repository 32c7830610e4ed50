// One keccak-f[1600] round and the main-trace columns of the reference's KeccakRound component for it (prover/src/extensions/keccak/
// round/trace.rs:297-366): every intermediate 64-bit lane of theta, rho-pi, chi and iota as 8 byte columns, low byte first, in the order
// the reference's builder allocates them.  ONE text with two readers: keccak_round.hip compiles it for the device, and
// tests/native/keccak_round_host.cpp compiles it as plain C++ under the sanitizers.  Plain NX_HD functions templated on the store:
//   S::put(col, lane)   the 8 byte columns col .. col + 7 of this row get the bytes of `lane`
//   S::word(col, w)     column col of this row gets w
// u32, u64 and NX_HD come from the includer.  Every loop below has constant bounds and is unrolled, so the lane arrays are indexed by
// constants only and live in registers.  RC and the rotation offsets are written out from FIPS 202 (sections 3.2.2 and 3.2.5); the tests
// pin them to hashlib.
constexpr u32 KR_LANES = 25, KR_MAIN_COLS = 1705, KR_PRE_COLS = 9, KR_MAX_ROUNDS = 24;

// iota: RC[round] (FIPS 202 algorithm 5 evaluated for l = 6)
NX_HD u64 kr_rc(u32 round) {
    const u64 rc[KR_MAX_ROUNDS] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
        0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
        0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
        0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return rc[round];
}

// rho: the offset of lane (x, y) at index x + 5 y (FIPS 202 table 2 reduced mod 64)
NX_HD constexpr u32 kr_rot(u32 lane) {
    constexpr u32 rot[KR_LANES] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return rot[lane];
}

struct KrNoStore {      // the untraced rounds: the same round, nothing written
    NX_HD void put(u32, u64) const {}
    NX_HD void word(u32, u32) const {}
};

// rot(v, R) as the reference's rotate_left writes it: low = (byte << R % 8) & 255 and high = byte >> (8 - R % 8) of every byte, then
// out byte i = low[(i - R / 8) & 7] + high[(i - R / 8 + 7) & 7], which is the 64-bit rotation.  Three lanes at col; a rotation by a
// whole number of bytes still has them (high = 0).
template <u32 R, class S> NX_HD u64 kr_rotate(const S& st, u32& col, u64 v) {
    constexpr u32 bits = R % 8;
    constexpr u64 ones = 0x0101010101010101ull;
    const u64 low = (v & (ones * (0xFFu >> bits))) << bits;
    const u64 high = bits ? (v >> ((8 - bits) & 7)) & (ones * ((1u << bits) - 1)) : 0;
    const u64 out = (v << R) | (v >> (64 - R));
    st.put(col, low); st.put(col + 8, high); st.put(col + 16, out);
    col += 24;
    return out;
}

template <u32 XY, class S> NX_HD void kr_rho_pi(const S& st, u32& col, const u64 (&a)[KR_LANES], u64 (&b)[KR_LANES]) {
    if constexpr (XY < KR_LANES) {
        constexpr u32 x = XY / 5, y = XY % 5, src = x + 5 * y, dst = y + 5 * ((2 * x + 3 * y) % 5), r = kr_rot(src);
        if constexpr (r == 0) b[dst] = a[src];
        else b[dst] = kr_rotate<r>(st, col, a[src]);
        kr_rho_pi<XY + 1>(st, col, a, b);
    }
}

// a: the state before the round on entry, after it on return (index x + 5 y).  Writes main columns 0 .. 1703 of the row through st.
template <class S> NX_HD void kr_round(const S& st, u64 (&a)[KR_LANES], u64 rc) {
    u32 col = 0;
#pragma unroll
    for (u32 l = 0; l < KR_LANES; l++) { st.put(col, a[l]); col += 8; }
    // theta: C[x] as four chained xors, D[x] = C[x - 1] ^ rot(C[x + 1], 1), A[x, y] ^= D[x]
    u64 c[5], d[5];
#pragma unroll
    for (u32 x = 0; x < 5; x++) {
        u64 v = a[x];
#pragma unroll
        for (u32 y = 1; y < 5; y++) { v ^= a[x + 5 * y]; st.put(col, v); col += 8; }
        c[x] = v;
    }
#pragma unroll
    for (u32 x = 0; x < 5; x++) {
        d[x] = c[(x + 4) % 5] ^ kr_rotate<1>(st, col, c[(x + 1) % 5]);
        st.put(col, d[x]); col += 8;
    }
#pragma unroll
    for (u32 x = 0; x < 5; x++)
#pragma unroll
        for (u32 y = 0; y < 5; y++) { a[x + 5 * y] ^= d[x]; st.put(col, a[x + 5 * y]); col += 8; }
    // rho and pi: B[y, 2 x + 3 y] = rot(A[x, y], r[x, y]), x outer
    u64 b[KR_LANES];
    kr_rho_pi<0>(st, col, a, b);
    // chi: A[x, y] = B[x, y] ^ (~B[x + 1, y] & B[x + 2, y])
#pragma unroll
    for (u32 x = 0; x < 5; x++)
#pragma unroll
        for (u32 y = 0; y < 5; y++) {
            const u64 na = ~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y];
            st.put(col, na); col += 8;
            a[x + 5 * y] = b[x + 5 * y] ^ na;
            st.put(col, a[x + 5 * y]); col += 8;
        }
    // iota
    a[0] ^= rc;
    st.put(col, a[0]);
}

// One trace row: a is the instance's input state; round i of the component is traced after i untraced ones.  A padding row holds the
// round of the zero state itself (a is zero and no untraced round runs), with the round constant of its i.
// The loop runs to `rounds` for every row so that its round constant has one index for all of them.  On return a is the state after
// round i.  pre (has_pre): the 8 bytes of the row's round constant and is_last.
template <class SM, class SP> NX_HD void kr_fill_row(const SM& main, const SP& pre, bool has_pre, u64 (&a)[KR_LANES], u32 i, u32 first_round, u32 rounds,
                                                      bool padding, bool last_row) {
    u64 rc_i = 0;
    for (u32 k = 0; k < rounds; k++) {
        const u64 rc = kr_rc(first_round + k);
        if (k == i) rc_i = rc;
        if (k < i && !padding) kr_round(KrNoStore(), a, rc);
    }
    kr_round(main, a, rc_i);
    main.word(KR_MAIN_COLS - 1, padding ? 1u : 0u);
    if (has_pre) { pre.put(0, rc_i); pre.word(KR_PRE_COLS - 1, last_row ? 1u : 0u); }
}
