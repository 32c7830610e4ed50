"""The keccak memory-check AIR of the reference (prover/src/extensions/keccak/memory_check/constraints.rs:18-128,
PermutationMemoryCheckEval::eval) restated with ProgramBuilder, literally, quirks included: the trace masks in the same order (input
state, output state, address limbs, previous and next timestamp limbs, address carries, timestamp carries), is_padding read at mask
(0, 1) and the preprocessed is_last read and not used; the boolean constraint on is_padding; the state entry with numerator
1 - is_padding on the input and is_padding - 1 on the output, both 200 wide; per byte two memory entries of width 5 (address limbs,
value, timestamp limbs), is_padding - 1 on the previous access and 1 - is_padding on the next; the address-chain loop that runs i over
(0..200).step_by(2) on the 400 limb columns with addr_carries[i / 2], so that it holds only the first 100 address pairs to their
successors (200 constraints); the 400 timestamp constraints; finalize_logup_in_pairs.
The recorded program: 601 plain constraints and 201 logup constraints (802), 402 relation entries in 201 logup columns, masks on
2001 main columns, is_last and 804 interaction columns; 11125 instructions in the constraint program and 6412 in the fraction program
(tests/test_keccak_memcheck_cpu.py holds every one of these counts).

The closed statement: the round, xor, not-and and rotate components of tests/keccak_air.py as they are, `mem_check` in the place of
its two boundary stand-ins — the state relation closes through the reference's own component — and ONE stand-in, `mem_side`, for the
main machine's load/store chip: one row per (instance, byte), nine main columns (address limbs, previous value, next value, previous
and next timestamp limbs, is_padding), the two memory entries of a row with the opposite numerators; filled from the model on the host."""
import numpy as np

import keccak_air as K
import keccak_memcheck_model as MM
import keccak_round_model as M

P = M.P
MAIN, PRE, LOGUP_COLS = MM.MAIN_COLS, MM.PRE_COLS, MM.LOGUP_COLS
RELATIONS = K.RELATIONS + (("memory", 5),)
WORD_SIZE_HALVED = 2


def memcheck_program(ap, elems, shift):
    """elems: {relation name: (z, alpha)}; shift: claimed sum / rows.  Columns: 0 .. 2000 main, 2001 is_last, then the 4 x 201
    interaction columns."""
    pb = ap.ProgramBuilder()
    state, memory = pb.relation(elems["state"][0], elems["state"][1], 200), pb.relation(elems["memory"][0], elems["memory"][1], 5)
    nxt = [0]

    def next_state_with_size(size):
        out = [pb.next_trace_mask(nxt[0] + i)[0] for i in range(size)]
        nxt[0] += size
        return out

    input_state, output_state = next_state_with_size(200), next_state_with_size(200)
    addrs = next_state_with_size(200 * WORD_SIZE_HALVED)
    prev_ts, next_ts = next_state_with_size(200 * WORD_SIZE_HALVED), next_state_with_size(200 * WORD_SIZE_HALVED)
    addr_carries, ts_carries = next_state_with_size(200), next_state_with_size(200)
    assert nxt[0] == MAIN - 1
    is_padding, _next_is_padding = pb.next_trace_mask(MAIN - 1, (0, 1))
    _next_is_first = pb.next_trace_mask(MAIN)[0]                              # the preprocessed is_last: its constraint is commented out
    pb.add_constraint(is_padding * (1 - is_padding))
    pb.add_to_relation(state, 1 - is_padding, input_state)
    pb.add_to_relation(state, is_padding - 1, output_state)
    for i in range(200):
        j = i * WORD_SIZE_HALVED
        pb.add_to_relation(memory, is_padding - 1, addrs[j:j + 2] + [input_state[i]] + prev_ts[j:j + 2])
        pb.add_to_relation(memory, 1 - is_padding, addrs[j:j + 2] + [output_state[i]] + next_ts[j:j + 2])
    for i in range(0, 200, WORD_SIZE_HALVED):
        addr, next_addr = addrs[i:i + 2], addrs[i + 2:i + 4]
        if len(next_addr) < 2:
            break
        carry = addr_carries[i // WORD_SIZE_HALVED]
        pb.add_constraint((1 - is_padding) * (next_addr[0] + carry * (1 << 16) - addr[0] - 1))
        pb.add_constraint((1 - is_padding) * (next_addr[1] - addr[1] - carry))
    for i in range(200):
        p, n, carry = prev_ts[2 * i:2 * i + 2], next_ts[2 * i:2 * i + 2], ts_carries[i]
        pb.add_constraint((1 - is_padding) * (n[0] + carry * (1 << 16) - p[0] - 1))
        pb.add_constraint((1 - is_padding) * (n[1] - p[1] - carry))
    assert len(pb.constraints) == MM.PLAIN_CONSTRAINTS and len(pb.entries) == 2 * LOGUP_COLS
    pb.finalize_logup_in_pairs(MAIN + PRE, shift)
    assert len(pb.constraints) == MM.PLAIN_CONSTRAINTS + LOGUP_COLS
    return pb


SIDE_MAIN = 9


def mem_side_program(ap, elem, shift):
    """the stand-in for the load/store chip: address limbs, previous value, next value, previous and next timestamp limbs, is_padding;
    per row (1 - is_padding) / combine(previous access) and (is_padding - 1) / combine(next access), one logup column"""
    pb = ap.ProgramBuilder()
    a_lo, a_hi, prev_val, next_val, p_lo, p_hi, n_lo, n_hi, is_padding = [pb.next_trace_mask(k)[0] for k in range(SIDE_MAIN)]
    memory = pb.relation(elem[0], elem[1], 5)
    pb.add_constraint(is_padding * (1 - is_padding))
    pb.add_to_relation(memory, 1 - is_padding, [a_lo, a_hi, prev_val, p_lo, p_hi])
    pb.add_to_relation(memory, is_padding - 1, [a_lo, a_hi, next_val, n_lo, n_hi])
    pb.finalize_logup_in_pairs(SIDE_MAIN, shift)
    return pb


def mem_side_columns(memcheck_main_natural, n_instances, log_size):
    """the nine columns over 2^log_size rows from the memory-check columns in NATURAL order: row 200 r + i is byte i of instance r (the
    component is row-local: any order of its rows serves)"""
    m = np.asarray(memcheck_main_natural, np.uint32)
    cols = np.zeros((SIDE_MAIN, 1 << log_size), np.uint32)
    cols[8] = 1
    for r in range(n_instances):
        for i in range(200):
            cols[:, 200 * r + i] = [m[MM.ADDR + 2 * i, r], m[MM.ADDR + 2 * i + 1, r], m[MM.IN + i, r], m[MM.OUT + i, r], m[MM.PREV_TS + 2 * i, r],
                                    m[MM.PREV_TS + 2 * i + 1, r], m[MM.NEXT_TS + 2 * i, r], m[MM.NEXT_TS + 2 * i + 1, r], 0]
    return cols


# ---- the closed statement of tests/test_gpu_keccak_memcheck.py and tests/test_keccak_memcheck_cpu.py: layout, programs, the model's columns
# Seven components: the two round components and the three tables of tests/keccak_air.py, mem_check over 2^2 rows and mem_side over
# 2^10 rows (3 instances x 200 bytes).  Trees: 0 preprocessed, 1 main, 2 interaction.
N_INST, LOG_A, LOG_B, LOG_BIT, LOG_ROT = K.N_INST, K.LOG_A, K.LOG_B, K.LOG_BIT, K.LOG_ROT
LOG_MC, LOG_SIDE = 2, 10
N_INTER = K.N_INTER
COMPONENTS = ("round_a", "round_b", "xor", "not_and", "rotate", "mem_check", "mem_side")
TREE_LOGS = [[LOG_A] * K.PRE + [LOG_B] * K.PRE + [LOG_BIT] * 6 + [LOG_ROT] * 4 + [LOG_MC] * PRE,
             [LOG_A] * K.MAIN + [LOG_B] * K.MAIN + [LOG_BIT] * 2 + [LOG_ROT] + [LOG_MC] * MAIN + [LOG_SIDE] * SIDE_MAIN,
             [LOG_A] * N_INTER + [LOG_B] * N_INTER + [LOG_BIT] * 8 + [LOG_ROT] * 4 + [LOG_MC] * (4 * LOGUP_COLS) + [LOG_SIDE] * 4]
PRE_AT = dict(K.PRE_AT, mem_check=28)                                                                # first column in tree 0
MAIN_AT = {"round_a": 0, "round_b": 1705, "xor": 3410, "not_and": 3411, "rotate": 3412, "mem_check": 3413, "mem_side": 3413 + MAIN}
INTER_AT = {"round_a": 0, "round_b": N_INTER, "xor": 2 * N_INTER, "not_and": 2 * N_INTER + 4, "rotate": 2 * N_INTER + 8, "mem_check": 2 * N_INTER + 12,
            "mem_side": 2 * N_INTER + 12 + 4 * LOGUP_COLS}
COMP_LOG = {"round_a": LOG_A, "round_b": LOG_B, "xor": LOG_BIT, "not_and": LOG_BIT, "rotate": LOG_ROT, "mem_check": LOG_MC, "mem_side": LOG_SIDE}
N_PRE = {"round_a": 9, "round_b": 9, "xor": 3, "not_and": 3, "rotate": 4, "mem_check": PRE, "mem_side": 0}
N_MAIN = {"round_a": 1705, "round_b": 1705, "xor": 1, "not_and": 1, "rotate": 1, "mem_check": MAIN, "mem_side": SIDE_MAIN}
N_INT = {"round_a": N_INTER, "round_b": N_INTER, "xor": 4, "not_and": 4, "rotate": 4, "mem_check": 4 * LOGUP_COLS, "mem_side": 4}
KEY_BITS = K.KEY_BITS
assert [len(t) for t in TREE_LOGS] == [29, MAIN_AT["mem_side"] + SIDE_MAIN, INTER_AT["mem_side"] + 4]


def statement_programs(ap, elems, shifts):
    return {"round_a": K.round_program(ap, elems, shifts["round_a"])[0], "round_b": K.round_program(ap, elems, shifts["round_b"])[0],
            "xor": K.table_program(ap, elems["xor"], 3, shifts["xor"]), "not_and": K.table_program(ap, elems["not_and"], 3, shifts["not_and"]),
            "rotate": K.table_program(ap, elems["rotate"], 4, shifts["rotate"]),
            "mem_check": memcheck_program(ap, elems, shifts["mem_check"]), "mem_side": mem_side_program(ap, elems["memory"], shifts["mem_side"])}


def statement_inputs(seed=7):
    """3 instances: states as the existing keccak statement draws them, addresses with a carry inside the 200 bytes, random timestamps"""
    states = M.test_states(N_INST, seed=seed)
    states[0] = M.sha3_256_block(b"keccak")
    rng = np.random.default_rng(6900 + seed)
    return states, np.array([0xFFFE, 0x0001FFFF, 0x80000000], np.uint32), rng.integers(0, MM.MASK32, (N_INST, 200), dtype=np.uint32)


def host_statement(states, addresses, timestamps):
    """every preprocessed and main column of the statement from the models alone, in tree order (storage order)"""
    k_pre, k_main, final = K.host_statement(states)
    mc = MM.fill(states, addresses, timestamps, LOG_MC, natural=True)
    assert np.array_equal(mc["out"], final)
    pre = k_pre + list(M.to_storage(mc["pre"], LOG_MC))
    main = k_main[:3413] + list(M.to_storage(mc["main"], LOG_MC)) + list(mem_side_columns(mc["main"], len(states), LOG_SIDE))
    return pre, main, final


def total(claimed):
    """the sum of the components' claimed sums, coordinate by coordinate"""
    return [int(sum(int(claimed[name][q]) for name in COMPONENTS) % P) for q in range(4)]
