"""The keccak round AIR of the reference (prover/src/extensions/keccak/round/constraints.rs, KeccakRoundEval::eval) restated with
ProgramBuilder: the same trace masks in the same order, `low + high - out` for every rotation byte, is_padding boolean and read at
mask (0, 1), one relation entry of numerator 1 per byte of every xor / not-and / rotate site ON EVERY ROW (padding rows look the
round of the zero state up), the two 200-wide state entries with numerators is_padding - 1 and 1 - is_padding, finalize_logup_in_pairs.

The tables are in this repository's preprocessed-table form: one component per table, the tuple in preprocessed columns — xor and
not-and over 2^16 rows (a, b, c), rotate over 2^11 rows (byte, shift, high, low) — and ONE multiplicity column in the main trace.  The
reference splits its bitwise tables into 16 multiplicity columns of 2^12 rows (extensions/keccak/bitwise_table.rs); that is a layout
of the table component only: the relation entries of the round component, restated here, are the same.

A boundary component pair stands in for PermutationMemoryCheck, which in the reference hands the input state to the first round
component and takes the final state from the last: +1 / combine(input) and -1 / combine(final state) per instance."""
import numpy as np

import keccak_round_model as M

P = M.P
MAIN, PRE, LOGUP_COLS = 1705, 9, 521
RELATIONS = (("state", 200), ("xor", 3), ("not_and", 3), ("rotate", 4))


def round_program(ap, elems, shift):
    """elems: {relation name: (z, alpha)}; shift: claimed sum / rows.  Columns: 0 .. 1704 main, 1705 .. 1712 round-constant bytes,
    1713 is_last, then the 4 x 521 interaction columns.  -> (the builder, the looked-up tuples as column numbers per table)"""
    pb = ap.ProgramBuilder()
    rel = {name: pb.relation(elems[name][0], elems[name][1], n) for name, n in RELATIONS}
    nxt, lookups, n_entries = [0], {"xor": [], "not_and": [], "rotate": []}, [0]

    def next_u64():
        lane = [(nxt[0] + i, pb.next_trace_mask(nxt[0] + i)[0]) for i in range(8)]
        nxt[0] += 8
        return lane

    def bitwise(name, a, b):
        out = next_u64()
        for i in range(8):
            pb.add_to_relation(rel[name], 1, [a[i][1], b[i][1], out[i][1]])
            lookups[name].append((a[i][0], b[i][0], out[i][0]))
        n_entries[0] += 8
        return out

    def rotate_left(a, r):
        if r == 0:
            return a
        bits, limb = r % 8, r // 8
        low, high, out = next_u64(), next_u64(), next_u64()
        for i in range(8):
            pb.add_to_relation(rel["rotate"], 1, [a[i][1], pb.const(bits), high[i][1], low[i][1]])
            lookups["rotate"].append((a[i][0], bits, high[i][0], low[i][0]))
            pb.add_constraint(low[(i - limb) & 7][1] + high[(i - limb + 7) & 7][1] - out[i][1])
        n_entries[0] += 8
        return out

    a = [next_u64() for _ in range(25)]
    input_state = [e for lane in a for _, e in lane]
    c = []
    for x in range(5):
        v = a[x]
        for i in range(1, 5):
            v = bitwise("xor", v, a[x + 5 * i])
        c.append(v)
    d = [bitwise("xor", c[(x + 4) % 5], rotate_left(c[(x + 1) % 5], 1)) for x in range(5)]
    for x in range(5):
        for y in range(5):
            a[x + 5 * y] = bitwise("xor", a[x + 5 * y], d[x])
    b = [None] * 25
    for x in range(5):
        for y in range(5):
            b[y + 5 * ((2 * x + 3 * y) % 5)] = rotate_left(a[x + 5 * y], M.ROT[x + 5 * y])
    for x in range(5):
        for y in range(5):
            a[x + 5 * y] = bitwise("xor", b[x + 5 * y], bitwise("not_and", b[(x + 1) % 5 + 5 * y], b[(x + 2) % 5 + 5 * y]))
    rc = [(MAIN + i, pb.next_trace_mask(MAIN + i)[0]) for i in range(8)]
    a[0] = bitwise("xor", a[0], rc)
    assert nxt[0] == MAIN - 1
    is_padding, _next_is_padding = pb.next_trace_mask(MAIN - 1, (0, 1))
    pb.add_constraint(is_padding * (1 - is_padding))
    output_state = [e for lane in a for _, e in lane]
    pb.add_to_relation(rel["state"], is_padding - 1, input_state)
    pb.add_to_relation(rel["state"], 1 - is_padding, output_state)
    assert n_entries[0] + 2 == len(pb.entries) == 2 * LOGUP_COLS
    assert [len(lookups[k]) for k in ("xor", "not_and", "rotate")] == [8 * M.N_XOR, 8 * M.N_NOT_AND, 8 * M.N_ROT]
    pb.finalize_logup_in_pairs(MAIN + PRE, shift)
    return pb, lookups


def table_program(ap, elem, width, shift):
    """a table component: `width` preprocessed tuple columns, then the multiplicity; -multiplicity / combine(tuple) per row"""
    pt = ap.ProgramBuilder()
    t = [pt.next_trace_mask(k)[0] for k in range(width + 1)]
    pt.add_to_relation(pt.relation(elem[0], elem[1], width), -t[width], t[:width])
    pt.finalize_logup(width + 1, shift)
    return pt


def boundary_program(ap, elem, sign, shift):
    """200 state bytes and is_real: sign * is_real / combine(state) per row"""
    pb = ap.ProgramBuilder()
    t = [pb.next_trace_mask(k)[0] for k in range(201)]
    pb.add_constraint(t[200] * (t[200] - 1))
    pb.add_to_relation(pb.relation(elem[0], elem[1], 200), t[200] if sign > 0 else -t[200], t[:200])
    pb.finalize_logup(201, shift)
    return pb


def bitwise_table(op):
    """(a, b, c) over 2^16 rows, row a + 256 b"""
    idx = np.arange(1 << 16, dtype=np.uint32)
    a, b = idx & 255, idx >> 8
    return [a, b, (a ^ b) if op == "xor" else ((a ^ 255) & b)]


def rotate_table():
    """(byte, shift, high, low) over 2^11 rows, row byte + 256 shift"""
    idx = np.arange(1 << 11, dtype=np.uint32)
    byte, s = idx & 255, idx >> 8
    return [byte, s, np.where(s > 0, byte >> (8 - np.minimum(s, 8)), 0).astype(np.uint32), (byte << s) & 255]


def boundary_columns(states, log_size):
    """(n, 25) lanes -> the 200 byte columns and is_real over 2^log_size rows (storage order = any: the component is row-local)"""
    n = len(states)
    cols = np.zeros((201, 1 << log_size), np.uint32)
    cols[:200, :n] = np.ascontiguousarray(states, "<u8").view(np.uint8).reshape(n, 200).T
    cols[200, :n] = 1
    return cols


# ---- the statement of tests/test_gpu_keccak_round.py and tests/test_keccak_round_cpu.py: layout, programs, the model's columns ----
# Seven components: the two round components (16 rounds from 0 over 2^6 rows, 8 rounds from 16 over 2^5 rows; the second is fed the
# first's d_states_out), the xor, not-and and rotate tables, and the two boundary components.  Trees: 0 preprocessed, 1 main, 2 interaction.
N_INST, LOG_A, LOG_B, LOG_BND = 3, 6, 5, 2
LOG_BIT, LOG_ROT = 16, 11
N_INTER = 4 * LOGUP_COLS
COMPONENTS = ("round_a", "round_b", "xor", "not_and", "rotate", "bnd_in", "bnd_out")
TREE_LOGS = [[LOG_A] * PRE + [LOG_B] * PRE + [LOG_BIT] * 6 + [LOG_ROT] * 4,
             [LOG_A] * MAIN + [LOG_B] * MAIN + [LOG_BIT] * 2 + [LOG_ROT] + [LOG_BND] * 402,
             [LOG_A] * N_INTER + [LOG_B] * N_INTER + [LOG_BIT] * 8 + [LOG_ROT] * 4 + [LOG_BND] * 8]
PRE_AT = {"round_a": 0, "round_b": 9, "xor": 18, "not_and": 21, "rotate": 24}                        # first column in tree 0
MAIN_AT = {"round_a": 0, "round_b": 1705, "xor": 3410, "not_and": 3411, "rotate": 3412, "bnd_in": 3413, "bnd_out": 3614}
INTER_AT = {"round_a": 0, "round_b": N_INTER, "xor": 2 * N_INTER, "not_and": 2 * N_INTER + 4, "rotate": 2 * N_INTER + 8, "bnd_in": 2 * N_INTER + 12, "bnd_out": 2 * N_INTER + 16}
COMP_LOG = {"round_a": LOG_A, "round_b": LOG_B, "xor": LOG_BIT, "not_and": LOG_BIT, "rotate": LOG_ROT, "bnd_in": LOG_BND, "bnd_out": LOG_BND}
N_PRE = {"round_a": 9, "round_b": 9, "xor": 3, "not_and": 3, "rotate": 4, "bnd_in": 0, "bnd_out": 0}
N_MAIN = {"round_a": 1705, "round_b": 1705, "xor": 1, "not_and": 1, "rotate": 1, "bnd_in": 201, "bnd_out": 201}
N_INT = {"round_a": N_INTER, "round_b": N_INTER, "xor": 4, "not_and": 4, "rotate": 4, "bnd_in": 4, "bnd_out": 4}
KEY_BITS = {"xor": [8, 8], "not_and": [8, 8], "rotate": [8, 3]}


def statement_programs(ap, elems, shifts):
    return {"round_a": round_program(ap, elems, shifts["round_a"])[0], "round_b": round_program(ap, elems, shifts["round_b"])[0],
            "xor": table_program(ap, elems["xor"], 3, shifts["xor"]), "not_and": table_program(ap, elems["not_and"], 3, shifts["not_and"]),
            "rotate": table_program(ap, elems["rotate"], 4, shifts["rotate"]),
            "bnd_in": boundary_program(ap, elems["state"], +1, shifts["bnd_in"]), "bnd_out": boundary_program(ap, elems["state"], -1, shifts["bnd_out"])}


def host_statement(states):
    """every preprocessed and main column of the statement from the model alone, in tree order (storage order)"""
    fa = M.fill(states, 0, 4, LOG_A)
    fb = M.fill(fa["out"], 16, 3, LOG_B)
    tables = {"xor": bitwise_table("xor"), "not_and": bitwise_table("not_and"), "rotate": rotate_table()}
    pre = list(fa["pre"]) + list(fb["pre"]) + tables["xor"] + tables["not_and"] + tables["rotate"]
    counts = {"xor": np.zeros(1 << 16, np.int64), "not_and": np.zeros(1 << 16, np.int64), "rotate": np.zeros(1 << 11, np.int64)}
    for f in (fa, fb):
        cols = np.concatenate([f["main"], f["pre"]])                    # the round program's numbering: rc bytes behind the main columns
        lane = lambda l, i: cols[(8 * l if l != "rc" else MAIN) + i].astype(np.int64)
        for name in ("xor", "not_and"):
            for a, b, _ in f["sites"][name]:
                for i in range(8):
                    np.add.at(counts[name], lane(a, i) | (lane(b, i) << 8), 1)
        for a, bits, _, _ in f["sites"]["rot"]:
            for i in range(8):
                np.add.at(counts["rotate"], lane(a, i) | (bits << 8), 1)
    main = list(fa["main"]) + list(fb["main"]) + [(counts[k] % P).astype(np.uint32) for k in ("xor", "not_and", "rotate")]
    main += list(boundary_columns(states, LOG_BND)) + list(boundary_columns(fb["out"], LOG_BND))
    return pre, main, fb["out"]


def total(claimed):
    """the sum of the components' claimed sums, coordinate by coordinate"""
    return [int(sum(int(claimed[name][q]) for name in COMPONENTS) % P) for q in range(4)]
