"""The CPU side of the placement axis (tests/placement.py): the pins of the case list and of the classification table, the self-test of
the checker on four deliberate mistakes, the oracle on every case, and the refusals of the W contract that need no device (the check
runs on the host before anything is launched, so a NULL context and made-up addresses that are never dereferenced are enough)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import placement as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "nexus_hip.h")
P = O.P

# every public entry that reads or writes device columns
ENTRIES = """nx_interpolate_batch nx_evaluate_batch nx_lde_batch nx_lde_commit nx_commit_root
nx_merkle_commit nx_merkle_commit_on_layer nx_merkle_leaf_chain nx_merkle_from_leaves
nx_eval_at_points nx_accumulate_quotients nx_accumulate_quotients_partial nx_fold_circle_into_line nx_fold_line nx_fri_decompose
nx_secure_accumulate nx_batch_inverse_m31 nx_batch_inverse_qm31 nx_m31_add_into nx_m31_widen nx_m31_narrow
nx_bit_reverse nx_bit_reverse_secure nx_finalize_columns nx_upload_coset_order nx_upload_columns nx_upload_columns_narrow nx_copy
nx_logup_combine nx_logup_finalize_col nx_logup_col nx_logup_cols nx_logup_cols_batched nx_logup_finalize_last nx_logup_finalize_last_batch
nx_logup_program nx_logup_multiplicities
nx_eval_constraint_program nx_air_eval
nx_trace_prev_access nx_trace_partition_fill nx_trace_program nx_trace_keccak_round nx_trace_keccak_memory_check""".split()

CLASSES = {"S": """nx_eval_at_points nx_fri_decompose nx_secure_accumulate nx_batch_inverse_m31 nx_batch_inverse_qm31 nx_m31_add_into nx_bit_reverse
                   nx_bit_reverse_secure nx_finalize_columns nx_upload_coset_order nx_upload_columns nx_logup_combine nx_logup_finalize_col nx_logup_col
                   nx_logup_cols nx_logup_cols_batched nx_logup_finalize_last nx_logup_finalize_last_batch nx_logup_program nx_eval_constraint_program
                   nx_air_eval nx_trace_partition_fill""".split(),
           "B": "nx_merkle_commit nx_merkle_from_leaves nx_upload_columns_narrow nx_copy nx_logup_multiplicities nx_trace_prev_access nx_trace_program".split(),
           "W": """nx_interpolate_batch nx_evaluate_batch nx_lde_batch nx_lde_commit nx_commit_root nx_merkle_commit_on_layer nx_merkle_leaf_chain
                   nx_accumulate_quotients nx_accumulate_quotients_partial nx_fold_circle_into_line nx_fold_line nx_m31_widen nx_m31_narrow
                   nx_trace_keccak_round nx_trace_keccak_memory_check""".split()}

WIDE_ACCESS = re.compile(r"uint4|uint2|gld4|gst4|gload4|gload2|gstore4|u64\s*\*|KmQuad\s*\*")
CITE = re.compile(r"^([a-z_0-9]+\.(?:hip|h|cuh)):(\d+)")

_LINES = {}


def source_line(cite):
    m = CITE.match(cite)
    assert m, f"citation {cite!r} is not file:line"
    name, line = m.group(1), int(m.group(2))
    if name not in _LINES:
        with open(os.path.join(CSRC, name)) as f:
            _LINES[name] = f.read().split("\n")
    assert 1 <= line <= len(_LINES[name]), cite
    return _LINES[name][line - 1]


# ---------------------------------------------------------------------------------------------------------------- the pins

def test_every_entry_is_classified_and_the_classes_are_pinned():
    assert sorted(PL.TABLE) == sorted(ENTRIES)
    for cls, names in CLASSES.items():
        assert sorted(n for n, r in PL.TABLE.items() if r.cls == cls) == sorted(names), cls
    assert set(r.family for r in PL.TABLE.values()) <= set(PL.FAMILIES)
    assert sum(len(PL.family_cases(f)) for f in PL.FAMILIES) == len(PL.CASES)
    assert len(set(PL.case_id(c) for c in PL.CASES)) == len(PL.CASES)


def test_every_citation_names_a_line_of_the_sources():
    for row in PL.TABLE.values():
        assert row.cites, row.entry
        for cite in row.cites:
            assert source_line(cite).strip(), (row.entry, cite)


def test_w_holds_only_entries_that_cite_a_wide_access_on_a_caller_pointer():
    """the cap that keeps W from swallowing the work: a W row names the argument, the width and the source line of a 16- or 8-byte access;
    an S or B row names none"""
    for row in PL.TABLE.values():
        if row.cls != "W":
            assert not row.wide and row.exempt_below is None, row.entry
            continue
        assert row.wide, row.entry
        for w in row.wide:
            assert w.bytes in (8, 16) and w.arg.startswith("d_"), (row.entry, w)
            line = source_line(w.cite)
            assert WIDE_ACCESS.search(line), f"{row.entry}: {w.cite} is not a wide access: {line.strip()}"


def test_every_entry_runs_at_shift_0_and_every_s_or_b_entry_at_every_shift():
    for name, row in PL.TABLE.items():
        mine = [c for c in PL.CASES if c.entry == name and not c.refuse]
        for log in row.sizes:
            shifts = sorted(set(c.shift for c in mine if c.log == log))
            assert 0 in shifts, (name, log)
            if row.cls in "SB":
                assert shifts == [0, 1, 2, 3], (name, log, shifts)
        if row.cls == "B":                       # at a size where the 16-byte path would otherwise run, named from the dispatch condition
            assert row.vector_from, name
    vector_size = {"nx_merkle_commit": PL.FUSED_LOG, "nx_merkle_from_leaves": 0, "nx_upload_columns_narrow": 4, "nx_copy": PL.COPY_SIZES.index(1024),
                   "nx_logup_multiplicities": PL.MULT_TILE_LOG, "nx_trace_prev_access": 2, "nx_trace_program": 2}
    assert sorted(vector_size) == sorted(CLASSES["B"])
    for name, log in vector_size.items():
        assert sorted(c.shift for c in PL.CASES if c.entry == name and c.log == log and c.variant == PL.VARIANTS.get(name, ("",))[0]) == [0, 1, 2, 3], name
    assert PL.COPY_SIZES[PL.COPY_SIZES.index(1024)] % 4 == 0 and 257 in PL.COPY_SIZES


def test_the_dispatch_thresholds_are_the_sources():
    """the sizes named after a dispatch condition, read from the line that holds it"""
    assert f"FUSED_MIN_LOG = {PL.FUSED_LOG}" in source_line("merkle.hip:601")
    assert "MULT_TILE = MULT_THREADS * MULT_QUADS * 4" in source_line("multiplicity.hip:27") and 256 * 4 * 4 == 1 << PL.MULT_TILE_LOG
    assert "SC_MIN_LOG = SC_H + SC_T + 1" in source_line("logup.hip:293") and "SC_H = 7, SC_T = 5" in source_line("logup.hip:293") and PL.SCAN_TILED_LOG == 13
    assert "n >= 4 && !(align & 15)" in source_line("access_history.cuh:532")
    assert "n >= per_lane && !((uintptr_t)d_cols[c] & 15)" in source_line("fft.hip:783")
    assert "(n_words & 3) || ((uintptr_t)d_dst & 15) || ((uintptr_t)d_src & 15)" in source_line("ctx.hip:555")
    assert "& 15)) vec4 = false" in source_line("air_jit.hip:1603")
    assert "aligned16 && ((uintptr_t)sorted[i] & 15u) == 0" in source_line("merkle.hip:995")
    assert "EVAL_LOG_LO = 10" in source_line("pcs.hip:19")
    assert "log_size >= 14" in source_line("fft.hip:432")


def test_w_entries_are_refused_at_every_forbidden_offset_and_only_there():
    for name in CLASSES["W"]:
        row = PL.TABLE[name]
        refusals = [c for c in PL.CASES if c.entry == name and c.refuse]
        for w in row.wide:
            got = sorted(c.refuse[1] for c in refusals if c.refuse[0] == w.arg)
            assert got == ([1, 2, 3] if w.bytes == 16 else [1, 3]), (name, w.arg, got)
        for c in refusals:
            assert row.exempt_below is None or c.log >= row.exempt_below
    stems = {"d_cols": "col", "d_polys": "poly", "d_out": "out", "d_lde": "lde", "d_out4": "out", "d_prev_layer": "prev", "d_state_in": "state", "d_state_out": "state",
             "d_src4": "src", "d_dst": "dst", "d_src": "src", "d_states": "states", "d_states_out": "states_out", "d_timestamps": "timestamps"}
    # a refusal case places exactly the named column of the named argument at the forbidden offset
    for case in PL.CASES:
        if not case.refuse:
            continue
        arg, shift, index = case.refuse
        width = [w.bytes for w in PL.TABLE[case.entry].wide if w.arg == arg][0]
        plan = PL.build(case)
        cols = plan.arena.cols
        name = stems[arg] + (str(index) if stems[arg] + str(index) in cols else "")
        assert cols[name].start % 4 == shift and (4 * cols[name].start) % width, PL.case_id(case)
        others = [c for n, c in cols.items() if n != name and any(re.fullmatch(stems[w.arg] + r"\d*", n) for w in PL.TABLE[case.entry].wide)]
        assert all((4 * c.start) % 8 == 0 for c in others if c.words >= 4), PL.case_id(case)
    # a plan never places a wide argument at an offset the header forbids, except in a refusal case
    for case in PL.CASES:
        row = PL.TABLE[case.entry]
        if row.cls != "W" or case.refuse or (row.exempt_below is not None and case.log < row.exempt_below):
            continue
        plan = PL.build(case)
        for w in row.wide:
            stem = stems[w.arg]
            cols = [c for n, c in plan.arena.cols.items() if re.fullmatch(stem + r"\d*", n)]
            assert cols or w.arg == "d_prev_layer", (PL.case_id(case), w.arg)
            for c in cols:
                if case.entry == "nx_commit_root" and c.words < 4:
                    continue                     # its 2-row columns are exempt
                assert (4 * c.start) % w.bytes == 0, (PL.case_id(case), c.name)


def test_the_header_states_the_rule_once_and_names_the_entries():
    text = open(HEADER).read()
    assert text.count("ALIGNMENT.") == 1
    para = text[text.index("ALIGNMENT."):]
    para = para[:para.index("*/")]
    for name in CLASSES["W"]:
        assert name in para, name
    for name in CLASSES["B"]:
        assert name in para, name


# ---------------------------------------------------------------------------------------------------------------- the checker judges itself

def _stand_in_plan():
    plan = PL.Plan()
    rng = np.random.default_rng(1)
    a, b = PL.m31(rng, 37), PL.m31(rng, 37)
    plan.add("a", a, shift=1)
    plan.add("b", b, shift=3)
    plan.add("sum", words=37, shift=2)
    plan.want("sum", ((a.astype(np.uint64) + b) % P).astype(np.uint32))
    return plan


def _stand_in_kernel(plan, mistake=None):
    """numpy in the place of a kernel: sum = a + b in the slab, with one deliberate mistake"""
    mem, ar = plan.arena.image(), plan.arena
    a, b = mem[ar.offset("a"):ar.offset("a") + 37].astype(np.uint64), mem[ar.offset("b"):ar.offset("b") + 37].astype(np.uint64)
    out = ar.offset("sum")
    mem[out:out + 37] = ((a + b) % P).astype(np.uint32)
    if mistake == "past":
        mem[out + 37] = 5                       # a 16-byte store that runs one word over
    elif mistake == "before":
        mem[out - 1] = 5
    elif mistake == "input":
        mem[ar.offset("b", 11)] ^= 1
    elif mistake == "unwritten":
        mem[out + 36] = PL.FILL                 # the tail the vector path forgot
    return mem


def test_the_checker_accepts_a_correct_stand_in():
    plan = _stand_in_plan()
    assert plan.arena.check(_stand_in_kernel(plan), plan.expect) == []
    assert (plan.arena.image()[plan.arena.guard_mask()] == PL.FILL).all() and plan.arena.guard_mask().sum() >= 4 * PL.GUARD
    for c in plan.arena.cols.values():
        assert c.start % 4 == {"a": 1, "b": 3, "sum": 2}[c.name]


@pytest.mark.parametrize("mistake,column,word,what", [("past", "sum", 37, "1 word(s) past its last word"), ("before", "sum", -1, "1 word(s) before its first word"),
                                                       ("input", "b", 11, "input column b changed"), ("unwritten", "sum", 36, "still the fill value")])
def test_the_checker_reports_each_mistake_with_the_column_and_the_word_index(mistake, column, word, what):
    plan = _stand_in_plan()
    errs = plan.arena.check(_stand_in_kernel(plan, mistake), plan.expect)
    assert len(errs) == 1, errs
    assert f"column {column} " in errs[0] and f"word index {word}" in errs[0] and what in errs[0], errs[0]


def test_guards_are_at_least_64_words_of_a_value_that_is_no_field_element():
    assert PL.GUARD >= 64 and PL.FILL == 0xDEADBEEF and PL.FILL >= P
    for case in PL.CASES[::7]:
        ar = PL.build(case).arena
        cols = sorted(ar.cols.values(), key=lambda c: c.start)
        assert cols[0].start >= PL.GUARD and ar.size - cols[-1].end >= PL.GUARD
        for x, y in zip(cols, cols[1:]):
            assert y.start - x.end >= PL.GUARD, (PL.case_id(case), x.name, y.name)


# ---------------------------------------------------------------------------------------------------------------- the oracle's side

HASHES = ("nx_merkle_commit_on_layer", "nx_merkle_leaf_chain")       # their outputs are digests, not field elements


@pytest.mark.parametrize("family", PL.FAMILIES)
def test_the_oracle_alone_gives_canonical_words_for_every_case(oracle, family):
    for case in PL.family_cases(family):
        plan = PL.build(case)
        assert plan.arena.size % 4 == 0
        if case.refuse:
            assert not plan.expect and not plan.host
            continue
        assert plan.expect or plan.host, PL.case_id(case)
        for name, words in plan.expect.items():
            assert words.dtype == np.uint32 and words.size == plan.arena.cols[name].words, (PL.case_id(case), name)
            if case.entry not in HASHES + ("nx_m31_widen", "nx_copy", "nx_trace_partition_fill", "nx_trace_program", "nx_trace_keccak_round", "nx_trace_keccak_memory_check"):
                assert int(words.max()) < P, (PL.case_id(case), name)
        for c in plan.arena.cols.values():       # no output aliases an input by accident: every column has its own words
            assert c.words > 0
        mem = plan.arena.image()
        for name, words in plan.expect.items():
            mem[plan.arena.offset(name):plan.arena.offset(name) + words.size] = words
        assert plan.arena.check(mem, plan.expect) == [], PL.case_id(case)
        if any(plan.arena.cols[n].data is None for n in plan.expect):      # and an output nobody wrote is reported
            assert plan.arena.check(plan.arena.image(), plan.expect), PL.case_id(case)


def test_the_shared_twiddle_tree_gives_the_words_of_a_tree_of_the_columns_own_size(oracle):
    for log in (1, 2, 3, 6, 13):
        v = PL.m31(np.random.default_rng(log), 1 << log)
        own = O.Twiddles(log + 1)
        coef = own.interpolate(v)
        assert np.array_equal(PL.otw().interpolate(v), coef) and np.array_equal(PL.otw().evaluate(coef, log + 1), own.evaluate(coef, log + 1))


def test_the_session_case_commits_columns_of_two_rows_in_the_oracle(oracle):
    for mode in (0, 1):
        logs, host, root = PL.session_case(mode)
        assert logs == [1, 1, 1, 2, 2, 5] and [h.size for h in host] == [2, 2, 2, 4, 4, 32] and root.shape == (8,)
    assert not np.array_equal(PL.session_case(0)[2], PL.session_case(1)[2])


# ---------------------------------------------------------------------------------------------------------------- refusals on the host

def _lib():
    import nexus_zkvm_amd as nz
    return nz.load_library()


BASE = 0x7F0000001000       # a made-up device address, 4096-byte aligned: a refused call never dereferences it


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_the_transform_and_quotient_entries_refuse_before_anything_is_launched(shift):
    """NULL context, made-up addresses: the refusal comes from the host-side check alone (a launch would need a device)"""
    L = _lib()
    good, bad = BASE, BASE + 0x1000 + 4 * shift
    ptrs = lambda *a: (C.c_void_p * len(a))(*a)
    err = lambda: L.nx_last_error(None).decode()
    assert L.nx_interpolate_batch(None, None, ptrs(good, bad), 2, 3) == -2 and "nx_interpolate_batch: d_cols[1] must be 16-byte aligned" in err()
    assert L.nx_evaluate_batch(None, None, ptrs(bad, good), 2, 2, 1, ptrs(good, good)) == -2 and "nx_evaluate_batch: d_polys[0] must be 16-byte aligned" in err()
    assert L.nx_evaluate_batch(None, None, ptrs(good, good), 2, 2, 1, ptrs(good, bad)) == -2 and "nx_evaluate_batch: d_out[1] must be 16-byte aligned" in err()
    assert L.nx_lde_batch(None, None, ptrs(good, good, bad), 3, 5, 1, ptrs(good, good, good)) == -2 and "nx_lde_batch: d_cols[2] must be 16-byte aligned" in err()
    assert L.nx_lde_batch(None, None, ptrs(good), 1, 5, 1, ptrs(bad)) == -2 and "nx_lde_batch: d_lde[0] must be 16-byte aligned" in err()
    z = (C.c_uint32 * 8)()
    assert L.nx_accumulate_quotients(None, 2, ptrs(good, bad), 2, z, 0, z, z, z, z, ptrs(good, good, good, good)) == -2 and "nx_accumulate_quotients: d_cols[1]" in err()
    assert L.nx_accumulate_quotients_partial(None, 2, ptrs(good, good), 2, z, 0, z, z, z, z, None, 1, ptrs(good, good, bad, good)) == -2
    assert "nx_accumulate_quotients_partial: d_out4[2] must be 16-byte aligned" in err()


@pytest.mark.parametrize("shift", [1, 3])
def test_widen_and_narrow_refuse_a_64_bit_side_that_is_not_8_byte_aligned(shift):
    L = _lib()
    bad = C.c_void_p(BASE + 4 * shift)
    assert L.nx_m31_widen(None, bad, C.c_void_p(BASE), C.c_size_t(4)) == -2 and "nx_m31_widen: d_dst must be 8-byte aligned" in L.nx_last_error(None).decode()
    assert L.nx_m31_narrow(None, C.c_void_p(BASE), bad, C.c_size_t(4)) == -2 and "nx_m31_narrow: d_src must be 8-byte aligned" in L.nx_last_error(None).decode()
