"""tests/poison_sites.py against the sources: every place that takes a block from the context's caching allocator has its row (what writes
each region of the block before its first reader), the kernels and functions the rows cite exist, and the sweep of
tests/test_gpu_poison.py names real entries."""
import collections
import glob
import os
import re

import placement as PL
import poison_sites as S

ROOT = S.ROOT


def _sources():
    text = ""
    for ext in ("hip", "h", "cuh"):
        for path in sorted(glob.glob(os.path.join(S.CSRC, "*." + ext))):
            with open(path) as f:
                text += f.read()
    return text


def test_the_scanner_finds_the_sites_it_is_meant_to():
    sites = S.scan_sites()
    assert sum(sites.values()) >= 90 and len(sites) >= 40
    # one of each shape of call: dev_alloc in an extern "C" entry, in a template of a .cuh, in a struct's method; DevBuf::alloc behind . and ->;
    # SecureColumn::alloc_rows; nx_alloc in a transport callback
    for key in (("multiplicity.hip", "nx_logup_multiplicities"), ("access_history.cuh", "access_history"), ("fft.hip", "HostFeed::begin"), ("merkle.hip", "alloc"),
                ("prover.hip", "TreeBuilder::commit_begin"), ("prover.hip", "upload_owned"), ("prover.hip", "composition_accumulator"), ("comm_local.hip", "cb_allreduce_m31")):
        assert key in sites, key
    assert sites[("fft.hip", "nx_twiddles_create")] == 4 and sites[("comm_local.hip", "cb_allreduce_m31")] == 2
    # the allocator's own definition and declaration are no sites
    assert ("ctx.hip", "dev_alloc") not in sites and not any(f == "internal.h" for f, _ in sites)
    assert None not in {fn for _, fn in sites}, "an allocation call outside every function the scanner recognises"


def test_every_allocation_site_has_its_row():
    sites = S.scan_sites()
    rows = collections.Counter()
    for s in S.TABLE:
        rows[(s.file, s.function)] += s.calls
    assert len(rows) == len(S.TABLE), "two rows for one function"
    without = {k: v for k, v in sites.items() if k not in rows}
    assert not without, f"allocation sites without a row in tests/poison_sites.py (say what writes the block before its first reader): {without}"
    stale = {k: v for k, v in rows.items() if k not in sites}
    assert not stale, f"rows of tests/poison_sites.py whose function takes no block any more: {stale}"
    differ = {k: (sites[k], rows[k]) for k in sites if sites[k] != rows[k]}
    assert not differ, f"(calls in the sources, calls in the row): {differ}"


def test_every_row_names_a_writer_for_every_region():
    for s in S.TABLE:
        assert s.regions, s
        for region in s.regions:
            assert len(region) == 2 and all(isinstance(x, str) and x.strip() for x in region), (s.function, region)
        assert not re.search(r":\d+", " ".join(w for _, w in s.regions)), f"{s.function}: rows cite names, not lines"


def test_the_kernels_and_functions_the_rows_cite_exist():
    src = _sources()
    missing = []
    for s in S.TABLE:
        assert re.search(r"\b%s\s*\(" % re.escape(s.function.split("::")[-1]), src), s.function
        for _, writer in s.regions:
            for name in re.findall(r"\b(?:\w+_kernel|nx_\w+|\w+_launch|count_pass|upload_async_staged|synth_fill_range|lde_batch_from|axpy_scale|transpose_blocks|reduce_to_root|"
                                   r"build_inner_layers|logup_columns|air_eval_rows|copy_d2h_blocking)\b", writer):
                if not re.search(r"\b%s\b" % re.escape(name), src):
                    missing.append((s.function, name))
    assert not missing, f"cited, but nowhere under csrc/: {missing}"


def test_the_sweep_names_real_entries():
    with open(os.path.join(ROOT, "include", "nexus_hip.h")) as f:
        hdr = f.read()
    unknown = [n for n in S.SWEEP_EXTRA if n not in PL.TABLE and not re.search(r"\b%s\s*\(" % re.escape(n), hdr)]
    assert not unknown, unknown
    assert not (set(S.SWEEP_EXTRA) & set(PL.TABLE)), "the placement table's entries are swept through their cases"
    for n in PL.TABLE:
        assert re.search(r"\b%s\s*\(" % re.escape(n), hdr), n


def test_the_gpu_sweep_covers_the_list():
    """every name of the sweep list stands in tests/test_gpu_poison.py: as the entry a binding method is cited for, or called through the library"""
    with open(os.path.join(ROOT, "tests", "test_gpu_poison.py")) as f:
        text = f.read()
    absent = [n for n in S.SWEEP_EXTRA if n not in text]
    assert not absent, absent


def test_the_host_twins_poison_every_block():
    for shim in ("mult_emul", "prev_emul"):
        with open(os.path.join(ROOT, "tests", "native", shim, "internal.h")) as f:
            text = f.read()
        alloc = text[text.index("inline int dev_alloc("):]
        alloc, free = alloc[:alloc.index("inline void dev_free(")], alloc[alloc.index("inline void dev_free("):]
        assert "0xA5A5A5A5u" in alloc and "0xFFFFFFFFu" in free[:free.index("\n")], shim


def test_the_options_are_in_the_table_with_their_ranges():
    with open(os.path.join(S.CSRC, "ctx.hip")) as f:
        src = f.read()
    assert re.search(r'\{"debug\.poison", &nx_options::debug_poison, 0, 3\}', src)
    assert re.search(r'\{"debug\.poison_free", &nx_options::debug_poison_free, 0, 1\}', src)
    assert 'env_int("NX_DEBUG_POISON", 0)' in src and 'env_int("NX_DEBUG_POISON_FREE", 0)' in src
