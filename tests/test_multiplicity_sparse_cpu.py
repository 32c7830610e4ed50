"""nx_logup_multiplicities_sparse, what needs no GPU: the numpy model (tests/multiplicity_sparse_model.py) pinned against a dictionary
restatement and against the dense call's rule, the export and its refusals with a NULL context, the constant the GPU tests read the
LDS cut-off from, the Rust binding — and the kernels themselves, compiled as host C++ and run in lock step under the sanitizers
(tests/native/multiplicity_sparse_emul.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiplicity_sparse_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_ERR_ARG = -2
P = M.P


def _lib():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nz, nz.load_library()


# ---------------------------------------------------------------- the model ----------
def _by_dictionary(uses, table, valid, key_bits):
    """The rule of include/nexus_hip.h word by word, one row at a time over a dict."""
    shifts = [sum(key_bits[:i]) for i in range(len(key_bits))]

    def key_of(cols, r):
        vals = [int(c[r]) for c in cols]
        if any(v >> b for v, b in zip(vals, key_bits)):
            return None
        return sum(v << s for v, s in zip(vals, shifts))

    row_of = {}
    for p in range(len(table[0])):
        if valid is not None and int(valid[p]) == 0:
            continue
        k = key_of(table, p)
        if k is None:
            return ("range", p)
        if k in row_of:
            return ("duplicate", row_of[k], p)
        row_of[k] = p
    sums, missing = {}, []
    for u, (cols, w) in enumerate(uses):
        for r in range(len(cols[0])):
            x = 1 if w is None else int(w[r])
            if x == 0:
                continue
            k = key_of(cols, r)
            if k is None or k not in row_of:
                missing.append((u, r))
            else:
                sums[row_of[k]] = sums.get(row_of[k], 0) + x
    return [sums.get(p, 0) % P for p in range(len(table[0]))], missing


def _random_case(rng, key_bits, log_table, n_valid, logs, break_table=None):
    tb, n = sum(key_bits), 1 << log_table
    n_valid = min(n_valid, 1 << tb)
    keys = set()
    while len(keys) < n_valid:
        keys.add(int(rng.integers(0, 1 << tb)))
    keys = np.array(sorted(keys), np.uint64)
    rng.shuffle(keys)
    where = rng.permutation(n)
    table = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in key_bits]      # garbage, outside the bits too
    valid = np.zeros(n, np.uint32)
    for c, col in zip(table, M.split(keys, key_bits)):
        c[where[:n_valid]] = col
    valid[where[:n_valid]] = rng.integers(1, 1 << 32, n_valid, dtype=np.uint64).astype(np.uint32)
    for r in where[n_valid:][::2]:                       # rows that are no table rows: copies of valid keys among them
        if n_valid:
            src = where[int(rng.integers(0, n_valid))]
            for c in table:
                c[r] = c[src]
    if break_table == "duplicate" and n_valid >= 2:
        a, b = sorted(where[:2])
        for c in table:
            c[b] = c[a]
    if break_table == "range":
        i = int(np.argmin(key_bits))
        if key_bits[i] < 32 and n_valid:
            table[i][where[0]] = 1 << key_bits[i]
    uses = []
    for log in logs:
        m = 1 << log
        pick = keys[rng.integers(0, n_valid, m)] if n_valid else np.zeros(m, np.uint64)
        stray = rng.random(m) < 0.1
        pick = np.where(stray, rng.integers(0, 1 << tb, m, dtype=np.uint64), pick)
        cols = M.split(pick, key_bits)
        if key_bits[0] < 32 and m > 2:
            cols[0][int(rng.integers(0, m))] = 1 << key_bits[0]       # one entry outside its bits
        w = None if log % 2 else rng.choice(np.array([0, 1, 2, P - 1], np.uint32), m)
        uses.append((cols, w))
    return uses, table, (valid if n_valid < n or rng.random() < 0.5 else None)


@pytest.mark.parametrize("key_bits", [[32], [16, 16], [8, 8, 8, 8], [20], [1], [3, 2, 4, 5]])
def test_model_equals_the_dictionary_restatement(key_bits):
    rng = np.random.default_rng(sum(key_bits) * 7 + len(key_bits))
    for log_table, n_valid in ((0, 1), (0, 0), (2, 3), (5, 32), (5, 11), (6, 1), (4, 0)):
        for break_table in (None, "duplicate", "range"):
            uses, table, valid = _random_case(rng, key_bits, log_table, n_valid, (0, 1, 3, 6), break_table)
            want = _by_dictionary(uses, table, valid, key_bits)
            try:
                got = M.multiplicities(uses, table, valid, key_bits)
            except M.TableRefused as e:
                assert want == (("range", e.pos) if e.kind == "range" else ("duplicate", e.first, e.second))
                continue
            assert isinstance(want[0], list), want
            assert got[0].tolist() == want[0] and got[1] == sorted(want[1])
            assert all(got[0][p] == 0 for p in range(len(table[0])) if valid is not None and valid[p] == 0)


def test_model_keeps_sums_exact_beyond_64_bits_of_float():
    """2^10 rows of weight p - 1 on one key: the sum is 2^10 (p - 1), mod p = p - 2^10"""
    table, uses = [np.array([5, 0xFFFFFFFF], np.uint32)], [([np.full(1 << 10, 0xFFFFFFFF, np.uint32)], np.full(1 << 10, P - 1, np.uint32))]
    mult, missing = M.multiplicities(uses, table, None, [32])
    assert mult.tolist() == [0, P - (1 << 10)] and missing == []


def _dense_rule(uses, table, key_bits):
    """The dense call's rule as tests/test_gpu_multiplicities.py states it: one 64-bit counter per key of the key space, np.add.at,
    read through the table."""
    def pack(cols):
        key, ok, shift = np.zeros(len(cols[0]), np.int64), np.ones(len(cols[0]), bool), 0
        for c, b in zip(cols, key_bits):
            c = np.asarray(c, np.int64)
            ok &= c < (1 << b)
            key |= (c & ((1 << b) - 1)) << shift
            shift += b
        return key, ok
    tkey, tok = pack(table)
    assert tok.all() and len(set(tkey.tolist())) == len(tkey)
    count, present = np.zeros(1 << sum(key_bits), np.uint64), np.zeros(1 << sum(key_bits), bool)
    present[tkey] = True
    missing = []
    for u, (cols, w) in enumerate(uses):
        key, ok = pack(cols)
        w = np.ones(len(key), np.uint64) if w is None else np.asarray(w, np.uint64)
        live = w != 0
        np.add.at(count, key[live & ok], w[live & ok])
        missing += [(u, int(p)) for p in np.nonzero(live & ~(ok & present[key]))[0]]
    return (count[tkey] % np.uint64(P)).astype(np.uint32), sorted(missing)


@pytest.mark.parametrize("key_bits", [[8], [12], [8, 8], [3, 2, 4, 5]])
def test_model_on_a_full_dense_table_is_the_dense_rule(key_bits):
    rng = np.random.default_rng(len(key_bits) + sum(key_bits))
    tb = sum(key_bits)
    table = M.split(rng.permutation(1 << tb), key_bits)
    uses = []
    for log in (0, 3, 9, 12):
        cols = [rng.integers(0, 1 << b, 1 << log, dtype=np.uint32) for b in key_bits]
        cols[0][0] = 1 << key_bits[0]
        uses.append((cols, None if log == 9 else rng.choice(np.array([0, 1, P - 1, P - 2], np.uint32), 1 << log)))
    want = _dense_rule(uses, table, key_bits)
    for valid in (None, np.full(1 << tb, 7, np.uint32)):
        got = M.multiplicities(uses, table, valid, key_bits)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]


# ---------------------------------------------------------------- the library ----------
def test_symbol_is_declared_exported_and_bound():
    nz, lib = _lib()
    assert "nx_logup_multiplicities_sparse" in nz.declared_symbols()
    assert hasattr(lib, "nx_logup_multiplicities_sparse")
    assert hasattr(nz.HipBackend, "logup_multiplicities_sparse")


def test_lds_cut_off_constant_is_the_headers():
    nz, _ = _lib()
    m = re.search(r"^#define NX_MULT_SPARSE_LDS_LOG_KEYS (\d+)\s*$", open(nz.HEADER_PATH).read(), flags=re.M)
    assert m and int(m.group(1)) == nz.MULT_SPARSE_LDS_LOG_KEYS
    assert 6 < nz.MULT_SPARSE_LDS_LOG_KEYS < 13          # the GPU tests reach the two-level search with a table of 2^13 rows at most
    src = open(os.path.join(ROOT, "nexus-zkvm_amd", "csrc", "multiplicity_sparse.hip")).read()
    assert "log_table > MS_LDS_LOG_KEYS" in src and "MS_LDS_LOG_KEYS = NX_MULT_SPARSE_LDS_LOG_KEYS" in src


def test_argument_errors_with_a_null_context_are_errors_not_crashes():
    nz, lib = _lib()
    f = lib.nx_logup_multiplicities_sparse
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert f(None, None, 0, 0, None, None, None, 0, None, None, None, None) == NX_ERR_ARG
    assert b"nx_logup_multiplicities_sparse" in lib.nx_last_error(None)
    bits = (C.c_uint32 * 2)(16, 16)
    vals = (C.c_void_p * 2)(0x1000, 0x2000)
    use = nz.LookupUse(C.cast(vals, C.c_void_p), None, 4)
    table = (C.c_void_p * 2)(0x3000, 0x4000)
    n, fu, fp = C.c_uint64(77), C.c_uint32(78), C.c_uint64(79)
    assert f(None, C.byref(use), 1, 2, bits, table, C.c_void_p(0x6000), 5, C.c_void_p(0x5000), C.byref(n), C.byref(fu), C.byref(fp)) == NX_ERR_ARG
    assert (n.value, fu.value, fp.value) == (77, 78, 79)


def test_sys_crate_is_the_generators_output_and_the_wrapper_calls_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    assert "pub fn nx_logup_multiplicities_sparse(ctx: *mut nx_ctx, uses: *const nx_lookup_use," in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    assert "pub fn logup_multiplicities_sparse(&mut self" in hip and "sys::nx_logup_multiplicities_sparse(" in hip
    patch = open(os.path.join(ROOT, "rust", "nexus-hip", "reference_patch", "prove2_hip.rs")).read()
    assert "logup_multiplicities_sparse(" in patch


def test_kernels_in_lock_step_on_the_host_under_sanitizers(tmp_path):
    """csrc/multiplicity_sparse.hip as host C++ (tests/native/mults_emul/internal.h over the fiber engine of prev_emul: 256 lock-step
    fibers per block, waves of 64): every keying, table size, valid-row pattern, weight kind, missing row and refusal against a count
    over a map, with ASan and UBSan watching every LDS, splitter, segment, counter and position index — and the device-memory bound of
    the header.  Twice: as built (tables up to 2^12 rows searched in LDS, 2^13 behind splitters), and with a block cap of 2 and two
    splitters, where a block of the sort takes eight tiles and every table of more than two rows is searched in global memory."""
    gxx = shutil.which("g++")
    native = os.path.join(ROOT, "tests", "native")
    csrc = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")
    shutil.copy(os.path.join(csrc, "multiplicity_sparse.hip"), str(tmp_path / "multiplicity_sparse_emu.cpp"))
    shutil.copy(os.path.join(csrc, "count_pass.cuh"), str(tmp_path / "count_pass.cuh"))
    shutil.copy(os.path.join(native, "prev_emul", "internal.h"), str(tmp_path / "prev_internal.h"))
    shutil.copy(os.path.join(native, "mults_emul", "internal.h"), str(tmp_path / "internal.h"))
    for cap, lds, flags in ((1024, 4096, []), (2, 2, ["-DNX_COUNT_PASS_MAX_BLOCKS=2", "-DNX_MULT_SPARSE_LDS_LOG_KEYS=1"])):
        exe = str(tmp_path / ("multiplicity_sparse_emul_%d" % cap))
        subprocess.run([gxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-Wno-unknown-pragmas"] + flags +
                       ["-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"), os.path.join(native, "multiplicity_sparse_emul.cpp"), "-o", exe], check=True, capture_output=True)
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "\n0 failures" in r.stdout and r.stdout.count(" OK ") >= 100 and "FAIL" not in r.stdout
        assert ("block cap %d\nLDS keys %d\n" % (cap, lds)) in r.stdout and "PLAN NOT REACHED" not in r.stdout
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
