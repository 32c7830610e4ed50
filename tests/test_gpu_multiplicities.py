"""nx_logup_multiplicities on the device against numpy's exact integer count.

The expected column is np.add.at over 64-bit integers (the largest sum of this file is 2^12 (p - 1) < 2^43: exact), reduced mod
p = 2^31 - 1 once, read through the table: mult[pos] = count[key of table row pos].  Every comparison is an equality.
1. shapes: rows 2^0 .. 2^14 in 1 / 3 / 17 uses of mixed sizes, tables of 2^4, 2^8, the largest LDS-counted key space
   (NX_MULT_LDS_MAX_KEY_BITS) and the next one, two 8-bit key columns, a 20-bit key; identity / bit-reversed / random table order;
2. skew;  3. weights;  4. missing rows;  5. refusals;  6. determinism;  7. memory;  8. a statement whose lookups balance: the three
claimed sums add up to zero, the trace checker, the product's verifier and the oracle's verifier accept — and one multiplicity off by
one makes the sum nonzero."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P
NX_OK, NX_ERR_ARG, NX_ERR_PROTOCOL = 0, -2, -4


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def _order(kind, log_table, rng):
    n = 1 << log_table
    if kind == "identity":
        return np.arange(n, dtype=np.int64)
    if kind == "bitrev":
        return np.array([_bitrev(i, log_table) for i in range(n)], dtype=np.int64)
    return rng.permutation(n).astype(np.int64)


def _split(keys, key_bits):
    """keys -> one uint32 column per key column"""
    out, shift = [], 0
    for b in key_bits:
        out.append(((np.asarray(keys, np.int64) >> shift) & ((1 << b) - 1)).astype(np.uint32))
        shift += b
    return out


def _pack(cols, key_bits):
    """(keys, in-range mask) of rows given as one column per key column"""
    key, ok, shift = np.zeros(len(cols[0]), np.int64), np.ones(len(cols[0]), bool), 0
    for c, b in zip(cols, key_bits):
        c = np.asarray(c, np.int64)
        ok &= c < (1 << b)
        key |= (c & ((1 << b) - 1)) << shift
        shift += b
    return key, ok


def expected(uses, table, key_bits):
    """uses: (columns, weights or None) of host arrays; table: columns.  -> (mult column, sorted (use, pos) of the missing rows)"""
    tkey, tok = _pack(table, key_bits)
    assert tok.all() and len(set(tkey.tolist())) == len(tkey)
    count = np.zeros(1 << sum(key_bits), np.uint64)
    present = np.zeros(1 << sum(key_bits), bool)
    present[tkey] = True
    missing = []
    for u, (cols, w) in enumerate(uses):
        key, ok = _pack(cols, key_bits)
        w = np.ones(len(key), np.uint64) if w is None else np.asarray(w, np.uint64)
        live = w != 0
        good = live & ok
        np.add.at(count, key[good], w[good])
        missing += [(u, int(p)) for p in np.nonzero(live & ~(ok & present[key]))[0]]
    return (count[tkey] % np.uint64(P)).astype(np.uint32), sorted(missing)


def run(be, uses, table, key_bits, prefill=0xDEADBEEF):
    """Uploads, calls, reads back: (mult words, (n_missing, first_use, first_pos), rc)."""
    keep, dev_uses = [], []
    for cols, w in uses:
        d = be.columns_from_host(np.stack([np.asarray(c, np.uint32) for c in cols]))
        dw = be.columns_from_host(np.asarray(w, np.uint32)) if w is not None else None
        keep += [d, dw]
        dev_uses.append(([d.ptr.value + k * (4 << d.log_size) for k in range(len(cols))], dw.ptr.value if dw is not None else None, d.log_size))
    t = be.columns_from_host(np.stack([np.asarray(c, np.uint32) for c in table]))
    out = be.columns_from_host(np.full(len(table[0]), prefill, np.uint32))
    res, rc = be.logup_multiplicities(dev_uses, [t.ptr.value + k * (4 << t.log_size) for k in range(len(table))], t.log_size, key_bits, out.ptr.value, want_rc=True)
    return out.to_cpu().reshape(-1), res, rc


def check(be, uses, table, key_bits):
    want, missing = expected(uses, table, key_bits)
    got, res, rc = run(be, uses, table, key_bits)
    assert np.array_equal(got, want)
    if missing:
        assert rc == NX_ERR_PROTOCOL and res == (len(missing),) + missing[0]
    else:
        assert rc == NX_OK and res == (0, 0, 0)
    return got


def _uniform_use(rng, log, key_bits, weights=None):
    return ([rng.integers(0, 1 << b, 1 << log, dtype=np.uint32) for b in key_bits], weights)


# ---------------------------------------------------------------- 1. shapes ----------
def _shape_tables(nz):
    L = nz.MULT_LDS_MAX_KEY_BITS
    return [([4], 4), ([8], 8), ([L], L), ([L + 1], L + 1), ([8, 8], 16), ([20], 20)]


USE_LOGS = {1: (14,), 3: (0, 3, 11), 17: (0, 3, 6, 11, 14, 6, 3, 0, 11, 6, 3, 0, 14, 6, 3, 11, 0)}


@pytest.mark.parametrize("order", ["identity", "bitrev", "random"])
@pytest.mark.parametrize("which", range(6))
def test_counts_equal_numpy_on_every_shape(be, nz, which, order):
    key_bits, log_table = _shape_tables(nz)[which]
    rng = np.random.default_rng(100 + which)
    table = _split(_order(order, log_table, rng), key_bits)
    for n_uses, logs in USE_LOGS.items():
        uses = [_uniform_use(rng, log, key_bits) for log in logs]
        assert len(uses) == n_uses
        check(be, uses, table, key_bits)


def test_no_use_at_all_gives_a_zero_column(be):
    got = check(be, [], _split(np.arange(16), [4]), [4])
    assert not got.any()


# ---------------------------------------------------------------- 2. skew ----------
@pytest.mark.parametrize("key_bits", [[8], [5], [8, 8], [14]])
def test_skewed_columns(be, key_bits):
    rng = np.random.default_rng(7)
    log_table, n = sum(key_bits), 1 << 14
    table = _split(_order("random", log_table, rng), key_bits)
    constant = ([np.full(n, 7 % (1 << b), np.uint32) for b in key_bits], None)
    one_row = [np.zeros(n, np.uint32) for _ in key_bits]
    for c, b in zip(one_row, key_bits):
        c[4097] = (1 << b) - 1
    mostly_zero = [np.where(rng.random(n) < 0.9, 0, rng.integers(0, 1 << b, n)).astype(np.uint32) for b in key_bits]
    got = check(be, [constant, (one_row, None), _uniform_use(rng, 14, key_bits), (mostly_zero, None)], table, key_bits)
    assert int(got.astype(np.uint64).sum()) == 4 * n


# ---------------------------------------------------------------- 3. weights ----------
@pytest.mark.parametrize("key_bits", [[8], [8, 8]])
def test_weights(be, key_bits):
    rng = np.random.default_rng(11)
    log_table = sum(key_bits)
    table = _split(_order("bitrev", log_table, rng), key_bits)
    n = 1 << 12
    flags = rng.integers(0, 2, n, dtype=np.uint32)
    heavy = ([np.full(n, 5, np.uint32) for _ in key_bits], np.full(n, P - 1, np.uint32))          # 2^12 (p - 1) on one key: ~2^43
    mixed_w = rng.choice(np.array([0, 1, P - 1, P - 2], np.uint32), n)
    skew_cols = [np.where(rng.random(n) < 0.8, 3, rng.integers(0, 1 << b, n)).astype(np.uint32) for b in key_bits]
    uses = [_uniform_use(rng, 12, key_bits), _uniform_use(rng, 12, key_bits, flags), heavy, (skew_cols, mixed_w)]
    check(be, uses, table, key_bits)
    got = check(be, [heavy], table, key_bits)
    tkey, _ = _pack(table, key_bits)
    heavy_key, _ = _pack([np.array([5])] * len(key_bits), key_bits)
    assert int(got[np.nonzero(tkey == heavy_key[0])[0][0]]) == ((1 << 12) * (P - 1)) % P
    assert np.count_nonzero(got) == 1


# ---------------------------------------------------------------- 4. missing rows ----------
def _three_uses(rng, key_bits=(8,)):
    return [_uniform_use(rng, 6, key_bits), _uniform_use(rng, 13, key_bits), _uniform_use(rng, 3, key_bits)]


def test_one_out_of_range_value_is_named_and_the_rest_is_counted(be):
    rng = np.random.default_rng(21)
    table = _split(np.arange(256), [8])
    uses = _three_uses(rng)
    uses[1][0][0][4321] = 300
    want, missing = expected(uses, table, [8])
    assert missing == [(1, 4321)]
    got, res, rc = run(be, uses, table, [8])
    assert rc == NX_ERR_PROTOCOL and res == (1, 1, 4321)
    text = be.L.nx_last_error(be.ctx).decode()
    assert "use 1 row position 4321" in text and "(300)" in text and "not a row of the table" in text
    assert np.array_equal(got, want)                                  # all other counts are still right
    assert int(got.astype(np.uint64).sum()) == 64 + 8192 + 8 - 1
    # the same value under weight 0 is no lookup at all
    w = np.ones(1 << 13, np.uint32)
    w[4321] = 0
    uses[1] = (uses[1][0], w)
    got, res, rc = run(be, uses, table, [8])
    assert rc == NX_OK and res == (0, 0, 0)
    assert np.array_equal(got, expected(uses, table, [8])[0])


def test_two_missing_rows_give_the_smaller_use_and_position(be):
    rng = np.random.default_rng(22)
    table = _split(np.arange(256), [8])
    uses = _three_uses(rng)
    uses[2][0][0][5] = 1 << 20
    uses[1][0][0][8000] = 256
    uses[1][0][0][77] = P - 1
    got, res, rc = run(be, uses, table, [8])
    assert rc == NX_ERR_PROTOCOL and res == (3, 1, 77)
    assert "use 1 row position 77: (%d)" % (P - 1) in be.L.nx_last_error(be.ctx).decode()
    assert np.array_equal(got, expected(uses, table, [8])[0])


@pytest.mark.parametrize("key_bits,log_table", [([8], 7), ([7, 7], 13)])
def test_a_key_in_range_but_absent_from_the_table_is_missing(be, key_bits, log_table):
    """A table that lists only even keys; both counting forms."""
    rng = np.random.default_rng(23)
    table = _split(2 * _order("random", log_table, rng), key_bits)
    cols = _split(2 * rng.integers(0, 1 << log_table, 1 << 11), key_bits)
    odd = 2 * 9 + 1
    for c, v in zip(cols, _split([odd], key_bits)):
        c[1500] = v[0]
    flags = np.ones(1 << 11, np.uint32)
    uses = [(cols, None), (cols, flags)]
    want, missing = expected(uses, table, key_bits)
    assert missing == [(0, 1500), (1, 1500)]
    got, res, rc = run(be, uses, table, key_bits)
    assert rc == NX_ERR_PROTOCOL and res == (2, 0, 1500) and np.array_equal(got, want)
    tup = ", ".join(str(int(v[0])) for v in _split([odd], key_bits))
    assert "use 0 row position 1500: (%s)" % tup in be.L.nx_last_error(be.ctx).decode()


# ---------------------------------------------------------------- 5. refusals ----------
def test_refusals_leave_the_context_usable(be, nz):
    rng = np.random.default_rng(31)
    uses = [_uniform_use(rng, 9, [8])]
    dup = np.arange(256)
    dup[200] = 17
    with pytest.raises(nz.NexusHipError, match=r"error -2: .*two table rows hold \(17\)"):
        run(be, uses, _split(dup, [8]), [8])
    far = np.arange(256, dtype=np.uint32)
    far[31] = 256
    with pytest.raises(nz.NexusHipError, match=r"error -2: .*table row position 31 "):
        run(be, uses, [far], [8])
    wide = [rng.integers(0, 2, 512, dtype=np.uint32) for _ in range(3)]
    with pytest.raises(nz.NexusHipError, match=r"error -2: .*add up to 25"):
        run(be, [(wide, None)], [np.zeros(16, np.uint32)] * 3, [12, 12, 1])
    with pytest.raises(nz.NexusHipError, match="error -2"):
        run(be, uses, _split(np.arange(512), [9]), [8])              # more table rows than keys
    with pytest.raises(nz.NexusHipError, match="error -2"):
        be.logup_multiplicities([([0x1000], None, 31)], [0x1000], 8, [8], 0x1000)
    check(be, uses, _split(np.arange(256), [8]), [8])
    comps, cfg = [(8, 2, 6, 3)], nz.default_config(pow_bits=3)
    words = be.prove(comps, cfg, seed=3, ad=b"m")
    assert nz.verify_synth(comps, cfg, words, ad=b"m") is None


# ---------------------------------------------------------------- 6. determinism, 7. memory ----------
@pytest.mark.parametrize("key_bits", [[8], [16]])
def test_same_words_on_every_run_and_nothing_is_kept(be, key_bits):
    rng = np.random.default_rng(41)
    n = 1 << 14
    table = _split(_order("random", sum(key_bits), rng), key_bits)
    w = rng.choice(np.array([0, 1, P - 1, P - 2], np.uint32), n)
    cols = [np.where(rng.random(n) < 0.9, 0, rng.integers(0, 1 << b, n)).astype(np.uint32) for b in key_bits]
    uses = [(cols, w), _uniform_use(rng, 14, key_bits)]
    d = be.columns_from_host(np.stack(cols + [w] + uses[1][0]))
    ptr = lambda k: d.ptr.value + k * (4 << 14)
    k = len(key_bits)
    dev_uses = [([ptr(i) for i in range(k)], ptr(k), 14), ([ptr(k + 1 + i) for i in range(k)], None, 14)]
    t = be.columns_from_host(np.stack(table))
    tp = [t.ptr.value + i * (4 << t.log_size) for i in range(k)]
    outs = [be.columns(1, t.log_size) for _ in range(2)]
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    for o in outs:
        assert be.logup_multiplicities(dev_uses, tp, t.log_size, key_bits, o.ptr.value) == (0, 0, 0)
    live1, peak = be.memory()
    assert live1 == live0 and peak > live0                             # temporaries came from the context's allocator and went back
    a, b = outs[0].to_cpu().reshape(-1), outs[1].to_cpu().reshape(-1)
    assert np.array_equal(a, b)
    assert np.array_equal(a, expected(uses, table, key_bits)[0])


# ---------------------------------------------------------------- 8. a balanced lookup through the session ----------
LOG_A, LOG_B, LOG_T = 10, 4, 8


def _statement_columns():
    rng = np.random.default_rng(808)
    n = 1 << LOG_A
    flag = rng.integers(0, 2, n, dtype=np.uint32)
    a = [np.zeros(n, np.uint32), rng.integers(0, 256, n, dtype=np.uint32),
         np.where(rng.random(n) < 0.9, 0, rng.integers(0, 256, n)).astype(np.uint32), np.where(rng.random(n) < 0.7, 255, rng.integers(0, 256, n)).astype(np.uint32),
         flag, np.where(flag == 1, rng.integers(0, 256, n), 300).astype(np.uint32)]
    b = [rng.integers(0, 256, 1 << LOG_B, dtype=np.uint32) for _ in range(2)]
    return a, b


def _programs(ap, z, alpha, shifts):
    """The three components as the recorder sees them (add_to_relation + finalize_logup); column numbering per component."""
    pa = ap.ProgramBuilder()
    cols = [pa.next_trace_mask(k)[0] for k in range(6)]
    rel = pa.relation(z, alpha, 1)
    pa.add_constraint(cols[4] * (cols[4] - 1))                         # the numerator is a flag
    for k in range(4):
        pa.add_to_relation(rel, 1, [cols[k]])
    pa.add_to_relation(rel, cols[4], [cols[5]])
    pa.finalize_logup(6, shifts[0])
    pb = ap.ProgramBuilder()
    cols = [pb.next_trace_mask(k)[0] for k in range(2)]
    rel = pb.relation(z, alpha, 1)
    for k in range(2):
        pb.add_to_relation(rel, 1, [cols[k]])
    pb.finalize_logup(2, shifts[1])
    pt = ap.ProgramBuilder()
    (value,), (m,) = pt.next_trace_mask(0), pt.next_trace_mask(1)      # preprocessed RangeValues, the multiplicity
    rel = pt.relation(z, alpha, 1)
    pt.add_to_relation(rel, -m, [value])
    pt.finalize_logup(2, shifts[2])
    return pa, pb, pt


def _balanced_session(be, nz, bump):
    """Returns (claimed sums, and — unless bump — session, components, proof words, the roots and tree log sizes)."""
    import nexus_zkvm_amd.air_program as ap
    ocfg = O.default_cfg(pow_bits=2)
    cfg = nz.PcsConfig(*[int(x) for x in ocfg])
    a, b = _statement_columns()
    range_values = np.arange(1 << LOG_T, dtype=np.uint32)             # value i at storage position i
    tree_logs = [[LOG_T], [LOG_A] * 6 + [LOG_B] * 2 + [LOG_T], [LOG_A] * 20 + [LOG_B] * 8 + [LOG_T] * 4]
    s = be.prover_session(cfg, LOG_A)
    s.mix_u64(3)
    roots = [s.commit([range_values])]
    table = be.columns_from_host(range_values)
    main = s.tree_begin(tree_logs[1])
    for host, d in zip(a + b, main):
        be._chk(be.L.nx_upload(be.ctx, C.c_void_p(d), host.ctypes.data_as(C.c_void_p), C.c_size_t(len(host))))
    uses = [([main[k]], None, LOG_A) for k in range(4)] + [([main[5]], main[4], LOG_A)] + [([main[6 + k]], None, LOG_B) for k in range(2)]
    assert be.logup_multiplicities(uses, [table.ptr.value], LOG_T, [8], main[8]) == (0, 0, 0)      # written in place: the table component's main column
    mult = nz.DeviceColumns.view(be, main[8], 1, LOG_T)
    want, _ = expected([([c], None) for c in a[:4]] + [([a[5]], a[4])] + [([c], None) for c in b], [range_values], [8])
    got = mult.to_cpu().reshape(-1)
    assert np.array_equal(got, want)
    if bump:
        got[129] = (int(got[129]) + 1) % P
        mult.upload(got[None, :])
    kept = [be.clone_columns(nz.DeviceColumns.view(be, d, 1, lg)) for d, lg in zip(main, tree_logs[1])]      # the commit turns columns into coefficients
    roots.append(s.tree_commit())
    z, alpha = s.draw_felt(), s.draw_felt()
    fracs = [p.build_logup() for p in _programs(ap, z, alpha, [(0, 0, 0, 0)] * 3)]
    inter = s.tree_begin(tree_logs[2])
    ins = [[k.ptr.value for k in kept[:6]], [k.ptr.value for k in kept[6:8]], [table.ptr.value, kept[8].ptr.value]]
    outs, logs = [inter[:20], inter[20:28], inter[28:]], [LOG_A, LOG_B, LOG_T]
    claimed, shifts = [], []
    for frac, cols, out, log in zip(fracs, ins, outs, logs):
        assert 4 * frac.n_logup_cols == len(out)
        be.logup_program(frac, cols + [None] * len(out), log, out_ptrs=out)
        claimed.append(be.logup_finalize_last(out[-4:], log_size=log))
        n_inv = pow((1 << log) % P, P - 2, P)
        shifts.append([(int(x) * n_inv) % P for x in claimed[-1]])
    claimed = np.array(claimed, np.uint32)
    if bump:
        s.close()
        return claimed, None
    s.mix_felts(claimed)
    roots.append(s.tree_commit())
    pa, pb, pt = _programs(ap, z, alpha, shifts)
    comps = [ap.Component(LOG_A, pa.build(), [(1, k) for k in range(6)] + [(2, k) for k in range(20)]),
             ap.Component(LOG_B, pb.build(), [(1, 6), (1, 7)] + [(2, 20 + k) for k in range(8)]),
             ap.Component(LOG_T, pt.build(), [(0, 0), (1, 8)] + [(2, 28 + k) for k in range(4)])]
    return claimed, (s, cfg, ocfg, comps, roots, tree_logs, (z, alpha))


def test_a_statement_whose_lookups_balance_is_proved_and_verified(be, nz, oracle):
    claimed, (s, cfg, ocfg, comps, roots, tree_logs, (z, alpha)) = _balanced_session(be, nz, bump=False)
    total = [int(sum(int(c[q]) for c in claimed) % P) for q in range(4)]
    assert total == [0, 0, 0, 0]                                      # the reference verifier's zero-sum rule (machine.rs:343)
    assert any(c.any() for c in claimed)
    report = s.check(comps)
    assert report.ok, report
    words = s.prove(comps)
    for v in (nz.VerifierSession(cfg), O.VerifierSession(ocfg)):
        v.mix_u64(3)
        v.commit(roots[0], tree_logs[0])
        v.commit(roots[1], tree_logs[1])
        assert np.array_equal(v.draw_felt(), z) and np.array_equal(v.draw_felt(), alpha)
        v.mix_felts(claimed)
        v.commit(roots[2], tree_logs[2])
        assert v.verify(comps, words) is None
        assert np.array_equal(v.digest(), s.digest())
    s.close()
    # the control: one multiplicity off by one and the sums no longer cancel
    off, _ = _balanced_session(be, nz, bump=True)
    assert [int(sum(int(c[q]) for c in off) % P) for q in range(4)] != [0, 0, 0, 0]
    # (the other main root draws other lookup elements, so none of the three sums is comparable with the balanced run's)
