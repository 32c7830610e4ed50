"""The product's proof verifier (nx_verifier_*, nx_verify_synth, nx_verify_machine — csrc/host/verifier.{h,cpp}) without a GPU: proofs
made by the CPU oracle's PROVER are judged by the product's VERIFIER, and wherever the oracle's verifier has a verdict the two must
agree — two statements of the protocol that share no code.

1. round trips of the synthetic machine under every hash rule x FRI alpha rule x constraint-degree bound, wrong transcript, wrong shape,
   changed configurations;  2. the machine with a real logup trace (tests/machine_ref.py);  3. recorded AIRs through the session
   (tests/air_examples.py), the channel digest after verify;  4. EVERY word of a proof changed twice and the proof cut to every length
   0, 7, 14, ...: the product refuses each one, as the oracle does;  5. the same sweep through a CPU build of the verifier under
   AddressSanitizer + UBSan (tests/native/verifier_selftest.cpp);  6. the library's verifier in a process that sees no GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import air_examples as X
import machine_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = O.P
SYNTH = [(7, 3, 21, 6), (5, 2, 4, 3), (7, 2, 3, 0)]
AD = b"\x01\x02"
# MACHINE_CASES-style statements (tests/test_gpu_machine.py proves the same shapes on the GPU and on the oracle)
MACHINE = [
    ([(8, 3, 20, 8)], dict(pow_bits=6)),
    ([(9, 4, 18, 4)], dict(pow_bits=5, log_constraint_degree=2)),
    ([(8, 3, 20, 24), (8, 2, 3, 0), (5, 2, 2, 8)], dict(pow_bits=6, hash_mode=1, fri_alpha_mode=1)),
    ([(9, 5, 35, 16, 1), (8, 3, 17, 8, 2), (7, 2, 6, 4, 1)], dict(pow_bits=5, log_constraint_degree=2)),
    ([(9, 3, 20, 12, 0, M.PAIRS)], dict(pow_bits=5)),
    ([(8, 2, 9, 4, 0, M.PAIRS | M.ODD), (6, 3, 5, 4, 0, M.PAIRS)], dict(pow_bits=4, hash_mode=1, fri_alpha_mode=1)),
    ([(8, 5, 12, 8, 1, M.PAIRS | M.ODD), (7, 4, 3, 4, 1, M.TABLE)], dict(pow_bits=4)),
]
SWEEP_MACHINE = ([(7, 2, 20, 12), (5, 2, 4, 4), (4, 2, 3, 0)], dict(pow_bits=3, log_constraint_degree=2), 11, b"\x05")


@pytest.fixture(scope="module")
def nz(oracle):
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    nz.load_library()
    return nz


def _ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


def _nzcfg(nz, ocfg):
    return nz.PcsConfig(*[int(x) for x in ocfg])


def _mutations(w):
    """(index, value) of item 4: every word + 1 mod 2^32 and every word with its top bit flipped; the truncation lengths 0, 7, 14, ..."""
    muts = []
    for i in range(len(w)):
        muts += [(i, (int(w[i]) + 1) & 0xFFFFFFFF), (i, int(w[i]) ^ 0x80000000)]
    return muts, list(range(0, len(w), 7))


def prove_machine_with_claimed(comps, ocfg, seed, ad):
    """machine_ref.prove_machine plus `Proof.claimed_sum`: the claimed sum of a component is its shift x N, and the shift is what the
    component builder is handed."""
    claimed = []

    def capture(ap, c, l, z, alpha, sh, lcd):
        claimed.append([(int(x) << c[0]) % P for x in sh])
        return M.machine_component(ap, c, l, z, alpha, sh, lcd)
    words = M.prove_machine(comps, ocfg, seed=seed, ad=ad, threads=4, component_fn=capture)
    return words, np.array(claimed, np.uint32)


# ---------------------------------------------------------------- 1. the synthetic machine ----------
@pytest.mark.parametrize("lcd", [1, 2])
@pytest.mark.parametrize("fri_mode", [0, 1])
@pytest.mark.parametrize("hash_mode", [0, 1])
def test_synth_round_trip_wrong_transcript_and_changed_config(nz, oracle, hash_mode, fri_mode, lcd):
    kw = dict(pow_bits=6, hash_mode=hash_mode, fri_alpha_mode=fri_mode, log_constraint_degree=lcd)
    ocfg, cfg = O.default_cfg(**kw), nz.default_config(**kw)
    w = oracle.prove_synth(SYNTH, ocfg, seed=3, ad=AD)
    assert oracle.verify_synth(SYNTH, ocfg, w, ad=AD) is None
    assert nz.verify_synth(SYNTH, cfg, w, ad=AD) is None
    text, rc = nz.verify_synth(SYNTH, cfg, w, ad=b"\x01\x03", want_rc=True)                    # the transcript prefix matters
    assert rc == nz.NX_ERR_VERIFY and text, (rc, text)
    wrong_shape = [(7, 3, 21, 6), (5, 2, 4, 3), (7, 2, 4, 0)]
    assert oracle.verify_synth(wrong_shape, ocfg, w, ad=AD) is not None
    text, rc = nz.verify_synth(wrong_shape, cfg, w, ad=AD, want_rc=True)
    assert rc in (nz.NX_ERR_VERIFY, nz.NX_ERR_ARG) and text, (rc, text)
    # the other node-hash rule: the proof's decommitments no longer hash to its roots
    assert nz.verify_synth(SYNTH, cfg, w, ad=AD, hash_mode=1 - hash_mode) is not None
    for field, base in (("n_queries", 3), ("log_blowup", 1), ("pow_bits", 6)):
        for delta in (+1, -1):
            kw2 = dict(kw); kw2[field] = base + delta
            o = oracle.verify_synth(SYNTH, O.default_cfg(**kw2), w, ad=AD)
            p = nz.verify_synth(SYNTH, nz.default_config(**kw2), w, ad=AD)
            assert (o is None) == (p is None), (field, delta, o, p)


# ---------------------------------------------------------------- 2. the machine with a real logup trace ----------
@pytest.mark.parametrize("comps,kw", MACHINE)
def test_machine_proofs_of_the_oracle_are_accepted_and_a_changed_claimed_sum_is_refused(nz, oracle, comps, kw):
    ocfg, cfg = O.default_cfg(**kw), nz.default_config(**kw)
    words, claimed = prove_machine_with_claimed(comps, ocfg, 0xBEEF, AD)
    assert M.verify_machine(comps, ocfg, words, claimed, ad=AD) is None
    assert nz.verify_machine(comps, cfg, words, claimed, ad=AD) is None
    # verify_logup_sum: the sum the caller expects of the claimed sums
    total = [int(sum(int(x) for x in claimed[:, q]) % P) for q in range(4)]
    assert nz.verify_machine(comps, cfg, words, claimed, ad=AD, expected_logup_sum=total) is None
    text, rc = nz.verify_machine(comps, cfg, words, claimed, ad=AD, expected_logup_sum=[(total[0] + 1) % P] + total[1:], want_rc=True)
    assert rc == nz.NX_ERR_VERIFY and "logup sum" in text
    k = next(i for i, c in enumerate(comps) if c[3])          # a component that has logup columns
    bad = claimed.copy(); bad[k, 0] = (int(bad[k, 0]) + 1) % P
    assert M.verify_machine(comps, ocfg, words, bad, ad=AD) is not None
    text, rc = nz.verify_machine(comps, cfg, words, bad, ad=AD, want_rc=True)
    assert rc == nz.NX_ERR_VERIFY and text
    assert nz.verify_machine(comps, cfg, words, claimed, ad=b"\x01\x03") is not None


# ---------------------------------------------------------------- 3. recorded AIRs through the session ----------
def _both_verifiers(nz, ocfg, replay, components, words):
    """Runs replay(session, commit) on the oracle's and the product's verifier session, verifies, compares verdict and channel digest."""
    ov = O.VerifierSession(ocfg)
    replay(ov, ov.commit)
    pv = nz.VerifierSession(_nzcfg(nz, ocfg))
    replay(pv, pv.commit)
    assert np.array_equal(ov.digest(), pv.digest())
    o, p = ov.verify(components, words), pv.verify(components, words)
    assert (o is None) == (p is None), (o, p)
    if o is None:
        assert np.array_equal(ov.digest(), pv.digest())           # the transcript's final state
    else:
        assert pv.rc in (nz.NX_ERR_VERIFY, nz.NX_ERR_ARG)
    # the same answer when asked again (a refusal restores the channel, an acceptance restarts from the state it found)
    d = pv.digest()
    assert (pv.verify(components, words) is None) == (p is None)
    assert np.array_equal(d, pv.digest())
    pv.close()
    return o


def _roots(words):
    w = np.asarray(words, np.uint32)
    h = O.proof_header_words()
    return [w[h + 1 + 8 * t: h + 9 + 8 * t].copy() for t in range(int(w[h]))]


@pytest.mark.parametrize("comps,lcd", [([(6, 3, 20, 19)], 1), ([(5, 2, 18, 4), (7, 3, 5, 17)], 2), ([(6, 2, 3, 0)], 1)])
def test_session_accepts_the_recorded_synthetic_machine(nz, oracle, comps, lcd):
    from test_prover_session_cpu import drive_synthetic, synthetic_components
    ocfg = O.default_cfg(pow_bits=3, log_constraint_degree=lcd, log_blowup=max(1, lcd))
    ad = b"\x07\x2a"
    s = O.ProverSession(ocfg, max(c[0] for c in comps))
    drive_synthetic(None, comps, 9, ad, s.commit, s)
    air = synthetic_components(comps)
    words = s.prove(air)
    roots = _roots(words)

    def replay(v, commit):
        for b in ad:
            v.mix_u64(b)
        for c in comps:
            v.mix_u64(c[0])
        commit(roots[0], [c[0] for c in comps for _ in range(c[1])])
        commit(roots[1], [c[0] for c in comps for _ in range(c[2])])
        v.draw_felt()
        v.mix_felts(np.zeros((len(comps), 4), np.uint32))
        commit(roots[2], [c[0] for c in comps for _ in range(c[3])])
    assert _both_verifiers(nz, ocfg, replay, air, words) is None
    # and the one-call form agrees with the session on the same bytes
    assert nz.verify_synth(comps, _nzcfg(nz, ocfg), words, ad=ad) is None
    bad = words.copy(); bad[len(bad) // 2] ^= 4
    assert _both_verifiers(nz, ocfg, replay, air, bad) is not None


@pytest.mark.parametrize("logs,lcd,bounds,hd", [((5, 7), 1, None, False), ((6,), 2, None, False), ((7, 5, 6), 2, (1, 2, 1), False),
                                                ((6, 5), 2, (2, 1), True), ((5, 6), 2, None, True)])
def test_session_accepts_the_logup_air_with_mask_offsets_and_secure_columns(nz, oracle, logs, lcd, bounds, hd):
    from test_prover_session_cpu import build_mixed_air
    ocfg = O.default_cfg(pow_bits=2, log_constraint_degree=lcd, log_blowup=lcd)
    drive, tree_logs = build_mixed_air(logs, lcd=lcd, bounds=bounds, high_degree=hd)
    s = O.ProverSession(ocfg, max(logs))
    roots = []
    comps = drive(s, lambda cols: roots.append(s.commit(cols)))
    words = s.prove(comps)

    def replay(v, commit):
        it = iter(zip(roots, tree_logs))
        drive(v, lambda cols: commit(*next(it)))
    assert _both_verifiers(nz, ocfg, replay, comps, words) is None
    # other lookup elements in the components: the composition value no longer matches
    import copy
    wrong = copy.deepcopy(comps)
    ec = np.array(wrong[0].program.econsts, np.uint32).reshape(-1, 4).copy()
    ec[0, 0] = (int(ec[0, 0]) + 1) % P
    wrong[0].program.econsts = [tuple(int(x) for x in r) for r in ec]
    assert _both_verifiers(nz, ocfg, replay, wrong, words) is not None


@pytest.mark.parametrize("n_trees", [2, 3, 4])
def test_session_takes_any_number_of_trace_trees(nz, oracle, n_trees):
    trees, comp = X.tree_count_statement(_ap(), n_trees)
    ocfg = O.default_cfg(pow_bits=2)
    s = O.ProverSession(ocfg, 6)
    s.mix_u64(n_trees)
    roots = [s.commit(t) for t in trees]
    words = s.prove([comp])

    def replay(v, commit):
        v.mix_u64(n_trees)
        for r, t in zip(roots, trees):
            commit(r, [6] * len(t))
    assert _both_verifiers(nz, ocfg, replay, [comp], words) is None

    def replay_wrong(v, commit):          # another root than the proof's for the last tree
        v.mix_u64(n_trees)
        for k, (r, t) in enumerate(zip(roots, trees)):
            commit(r if k + 1 < len(roots) else roots[0], [6] * len(t))
    assert _both_verifiers(nz, ocfg, replay_wrong, [comp], words) is not None


def test_session_refuses_inconsistent_statements_with_arg_errors(nz, oracle):
    trees, comp = X.tree_count_statement(_ap(), 3)
    ocfg = O.default_cfg(pow_bits=2)
    s = O.ProverSession(ocfg, 6)
    roots = [s.commit(t) for t in trees]
    words = s.prove([comp])
    v = nz.VerifierSession(_nzcfg(nz, ocfg))
    assert v.verify([comp], words) is not None and v.rc == nz.NX_ERR_ARG            # no tree committed
    for r, t in zip(roots[:2], trees):
        v.commit(r, [6] * len(t))
    assert v.verify([comp], words) is not None and v.rc == nz.NX_ERR_ARG            # a component column outside the committed trees
    v.commit(roots[2], [6] * len(trees[2]))
    assert v.verify([comp], words) is None
    with pytest.raises(nz.NexusHipError):
        v.commit(roots[2], [40])
    with pytest.raises(nz.NexusHipError):
        nz.VerifierSession(nz.default_config(log_blowup=0))
    with pytest.raises(nz.NexusHipError):
        nz.VerifierSession(nz.default_config(), hash_mode=7)


# ---------------------------------------------------------------- 4. exhaustive tampering ----------
def test_every_word_changed_and_every_truncation_of_a_synth_proof_is_refused(nz, oracle):
    ocfg, cfg = O.default_cfg(pow_bits=4), nz.default_config(pow_bits=4)
    w = oracle.prove_synth(SYNTH, ocfg, seed=3, ad=AD)
    assert oracle.verify_synth(SYNTH, ocfg, w, ad=AD) is None and nz.verify_synth(SYNTH, cfg, w, ad=AD) is None
    muts, truncs = _mutations(w)
    disagree = []
    for i, v in muts:
        m = w.copy(); m[i] = v
        o = oracle.verify_synth(SYNTH, ocfg, m, ad=AD)
        text, rc = nz.verify_synth(SYNTH, cfg, m, ad=AD, want_rc=True)
        if o is None or rc not in (nz.NX_ERR_VERIFY, nz.NX_ERR_ARG):
            disagree.append((i, v, o, rc, text))
    for n in truncs:
        o = oracle.verify_synth(SYNTH, ocfg, w[:n], ad=AD)
        text, rc = nz.verify_synth(SYNTH, cfg, w[:n], ad=AD, want_rc=True)
        if o is None or rc not in (nz.NX_ERR_VERIFY, nz.NX_ERR_ARG):
            disagree.append(("cut", n, o, rc, text))
    assert not disagree, disagree[:10]


def test_every_word_changed_and_every_truncation_of_a_machine_proof_is_refused(nz, oracle):
    comps, kw, seed, ad = SWEEP_MACHINE
    ocfg, cfg = O.default_cfg(**kw), nz.default_config(**kw)
    w, claimed = prove_machine_with_claimed(comps, ocfg, seed, ad)
    assert M.verify_machine(comps, ocfg, w, claimed, ad=ad) is None and nz.verify_machine(comps, cfg, w, claimed, ad=ad) is None
    bad = claimed.copy(); bad[0, 0] = (int(bad[0, 0]) + 1) % P
    assert "OodsNotMatching" in M.verify_machine(comps, ocfg, w, bad, ad=ad)
    assert "composition" in nz.verify_machine(comps, cfg, w, bad, ad=ad)
    muts, truncs = _mutations(w)
    disagree = []
    for i, v in muts:
        m = w.copy(); m[i] = v
        o = M.verify_machine(comps, ocfg, m, claimed, ad=ad)
        text, rc = nz.verify_machine(comps, cfg, m, claimed, ad=ad, want_rc=True)
        if o is None or rc not in (nz.NX_ERR_VERIFY, nz.NX_ERR_ARG):
            disagree.append((i, v, o, rc, text))
    need = O.proof_header_words() + 1 + 3 * 8          # shorter streams make the checker's Python replay raise before it reaches the oracle
    for n in truncs:
        o = M.verify_machine(comps, ocfg, w[:n], claimed, ad=ad) if n >= need else "too short for the checker's replay"
        text, rc = nz.verify_machine(comps, cfg, w[:n], claimed, ad=ad, want_rc=True)
        if o is None or rc not in (nz.NX_ERR_VERIFY, nz.NX_ERR_ARG):
            disagree.append(("cut", n, o, rc, text))
    assert not disagree, disagree[:10]


# ---------------------------------------------------------------- 5. the CPU build under the sanitizers ----------
def _case_words(kind, ocfg, body, proof):
    muts, truncs = _mutations(proof)
    parts = [np.array([kind] + [int(x) for x in ocfg] + [int(ocfg[4])], np.uint32), body, np.array([len(proof)], np.uint32), np.asarray(proof, np.uint32),
             np.array([len(muts)], np.uint32), np.array(muts, np.uint32).reshape(-1), np.array([len(truncs)], np.uint32), np.array(truncs, np.uint32)]
    return np.concatenate(parts)


def test_native_selftest_under_address_and_undefined_behaviour_sanitizers(nz, oracle, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    # case 0: the synthetic machine through nx_verify_synth
    ocfg = O.default_cfg(pow_bits=4)
    w = oracle.prove_synth(SYNTH, ocfg, seed=3, ad=AD)
    body = np.array([len(SYNTH)] + [x for c in SYNTH for x in (tuple(c) + (0, 0))[:6]] + [len(AD)] + list(AD), np.uint32)
    cases = [_case_words(0, ocfg, body, w)]
    # case 1: the machine through a verifier session, its components recorded by the checker's emitter with the lookup elements of the
    # untouched proof (a changed root changes the transcript: refused whatever the components hold)
    import ref_emitter as ap
    comps, kw, seed, ad = SWEEP_MACHINE
    mcfg = O.default_cfg(**kw)
    mw, claimed = prove_machine_with_claimed(comps, mcfg, seed, ad)
    v = nz.VerifierSession(_nzcfg(nz, mcfg))
    ops = []
    for b in list(ad) + [c[0] for c in comps]:
        v.mix_u64(b); ops.append([0, b, 0])
    tree_logs = [[c[0] for c in comps for _ in range(c[1 + t])] for t in range(3)]
    roots = _roots(mw)
    for t in (0, 1):
        v.commit(roots[t], tree_logs[t]); ops.append([3, t, len(tree_logs[t])] + tree_logs[t])
    z, alpha = v.draw_felts(2); ops.append([2, 2])
    v.mix_felts(claimed); ops.append([1, len(comps)] + [int(x) for x in claimed.reshape(-1)])
    v.commit(roots[2], tree_logs[2]); ops.append([3, 2, len(tree_logs[2])] + tree_logs[2])
    locs, a, b, d = [], 0, 0, 0
    for c in comps:
        locs.append((a, b, d)); a += c[1]; b += c[2]; d += c[3]
    shifts = [np.array([(int(x) * pow((1 << c[0]) % P, P - 2, P)) % P for x in cs], np.uint32) for c, cs in zip(comps, claimed)]
    components = [M.machine_component(ap, c, l, z, alpha, sh, int(mcfg[6])) for c, l, sh in zip(comps, locs, shifts)]
    assert v.verify(components, mw) is None
    body = np.concatenate([np.array([len(ops)] + [x for op in ops for x in op], np.uint32), O.encode_air(components)])
    cases.append(_case_words(1, mcfg, body, mw))
    path = tmp_path / "cases.bin"
    np.concatenate([np.array([0x5456584E, len(cases)], np.uint32)] + cases).tofile(path)
    exe = str(tmp_path / "verifier_selftest")
    csrc = os.path.join(ROOT, "nexus-zkvm_amd", "csrc", "host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "native", "verifier_selftest.cpp"), os.path.join(csrc, "verifier.cpp"), "-o", exe], check=True, capture_output=True)
    # the sanitizer runtimes are linked statically, so the executable does not care what else the process has loaded before it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 unexpected" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    n_expected = sum(1 + 2 * len(p) + len(range(0, len(p), 7)) for p in (w, mw))
    assert r.stdout.startswith(f"{n_expected} verdicts"), r.stdout


# ---------------------------------------------------------------- 6. no GPU in sight ----------
def test_library_verifier_runs_in_a_process_without_a_gpu(nz, oracle, tmp_path):
    ocfg = O.default_cfg(pow_bits=4)
    w = oracle.prove_synth(SYNTH, ocfg, seed=3, ad=AD)
    np.asarray(w, np.uint32).tofile(tmp_path / "proof.bin")
    code = (
        "import sys, numpy as np\n"
        f"sys.path[:0] = [{ROOT!r}]\n"
        "import nexus_zkvm_amd as nz\n"
        f"w = np.fromfile({str(tmp_path / 'proof.bin')!r}, np.uint32)\n"
        f"comps, ad = {SYNTH!r}, {AD!r}\n"
        "cfg = nz.default_config(pow_bits=4)\n"
        "L = nz.load_library()\n"
        "import ctypes as C\n"
        "ctx = C.c_void_p()\n"
        "print('ctx', L.nx_ctx_create(0, C.byref(ctx)))\n"
        "print('verdict', nz.verify_synth(comps, cfg, w, ad=ad))\n"
        "w[100] ^= 1\n"
        "print('tampered', nz.verify_synth(comps, cfg, w, ad=ad, want_rc=True)[1])\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    assert lines["ctx"] == "-5", r.stdout                 # NX_ERR_NO_DEVICE: the process has no GPU ...
    assert lines["verdict"] == "None" and lines["tampered"] == "-6", r.stdout      # ... and the verifier does not need one
