"""The product's verifier against proofs the library itself makes on the GPU, and the root-only commit (nx_commit_root).

7. every proof of this file — nx_prove_machine, nx_prove_synth, the prover session; blowup 2 and 4, both hash rules, a +2 component
   (quarter domain), a prover2-shaped statement of many small components, one proof on 4 thread-ranks — is accepted by the product's
   verifier AND by the CPU oracle's, and a flipped word is refused by both;  8. a 2^20-row machine proof is verified by the product (the
   oracle's prover could not make it in test time): the verifier's wall time is printed next to the prove time;  9. nx_commit_root ==
   nx_lde_commit's root on 1 / 15 / 16 / 17 / 33 columns, mixed sizes, the empty tree, both hash rules, == the preprocessed root inside a
   proof, and its device-memory bound (include/nexus_hip.h) holds by the allocator's own count;  10. examples/session_prove.c verifies."""
import os
import shutil
import subprocess
import threading
import time

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O
import machine_ref as M

pytestmark = pytest.mark.gpu
P = O.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    import nexus_zkvm_amd as nz
    b = nz.HipBackend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


def _flip(words):
    w = words.copy()
    w[len(w) // 2] ^= 2
    return w


MACHINE = [
    ([(8, 3, 20, 8)], dict(pow_bits=6)),
    ([(9, 4, 18, 4), (6, 2, 5, 4)], dict(pow_bits=5, log_blowup=2, log_constraint_degree=2)),                 # blowup 4
    ([(8, 3, 20, 24), (8, 2, 3, 0), (5, 2, 2, 8)], dict(pow_bits=6, hash_mode=1, fri_alpha_mode=1)),
    ([(10, 3, 20, 8, 2), (7, 2, 6, 4, 1)], dict(pow_bits=4, log_constraint_degree=2)),                        # a +2 component: the quarter domain
    ([(8, 5, 12, 8, 1, M.PAIRS | M.ODD), (7, 4, 3, 4, 1, M.TABLE)], dict(pow_bits=4)),
    # prover2-shaped: many small components, bound 1, logup in pairs
    ([(5 + k % 4, 2, 4 + k % 3, 4, 1, M.PAIRS) for k in range(24)], dict(pow_bits=4, log_constraint_degree=2, hash_mode=1)),
]


@pytest.mark.parametrize("comps,kw", MACHINE)
def test_machine_proofs_of_the_library_are_accepted_by_both_verifiers(be, nz, oracle, comps, kw):
    cfg, ocfg = nz.default_config(**kw), O.default_cfg(**kw)
    words = be.prove_machine(comps, cfg, seed=0xBEEF, ad=b"\x01\x02")
    claimed = be.machine_claimed_sums()
    assert nz.verify_machine(comps, cfg, words, claimed, ad=b"\x01\x02") is None
    assert M.verify_machine(comps, ocfg, words, claimed, ad=b"\x01\x02") is None
    bad = _flip(words)
    text, rc = nz.verify_machine(comps, cfg, bad, claimed, ad=b"\x01\x02", want_rc=True)
    assert rc in (nz.NX_ERR_VERIFY, nz.NX_ERR_ARG) and text
    assert M.verify_machine(comps, ocfg, bad, claimed, ad=b"\x01\x02") is not None
    k = next(i for i, c in enumerate(comps) if c[3])
    wrong = claimed.copy(); wrong[k, 1] = (int(wrong[k, 1]) + 1) % P
    assert nz.verify_machine(comps, cfg, words, wrong, ad=b"\x01\x02") is not None


@pytest.mark.parametrize("kw", [dict(pow_bits=5), dict(pow_bits=4, log_blowup=2, log_constraint_degree=2, hash_mode=1, fri_alpha_mode=1)])
def test_synth_proofs_of_the_library_are_accepted_by_both_verifiers(be, nz, oracle, kw):
    comps = [(9, 3, 21, 6), (6, 2, 4, 3), (9, 2, 3, 0)]
    cfg, ocfg = nz.default_config(**kw), O.default_cfg(**kw)
    words = be.prove(comps, cfg, seed=21, ad=b"sy")
    assert nz.verify_synth(comps, cfg, words, ad=b"sy") is None
    assert O.verify_synth(comps, ocfg, words, ad=b"sy") is None
    assert nz.verify_synth(comps, cfg, _flip(words), ad=b"sy") is not None
    assert O.verify_synth(comps, ocfg, _flip(words), ad=b"sy") is not None


@pytest.mark.parametrize("logs,lcd,bounds,hd", [((7, 9), 1, None, False), ((10, 8), 2, (2, 1), True)])
def test_session_proofs_are_accepted_and_both_sessions_end_in_the_same_transcript_state(be, nz, oracle, logs, lcd, bounds, hd):
    from test_prover_session_cpu import build_mixed_air
    ocfg = O.default_cfg(pow_bits=2, log_constraint_degree=lcd, log_blowup=lcd)
    cfg = nz.PcsConfig(*[int(x) for x in ocfg])
    drive, tree_logs = build_mixed_air(logs, lcd=lcd, bounds=bounds, high_degree=hd)
    s = be.prover_session(cfg, max(logs))
    roots = []
    comps = drive(s, lambda cols: roots.append(s.commit(cols)))
    words = s.prove(comps)
    pv, ov = nz.VerifierSession(cfg), O.VerifierSession(ocfg)
    for v in (pv, ov):
        it = iter(zip(roots, tree_logs))
        drive(v, lambda cols, v=v, it=it: v.commit(*next(it)))
    assert pv.verify(comps, words) is None and ov.verify(comps, words) is None
    assert np.array_equal(pv.digest(), s.digest()) and np.array_equal(ov.digest(), s.digest())      # prover and verifiers: one transcript
    assert pv.verify(comps, _flip(words)) is not None and ov.verify(comps, _flip(words)) is not None
    pv.close(); s.close()


def test_one_proof_on_four_thread_ranks_verifies(be, nz, oracle):
    comps, kw = [(10, 3, 20, 8), (8, 2, 6, 4)], dict(pow_bits=4)
    cfg, ocfg = nz.default_config(**kw), O.default_cfg(**kw)
    world = 4
    group = nz.LocalGroup(world)
    out, errors = [None] * world, []

    def run(rank):
        b = comm = None
        try:
            b = nz.HipBackend(0)
            comm = b.local_comm(group, rank)
            out[rank] = (b.prove_machine(comps, cfg, seed=77, ad=b"4r", comm=comm), b.machine_claimed_sums())
        except Exception as e:   # noqa: BLE001
            errors.append((rank, repr(e)))
            if comm is not None:
                comm.abort(comm.user)
        finally:
            if comm is not None:
                b.free_local_comm(comm)
            if b is not None:
                b.close()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    group.close()
    assert not errors, errors
    words, claimed = out[0]
    assert all(np.array_equal(words, o[0]) for o in out)
    assert np.array_equal(words, be.prove_machine(comps, cfg, seed=77, ad=b"4r"))       # the same bytes as on one GPU
    assert nz.verify_machine(comps, cfg, words, claimed, ad=b"4r") is None
    assert M.verify_machine(comps, ocfg, words, claimed, ad=b"4r") is None


def test_verifying_a_2pow20_row_machine_proof_takes_milliseconds(be, nz):
    """The bench's machine at 2^20 rows.  Nothing is asserted about time; the two wall times are printed (DESIGN.md section 8 quotes them)."""
    comps, cfg = [(20, 27, 347, 64)], nz.default_config(pow_bits=10)
    be.prove_machine(comps, cfg, seed=4242)                                                # kernels compiled, buffers cached
    t0 = time.perf_counter()
    words = be.prove_machine(comps, cfg, seed=4242)
    t_prove = time.perf_counter() - t0
    claimed = be.machine_claimed_sums()
    t0 = time.perf_counter()
    verdict = nz.verify_machine(comps, cfg, words, claimed)
    t_verify = time.perf_counter() - t0
    print(f"\n2^20-row machine: prove {t_prove * 1e3:.1f} ms wall, product verifier {t_verify * 1e3:.2f} ms wall, {len(words)} proof words")
    assert verdict is None
    assert nz.verify_machine(comps, cfg, _flip(words), claimed) is not None
    be.trim()


# ---------------------------------------------------------------- 9. nx_commit_root ----------
def _random_columns(be, rng, n_cols, log):
    host = rng.integers(0, P, (n_cols, 1 << log), dtype=np.uint32)
    return host, be.columns_from_host(host)


def _lde_commit_root(be, tw, host_sets, log_blowup):
    """The root the keeping path gives: every set extended whole (nx_lde_batch), all extensions committed by nx_merkle_commit."""
    ext = [be.lde(tw, be.columns_from_host(h), log_blowup) for h in host_sets]
    tree = be.merkle_commit(ext)
    root = tree.root()
    del tree, ext
    return root


@pytest.mark.parametrize("hash_mode", [0, 1])
def test_commit_root_equals_the_keeping_commit(nz, hash_mode):
    be = nz.HipBackend(0)
    be.set_hash_mode(hash_mode)
    rng = np.random.default_rng(5 + hash_mode)
    for log_blowup in (1, 2):
        tw = be.precompute_twiddles(13 + log_blowup - 1)
        for n_cols in (1, 15, 16, 17, 33):
            host, dev = _random_columns(be, rng, n_cols, 13)
            _, ref = be.lde_commit(tw, be.columns_from_host(host), log_blowup)
            assert np.array_equal(be.commit_root(tw, [dev], log_blowup), ref), (hash_mode, log_blowup, n_cols)
        # mixed sizes in commit order: small, large, half the largest size, large again, tiny
        shapes = [(3, 9), (17, 13), (2, 12), (5, 13), (1, 4), (4, 11)]
        hosts = [rng.integers(0, P, (n, 1 << lg), dtype=np.uint32) for n, lg in shapes]
        ref = _lde_commit_root(be, tw, hosts, log_blowup)
        assert np.array_equal(be.commit_root(tw, [be.columns_from_host(h) for h in hosts], log_blowup), ref), (hash_mode, log_blowup, "mixed")
        # one small tree (fewer levels than one reduction launch takes)
        h2 = [rng.integers(0, P, (3, 8), dtype=np.uint32)]
        assert np.array_equal(be.commit_root(tw, [be.columns_from_host(h) for h in h2], log_blowup), _lde_commit_root(be, tw, h2, log_blowup))
    empty = be.merkle_commit([]).root()
    assert np.array_equal(be.commit_root(None, [], 1), empty)
    be.close()


def test_commit_root_is_the_preprocessed_root_inside_a_proof_and_feeds_the_verifier_session(be, nz, oracle):
    comps, kw = [(10, 5, 20, 8), (7, 3, 6, 4)], dict(pow_bits=4)
    cfg = nz.default_config(**kw)
    words = be.prove_machine(comps, cfg, seed=9, ad=b"p")
    h = O.proof_header_words()
    root0 = words[h + 1: h + 9]
    pre = [np.stack(O.synth_tree_columns([c], 0, 9)) for c in comps]                       # the preprocessed columns, per component
    tw = be.precompute_twiddles(10)
    be.set_hash_mode(0)
    assert np.array_equal(be.commit_root(tw, [be.columns_from_host(p) for p in pre], 1), root0)
    v = nz.VerifierSession(cfg)
    v.mix_u64(ord("p"))
    for c in comps:
        v.mix_u64(c[0])
    assert np.array_equal(v.commit_columns(be, tw, [be.columns_from_host(p) for p in pre]), root0)
    ref = nz.VerifierSession(cfg)
    ref.mix_u64(ord("p"))
    for c in comps:
        ref.mix_u64(c[0])
    ref.commit(root0, [c[0] for c in comps for _ in range(c[1])])
    assert np.array_equal(v.digest(), ref.digest())
    v.close(); ref.close()


def _r256(x):
    return (x + 255) & ~255


def test_commit_root_memory_bound_by_the_allocators_own_count(nz):
    """64 columns of 2^18 rows, blowup 2: the bound of include/nexus_hip.h — ring + leaf state + second reduction buffer — holds, and the
    peak lies below nx_lde_commit's by at least the extensions minus the ring."""
    be = nz.HipBackend(0)
    n_cols, log, log_blowup = 64, 18, 1
    M = 1 << (log + log_blowup)
    tw = be.precompute_twiddles(log + log_blowup - 1)
    rng = np.random.default_rng(64)
    host = rng.integers(0, P, (n_cols, 1 << log), dtype=np.uint32)
    ring = 4 * M * 16 * 2
    bound = _r256(ring // 2) * 2 + _r256(32 * M) + _r256(32 * M >> 3)
    dev = be.columns_from_host(host)
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    root = be.commit_root(tw, [dev], log_blowup)
    live1, peak = be.memory()
    print(f"\nnx_commit_root: peak above inputs {peak - live0} B, bound {bound} B")
    assert live1 == live0                                   # nothing kept
    assert peak - live0 <= bound
    del dev
    dev = be.columns_from_host(host)
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    ext, ref = be.lde_commit(tw, dev, log_blowup)           # the caller holds the extension, the call builds the whole tree
    _, peak_keep = be.memory()
    keep_formula = 4 * M * n_cols + 64 * M - 32
    print(f"nx_lde_commit: peak above inputs {peak_keep - live0} B, formula {keep_formula} B")
    assert np.array_equal(root, ref)
    assert abs((peak_keep - live0) - keep_formula) <= 4096
    assert (peak_keep - live0) - (peak - live0) >= 4 * M * n_cols - ring
    assert keep_formula - bound >= 4 * M * n_cols - ring     # the same statement from the two formulas
    del ext, dev
    be.close()


# ---------------------------------------------------------------- 10. the C example ----------
def test_c_example_verifies_its_proof_and_refuses_a_flipped_word(tmp_path):
    lib_dir = os.path.join(ROOT, "nexus-zkvm_amd")
    exe = str(tmp_path / "session_prove")
    subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "session_prove.c"),
                    "-L" + lib_dir, "-lnexus_hip", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].startswith("ok ")
    assert out[1] == "verified: accepted"
    assert out[2].startswith("verified: refused (") and len(out) == 3
