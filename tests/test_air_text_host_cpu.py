"""The generated kernel text on the host: the CPU twin of tests/test_gpu_saturated.py.

nx_air_compile and nx_logup_program hand hiprtc a text that carries its own copy of field.cuh's arithmetic (AIR_PRELUDE, LOGUP_PRELUDE in
csrc/air_jit.hip) and the generator's own fold schedule (the dot-product peephole's lazy accumulators, the constraint sum).  The text is
header-free C++ apart from two work-item builtins, so tests/native/air_text_host.cpp includes it, gives the builtins a meaning and calls
every kernel once per row — built with the address and undefined-behaviour sanitizers, as a stand-alone program.  Operands are saturated
(every word p-1) or enumerate {0, 1, p-1, p-2}; the expected words come from tests/saturated_programs.py::interp (every operation
reduced at once) and, for fractions, from the oracle.  The rule pinned: at most 4 products between two folds, at every site of the text.
Check kernels (wave votes, LDS) stay with the GPU suite."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import saturated_programs as SP

P = O.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "native", "air_text_host.cpp")
LOG_SIZE, LOG_EVAL = 5, 6


@pytest.fixture(scope="module", autouse=True)
def clangxx():
    """resolved once, before any reference is computed: without the ROCm compiler the whole module is skipped, visibly, at its first test"""
    global CLANGXX
    CLANGXX = _clangxx()
    return CLANGXX


CLANGXX = None


def _clangxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.skip("no clang++ (the ROCm compiler) available")


def _run_text(tmp_path, name, src, logup, header, operand_sets):
    """Writes the text, builds the driver around it with the sanitizers and runs it once per operand set (a list of arrays each);
    every run must report zero mismatches and only canonical words.  Returns the number of kernels in the text."""
    (tmp_path / f"{name}.hip").write_text(src)
    kernels = re.findall(r'extern "C" __attribute__\(\(global\)\)[^\n]*? void (\w+)\(', src)
    assert kernels and kernels[0] == "air_kernel"
    exe = str(tmp_path / name)
    cmd = [CLANGXX, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-attributes",
           "-Wno-ignored-attributes", f'-DGEN_SRC="{tmp_path / (name + ".hip")}"', "-DGEN_KERNELS=" + ",".join(kernels), f"-DGEN_LOGUP={int(logup)}", DRIVER, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    for i, arrays in enumerate(operand_sets):
        path = tmp_path / f"{name}.{i}.bin"
        with open(path, "wb") as f:
            f.write(np.asarray(header, np.uint32).tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a, dtype=np.uint32).tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and f"{header[0]} rows, 0 mismatches, 0 words not below p" in r.stdout, (i, (r.stdout + r.stderr)[-3000:])
    return len(kernels)


def _constraint_case(tmp_path, name, nz, prog, cols, log_size, log_eval, denom_words):
    """SAT alpha powers and start accumulator; one run per word of denom_words (the whole denom_inv table is that word)"""
    n = 1 << log_eval
    cons, _ = SP.interp(prog, cols)
    pw = np.full((prog.n_constraints, 4), P - 1, np.uint32)
    start = np.full((4, n), P - 1, np.uint32)
    ec = np.asarray(prog.econsts, np.uint32).reshape(-1, 4)
    sets = []
    for d in denom_words:
        den = np.full(1 << (log_eval - log_size), d, np.uint32)
        want = SP.accumulate(cons, pw, den, log_size, start)
        assert np.array_equal(want, np.stack(O.eval_constraint_program(prog, list(cols), pw, den, log_size, log_eval, acc4=list(start)))), "the two references disagree"
        sets.append([cols, ec, pw, den, start, want])
    src = nz.air_source(prog, cols.shape[0])
    header = [n, log_size, log_eval, cols.shape[0], len(ec), prog.n_constraints]
    return src, _run_text(tmp_path, name, src, False, header, sets)


def _logup_case(tmp_path, name, nz, prog, cols, log_size):
    want = O.logup_program(prog, list(cols), log_size, prog.n_logup_cols)
    src = nz.logup_program_source(prog, cols.shape[0], prog.n_logup_cols)
    ec = np.asarray(prog.econsts, np.uint32).reshape(-1, 4)
    header = [1 << log_size, log_size, log_size, cols.shape[0], len(ec), prog.n_logup_cols]
    return src, _run_text(tmp_path, name, src, True, header, [[cols, ec] + [c for col in want for c in col]])


def products_between_folds(src):
    """Per 64-bit accumulator of the text (z<reg>_<k> of the peephole, s0..s3 of the constraint sum): the largest number of terms added
    between two acc_fold / acc_final of it (an accumulator starts folded: from 0 or from a canonical register)."""
    pending, worst = {}, {}
    tok = re.compile(r"(\w+) = acc_mad\(\1,|(\w+) = acc_fold\(\2\)|acc_final\((\w+)\)|\b(s[0-3]) \+= |\b(z\d+_\d) = r\d+[,;]")
    for line in src.splitlines():
        if line.startswith("FI ") or line.startswith("//"):
            continue                                  # the prelude's own functions: their sums are fixed, and run on boundary values above
        if 'extern "C"' in line:
            pending = {}
        for m in tok.finditer(line):
            mad, fold, final, plus, init = m.groups()
            if mad or plus:
                k = mad or plus
                pending[k] = pending.get(k, 0) + 1
                worst[k] = max(worst.get(k, 0), pending[k])
            else:
                pending[fold or final or init] = 0
    return worst


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    nexus_zkvm_amd.load_library()
    return nexus_zkvm_amd


def test_dot_chains_of_the_generated_text_on_saturated_operands(tmp_path, nz, oracle):
    """Program A: chains of 1 ... 200 terms, both ADDE operand orders, every word p-1.  The text must fuse them (that is what is tested),
    fold every 4 terms, and still give the reduce-every-step sums."""
    prog = SP.chains_program().program(SP.sat_econsts())
    cols, _ = SP.sat_inputs(prog, 1 << LOG_EVAL)
    src, _ = _constraint_case(tmp_path, "chains", nz, prog, cols, LOG_SIZE, LOG_EVAL, (1, P - 1))
    worst = products_between_folds(src)
    z = {k: v for k, v in worst.items() if k.startswith("z")}
    assert len(z) == 4 * 2 * len(SP.CHAIN_TERMS), "every chain is fused into its own lazy accumulator"
    assert src.count("acc_mad(z") == 4 * 2 * sum(SP.CHAIN_TERMS)
    assert max(worst.values()) == 4, worst             # the 200-term chains reach the period, nothing exceeds it


def test_peephole_guards_of_the_generated_text(tmp_path, nz, oracle):
    """Program B: interleaved chains, materialise-and-restart, a pending accumulator as a factor, the shapes that must stay unfused"""
    prog = SP.guards_program().program(SP.sat_econsts())
    cols, _ = SP.sat_inputs(prog, 1 << LOG_EVAL)
    src, n1 = _constraint_case(tmp_path, "guards", nz, prog, cols, LOG_SIZE, LOG_EVAL, (1, P - 1))
    assert n1 == 1 and max(products_between_folds(src).values()) == 4
    fused = set(re.findall(r"acc_mad\(z(\d+)_0", src))
    assert len(fused) == 6, fused                       # D1, D2, D3, D4, D5 and D9: nothing else may be summed lazily


def test_constraint_runs_of_the_generated_text(tmp_path, nz, oracle):
    """Program C: 9 consecutive CONSTRAINT_B, then CONSTRAINT_B / CONSTRAINT_E alternating for 9 — the emitted sum's own folds"""
    prog = SP.runs_program().program(SP.sat_econsts())
    cols, _ = SP.sat_inputs(prog, 1 << LOG_EVAL)
    src, _ = _constraint_case(tmp_path, "runs", nz, prog, cols, LOG_SIZE, LOG_EVAL, (1, P - 1))
    assert "acc_mad(z" not in src and products_between_folds(src) == {"s0": 4, "s1": 4, "s2": 4, "s3": 4}


def test_segmented_text_of_guards_and_runs(tmp_path, nz, oracle, monkeypatch):
    """Programs B + C under a small segment budget: several kernels, every one with its own accumulators and fold count; the cuts fall
    inside the materialise-and-restart chain and inside the run of CONSTRAINT_B."""
    prog = SP.guards_program(runs=True).program(SP.sat_econsts())
    cols, _ = SP.sat_inputs(prog, 1 << LOG_EVAL)
    monkeypatch.setenv("NX_AIR_SEGMENT", "200")
    src, n = _constraint_case(tmp_path, "guards_seg", nz, prog, cols, LOG_SIZE, LOG_EVAL, (1, P - 1))
    assert n >= 3 and max(products_between_folds(src).values()) == 4
    kernels = src.split('extern "C"')[1:]
    d3 = SP.guards_program(runs=True).marks["D3"]
    assert sum(1 for k in kernels if f"acc_mad(z{d3}_0," in k) >= 2                    # the restarted chain's two roots are in different kernels
    per_kernel = [k.count("acc_mad(s0,") for k in kernels]
    assert sum(per_kernel) == 14 and max(per_kernel) < 9 and sum(1 for c in per_kernel if c) >= 2, per_kernel    # the run of 9 is cut


@pytest.mark.parametrize("name", ["chains", "guards"])
def test_fraction_text_on_saturated_chains(tmp_path, nz, oracle, name):
    """Programs A and B as fraction programs: every chain is the denominator of a FRAC / FRACB (what machine.hip's emit_den writes),
    so the lazy accumulator is materialised by the fraction that reads it; groups of 8 denominators share one inverse."""
    prog = {"chains": SP.chains_program, "guards": SP.guards_program}[name]("frac").program(SP.sat_econsts())
    cols, _ = SP.sat_inputs(prog, 1 << LOG_SIZE)
    src, _ = _logup_case(tmp_path, name + "_frac", nz, prog, cols, LOG_SIZE)
    assert "acc_mad(z" in src and max(products_between_folds(src).values()) == 4


def test_enumerated_products_through_the_prelude_copy(tmp_path, nz, oracle):
    """x * y over all 4^8 combinations of {0, 1, p-1, p-2} in the 8 coordinates, times a saturated alpha power: q_mul of AIR_PRELUDE"""
    prog = SP.mul_program()
    _constraint_case(tmp_path, "mul", nz, prog, SP.edge_enum(8), 15, 16, (P - 1,))


def test_enumerated_fractions_through_the_logup_prelude(tmp_path, nz, oracle):
    """num / den with den over all 4^4 combinations (the zero element among them: it contributes 0, like the oracle's inverse) and
    secure and base-field numerators from the same set: q_norm, q_inv_from, q_frac_add of LOGUP_PRELUDE"""
    cols = SP.frac_columns()
    assert not cols[:4, 0].any() and cols.shape == (9, 1 << 16)
    _logup_case(tmp_path, "frac", nz, SP.frac_program(), cols, 16)
