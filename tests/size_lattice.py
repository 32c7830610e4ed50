"""The size lattice of tests/test_size_lattice_cpu.py and tests/test_gpu_size_lattice.py: plain data and small helpers.

Which kernel runs, and how often, is decided by the log sizes of a statement — the largest component and every smaller one that joins
below it (csrc/merkle.hip build_inner_layers / reduce_to_root, csrc/prover.hip FriProver::commit, csrc/pcs.hip, the transform plans).
The lists below sweep that axis: every size alone, every pair of sizes, a few triples.  Column widths are fixed per list: the cache key
of a generated AIR kernel (csrc/prover.hip cached_air_kernel, csrc/air_jit.hip) is the recorded program, its column, register and
constant counts — not the log size —, so a list compiles its kernels once, not once per size.

Configurations are keyword sets of oracle_lib.default_cfg; hip_config turns one into the library's."""

# ---- the ladder: one component, every size ----------------------------------------------------------------------------------------
LADDER = list(range(2, 18))
LADDER_SHAPE = (3, 20, 8)                   # n_pre, n_main, n_inter (two logup columns)
LADDER_CONFIGS = {
    "std": dict(pow_bits=3),
    "lcd2-raw0-alpha-first": dict(pow_bits=3, log_constraint_degree=2, hash_mode=1, fri_alpha_mode=1),
}
SYNTH_SHAPE = (2, 2, 0)                     # nx_prove_synth on the ladder
SYNTH_CONFIG = dict(pow_bits=3)


def ladder_statement(L):
    return [(L,) + LADDER_SHAPE]


def synth_statement(L):
    return [(L,) + SYNTH_SHAPE]


# ---- configuration variants on the low end of the ladder ------------------------------------------------------------------------
VARIANT_LADDER = list(range(2, 13))
VARIANTS = {
    "log-last-1": dict(pow_bits=3, log_last=1),
    "log-last-2": dict(pow_bits=3, log_last=2),
    "log-last-3": dict(pow_bits=3, log_last=3),
    "blowup-2": dict(pow_bits=3, log_blowup=2),
    "queries-20": dict(pow_bits=3, n_queries=20),      # more queries than the domain has points at the low end
}


def proves(L, log_last):
    """The rule of the oracle (oracle/pcs.h "fri: columns not consumed") and of the library (csrc/prover.hip commit_last_layer): a
    statement proves iff its smallest component has log_size >= log_last_layer_degree_bound + 2."""
    return L >= log_last + 2


VARIANT_CASES = [(name, L) for name in VARIANTS for L in VARIANT_LADDER if proves(L, VARIANTS[name].get("log_last", 0))]

# ---- pairs and triples: narrow components ---------------------------------------------------------------------------------------
NARROW_SHAPE = (2, 3, 4)                    # n_pre, n_main, n_inter (one logup column)
NARROW_CONFIG = dict(pow_bits=2)
FULL_PAIRS_UP_TO = 15                       # every (A, B) with 2 <= B < A <= 15; above, a subset of B


def big_pair_subset(A):
    """The smaller sizes paired with A = 16, 17.  In LDE logs (B + 1) they straddle "merkle.top" 7, the subtree launch's 6 .. 14, the
    pair-level launch's 13 and the FRI tail's 11, and sit right below A."""
    return sorted({2, 5, 6, 7, 10, 11, 12, 13, A - 2, A - 1})


PAIRS = ([(A, B) for A in range(3, FULL_PAIRS_UP_TO + 1) for B in range(2, A)]
         + [(A, B) for A in (16, 17) for B in big_pair_subset(A)])
TRIPLES = [(4, 3, 2), (8, 7, 6), (12, 11, 10), (14, 13, 12), (9, 7, 2), (13, 7, 2), (15, 7, 2)]


def narrow_statement(logs):
    return [(L,) + NARROW_SHAPE for L in logs]


def pairs_of(A):
    return [B for (a, B) in PAIRS if a == A]


# one GPU test case per entry, so that a case stays within a few seconds, the oracle's side included: every B of one A up to 13, one
# pair per case above (the oracle proves a 2^15-row pair in 0.3 s, a 2^17-row one in 1.7 s)
PAIR_GROUPS = ([(A, tuple(pairs_of(A))) for A in range(3, 14)]
               + [(A, (B,)) for A in range(14, 18) for B in pairs_of(A)])

# ---- the commit lattice -----------------------------------------------------------------------------------------------------------
COMMIT_BIG_COLS = 17                        # the leaf loop crosses one 16-column block


def commit_small_cols(B):
    return 17 if B & 1 else 1


def commit_shapes(A):
    """The column sets committed with largest size A: A alone, A with every paired B, and the triples led by A — [(log, n_cols), ...]."""
    shapes = [[(A, COMMIT_BIG_COLS)]]
    shapes += [[(A, COMMIT_BIG_COLS), (B, commit_small_cols(B))] for B in pairs_of(A)]
    shapes += [[(A, COMMIT_BIG_COLS)] + [(B, commit_small_cols(B)) for B in t[1:]] for t in TRIPLES if t[0] == A]
    return shapes


# ---- the session ladder -----------------------------------------------------------------------------------------------------------
SESSION_LOGS = [(L,) for L in range(2, 10)] + [(L, L - 1) for L in range(3, 10)]

# ---- refusals -----------------------------------------------------------------------------------------------------------------------
# the grid on which the oracle's rule was established: 396 statements prove, 180 are refused
GRID = dict(L=range(1, 9), log_blowup=(1, 2, 3), log_last=(0, 1, 2, 3), n_queries=(1, 3, 20), log_constraint_degree=(1, 2))
REFUSED = [(L, ll) for ll in GRID["log_last"] for L in GRID["L"] if not proves(L, ll)]
REFUSAL_CONFIGS = {
    "std": dict(pow_bits=2),
    "blowup-2-lcd2-queries-20": dict(pow_bits=2, log_blowup=2, log_constraint_degree=2, n_queries=20),
}
ORACLE_REFUSAL = "fri: columns not consumed"
LIBRARY_REFUSAL = "not consumed"


def hip_config(nz, kw):
    kw = dict(kw)
    if "log_last" in kw:
        kw["log_last_layer_degree_bound"] = kw.pop("log_last")
    return nz.default_config(**kw)
