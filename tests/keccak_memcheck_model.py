"""The judge of nx_trace_keccak_memory_check: the 2001 main columns and is_last of the reference's PermutationMemoryCheck component
(prover/src/extensions/keccak/memory_check/trace.rs:32-123) built row by row from plain Python integers:
  0 .. 199      input-state bytes, lane l byte b at 8 l + b
  200 .. 399    output-state bytes, keccak-f[1600] of the input (tests/keccak_round_model.py, pinned to hashlib)
  400 .. 799    address limbs: for i in 0..200 the low 16 bits of addr + i, then the high 16
  800 .. 1199   previous-timestamp limbs of ts[i]
  1200 .. 1599  next-timestamp limbs of ts[i] + 1
  1600 .. 1799  address carries, ((addr + i) & 0xFFFF) == 0xFFFF
  1800 .. 1999  timestamp carries, (ts[i] & 0xFFFF) == 0xFFFF
  2000          is_padding
addr + i and ts + 1 modulo 2^32.  Natural row r is instance r; a padding row is 0 everywhere except is_padding."""
import functools

import numpy as np

import keccak_round_model as R

P = R.P
STATE = 200
MAIN_COLS, PRE_COLS = 2001, 1
IN, OUT, ADDR, PREV_TS, NEXT_TS, ADDR_CARRY, TS_CARRY, IS_PADDING = 0, 200, 400, 800, 1200, 1600, 1800, 2000
RELATION_ENTRIES = 2 + 2 * STATE                 # the two 200-wide state entries, two memory entries per byte
LOGUP_COLS = RELATION_ENTRIES // 2               # finalize_logup_in_pairs
PLAIN_CONSTRAINTS = 1 + 2 * (STATE // 2) + 2 * STATE      # is_padding boolean, the first 100 address pairs, every timestamp
assert (LOGUP_COLS, PLAIN_CONSTRAINTS) == (201, 601)
MASK32 = (1 << 32) - 1


def keccak_f(states):
    states = np.asarray(states, np.uint64).reshape(-1, 25)
    return R.keccak_f(states) if len(states) else np.zeros((0, 25), np.uint64)


def _bytes(lanes):
    return [(int(lane) >> (8 * b)) & 255 for lane in lanes for b in range(8)]


def _limbs(words):
    return [x for w in words for x in (w & 0xFFFF, w >> 16)]


def fill(states, addresses, timestamps, log_size, natural=False):
    """What nx_trace_keccak_memory_check writes: {"main": (2001, 2^log_size) uint32, "pre": (1, 2^log_size), "out": (n_instances, 25)
    uint64}; columns in storage order unless natural."""
    states = np.asarray(states, np.uint64).reshape(-1, 25)
    n_inst, n = len(states), 1 << log_size
    assert n_inst <= n and len(addresses) == n_inst and len(timestamps) == n_inst
    out = keccak_f(states)
    rows = []
    for r in range(n):
        if r >= n_inst:
            rows.append([0] * IS_PADDING + [1])
            continue
        ts = [int(t) for t in timestamps[r]]
        assert len(ts) == STATE
        a = [(int(addresses[r]) + i) & MASK32 for i in range(STATE)]
        rows.append(_bytes(states[r]) + _bytes(out[r]) + _limbs(a) + _limbs(ts) + _limbs([(t + 1) & MASK32 for t in ts])
                    + [int(w & 0xFFFF == 0xFFFF) for w in a] + [int(t & 0xFFFF == 0xFFFF) for t in ts] + [0])
    main = np.array(rows, np.uint32).T
    pre = np.array([[int(r == n - 1) for r in range(n)]], np.uint32)
    assert main.shape == (MAIN_COLS, n)
    if not natural:
        main, pre = R.to_storage(main, log_size), R.to_storage(pre, log_size)
    return {"main": main, "pre": pre, "out": out}


# ---- the shapes of the CPU and GPU suites: (log_size, n_instances, addresses, timestamps).  addresses: one per instance.  timestamps:
# one entry per instance: an integer (every byte has it), "rand" (seeded random words, distinct per byte) or ("rand", byte, value)
# (random, but that byte's is value).
ADDRESSES = (0, 0xFFFE, 0xFF38, 0x0001FFFF, 0xFFFFFF38)      # 0xFF38 + 199 = 0xFFFF: the last carry is flagged with no successor;
#                                                            # 0xFFFFFF38 is the largest address that does not wrap
TIMESTAMPS = ("rand", 0, 0xFFFE, 0xFFFF, 0xFFFFFFFE)
SHAPES = [
    (1, 0, (), ()),
    (1, 1, (0,), (0,)),
    (1, 2, (0xFF38, 0x0001FFFF), (0xFFFF, "rand")),                                           # no padding
    (2, 3, (0xFFFFFF38, 0, 0xFFFE), (0xFFFFFFFE, "rand", 0xFFFE)),
    (4, 15, (0xFFFE,) * 15, (0xFFFE,) * 15),                                                  # the reference's prove_keccak input: a carry at byte 1
    (4, 16, tuple(0xFFFFFFFF if r == 5 else ADDRESSES[r % 5] for r in range(16)), tuple(TIMESTAMPS[r % 5] for r in range(16))),      # full; one address wraps
    (9, 300, tuple(ADDRESSES[r % 5] for r in range(300)), tuple(TIMESTAMPS[(r + 2) % 5] for r in range(299)) + (("rand", 199, 0xFFFFFFFF),)),
    # more than one block whether a block is 64 or 256 threads, padding begins inside one (300 = 4 * 64 + 44 = 256 + 44), positions and rows differ by the bit reversal; one timestamp wraps
]
# the shapes with a value that wraps: shape index -> (ordinal of the one plain constraint that fails, its natural row).
# Address 0xFFFFFFFF: addr + 1 = 0 has the high limb 0, not 0xFFFF + carry: the high-limb constraint of the first address pair, ordinal
# 1 + 2 * 0 + 1.  Timestamp 0xFFFFFFFF at byte 199: the high-limb constraint of that byte, ordinal 1 + 200 + 2 * 199 + 1.
WRAPPING = {5: (2, 5), 6: (600, 299)}


def shape_id(shape):
    return "%d-%d" % shape[:2]


def test_states(n_instances, seed=0):
    """random lanes with an all-zero state, an all-ones state and a SHA3-256 padded block among them where there is room"""
    s = R.test_states(n_instances, seed=seed)
    if n_instances > 3:
        s[2] = R.sha3_256_block(b"memory check")
    return s


@functools.lru_cache(maxsize=None)
def _inputs(k):
    log_size, n_inst, addresses, specs = SHAPES[k]
    assert len(addresses) == n_inst and len(specs) == n_inst
    rng = np.random.default_rng(6900 + k)
    ts = np.zeros((n_inst, STATE), np.uint32)
    for r, spec in enumerate(specs):
        if isinstance(spec, int):
            ts[r] = spec
            continue
        ts[r] = rng.integers(0, MASK32, STATE, dtype=np.uint32)                       # below 2^32 - 1: none wraps
        assert len(set(ts[r].tolist())) == STATE                                      # distinct per byte
        if spec != "rand":
            ts[r, spec[1]] = spec[2]
    states = test_states(n_inst, seed=k)
    if n_inst == 2:
        states[0], states[1] = np.uint64(MASK32 << 32 | MASK32), R.sha3_256_block(b"abc")
    return states, np.array(addresses, np.uint32), ts


def inputs(k):
    """-> (states (n, 25) uint64, addresses (n,) uint32, timestamps (n, 200) uint32) of SHAPES[k]; computed once, do not write to them"""
    return _inputs(k)


@functools.lru_cache(maxsize=None)
def want(k):
    """fill() of SHAPES[k] in storage order; computed once, do not write to it"""
    return fill(*inputs(k), SHAPES[k][0])
