"""The judge of nx_trace_keccak_round: an independent numpy restatement of the KeccakRound trace builder — column order, padding,
the remainder states — working on BYTES the way the trace does (a rotation is built from the low / high byte columns and only then
compared with the 64-bit rotation).  The round constants come from the LFSR of FIPS 202 algorithm 5 and the rotation offsets from the
(t + 1)(t + 2) / 2 walk of algorithm 2, not from a table; the module asserts on import that the column and lookup-site counts are the
component's and that 16 rounds from 0 followed by 8 rounds from 16 on the padded empty message give hashlib.sha3_256(b"")."""
import hashlib

import numpy as np

P = (1 << 31) - 1
MAIN_COLS, PRE_COLS = 1705, 9
N_XOR, N_NOT_AND, N_ROT = 76, 25, 29
RELATION_ENTRIES = 8 * (N_XOR + N_NOT_AND + N_ROT) + 2          # one per byte of every site, and the two 200-wide state entries
LOGUP_COLS = RELATION_ENTRIES // 2                              # finalize_logup_in_pairs


def _rc_bit(t):
    r = 1
    for _ in range(t % 255):
        r = ((r << 1) ^ ((r >> 7) * 0x71)) & 0xFF
    return r & 1


RC = [sum(_rc_bit(j + 7 * ir) << ((1 << j) - 1) for j in range(7)) for ir in range(24)]


def _rotations():
    rot, x, y = [0] * 25, 1, 0
    for t in range(24):
        rot[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


ROT = _rotations()


def _bytes(lane):
    """(n,) uint64 -> (n, 8) bytes as uint32, low byte first"""
    return np.ascontiguousarray(lane, dtype="<u8").view(np.uint8).reshape(-1, 8).astype(np.uint32)


def _lane(b):
    return np.ascontiguousarray(b.astype(np.uint8)).view("<u8").reshape(-1)


class _Builder:
    """lanes in allocation order; every lane is an (n, 8) byte array"""

    def __init__(self):
        self.lanes, self.sites = [], {"xor": [], "not_and": [], "rot": []}

    def alloc(self, b):
        self.lanes.append(b)
        return len(self.lanes) - 1

    def xor(self, a, b):
        self.sites["xor"].append((a, b, len(self.lanes)))
        return self.alloc(self.lanes[a] ^ self.lanes[b])

    def xor_rc(self, a, rc_bytes):
        self.sites["xor"].append((a, "rc", len(self.lanes)))
        return self.alloc(self.lanes[a] ^ rc_bytes)

    def not_and(self, a, b):
        self.sites["not_and"].append((a, b, len(self.lanes)))
        return self.alloc((self.lanes[a] ^ 255) & self.lanes[b])

    def rotate(self, a, r):
        if r == 0:
            return a
        bits, q, v = r % 8, r // 8, self.lanes[a]
        low, high = (v << bits) & 255, v >> (8 - bits)
        out = np.stack([low[:, (i - q) & 7] + high[:, (i - q + 7) & 7] for i in range(8)], axis=1)
        x = _lane(v)
        assert np.array_equal(_lane(out), (x << np.uint64(r)) | (x >> np.uint64(64 - r))) and int(out.max(initial=0)) < 256
        lo = self.alloc(low)
        hi = self.alloc(high)
        self.sites["rot"].append((a, bits, hi, lo))
        return self.alloc(out)


def trace_rows(inputs, rc):
    """inputs: (n, 25) uint64 round inputs, lane (x, y) at x + 5 y; rc: (n,) uint64.  -> (the builder, the 25 output lane indices)"""
    b = _Builder()
    a = [b.alloc(_bytes(inputs[:, k])) for k in range(25)]
    c = []
    for x in range(5):
        v = a[x]
        for i in range(1, 5):
            v = b.xor(v, a[x + 5 * i])
        c.append(v)
    d = []
    for x in range(5):
        d.append(b.xor(c[(x + 4) % 5], b.rotate(c[(x + 1) % 5], 1)))
    for x in range(5):
        for y in range(5):
            a[x + 5 * y] = b.xor(a[x + 5 * y], d[x])
    bb = [None] * 25
    for x in range(5):
        for y in range(5):
            bb[y + 5 * ((2 * x + 3 * y) % 5)] = b.rotate(a[x + 5 * y], ROT[x + 5 * y])
    for x in range(5):
        for y in range(5):
            a[x + 5 * y] = b.xor(bb[x + 5 * y], b.not_and(bb[(x + 1) % 5 + 5 * y], bb[(x + 2) % 5 + 5 * y]))
    a[0] = b.xor_rc(a[0], _bytes(rc))
    assert len(b.lanes) == 213 and [len(b.sites[k]) for k in ("xor", "not_and", "rot")] == [N_XOR, N_NOT_AND, N_ROT]
    assert 8 * len(b.lanes) + 1 == MAIN_COLS and RELATION_ENTRIES == 1042 and LOGUP_COLS == 521
    return b, a


def pos_of_coset_row(c, log):
    c = np.asarray(c, np.uint64)
    n = 1 << log
    d = np.where(c & np.uint64(1), np.uint64(n - 1) - (c >> np.uint64(1)), c >> np.uint64(1))
    out = np.zeros_like(d)
    for k in range(log):
        out |= ((d >> np.uint64(k)) & np.uint64(1)) << np.uint64(log - 1 - k)
    return out.astype(np.int64)


def to_storage(nat, log):
    """natural-row-order columns (..., 2^log) -> bit-reversed circle-domain order"""
    nat = np.asarray(nat)
    out = np.empty_like(nat)
    out[..., pos_of_coset_row(np.arange(1 << log), log)] = nat
    return out


def fill(states, first_round, log_rounds, log_size, natural=False):
    """What nx_trace_keccak_round writes: {"main": (1705, 2^log_size) uint32, "pre": (9, 2^log_size), "out": (n_instances, 25) uint64,
    "sites": the builder's lookup sites as lane numbers, "outputs": the 25 output lanes}; columns in storage order unless natural."""
    states = np.asarray(states, np.uint64).reshape(-1, 25)
    n_inst, rounds, n = len(states), 1 << log_rounds, 1 << log_size
    assert first_round + rounds <= 24 and n_inst * rounds <= n
    inputs, s = np.zeros((n, 25), np.uint64), states.copy()
    for i in range(rounds):                                      # row i of every instance: its state after i rounds
        inputs[np.arange(n_inst) * rounds + i] = s
        if n_inst:
            b, outs = trace_rows(s, np.full(n_inst, RC[first_round + i], np.uint64))
            s = np.stack([_lane(b.lanes[k]) for k in outs], axis=1)
    rc = np.array([RC[first_round + r % rounds] for r in range(n)], np.uint64)
    b, outs = trace_rows(inputs, rc)
    is_padding = (np.arange(n) >= n_inst * rounds).astype(np.uint32)
    main = np.concatenate([np.concatenate([l.T for l in b.lanes]), is_padding[None, :]]).astype(np.uint32)
    is_last = (np.arange(n) == n - 1).astype(np.uint32)
    pre = np.concatenate([_bytes(rc).T, is_last[None, :]]).astype(np.uint32)
    assert main.shape == (MAIN_COLS, n) and pre.shape == (PRE_COLS, n)
    if not natural:
        main, pre = to_storage(main, log_size), to_storage(pre, log_size)
    return {"main": main, "pre": pre, "out": s, "sites": b.sites, "outputs": outs}


def keccak_f(states):
    """keccak-f[1600] of (n, 25) lanes as the two components chain it"""
    return fill(fill(states, 0, 4, max(1, 4 + int(max(1, len(states)) - 1).bit_length()))["out"], 16, 3, max(1, 3 + int(max(1, len(states)) - 1).bit_length()))["out"]


def sha3_256_block(msg):
    """the padded one-block state of a message shorter than the rate (136 bytes)"""
    assert len(msg) < 136
    blk = bytearray(200)
    blk[:len(msg)] = msg
    blk[len(msg)] ^= 0x06
    blk[135] ^= 0x80
    return np.frombuffer(bytes(blk), "<u8").astype(np.uint64)


def digest(state):
    return np.asarray(state, "<u8").tobytes()[:32]


assert digest(keccak_f(sha3_256_block(b"")[None, :])[0]) == hashlib.sha3_256(b"").digest()


# the shapes of the CPU and GPU suites, (n_instances, first_round, log_rounds, log_size): no padding; one padding instance; all padding;
# the second component; one round per row with a padding tail; several workgroups with the real / padding boundary inside a wave; full
SHAPES = [(1, 0, 4, 4), (3, 0, 4, 6), (0, 0, 4, 4), (5, 16, 3, 6), (24, 23, 0, 5), (17, 0, 4, 9), (32, 0, 4, 9)]


def test_states(n_instances, seed=0):
    """random lanes, with one all-zero and one all-ones state among them where there is room"""
    s = np.random.default_rng(1000 + seed).integers(0, 1 << 64, size=(n_instances, 25), dtype=np.uint64)
    if n_instances > 1:
        s[1] = 0
    if n_instances > 2:
        s[n_instances - 1] = np.uint64((1 << 64) - 1)
    return s
