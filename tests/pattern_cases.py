"""Inputs of the erasure-pattern stage and its contract in plain Python.

The stage turns d_present rows into pattern indices and locator rows
(csrc/ec_kernels.hip: pattern_hash, pattern_insert, pattern_resolve,
pattern_broadcast, error_locator_g, error_locator_w).  This module holds

  * leaders(): the contract of ECCR_AMD_dedup_patterns.  leaders[b] is the
    smallest row whose flags (present[row, :nv] != 0) equal row b's.  The GPU
    tests compare the device's d_pattern with this and with nothing else;
  * a restatement of how the device gets there: the row hash (the sum mod 2^64
    of mix64(i) over the present i < nv, 0 replaced by 1; mix64(i) =
    synth.splitmix64_words(i, 1)[0]), the table size (a power of two >=
    max(64, 2 batch)) and a sequential open-addressing simulator of the table.
    The restatement only chooses inputs and asserts their properties (rows out
    of their home slot, a probe that wraps from the last slot to slot 0), and
    runs three deliberately wrong tables (WRONG_MODELS) to show that the named
    inputs tell them from the contract;
  * the named dedup inputs (NAMES, case()) and the pattern sets of the locator
    tests (degenerate_rows(), count_patterns(), small_batch(), large_batches()).

Every input varies what the contract says must not matter: present bytes are
drawn from {1, 2, 0x80, 0xFF} and the bytes at positions >= nv are noise.

A 64-bit hash collision between two different patterns cannot be constructed
(the hash is a subset sum of 64-bit mixes: finding one is a birthday search over
2^32 patterns with no structure to exploit), so the `differ` branch of
pattern_resolve, which lets a row whose hash-leader has other flags lead
itself, stays uncovered by every input here."""
from __future__ import annotations

import numpy as np

import synth

M64 = (1 << 64) - 1
PRESENT_BYTES = np.array([1, 2, 0x80, 0xFF], np.uint8)


# ------------------------------------------------------------------ the contract
def flag_rows(present, nv):
    return np.asarray(present)[:, :nv] != 0


def leaders(present, nv):
    """leaders[b] = the smallest row whose flags below nv equal row b's"""
    first, out = {}, []
    for b, row in enumerate(flag_rows(present, nv)):
        out.append(first.setdefault(row.tobytes(), b))
    return out


# ------------------------------------------------------------------ the restatement
_MIX = {}


def mix64(i):
    return int(synth.splitmix64_words(i, 1)[0])


def mix_table(nv):
    if nv not in _MIX:
        _MIX[nv] = np.array([mix64(i) for i in range(nv)], np.uint64)
    return _MIX[nv]


def row_hashes(present, nv):
    """per row: the sum mod 2^64 of mix64(i) over the present i < nv, 0 -> 1"""
    with np.errstate(over="ignore"):
        h = (flag_rows(present, nv).astype(np.uint64) * mix_table(nv)[None, :]).sum(axis=1, dtype=np.uint64)
    return [int(x) or 1 for x in h]


def table_cap(batch):
    c = 64
    while c < 2 * batch:
        c *= 2
    return c


class Table:
    """The table after inserting every row in row order, and what the probing
    did: home[b], displaced (rows that did not land in their home slot),
    longest (probe steps of the worst row), wraps (steps from slot cap - 1 to
    slot 0).  model: None, or one of WRONG_MODELS."""

    def __init__(self, hashes, cap, model=None):
        assert cap & (cap - 1) == 0
        self.cap, self.model, self.hashes = cap, model, list(hashes)
        self.keys, self.vals = [0] * cap, [None] * cap
        self.home = [h % cap for h in self.hashes]
        self.displaced = self.longest = self.wraps = 0
        for b, h in enumerate(self.hashes):
            if model == "drop_rows_from_256" and b >= 256:
                continue  # as if only the first block of pattern_insert ran
            slot, steps = self._probe(h, empty_ends=True, count=True)
            self.longest = max(self.longest, steps)
            self.displaced += steps > 0
            if slot is None:
                continue
            self.keys[slot] = h
            old = self.vals[slot]
            self.vals[slot] = b if old is None or model == "last_writer" else min(old, b)

    def _probe(self, h, empty_ends, count=False):
        """-> (slot holding h, or, inserting, the first empty one; None: not found), steps"""
        slot = h % self.cap
        for steps in range(self.cap):
            if self.keys[slot] == h or (empty_ends and self.keys[slot] == 0):
                return slot, steps
            if slot == self.cap - 1:
                if self.model == "stop_at_last_slot":
                    return None, steps
                self.wraps += count
            slot = (slot + 1) % self.cap
        return None, self.cap

    def resolve(self, present, nv):
        """the leader array this table gives (pattern_resolve in plain Python)"""
        fl = flag_rows(present, nv)
        out = []
        for b, h in enumerate(self.hashes):
            slot, _ = self._probe(h, empty_ends=False)
            l = b if slot is None else self.vals[slot]
            out.append(l if l != b and (fl[l] == fl[b]).all() else b)
        return out


WRONG_MODELS = ("stop_at_last_slot",     # the probe ends at slot cap - 1: the row leads itself
                "last_writer",           # a slot keeps the last row written, not the minimum
                "drop_rows_from_256")    # rows >= 256 are never inserted


def simulate(nv, present, model=None):
    present = np.asarray(present)
    return Table(row_hashes(present, nv), table_cap(len(present)), model)


# ------------------------------------------------------------------ building rows
def words(seed, count):
    return synth.splitmix64_words(0x9A77E2 + seed, count)


def dress(flags, nv, seed):
    """flags [B][n] (bool) -> present bytes: a set flag becomes one of
    PRESENT_BYTES, positions >= nv become noise (0 or one of PRESENT_BYTES)"""
    flags = np.asarray(flags, bool)
    B, n = flags.shape
    w = words(seed, B * n).reshape(B, n)
    val = PRESENT_BYTES[(w % np.uint64(4)).astype(np.int64)]
    out = np.where(flags, val, 0).astype(np.uint8)
    out[:, nv:] = np.where((w[:, nv:] >> np.uint64(8)) % np.uint64(2) == 1, val[:, nv:], 0)
    return out


def mask_flags(masks, nv, n):
    """integers (bit i = position i present) -> flags [B][n]"""
    m = np.asarray(masks, np.uint64)[:, None]
    fl = np.zeros((len(masks), n), bool)
    fl[:, :nv] = (m >> np.arange(nv, dtype=np.uint64)[None, :]) & np.uint64(1) == 1
    return fl


def distinct_masks(seed, count, bits=20):
    """`count` different non-zero masks of `bits` bits, in drawing order"""
    seen, out = set(), []
    for w in words(seed, 4 * count + 64):
        m = int(w) & ((1 << bits) - 1)
        if m and m not in seen:
            seen.add(m)
            out.append(m)
            if len(out) == count:
                return out
    raise AssertionError("not enough distinct masks")


def mask_hash(m, nv=20):
    t = mix_table(nv)
    return (sum(int(t[i]) for i in range(nv) if m >> i & 1) & M64) or 1


def random_flags(seed, rows, nv, n):
    fl = np.zeros((rows, n), bool)
    fl[:, :nv] = (words(seed, rows * nv).reshape(rows, nv) >> np.uint64(17)) % np.uint64(2) == 1
    return fl


# ------------------------------------------------------------------ the named dedup inputs
NV_SMALL, N_SMALL = 20, 32
DISTINCT_SEED = 11
WRAP_HOME = 60  # cap = 64: the "high" home slots are 60 .. 63


def _small(masks, seed):
    return NV_SMALL, dress(mask_flags(masks, NV_SMALL, N_SMALL), NV_SMALL, seed)


def _one():
    return _small(distinct_masks(1, 1), 1)


def _block_edge():
    m = distinct_masks(2, 255)
    return _small(m + [m[3], m[0]], 2)


def _distinct():
    return _small(distinct_masks(DISTINCT_SEED, 1000), 3)


def few_late_deal():
    """pattern number of each of the 3000 rows: six patterns dealt at random over
    the whole batch, the seventh over the rows from 2900 on only"""
    w = words(4, 3000)
    deal = (w % np.uint64(6)).astype(np.int64)
    late = np.arange(3000) >= 2900
    deal[late] = (w[late] % np.uint64(7)).astype(np.int64)
    return deal


def _few_late():
    m = distinct_masks(5, 7)
    return _small([m[j] for j in few_late_deal()], 5)


def _single():
    return _small(distinct_masks(6, 1) * 3000, 6)


def wrap_masks():
    """(8 patterns with a home slot >= WRAP_HOME, 4 with the home slots 0 .. 3, 4 others)"""
    high, low, other = [], {}, []
    for m in distinct_masks(7, 6000):
        home = mask_hash(m) % 64
        if home >= WRAP_HOME and len(high) < 8:
            high.append(m)
        elif home < 4 and home not in low:
            low[home] = m
        elif 4 <= home < WRAP_HOME and len(other) < 4:
            other.append(m)
    assert len(high) == 8 and len(low) == 4 and len(other) == 4
    return high, [low[s] for s in range(4)], other


def _wrap():
    high, low, other = wrap_masks()
    return _small(high + low + high + other, 7)


def edge_rows(nv, n, batch, edges, seed):
    """The construction of `wide` and `huge`.  Row 0 is a base row; rows
    1 .. len(edges) differ from it at one position of `edges` each (distinct
    patterns); the next row differs only at positions >= nv and the one after
    it only in the values of its present bytes (both: the base's pattern); two
    rows without a flag below nv (one pattern); a row that differs from the
    base at position nv alone (the base's pattern); random rows for the rest.
    -> present, {"same": rows with the base's pattern, "empty": the two rows}"""
    E = len(edges)
    fl = random_flags(seed, batch, nv, n)
    fl[0, list(edges)] = True
    for j, pos in enumerate(edges):
        fl[1 + j] = fl[0]
        fl[1 + j, pos] = False
    fl[E + 1] = fl[E + 2] = fl[0]
    fl[E + 3, :] = fl[E + 4, :] = False
    pr = dress(fl, nv, seed)
    pr[0] = np.where(fl[0], 1, 0)
    pr[0, nv:] = 0
    for j in range(E):  # the one difference is the edge, below nv and above
        pr[1 + j] = pr[0]
        pr[1 + j, edges[j]] = 0
    pr[E + 1] = pr[0]
    pr[E + 1, nv:] = 0xFF  # differs at every position >= nv
    pr[E + 2] = np.where(fl[0], PRESENT_BYTES[1 + np.arange(n) % 3], 0)  # 2, 0x80, 0xFF
    pr[E + 2, nv:] = 0
    pr[E + 3] = 0
    pr[E + 4] = 0
    pr[E + 4, nv:] = 0xFF
    pr[E + 5] = pr[0]
    pr[E + 5, nv] = 0x80  # differs at position nv alone
    return pr, {"same": [0, E + 1, E + 2, E + 5], "empty": [E + 3, E + 4], "edges": list(range(1, E + 1)),
                "random_from": E + 6}


# `huge`: single-position rows at 0, 4095, 4096 (one more than 0, 4095, 4999: both
# sides of the 4096 boundary) and 4999, distinct patterns; position 5000, the
# first one >= nv, has a row that differs from the base there alone and one that
# differs at every position >= nv, both the base's pattern.  `wide` likewise.
WIDE = dict(nv=1000, n=1024, batch=300, edges=(0, 255, 256, 999), seed=8)
HUGE = dict(nv=5000, n=8192, batch=64, edges=(0, 4095, 4096, 4999), seed=9)


def _wide():
    return WIDE["nv"], edge_rows(**WIDE)[0]


def _huge():
    return HUGE["nv"], edge_rows(**HUGE)[0]


_BUILD = dict(one=_one, block_edge=_block_edge, distinct=_distinct, few_late=_few_late, single=_single,
              wrap=_wrap, wide=_wide, huge=_huge)
NAMES = tuple(_BUILD)
_CASES = {}


def case(name):
    """(nv, present [batch][n] uint8, read-only) of a named dedup input"""
    if name not in _CASES:
        nv, pr = _BUILD[name]()
        pr.setflags(write=False)
        _CASES[name] = (nv, pr)
    return _CASES[name]


# ------------------------------------------------------------------ locator pattern sets
DEGENERATE = ("none_erased", "none_present", "one_present", "one_erased")


def degenerate_rows(nv, n, seed=0):
    """flags [4][n] in DEGENERATE order: nothing erased below nv, nothing
    present, exactly one present, exactly one erased (below nv)"""
    fl = np.zeros((4, n), bool)
    fl[0, :nv] = True
    fl[2, int(words(seed + nv, 2)[0] % np.uint64(nv))] = True
    fl[3, :nv] = True
    fl[3, int(words(seed + nv, 2)[1] % np.uint64(nv))] = False
    return fl


def count_flags(seed, nv, n, count):
    return synth.present_masks([0xC0FFEE + seed], nv, count, n)[0] != 0


def count_patterns(nv, n, k, thr, seed=0):
    """flags [4][n]: four distinct patterns with k, threshold, threshold and nv
    positions present"""
    fl = np.stack([count_flags(seed + 31 * nv + j, nv, n, c) for j, c in enumerate((k, thr, thr, nv))])
    assert len({r.tobytes() for r in fl}) == 4
    return fl


LEADER_DEAL = (0, 1, 0, 2, 1, 3, 0, 2, 3, 1, 0)  # pattern of each of the 11 rows


def late_leaders(deal):
    """a valid d_pattern in which every follower points to a LATER row: each
    pattern is led by its last row"""
    last = {p: b for b, p in enumerate(deal)}
    return [last[p] for p in deal]


def small_batch(nv, n, batch=300, pool=40, seed=0):
    """flags [batch][n]: the four degenerate rows and random patterns, at most
    `pool` distinct ones in all, dealt at random; every degenerate row occurs"""
    pats = np.concatenate([degenerate_rows(nv, n, seed), random_flags(100 + seed + nv, pool - 4, nv, n)])
    deal = (words(200 + seed + nv, batch) % np.uint64(pool)).astype(np.int64)
    deal[[17, 3, 250, 99]] = [0, 1, 2, 3]
    return pats[deal]


LARGE_DEAL = (0, 1, 2, 0, 3, 1, 3, 2, 0)  # 9 rows over 4 patterns: leaders 0, 1, 2, 4


def large_batches(nv, n, k, thr, seed=0):
    """two batches of 9 rows over 4 distinct patterns each: the four patterns of
    count_patterns(), and the four degenerate rows"""
    deal = list(LARGE_DEAL)
    return count_patterns(nv, n, k, thr, seed)[deal], degenerate_rows(nv, n, seed)[deal]
