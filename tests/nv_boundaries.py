"""The n_validators at which a kernel can change its path, computed from
ECCR_AMD_code_params (test_nv_boundaries.py runs every one of them).

The kernels branch on n_validators by hand: the coset count ceil(nv / k), the
last, partly filled coset, the quarters and halves of 1024 rows of
reconstruct_n4096, the `row < nv` masks of every gather and store.  All of
those sit at a multiple of k or of 1024, so for every class [lo, hi] of equal
(n, k) the table holds, clipped to the class,

  * lo and hi;
  * m - 1, m, m + 1 for every multiple m of k with k < m <= n;
  * the same three values for every multiple of 1024 below n;

every n_validators of 2 .. 45 (the per-call tiny and the generic kernels),
above 4096, where only the generic kernels run, the class edges up to 8193,
and, as controls away from every boundary, the n_validators of the two
hand-written lists of tests/test_gpu_parity.py (read from their marks).

Erasure patterns P0 - P2 of one n_validators (`present`), the two buffer
layouts of the uniform device batch and the kernel each class must name in
them, as literals (CLASSES)."""
from collections import namedtuple

import numpy as np

import ecc_amd as E
import synth

LO, HI = 2, 8193
TINY_HI = 45  # every n_validators up to here
FAST_HI = 4096  # the last n_validators with a kernel of its own

Class = namedtuple("Class", "lo hi n k")


def classes(lo=LO, hi=HI):
    """[lo, hi] cut into runs of equal (n, k), in order"""
    out = []
    for nv in range(lo, hi + 1):
        n, k, _ = E.code_params(nv)
        if out and (out[-1].n, out[-1].k) == (n, k):
            out[-1] = out[-1]._replace(hi=nv)
        else:
            out.append(Class(nv, nv, n, k))
    return out


def boundaries(c):
    """the values of one class between TINY_HI + 1 and FAST_HI"""
    marks = [c.lo, c.hi]
    for m in list(range(2 * c.k, c.n + 1, c.k)) + list(range(1024, c.n, 1024)):
        marks += [m - 1, m, m + 1]
    return sorted({v for v in marks if c.lo <= v <= c.hi})


def hand_listed():
    """the n_validators test_encode_kw_vs_oracle / test_encode_k512w_vs_oracle are parametrised with"""
    import test_gpu_parity as T
    out = set()
    for fn in (T.test_encode_kw_vs_oracle, T.test_encode_k512w_vs_oracle):
        (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert mark.args[0].split(",")[0] == "nv"
        out |= {int(row[0]) for row in mark.args[1]}
    return sorted(out)


_TABLE = None


def table():
    """every n_validators of the suite, ascending"""
    global _TABLE
    if _TABLE is None:
        vals = set(range(LO, TINY_HI + 1))
        for c in classes():
            if c.hi <= TINY_HI:
                continue
            if c.lo > FAST_HI:
                vals |= {c.lo, c.hi}  # hi of the last class is HI, one past the n = 8192 edge
            else:
                assert TINY_HI < c.lo and c.hi <= FAST_HI, c  # no class straddles either limit
                vals |= set(boundaries(c))
        vals |= set(hand_listed())
        _TABLE = sorted(vals)
    return _TABLE


def is_full_coset(nv):
    """n_validators is a multiple of k: the last coset is whole"""
    _, k, _ = E.code_params(nv)
    return nv % k == 0


# ------------------------------------------------------------------ kernel names
# What the queries must name for a class, as literals: the aligned layout (64-B
# pitches), and the narrow one, whose shard pitch is a multiple of 8 and not of
# 16: every fast encode keeps it (8-B row-by-row stores), the n = 1024
# reconstruct falls to its packed form and every other reconstruct to the
# generic kernel (16-B row loads).
#
# k = 256 dispatches its encode on a 128-piece tile: COLS_K256 columns reach the
# fast kernel, COLS columns (97 pieces) run packed in both layouts.  n = 1024
# has a third reconstruct, the 8-wave reconstruct_n1024 of 32 .. 47 columns:
# COLS_N1024.
Names = namedtuple("Names", "enc rec enc_narrow rec_narrow")
G, RG, P = "encode_g", "reconstruct_g", "encode_k256_packed"
CLASSES = {  # (n, k) -> names
    (1024, 256): Names("encode_k256w", "reconstruct_n1024x", "encode_k256w", "reconstruct_n1024_packed"),
    (2048, 256): Names("encode_kw", "reconstruct_n4096", "encode_kw", RG),
    (2048, 512): Names("encode_k512w", "reconstruct_n4096", "encode_k512w", RG),
    (4096, 512): Names("encode_k512w", "reconstruct_n4096", "encode_k512w", RG),
    (4096, 1024): Names("encode_k1024", "reconstruct_n4096", "encode_k1024", RG),
}
for _n, _k in ((64, 16), (128, 16), (128, 32), (256, 32), (256, 64), (512, 64), (512, 128), (1024, 128)):
    CLASSES[(_n, _k)] = Names("encode_kw", "reconstruct_gen", "encode_kw", RG)
GENERIC = Names(G, RG, G, RG)  # n_validators up to 45 and above 4096

COLS = 97  # one 64-column tile + 33 columns, three 32-column tiles + 1
COLS_K256 = 129  # two 64-piece tiles + 1 piece: above the 128 pieces encode_k256w / encode_kw<256> start at
COLS_N1024 = 40  # one 32-column tile + 8 columns of reconstruct_n1024
BATCH = 3
LAYOUTS = ("aligned", "narrow")


def names(nv, cols=COLS):
    n, k, _ = E.code_params(nv)
    if nv <= TINY_HI or nv > FAST_HI:
        return GENERIC
    nm = CLASSES[(n, k)]
    if k == 256 and cols < 128:
        nm = nm._replace(enc=P, enc_narrow=P)
    if n == 1024 and k == 256 and cols < 48:
        assert cols >= 32
        nm = nm._replace(rec="reconstruct_n1024")
    return nm


def column_counts(nv):
    """shard columns of the uniform cases of one n_validators"""
    n, k, _ = E.code_params(nv)
    if k != 256 or not TINY_HI < nv <= FAST_HI:
        return (COLS,)
    return (COLS, COLS_K256, COLS_N1024) if n == 1024 else (COLS, COLS_K256)


def payload_len(nv, cols=COLS):
    """`cols` shard columns with a ragged byte tail"""
    _, k, _ = E.code_params(nv)
    return 2 * k * cols - 3


def up(x, a):
    return (x + a - 1) // a * a


def pitches(layout, plen, shard_len):
    """(payload pitch, shard pitch) of a layout"""
    if layout == "aligned":
        return up(plen, 64), up(shard_len, 64)
    assert layout == "narrow"
    ss = up(shard_len, 8)
    return up(plen, 64), ss if ss % 16 else ss + 8


# ------------------------------------------------------------------ erasure patterns
KINDS = ("P0", "P1", "P2")


def present(nv, kind):
    """The flag row [n] of a pattern, as the caller writes it.

    P0: a random threshold-sized set.
    P1 "top": the k highest rows nv - k .. nv - 1 (every row of the last,
        partial coset and quarter is gathered; every systematic row is erased
        where nv >= 2 k), and every flag of [nv, n) set as well: those rows are
        erased by contract, whatever their flags.
    P2 "edge": rows 0 .. k - 2 and row nv - 1: exactly k present, and the single
        row nv - 1 decides the erased systematic row k - 1.

    With nv == k there would be no row to erase below k, P1 would be "all
    present" and P2 the same.  ECCR_AMD_code_params gives k < nv for every
    nv >= 2 (k = 1 at nv = 2), so no entry is such a case: asserted here, not
    skipped.  What does get weaker is P1 where nv < 2 k: the top k rows then
    include the systematic rows nv - k .. k - 1, and rows 0 .. nv - k - 1 are
    the erased ones."""
    n, k, thr = E.code_params(nv)
    assert kind in KINDS and k <= thr <= nv <= n and k < nv
    if kind == "P0":
        return synth.present_mask(10**6 + nv, nv, thr, n)
    m = np.zeros(n, np.uint8)
    if kind == "P1":
        m[nv - k:] = 1
    else:
        m[:k - 1] = 1
        m[nv - 1] = 1
    return m


def effective(nv, flags):
    """the pattern a flag row means: rows >= n_validators are erased"""
    m = (np.asarray(flags) != 0).astype(np.uint8)
    m[nv:] = 0
    return m
