"""Buffer-layout cases of the batch API and the guard arena they run in
(test_gpu_layouts.py runs them on the GPU; test_layout_cases.py checks the
arena and the tables' coverage without one).

A case = one shape (n_validators, payload length, the kernel each class of
layout must name, as literals) x one layout variant that differs from the
all-64-byte control in one respect."""
from collections import namedtuple

import numpy as np

GUARD = 256


def up(x, a):
    return (x + a - 1) // a * a


class Arena:
    """One byte buffer all buffers of a case are carved from, at chosen offsets
    from 256-byte boundaries, with at least GUARD bytes before each base and
    after each end.  The buffer is seeded noise; `allow` marks the bytes the
    API may write; `violations` compares everything else with the host copy."""

    def __init__(self, seed):
        self.seed = seed
        self.regions = []  # (name, base, nbytes)
        self.size = GUARD
        self.host = None
        self.mask = None

    def add(self, name, nbytes, off=0):
        base = up(self.size, 256) + GUARD + off
        self.regions.append((name, base, nbytes))
        self.size = base + nbytes + GUARD
        return base

    def build(self):
        self.size = up(self.size, 256)
        self.host = np.random.default_rng(self.seed).integers(0, 256, self.size, dtype=np.uint8)
        self.mask = np.zeros(self.size, dtype=bool)
        return self.host

    def allow(self, start, nbytes):
        self.mask[start:start + nbytes] = True

    def allow_rows(self, base, rows, stride, used):
        for r in range(rows):
            self.allow(base + r * stride, used)

    def where(self, pos):
        """'region+offset' / 'region-offset' (the guard before it) of an arena position"""
        best = None
        for name, base, nbytes in self.regions:
            if base - GUARD <= pos < base + nbytes + GUARD:
                best = (name, pos - base, nbytes)
                if base <= pos < base + nbytes:
                    break
        if best is None:
            return f"arena+{pos}"
        name, rel, nbytes = best
        return f"{name}{rel:+d} (of {nbytes})"

    def violations(self, got, limit=8):
        """positions outside the writable mask where `got` differs from the host copy"""
        got = np.asarray(got).reshape(-1)
        assert got.shape == self.host.shape
        bad = np.flatnonzero((got != self.host) & ~self.mask)
        return [self.where(int(p)) for p in bad[:limit]] + (["..."] if len(bad) > limit else [])


# ------------------------------------------------------------------ encode
# kernel named for: the control and every layout the fast kernel keeps / any
# payload base or pitch off 16 B / even shard rows off 8 B / odd shard rows
EncShape = namedtuple("EncShape", "nv plen keep anypay even odd")
P, G = "encode_k256_packed", "encode_g"
ENC_SHAPES = [
    # encode_kw: k = 32, 64, 128 and <8> (k = 256 at n = 2048)
    EncShape(100, 40_001, "encode_kw", G, G, G), EncShape(300, 40_001, "encode_kw", G, G, G),
    EncShape(700, 40_001, "encode_kw", G, G, G),
    # k = 256 dispatches on a 128-piece tile: 40,001 bytes (79 pieces) run packed
    # at n = 1024 and 2048, 70,001 (137 pieces: a whole tile and a partial one) unpacked
    EncShape(1400, 40_001, P, P, P, G), EncShape(1400, 70_001, "encode_kw", P, P, G),
    EncShape(1024, 40_001, P, P, P, G), EncShape(800, 40_001, P, P, P, G),
    EncShape(1024, 70_001, "encode_k256w", P, P, G), EncShape(800, 70_001, "encode_k256w", P, P, G),
    EncShape(1024, 5_000, P, P, P, G), EncShape(1400, 5_000, P, P, P, G),
    EncShape(1800, 40_001, "encode_k512w", G, G, G), EncShape(2500, 40_001, "encode_k512w", G, G, G),
    EncShape(4096, 70_001, "encode_k1024", G, G, G), EncShape(3500, 70_001, "encode_k1024", G, G, G),
    EncShape(20, 3_001, G, G, G, G), EncShape(5000, 3_001, G, G, G, G),
]
ENC_SHAPES_1 = [  # one-piece payloads: the shard-base and pitch variants
    EncShape(100, 1, "encode_kw", G, G, G), EncShape(1024, 1, P, P, P, G), EncShape(1400, 1, P, P, P, G),
    EncShape(1800, 1, "encode_k512w", G, G, G), EncShape(4096, 1, "encode_k1024", G, G, G),
    EncShape(20, 1, G, G, G, G),
]

# pay / sh: offset of the base; ps / ss: the pitch as a function of the used
# length; batch; cls: which of the shape's names the query must give
EncVariant = namedtuple("EncVariant", "name cls batch pay sh ps ss", defaults=(3, 0, 0, None, None))


def _p64(used):
    return up(used, 64)


ENC_VARIANTS = [
    EncVariant("control", "keep"),
    EncVariant("pay+1", "anypay", pay=1), EncVariant("pay+8", "anypay", pay=8),
    EncVariant("ps=8mod16", "anypay", ps=lambda u: up(u, 16) + 8),
    EncVariant("ps-odd", "anypay", ps=lambda u: up(u, 16) + 1),
    EncVariant("batch1,ps-odd", "keep", batch=1, ps=lambda u: up(u, 16) + 1),
    EncVariant("sh+8", "keep", sh=8), EncVariant("sh+2", "even", sh=2), EncVariant("sh+1", "odd", sh=1),
    EncVariant("ss=8mod16", "keep", ss=lambda u: up(u, 16) + 8),
    EncVariant("ss=2mod8", "even", ss=lambda u: up(u, 8) + 2),
    EncVariant("ss-odd", "odd", ss=lambda u: up(u, 16) + 1),
]
ENC_VARIANTS_1 = [v for v in ENC_VARIANTS if v.pay == 0 and v.batch == 3 and (v.sh or v.ss or v.name == "control")]


def enc_cases():
    return ([(s, v) for s in ENC_SHAPES for v in ENC_VARIANTS] +
            [(s, v) for s in ENC_SHAPES_1 for v in ENC_VARIANTS_1])


def enc_layout(shape, var, shard_len):
    """(pay_off, pstride, sh_off, sstride) of a case"""
    ps = (var.ps or _p64)(shape.plen)
    ss = (var.ss or _p64)(shard_len)
    return var.pay, ps, var.sh, ss


# ------------------------------------------------------------------ reconstruct
# kernel named for: the control and every layout the fast kernel keeps / out
# base or pitch at 8 mod 16 / out base or pitch off 8 / present or err_log base
# off 16 / even shard rows off 16 B / odd shard rows
RecShape = namedtuple("RecShape", "nv plen keep out8 outodd rows sheven shodd")
R, X, N, K, Q, GEN = ("reconstruct_g", "reconstruct_n1024x", "reconstruct_n1024", "reconstruct_n1024_packed",
                      "reconstruct_n4096", "reconstruct_gen")
REC_SHAPES = [
    RecShape(1024, 30_001, X, X, R, R, K, R), RecShape(800, 30_001, X, X, R, R, K, R),  # 59 columns
    RecShape(1024, 20_001, N, N, R, R, K, R),  # 40 columns: the 8-wave kernel
    RecShape(1024, 5_000, K, K, R, R, K, R),  # 10 columns
    RecShape(1500, 40_001, Q, R, R, Q, R, R),  # 2 halves, k = 256
    RecShape(2500, 40_001, Q, R, R, Q, R, R), RecShape(4096, 40_001, Q, R, R, Q, R, R),  # 4 quarters
    RecShape(46, 20_001, GEN, R, R, GEN, R, R), RecShape(100, 20_001, GEN, R, R, GEN, R, R),
    RecShape(600, 20_001, GEN, R, R, GEN, R, R),
    RecShape(20, 3_001, R, R, R, R, R, R), RecShape(5000, 3_001, R, R, R, R, R, R),
]
REC_SHAPES_1 = [  # one-column payloads: the shard-base and pitch variants
    RecShape(1024, 1, K, K, R, R, K, R), RecShape(2500, 1, Q, R, R, Q, R, R),
    RecShape(600, 1, GEN, R, R, GEN, R, R), RecShape(20, 1, R, R, R, R, R, R),
]

RecVariant = namedtuple("RecVariant", "name cls batch sh ss pr el out os",
                        defaults=(3, 0, None, 0, 0, 0, 0))
REC_VARIANTS = [
    RecVariant("control", "keep"),
    RecVariant("out+8", "out8", out=8), RecVariant("out+2", "outodd", out=2),
    RecVariant("out+1", "outodd", out=1),
    RecVariant("os+8", "out8", os=8), RecVariant("os+16", "keep", os=16), RecVariant("os+64", "keep", os=64),
    RecVariant("os+1", "outodd", os=1), RecVariant("batch1,os+1", "keep", batch=1, os=1),
    RecVariant("pr+1", "rows", pr=1), RecVariant("pr+16", "keep", pr=16),
    RecVariant("el+2", "rows", el=2), RecVariant("el+16", "keep", el=16),
    RecVariant("sh+8", "sheven", sh=8), RecVariant("sh+2", "sheven", sh=2), RecVariant("sh+1", "shodd", sh=1),
    RecVariant("ss=8mod16", "sheven", ss=lambda u: up(u, 16) + 8),
    RecVariant("ss=2mod16", "sheven", ss=lambda u: up(u, 16) + 2),
    RecVariant("ss-odd", "shodd", ss=lambda u: up(u, 16) + 1),
]
REC_VARIANTS_1 = [v for v in REC_VARIANTS if v.name == "control" or v.sh or v.ss]


def rec_cases():
    return ([(s, v) for s in REC_SHAPES for v in REC_VARIANTS] +
            [(s, v) for s in REC_SHAPES_1 for v in REC_VARIANTS_1])


def rec_layout(shape, var, shard_len, k):
    """(sh_off, sstride, pr_off, el_off, out_off, ostride) of a case"""
    ss = (var.ss or _p64)(shard_len)
    return var.sh, ss, var.pr, var.el, var.out, shard_len * k + var.os


def case_id(case):
    s, v = case
    return f"nv{s.nv}-{s.plen}B-{v.name}"


# ------------------------------------------------------------------ other entry points
LOCATOR_N = [32, 64, 1024, 4096, 8192]  # n_validators = n: error_locator_g below 64 and above 4096
SYSTEMATIC_NV = [6, 1024]
# host batches: (nv, plen, bytes added to the tight payload / shard pitch, to the out pitch)
HOST_CASES = [(nv, plen, pad, opad) for nv in (1024, 600) for plen in (40_001, 200)
              for pad, opad in ((3, 3), (64, 64))]
# out rows under 256 bytes (k = 32, one column): the short-row leg of the out copy
HOST_CASES += [(100, 50, 3, 3), (100, 50, 64, 64)]

# ------------------------------------------------------------------ coverage bookkeeping
KERNELS = ["encode_k256w", "encode_k256_packed", "encode_kw", "encode_k512w", "encode_k1024", "encode_g",
           "reconstruct_n1024x", "reconstruct_n1024", "reconstruct_n1024_packed", "reconstruct_n4096",
           "reconstruct_gen", "reconstruct_g"]
