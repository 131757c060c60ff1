"""Which kernel a batch call runs (csrc/ec_kernels.hip choose_encode /
choose_reconstruct, through the ECCR_AMD_encode_kernel / _reconstruct_kernel
queries).  Host-only: no GPU, nothing is allocated, every address is a made-up
integer (a 4 KiB-aligned constant plus an offset).

Every expected name is a literal written from DESIGN.md §5.6 and from the
kernels' access widths; the tests never ask the chooser for their own
expectation.  Each clause of each predicate has a case on both sides with the
other clauses held true (the `control` rows)."""
import pytest

import ecc_amd as E

PAY, SH, PR, EL, OUT = (0x7F00_0000_0000 + i * 0x1000_0000_0000 for i in range(5))  # 4 KiB aligned
PLEN = 300_001  # several tiles of every kernel (586 pieces at k = 256, 147 at k = 1024)


def up(x, a):
    return (x + a - 1) // a * a


def enc(nv, plen=PLEN, batch=3, pay=0, sh=0, ps=0, ss=0):
    """encode query; pay / sh: offsets of the bases, ps / ss: bytes added to the 64-B pitches"""
    sl = E.shard_len(nv, plen)
    return E.encode_kernel(nv, PAY + pay, plen, up(plen, 64) + ps, batch, SH + sh, up(sl, 64) + ss)


def rec(nv, plen=PLEN, batch=3, sh=0, ss=0, pr=0, el=0, out=0, os_=0, slen=None):
    _, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen) if slen is None else slen
    return E.reconstruct_kernel(nv, SH + sh, sl, up(sl, 64) + ss, PR + pr, EL + el, batch, OUT + out,
                                sl * k + os_)


# ------------------------------------------------------------ DESIGN.md §5.6
TABLE = [  # first and last n_validators of every class
    (2, "encode_g", "reconstruct_g"), (45, "encode_g", "reconstruct_g"),
    (46, "encode_kw", "reconstruct_gen"), (765, "encode_kw", "reconstruct_gen"),
    (766, "encode_k256w", "reconstruct_n1024x"), (1024, "encode_k256w", "reconstruct_n1024x"),
    (1025, "encode_kw", "reconstruct_n4096"), (1533, "encode_kw", "reconstruct_n4096"),
    (1534, "encode_k512w", "reconstruct_n4096"), (3069, "encode_k512w", "reconstruct_n4096"),
    (3070, "encode_k1024", "reconstruct_n4096"), (4096, "encode_k1024", "reconstruct_n4096"),
    (4097, "encode_g", "reconstruct_g"), (65536, "encode_g", "reconstruct_g"),
]


@pytest.mark.parametrize("nv,encode,reconstruct", TABLE)
def test_table_aligned(nv, encode, reconstruct):
    """everything 64-byte aligned, payloads of several tiles, batch 3 and 1"""
    for batch in (3, 1):
        assert enc(nv, batch=batch) == encode
        assert rec(nv, batch=batch) == reconstruct


# ------------------------------------------------------------ encode predicate
# One fast shape per kernel; what an alignment the fast kernels cannot take
# falls to: k = 256 has the packed kernel for any payload base / pitch and any
# even shard base / pitch, every other k has encode_g.
ENC_SHAPES = [(1024, "encode_k256w", "encode_k256_packed"), (1400, "encode_kw", "encode_k256_packed"),
              (300, "encode_kw", "encode_g"), (2500, "encode_k512w", "encode_g"),
              (4096, "encode_k1024", "encode_g")]

ENC_CLAUSES = [  # (id, query arguments, the side of the clause: True = the fast kernel keeps it)
    ("control", {}, True),
    # payload base mod 16 (16-B payload loads)
    ("pay+16", dict(pay=16), True), ("pay+8", dict(pay=8), False), ("pay+1", dict(pay=1), False),
    # shard base mod 8 (8-B stores where rows are off 16 B)
    ("sh+8", dict(sh=8), True), ("sh+4", dict(sh=4), False),
    # payload pitch mod 16, and its batch == 1 escape (the pitch is never applied)
    ("ps+16", dict(ps=16), True), ("ps+8", dict(ps=8), False), ("ps+1", dict(ps=1), False),
    ("ps+8,batch1", dict(ps=8, batch=1), True), ("ps+1,batch1", dict(ps=1, batch=1), True),
    # shard pitch mod 8
    ("ss+8", dict(ss=8), True), ("ss+4", dict(ss=4), False),
]


@pytest.mark.parametrize("nv,fast,fallback", ENC_SHAPES)
@pytest.mark.parametrize("name,kw,keeps", ENC_CLAUSES, ids=[c[0] for c in ENC_CLAUSES])
def test_encode_alignment_clauses(nv, fast, fallback, name, kw, keeps):
    assert enc(nv, **kw) == (fast if keeps else fallback)


@pytest.mark.parametrize("nv", [1024, 1400])
def test_encode_packed_needs_even_shard_rows(nv):
    """shard base / pitch mod 2: the packed kernel stores 2-byte symbols"""
    assert enc(nv, sh=2) == "encode_k256_packed"
    assert enc(nv, ss=2) == "encode_k256_packed"
    assert enc(nv, sh=1) == "encode_g"
    assert enc(nv, ss=1) == "encode_g"
    assert enc(nv, ss=3) == "encode_g"
    # one odd clause is enough, however the payload is laid out
    assert enc(nv, sh=1, batch=1) == "encode_g"
    assert enc(nv, plen=5000, ss=1) == "encode_g"


@pytest.mark.parametrize("nv", [300, 2500, 4096])
def test_encode_odd_shard_rows_other_k(nv):
    for kw in (dict(sh=2), dict(sh=1), dict(ss=2), dict(ss=1)):
        assert enc(nv, **kw) == "encode_g"


@pytest.mark.parametrize("nv,fast", [(1024, "encode_k256w"), (766, "encode_k256w"), (1400, "encode_kw")])
def test_encode_k256_pieces_per_payload(nv, fast):
    """k = 256: payloads under one 128-piece tile (512-byte pieces) run packed
    whatever their alignment.  (63 / 64 pieces, the tile of encode_k256w itself,
    is not a boundary of the dispatch.)"""
    for pieces, want in ((1, "encode_k256_packed"), (63, "encode_k256_packed"),
                         (64, "encode_k256_packed"), (127, "encode_k256_packed"), (128, fast)):
        assert enc(nv, plen=512 * pieces) == want, pieces
        assert enc(nv, plen=512 * (pieces - 1) + 1) == want, pieces  # the last piece ragged
        assert enc(nv, plen=512 * pieces, batch=1) == want, pieces


def test_encode_packed_flattened_space_bound():
    """packed k = 256: (pieces rounded up to 8) * batch + 128 < 2^32; past it
    the shape goes on down the list (encode_kw at n = 2048 if aligned, else
    encode_g)"""
    last = (2**32 - 128) // 8 - 1  # 8-piece payloads
    assert 8 * last + 128 < 2**32 <= 8 * (last + 1) + 128
    for nv, beyond in ((1024, "encode_g"), (1400, "encode_kw")):
        assert enc(nv, plen=4096, batch=last) == "encode_k256_packed"
        assert enc(nv, plen=4096, batch=last + 1) == beyond
        assert enc(nv, plen=4096 - 511, batch=last + 1) == beyond  # ragged last piece
        assert enc(nv, plen=4096, batch=last + 1, pay=1) == "encode_g"
    # one-piece payloads still round up to 8 slots
    assert enc(1024, plen=1, batch=last) == "encode_k256_packed"
    assert enc(1024, plen=1, batch=last + 1) == "encode_g"


# ------------------------------------------------------------ reconstruct predicate
# What a shape falls to when its fast kernel cannot take an alignment: n = 1024
# has the packed kernel for any even shard base / pitch; everything else (and
# every out / present / err_log clause) falls to reconstruct_g.
REC_SHAPES = [(1024, "reconstruct_n1024x"), (800, "reconstruct_n1024x"), (1400, "reconstruct_n4096"),
              (2500, "reconstruct_n4096"), (4096, "reconstruct_n4096"), (600, "reconstruct_gen"),
              (100, "reconstruct_gen")]
G = "reconstruct_g"

REC_CLAUSES = [  # (id, arguments, n = 1024 result or None = stays, n4096 / gen result or None = stays)
    ("control", {}, None, None),
    # shard base / pitch mod 16 (16-B row loads) and mod 2
    ("sh+16", dict(sh=16), None, None),
    ("sh+8", dict(sh=8), "reconstruct_n1024_packed", G), ("sh+2", dict(sh=2), "reconstruct_n1024_packed", G),
    ("sh+1", dict(sh=1), G, G),
    ("ss+16", dict(ss=16), None, None),
    ("ss+8", dict(ss=8), "reconstruct_n1024_packed", G), ("ss+2", dict(ss=2), "reconstruct_n1024_packed", G),
    ("ss+1", dict(ss=1), G, G),
    # out base / pitch: 8-B stores in the n = 1024 kernels, 16-B in reconstruct_n4096 / _gen
    ("out+16", dict(out=16), None, None), ("out+8", dict(out=8), None, G), ("out+4", dict(out=4), G, G),
    ("out+1", dict(out=1), G, G),
    ("os+16", dict(os_=16), None, None), ("os+64", dict(os_=64), None, None),
    ("os+8", dict(os_=8), None, G), ("os+4", dict(os_=4), G, G), ("os+1", dict(os_=1), G, G),
    # batch == 1: the out pitch is never applied
    ("os+8,batch1", dict(os_=8, batch=1), None, None), ("os+1,batch1", dict(os_=1, batch=1), None, None),
    ("out+8,batch1", dict(out=8, batch=1), None, G),
    # present / err_log base mod 16: vector loads of the rows in the n = 1024 kernels only
    ("pr+16", dict(pr=16), None, None), ("pr+1", dict(pr=1), G, None), ("pr+8", dict(pr=8), G, None),
    ("el+16", dict(el=16), None, None), ("el+2", dict(el=2), G, None), ("el+8", dict(el=8), G, None),
]


@pytest.mark.parametrize("nv,fast", REC_SHAPES)
@pytest.mark.parametrize("name,kw,n1024,other", REC_CLAUSES, ids=[c[0] for c in REC_CLAUSES])
def test_reconstruct_alignment_clauses(nv, fast, name, kw, n1024, other):
    want = n1024 if fast == "reconstruct_n1024x" else other
    assert rec(nv, **kw) == (want or fast)


def test_reconstruct_packed_clauses():
    """the packed n = 1024 kernel keeps the out8 clause (8-B stores, vector
    loads of the flag / locator rows) and needs even shard rows"""
    small = dict(plen=5000)  # 10 columns: packed by size
    assert rec(1024, **small) == "reconstruct_n1024_packed"
    assert rec(1024, batch=1, os_=1, **small) == "reconstruct_n1024_packed"
    assert rec(1024, out=8, os_=8, sh=2, ss=2, **small) == "reconstruct_n1024_packed"
    for kw in (dict(out=4), dict(os_=4), dict(os_=1), dict(pr=1), dict(el=2), dict(sh=1), dict(ss=1)):
        assert rec(1024, **kw, **small) == G, kw
        assert rec(1024, **{**dict(sh=8, ss=8), **kw}) == G, kw  # packed by alignment


@pytest.mark.parametrize("cols,want", [(1, "reconstruct_n1024_packed"), (31, "reconstruct_n1024_packed"),
                                        (32, "reconstruct_n1024"), (47, "reconstruct_n1024"),
                                        (48, "reconstruct_n1024x"), (49, "reconstruct_n1024x")])
def test_reconstruct_n1024_columns(cols, want):
    """n = 1024: under one 32-column tile packed, under one 48-column tile of
    the 12-wave kernel the 8-wave one"""
    for nv in (766, 1024):
        for batch in (1, 3):
            assert rec(nv, slen=2 * cols, batch=batch) == want


def test_reconstruct_packed_flattened_space_bound():
    """packed n = 1024: (columns rounded up to 4) * batch + 32 < 2^32; past it
    the call is an error and nothing is launched"""
    last = (2**32 - 32) // 4 - 1  # 4-column payloads
    assert 4 * last + 32 < 2**32 <= 4 * (last + 1) + 32
    for slen in (8, 6, 2):  # 4, 3 and 1 columns: all take 4 slots
        assert rec(1024, slen=slen, batch=last) == "reconstruct_n1024_packed"
        assert rec(1024, slen=slen, batch=last + 1) is None
    assert rec(1024, slen=8, batch=last + 1, sh=1) == G  # not the packed kernel's shape at all


def test_invalid_parameters_name_nothing():
    sl = E.shard_len(1024, 5000)
    assert E.encode_kernel(1024, PAY, 5000, 5000, 0, SH, sl) is None  # empty batch
    assert E.encode_kernel(1024, PAY, 0, 64, 1, SH, 64) is None  # empty payload
    assert E.encode_kernel(1024, PAY, 5000, 4999, 1, SH, sl) is None  # pitch below the row
    assert E.encode_kernel(1024, PAY, 5000, 5000, 1, SH, sl - 1) is None
    assert E.encode_kernel(1, PAY, 5000, 5000, 1, SH, sl) is None  # n_validators out of range
    assert E.encode_kernel(65537, PAY, 5000, 5000, 1, SH, 5000) is None
    assert E.reconstruct_kernel(1024, SH, sl, sl, PR, EL, 0, OUT, sl * 256) is None
    assert E.reconstruct_kernel(1024, SH, sl + 1, sl + 1, PR, EL, 1, OUT, (sl + 1) * 256) is None  # odd
    assert E.reconstruct_kernel(1024, SH, sl, sl - 2, PR, EL, 1, OUT, sl * 256) is None
    assert E.reconstruct_kernel(1024, SH, sl, sl, PR, EL, 1, OUT, sl * 256 - 1) is None
    assert E.reconstruct_kernel(1024, SH, 0, 0, PR, EL, 1, OUT, 0) is None  # no columns
    assert E.encode_kernel(1024, PAY, 5000, 5000, 1, SH, sl) == "encode_k256_packed"
    assert E.reconstruct_kernel(1024, SH, sl, sl, PR, EL, 1, OUT, sl * 256) == "reconstruct_n1024_packed"


# ------------------------------------------------------------ experiment overrides
_QUERY = """
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
f = L.ECCR_AMD_reconstruct_kernel
f.restype = C.c_char_p
f.argtypes = [C.c_ulong, C.c_void_p, C.c_ulong, C.c_ulong, C.c_void_p, C.c_void_p, C.c_ulong, C.c_void_p,
              C.c_ulong]
B = 0x7F0000000000
for cols in (10, 40, 59):
    print(f(1024, B, 2 * cols, 128, B + (1 << 40), B + (2 << 40), 3, B + (3 << 40), 512 * cols).decode())
"""


@pytest.mark.parametrize("env,want", [
    ({}, ["reconstruct_n1024_packed", "reconstruct_n1024", "reconstruct_n1024x"]),
    # the 8-wave kernel where the 12-wave one applies
    ({"ECCR_AMD_RECON_WAVES": "8"}, ["reconstruct_n1024_packed", "reconstruct_n1024", "reconstruct_n1024"]),
    # the 8-wave kernel runs packed at every size (the 12-wave one is chosen before it)
    ({"ECCR_AMD_RECON_PACKED": "1"},
     ["reconstruct_n1024_packed", "reconstruct_n1024_packed", "reconstruct_n1024x"]),
    ({"ECCR_AMD_RECON_WAVES": "8", "ECCR_AMD_RECON_PACKED": "1"}, ["reconstruct_n1024_packed"] * 3),
], ids=["none", "waves8", "packed", "waves8+packed"])
def test_reconstruct_experiment_overrides(env, want):
    """ECCR_AMD_RECON_WAVES / ECCR_AMD_RECON_PACKED are read once per process:
    10, 40 and 59 aligned columns at n = 1024 in a fresh process each"""
    import os
    import subprocess
    import sys
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ECCR_AMD_RECON_")}
    r = subprocess.run([sys.executable, "-c", _QUERY, E.LIB_PATH], env={**clean, **env},
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == want
