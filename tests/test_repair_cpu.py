"""The masked encode and the repair (ec_amd.h "repair": ECCR_AMD_encode_missing_*,
ECCR_AMD_repair_*), what needs no GPU: the symbols, the dispatch rule against
the plain encode's, the workspace queries, every refusal the host makes before
it touches a device, and the shard length a repair's encode stage works with."""
import pytest

import ecc_amd as E
from test_dispatch import ENC_CLAUSES, ENC_SHAPES, PAY, PLEN, SH, TABLE, up

T = E.Tag
NEW_SYMBOLS = ["ECCR_AMD_encode_missing_batch", "ECCR_AMD_encode_missing_batch_ws",
               "ECCR_AMD_encode_missing_workspace_bytes", "ECCR_AMD_encode_missing_kernel",
               "ECCR_AMD_repair_batch", "ECCR_AMD_repair_batch_ws", "ECCR_AMD_repair_workspace_bytes"]
FAST, GENERIC = "encode_k256w_missing", "encode_g_missing"


def test_symbols_are_exported_and_declared():
    L = E.lib()
    header = open(E.HEADERS[1]).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # mirrored in ecc_amd.lib()
        assert name + "(" in header, name
    for name in ("encode_missing_batch", "encode_missing_batch_ws", "encode_missing_workspace_bytes",
                 "encode_missing_kernel", "repair_batch", "repair_batch_ws", "repair_workspace_bytes"):
        assert callable(getattr(E, name)), name


# ------------------------------------------------------------ the dispatch rule
def both(nv, plen=PLEN, batch=3, pay=0, sh=0, ps=0, ss=0):
    """(plain, masked) kernel names for one set of made-up buffers"""
    sl = E.shard_len(nv, plen)
    args = (nv, PAY + pay, plen, up(plen, 64) + ps, batch, SH + sh, up(sl, 64) + ss)
    return E.encode_kernel(*args), E.encode_missing_kernel(*args)


def rule(plain):
    return None if plain is None else FAST if plain == "encode_k256w" else GENERIC


def follows(**kw):
    plain, masked = both(**kw)
    assert masked == rule(plain), (kw, plain, masked)
    return plain, masked


@pytest.mark.parametrize("nv,encode,_", TABLE)
def test_table(nv, encode, _):
    for batch in (3, 1):
        plain, masked = follows(nv=nv, batch=batch)
        assert plain == encode and masked == (FAST if encode == "encode_k256w" else GENERIC)


def test_n_validators_boundaries():
    assert [follows(nv=nv)[1] for nv in (765, 766, 1024, 1025)] == [GENERIC, FAST, FAST, GENERIC]


@pytest.mark.parametrize("nv,fast,fallback", ENC_SHAPES)
@pytest.mark.parametrize("name,kw,keeps", ENC_CLAUSES, ids=[c[0] for c in ENC_CLAUSES])
def test_alignment_clauses(nv, fast, fallback, name, kw, keeps):
    plain, masked = follows(nv=nv, **kw)
    assert plain == (fast if keeps else fallback)
    assert masked == (FAST if keeps and fast == "encode_k256w" else GENERIC)


@pytest.mark.parametrize("nv", [1024, 766])
def test_pieces_per_payload(nv):
    for pieces, want in ((1, GENERIC), (127, GENERIC), (128, FAST), (129, FAST)):
        assert follows(nv=nv, plen=512 * pieces)[1] == want, pieces
        assert follows(nv=nv, plen=512 * (pieces - 1) + 1)[1] == want, pieces  # the last piece ragged
        assert follows(nv=nv, plen=512 * pieces, batch=1)[1] == want, pieces


def test_odd_rows_and_the_packed_bound():
    for kw in (dict(sh=2), dict(ss=2), dict(sh=1), dict(ss=1), dict(plen=5000, ss=1)):
        assert follows(nv=1024, **kw)[1] == GENERIC
    last = (2**32 - 128) // 8 - 1
    for batch in (last, last + 1):
        assert follows(nv=1024, plen=4096, batch=batch)[1] == GENERIC


def test_invalid_parameters_name_nothing():
    sl = E.shard_len(1024, 5000)
    for args in ((1024, PAY, 5000, 5000, 0, SH, sl), (1024, PAY, 0, 64, 1, SH, 64), (1024, PAY, 5000, 4999, 1, SH, sl),
                 (1024, PAY, 5000, 5000, 1, SH, sl - 1), (1, PAY, 5000, 5000, 1, SH, sl),
                 (65537, PAY, 5000, 5000, 1, SH, 5000)):
        assert E.encode_kernel(*args) is None and E.encode_missing_kernel(*args) is None, args
    assert E.encode_missing_kernel(1024, PAY, 5000, 5000, 1, SH, sl) == GENERIC


# ------------------------------------------------------------ workspace queries
NVS = [6, 100, 765, 766, 1024, 1025, 1500, 4096, 5000, 40000]


@pytest.mark.parametrize("nv", NVS)
def test_workspace_queries(nv):
    _, k, _ = E.code_params(nv)
    enc, rep, rec = E.encode_missing_workspace_bytes, E.repair_workspace_bytes, E.lib().ECCR_AMD_reconstruct_workspace_bytes
    for sl in (2, 300, 4096):
        plen = sl * k
        assert E.shard_len(nv, plen) == sl
        sizes_e = [enc(nv, plen, b) for b in (1, 2, 16, 97, 4096)]
        sizes_r = [rep(nv, sl, b) for b in (1, 2, 16, 97, 4096)]
        assert all(x >= 256 and x % 256 == 0 for x in sizes_e + sizes_r), (sizes_e, sizes_r)  # never 0
        assert sizes_e == sorted(sizes_e) and sizes_r == sorted(sizes_r)  # monotone in batch
        for b, r in zip((1, 2, 16, 97, 4096), sizes_r):  # the repair's covers each stage's
            assert r >= enc(nv, plen, b) and r >= int(rec(nv, sl, b))
    # 0 for what the calls themselves refuse
    assert enc(nv, 1000, 0) == 0 and enc(nv, 0, 3) == 0
    assert rep(nv, 300, 0) == 0 and rep(nv, 0, 3) == 0 and rep(nv, 301, 3) == 0 and rep(nv, 1, 3) == 0
    for bad_nv in (0, 1, 65537):
        assert enc(bad_nv, 1000, 3) == 0 and rep(bad_nv, 300, 3) == 0


def test_workspace_holds_the_plan_and_the_transform_buffers():
    # n_validators 766 .. 1024: the tile counter's block and 33 words per payload
    for nv in (766, 1024):
        assert E.encode_missing_workspace_bytes(nv, 10**6, 4096) >= 256 + 4096 * 33 * 4
        assert E.repair_workspace_bytes(nv, 3910, 4096) >= 256 + 4096 * 33 * 4
    # k = 8192 does not fit LDS: the generic kernel's buffers, two of k points per block
    assert E.code_params(40000)[1] == 8192
    assert E.encode_missing_workspace_bytes(40000, 8 * 16384, 4) >= 2 * 8192 * 8
    # n = 8192: the repair's reconstruct stage
    assert E.repair_workspace_bytes(5000, 8, 4) >= 2 * 8192 * 8


# ------------------------------------------------------------ refusals, without a device
PR, EL, OUT, WS = (0x7E00_0000_0000 + i * 0x100_0000 for i in range(4))  # 256-B aligned, never dereferenced


def _enc(nv=1024, pay=PAY, plen=70_001, ps=70_016, batch=3, sh=SH, ss=320, pr=PR, pat=None, ws=None):
    L = E.lib()
    if ws is None:
        return T(L.ECCR_AMD_encode_missing_batch(nv, pay, plen, ps, batch, sh, ss, pr, pat, None).tag)
    return T(L.ECCR_AMD_encode_missing_batch_ws(nv, pay, plen, ps, batch, sh, ss, pr, pat, ws[0], ws[1], None).tag)


def _rep(nv=1024, sh=SH, sl=300, ss=320, pr=PR, el=EL, pat=None, batch=3, out=OUT, os_=300 * 256, ws=None):
    L = E.lib()
    if ws is None:
        return T(L.ECCR_AMD_repair_batch(nv, sh, sl, ss, pr, el, pat, batch, out, os_, None).tag)
    return T(L.ECCR_AMD_repair_batch_ws(nv, sh, sl, ss, pr, el, pat, batch, out, os_, ws[0], ws[1], None).tag)


def test_shapes_of_the_refusal_cases_are_valid():
    assert E.shard_len(1024, 70_001) <= 320 and E.encode_missing_kernel(1024, PAY, 70_001, 70_016, 3, SH, 320) == FAST


def test_invalid_n_validators():
    assert _enc(nv=1) == T.NOT_ENOUGH_VALIDATORS and _rep(nv=1) == T.NOT_ENOUGH_VALIDATORS
    assert _enc(nv=65537) == T.TOO_MANY_VALIDATORS and _rep(nv=65537) == T.TOO_MANY_VALIDATORS


@pytest.mark.parametrize("kw", [dict(pay=0), dict(sh=0), dict(pr=0)], ids=lambda kw: next(iter(kw)))
def test_encode_missing_null_buffers(kw):
    assert _enc(**kw) == T.BAD_PAYLOAD
    assert "encode_missing_batch: a NULL buffer" in E.last_error()
    assert _enc(ws=(WS, 1 << 30), **kw) == T.BAD_PAYLOAD


@pytest.mark.parametrize("kw", [dict(sh=0), dict(pr=0), dict(el=0), dict(out=0)], ids=lambda kw: next(iter(kw)))
def test_repair_null_buffers(kw):
    assert _rep(**kw) == T.BAD_PAYLOAD
    assert "repair_batch: a NULL buffer" in E.last_error()
    assert _rep(ws=(WS, 1 << 30), **kw) == T.BAD_PAYLOAD


def test_the_encodes_and_the_reconstructs_own_tags():
    assert _enc(plen=0) == T.BAD_PAYLOAD
    assert _enc(ps=70_000) == T.BAD_PAYLOAD  # payload pitch below the payload
    assert _enc(ss=E.shard_len(1024, 70_001) - 1) == T.BAD_PAYLOAD  # shard pitch below the row
    assert _rep(sl=301, ss=320) == T.UNEVEN_LENGTH
    assert _rep(ss=298) == T.NON_UNIFORM_CHUNKS  # shard pitch below the row
    assert _rep(os_=300 * 256 - 1) == T.NON_UNIFORM_CHUNKS  # out pitch below shard_len * k
    assert _rep(sl=0, os_=0) == T.BAD_PAYLOAD  # nothing to encode from


@pytest.mark.parametrize("nv", [1024, 100, 5000])
def test_workspace_refusals(nv):
    """NULL, short or misaligned: an error naming the sizes, before the device is
    touched (the addresses are made up: a launch would not return a tag)"""
    _, k, _ = E.code_params(nv)
    sl, batch = 300, 3
    plen = sl * k
    need_e, need_r = E.encode_missing_workspace_bytes(nv, plen, batch), E.repair_workspace_bytes(nv, sl, batch)
    for need, call, tag in ((need_e, lambda ws: _enc(nv=nv, plen=plen, ps=plen, ss=320, ws=ws), T.UNKNOWN_CODE_PARAM),
                            (need_r, lambda ws: _rep(nv=nv, os_=plen, ws=ws), T.UNKNOWN_RECONSTRUCTION)):
        for ws in ((None, 0), (None, need), (WS, need - 1), (WS, 0), (WS + 128, need + 128), (WS + 1, need + 1)):
            assert call(ws) == tag, (nv, ws)
            assert "workspace of %d bytes" % ws[1] in E.last_error() and str(need) in E.last_error()


def test_an_empty_batch_is_ok_and_does_nothing():
    assert _enc(batch=0) == T.OK and _rep(batch=0) == T.OK
    assert _enc(batch=0, ws=(None, 0)) == T.OK and _rep(batch=0, ws=(None, 0)) == T.OK


# ------------------------------------------------------------ the repair's encode stage
@pytest.mark.parametrize("nv", [6, 100, 766, 1024, 1500, 4096])
def test_shard_len_of_the_reconstructed_payload(nv):
    """the encode stage takes d_out as payloads of shard_len * k bytes: their shard
    length is shard_len again, for every even shard_len"""
    _, k, _ = E.code_params(nv)
    for sl in range(2, 4097, 2):
        assert E.shard_len(nv, sl * k) == sl, (nv, sl)
    # ... and the stage is dispatched on that length: a repair of 2 * 128 bytes a row is the first
    # whose payloads have the fast kernel's 128 pieces
    want = {766: (GENERIC, FAST), 1024: (GENERIC, FAST)}.get(nv, (GENERIC, GENERIC))
    for sl, name in zip((254, 256), want):
        assert E.encode_missing_kernel(nv, OUT, sl * k, sl * k, 3, SH, up(sl, 64)) == name, (nv, sl)
        assert E.repair_workspace_bytes(nv, sl, 3) >= E.encode_missing_workspace_bytes(nv, sl * k, 3) > 0
