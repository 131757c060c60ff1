"""Ragged device batches (ec_amd.h ECCR_AMD_*_ragged), what needs no GPU: the
symbols and the item layout, the workspace queries, every rejection the host
makes before it touches a device, the kernel names, and the item validation
(ECCR_AMD_ragged_check: the function the device's plan kernel runs, on a host
copy of the items)."""
import ctypes as C

import numpy as np
import pytest

import ecc_amd as E

T = E.Tag
NEW_SYMBOLS = ["ECCR_AMD_encode_ragged", "ECCR_AMD_encode_ragged_ws", "ECCR_AMD_reconstruct_ragged",
               "ECCR_AMD_reconstruct_ragged_ws", "ECCR_AMD_encode_ragged_workspace_bytes",
               "ECCR_AMD_reconstruct_ragged_workspace_bytes", "ECCR_AMD_ragged_check",
               "ECCR_AMD_encode_ragged_kernel", "ECCR_AMD_reconstruct_ragged_kernel"]


def test_symbols_and_item_layout():
    L = E.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert C.sizeof(E.RaggedItem) == 40
    assert [f for f, _ in E.RaggedItem._fields_] == ["payload_off", "payload_len", "shard_off", "shard_len",
                                                     "shard_stride"]
    assert [getattr(E.RaggedItem, f).offset for f in E.RAGGED_FIELDS] == [0, 8, 16, 24, 32]
    header = open(E.HEADERS[1]).read()
    for name in NEW_SYMBOLS + ["ECCR_AMD_RaggedItem"]:
        assert name in header, name
    section = header[header.index("/* ---- ragged batches"):header.index("/* ---- diagnostics")]
    assert "ECCR_AMD_RaggedItem" in section and "round " not in section


@pytest.mark.parametrize("nv", [6, 100, 765, 766, 1024, 1025, 5000, 40000])
def test_workspace_queries(nv):
    L = E.lib()
    enc, rec = L.ECCR_AMD_encode_ragged_workspace_bytes, L.ECCR_AMD_reconstruct_ragged_workspace_bytes
    for q in (enc, rec):
        # always needed, whole 256-B blocks, and it holds at least the 4 bytes per item of the plan
        assert q(nv, 1, 2) >= 512 and q(nv, 1, 2) % 256 == 0
        assert q(nv, 100_000, 2) >= 400_000
        sizes = [[q(nv, b, m) for m in (2, 1000, 1_000_000, 10_000_000)] for b in (1, 2, 97, 4096, 100_000)]
        for row in sizes:  # monotone in the maximum
            assert row == sorted(row), (nv, row)
        for col in zip(*sizes):  # monotone in the batch
            assert list(col) == sorted(col), (nv, col)
        # 0 for what the calls themselves reject
        assert q(nv, 0, 1000) == 0 and q(nv, 1 << 31, 1000) == 0 and q(nv, 3, 0) == 0
    for bad_nv in (0, 1, 65537):
        assert enc(bad_nv, 3, 1000) == 0 and rec(bad_nv, 3, 1000) == 0


def test_workspace_holds_what_the_kernels_need():
    # n = 1024: the reconstruct's gather order, 4 n bytes per item
    assert E.ragged_workspace_bytes(1024, 100, 1_000_000)[1] >= 100 * 4 * 1024
    # generic shapes whose transform does not fit LDS take their buffers from the workspace,
    # sized from the maximum: reconstruct at n = 8192, encode at k = 8192
    small, large = (E.lib().ECCR_AMD_reconstruct_ragged_workspace_bytes(5000, 4, m) for m in (8, 80))
    assert large > small >= 2 * 8192 * 8
    assert E.code_params(40000)[1] == 8192
    small, large = (E.lib().ECCR_AMD_encode_ragged_workspace_bytes(40000, 4, m) for m in (8 * 16384, 80 * 16384))
    assert large > small >= 2 * 8192 * 8
    # shapes that fit: the plan only
    assert E.lib().ECCR_AMD_encode_ragged_workspace_bytes(100, 4, 10**6) == 512


# made-up addresses: the host checks dereference nothing
PAY, ITEMS, SH, OUT, PR, EL, ST = (0x10000 * i for i in range(1, 8))


def _enc(nv=1024, pay=PAY, items=ITEMS, batch=4, mx=1000, sh=SH, st=ST, ws=None):
    L = E.lib()
    if ws is None:
        return T(L.ECCR_AMD_encode_ragged(nv, pay, items, batch, mx, sh, st, None).tag)
    return T(L.ECCR_AMD_encode_ragged_ws(nv, pay, items, batch, mx, sh, st, ws[0], ws[1], None).tag)


def _rec(nv=1024, sh=SH, items=ITEMS, pr=PR, el=EL, pat=None, batch=4, mx=1000, out=OUT, st=ST, ws=None):
    L = E.lib()
    if ws is None:
        return T(L.ECCR_AMD_reconstruct_ragged(nv, sh, items, pr, el, pat, batch, mx, out, st, None).tag)
    return T(L.ECCR_AMD_reconstruct_ragged_ws(nv, sh, items, pr, el, pat, batch, mx, out, st, ws[0], ws[1],
                                              None).tag)


@pytest.mark.parametrize("ws", [None, (0x900000, 1 << 30)], ids=["plain", "ws"])
def test_host_rejections_need_no_device(ws):
    """n_validators, NULL pointers, batch 0 / >= 2^31, a maximum of 0 and a
    tile count that reaches 2^32, each with its tag, checked before the device
    is touched (the pointers are made up: a launch would fault)"""
    for f in (_enc, _rec):
        assert f(nv=1, ws=ws) == T.NOT_ENOUGH_VALIDATORS and f(nv=0, ws=ws) == T.NOT_ENOUGH_VALIDATORS
        assert f(nv=65537, ws=ws) == T.TOO_MANY_VALIDATORS
        assert f(items=None, ws=ws) == T.BAD_PAYLOAD and f(sh=None, ws=ws) == T.BAD_PAYLOAD
        assert f(batch=0, ws=ws) == T.BAD_PAYLOAD and "batch" in E.last_error()
        assert f(batch=1 << 31, ws=ws) == T.BAD_PAYLOAD
        assert f(batch=(1 << 31) + 5, ws=ws) == T.BAD_PAYLOAD
    assert _enc(pay=None, ws=ws) == T.BAD_PAYLOAD
    for k in ("pr", "el", "out"):
        assert _rec(ws=ws, **{k: None}) == T.BAD_PAYLOAD, k
    assert _enc(mx=0, ws=ws) == T.BAD_PAYLOAD and "maximum" in E.last_error()
    assert _rec(mx=0, ws=ws) == T.NON_UNIFORM_CHUNKS
    # tiles: 64 pieces of 512 payload bytes / 64 columns of 2 shard bytes at n_validators 1024
    assert _enc(batch=1 << 20, mx=(1 << 12) * 64 * 512, ws=ws) == T.BAD_PAYLOAD and "2^32" in E.last_error()
    assert _rec(batch=1 << 20, mx=(1 << 12) * 64 * 2, ws=ws) == T.BAD_PAYLOAD and "2^32" in E.last_error()
    assert _enc(batch=1, mx=1 << 48, ws=ws) == T.BAD_PAYLOAD and _rec(batch=1, mx=1 << 40, ws=ws) == T.BAD_PAYLOAD
    # generic shapes count their own, smaller tiles (nv 5000: 16 pieces / 4 positions a block)
    assert _enc(nv=5000, batch=1 << 20, mx=(1 << 12) * 16 * 2048, ws=ws) == T.BAD_PAYLOAD
    assert _rec(nv=5000, batch=1 << 20, mx=(1 << 12) * 4 * 2, ws=ws) == T.BAD_PAYLOAD
    # buffers off their alignment
    assert _enc(pay=PAY + 8, ws=ws) == T.BAD_PAYLOAD and _enc(sh=SH + 4, ws=ws) == T.BAD_PAYLOAD
    assert _rec(out=OUT + 8, ws=ws) == T.BAD_PAYLOAD and _rec(pr=PR + 1, ws=ws) == T.BAD_PAYLOAD
    assert _enc(items=ITEMS + 4, ws=ws) == T.BAD_PAYLOAD


def test_workspace_rejections_need_no_device():
    need_e, need_r = E.ragged_workspace_bytes(1024, 4, 1000)
    assert _enc(ws=(0x900000, need_e - 1)) == T.UNKNOWN_CODE_PARAM and "workspace" in E.last_error()
    assert _rec(ws=(0x900000, need_r - 1)) == T.UNKNOWN_RECONSTRUCTION
    assert _enc(ws=(None, 1 << 30)) == T.UNKNOWN_CODE_PARAM and _rec(ws=(None, 1 << 30)) == T.UNKNOWN_RECONSTRUCTION
    assert _enc(ws=(0x900010, 1 << 30)) == T.UNKNOWN_CODE_PARAM  # not 256-B aligned
    assert _rec(ws=(0x900080, 1 << 30)) == T.UNKNOWN_RECONSTRUCTION


@pytest.mark.parametrize("nv,enc,rec", [
    (6, "encode_g_ragged", "reconstruct_g_ragged"), (100, "encode_g_ragged", "reconstruct_g_ragged"),
    (765, "encode_g_ragged", "reconstruct_g_ragged"),
    (766, "encode_k256w_ragged", "reconstruct_n1024x_ragged"),
    (1024, "encode_k256w_ragged", "reconstruct_n1024x_ragged"),
    (1025, "encode_g_ragged", "reconstruct_g_ragged"), (5000, "encode_g_ragged", "reconstruct_g_ragged")])
def test_kernel_names(nv, enc, rec):
    assert E.encode_ragged_kernel(nv) == enc and E.reconstruct_ragged_kernel(nv) == rec


def test_kernel_names_invalid():
    for nv in (0, 1, 65537):
        assert E.encode_ragged_kernel(nv) is None and E.reconstruct_ragged_kernel(nv) is None


# ---- ECCR_AMD_ragged_check on a hand-built list: (payload_off, payload_len,
# shard_off, shard_len, shard_stride), and whether the item is valid as an
# encode item (maximum payload length 1000) and as a reconstruct item (maximum
# shard length 64), at n_validators 1024 (k = 256: 1000 bytes -> shard_len 4)
MAX_P, MAX_S = 1000, 64
HAND = [
    # item                          encode reconstruct
    ((0, 1000, 0, 64, 64), True, True),        # 0: length = max on both sides
    ((1024, 15, 16384, 2, 16), True, True),    # 1: a 15-byte payload
    ((2048, 0, 32768, 0, 16), False, False),   # 2: length 0
    ((2048, 1001, 32768, 66, 80), False, False),  # 3: max + 1 (shard_len: max + 2, even)
    ((2048, 700, 32768, 7, 16), True, False),  # 4: odd shard_len (ignored by the encode)
    ((2048, 1000, 32768, 64, 62), False, False),  # 5: shard_stride = shard_len - 2 (and no multiple of 16)
    ((2048, 1000, 32768, 64, 48), True, False),  # 6: a multiple of 16 below shard_len (the encode's own: 4 <= 48)
    ((2048, 1000, 32768, 4, 2), False, False),  # 7: stride below the encode's own shard length (4)
    ((2056, 700, 32768, 8, 16), False, False),  # 8: payload_off off by 8
    ((2048, 700, 32776, 8, 16), False, False),  # 9: shard_off off by 8
    ((2048, 700, 32768, 8, 24), False, False),  # 10: shard_stride off by 8
    ((1 << 40, 513, 1 << 41, 6, 1 << 20), True, True),  # 11: 64-bit offsets, two pieces
]


def _items(rows):
    return np.array(rows, dtype=np.uint64).reshape(-1, 5)


def test_ragged_check_each_item():
    for i, (row, enc_ok, rec_ok) in enumerate(HAND):
        it = _items([row])
        assert E.ragged_check(1024, it, MAX_P, reconstruct=False) == ((0, 0) if enc_ok else (1, 0)), i
        assert E.ragged_check(1024, it, MAX_S, reconstruct=True) == ((0, 0) if rec_ok else (1, 0)), i


def test_ragged_check_counts_and_first_bad_index():
    rows = [r for r, _, _ in HAND]
    bad_enc = [i for i, (_, e, _) in enumerate(HAND) if not e]
    bad_rec = [i for i, (_, _, r) in enumerate(HAND) if not r]
    assert E.ragged_check(1024, _items(rows), MAX_P) == (len(bad_enc), bad_enc[0]) == (7, 2)
    assert E.ragged_check(1024, _items(rows), MAX_S, reconstruct=True) == (len(bad_rec), bad_rec[0]) == (9, 2)
    # the lowest bad index, wherever it is; {0, 0} when there is none
    good = [r for r, e, rr in HAND if e and rr]
    assert E.ragged_check(1024, _items(good), MAX_P) == (0, 0)
    assert E.ragged_check(1024, _items(good + [rows[2]]), MAX_P) == (1, len(good))
    assert E.ragged_check(1024, _items([rows[2]] + good), MAX_P) == (1, 0)
    # a ctypes array of RaggedItem is the same thing
    arr = (E.RaggedItem * 2)(E.RaggedItem(*rows[0]), E.RaggedItem(*rows[8]))
    assert E.ragged_check(1024, arr, MAX_P) == (1, 1)


def test_ragged_check_follows_the_code():
    # the encode's shard length is the code's: k = 2 at n_validators 6 (15 bytes -> 8), so a
    # 16-byte pitch holds a 15-byte payload's shards there and a 300-byte payload's need 160
    assert E.shard_len(6, 300) == 150
    assert E.ragged_check(6, _items([(0, 300, 0, 0, 160)]), 300) == (0, 0)
    assert E.ragged_check(6, _items([(0, 300, 0, 0, 144)]), 300) == (1, 0)
    status = (C.c_uint32 * 2)()
    L = E.lib()
    it = _items([(0, 300, 0, 0, 160)])
    assert T(L.ECCR_AMD_ragged_check(1, it.ctypes.data, 1, 300, 0, C.byref(status)).tag) == T.NOT_ENOUGH_VALIDATORS
    assert T(L.ECCR_AMD_ragged_check(6, None, 1, 300, 0, C.byref(status)).tag) == T.BAD_PAYLOAD
    assert T(L.ECCR_AMD_ragged_check(6, it.ctypes.data, 0, 300, 0, C.byref(status)).tag) == T.BAD_PAYLOAD


def test_ragged_items_helper():
    items, pay_bytes, sh_bytes, out_bytes = E.ragged_items(1024, [15, 512, 100_000], shard_pad=[0, 32, 0])
    assert items.shape == (3, 5) and items.dtype == np.uint64
    assert items[:, 1].tolist() == [15, 512, 100_000] and items[:, 3].tolist() == [2, 2, 392]
    assert items[:, 4].tolist() == [16, 48, 400]
    assert items[:, 2].tolist() == [0, 1024 * 16, 1024 * 64] and sh_bytes == 1024 * (16 + 48 + 400)
    assert items[:, 0].tolist() == [0, 512, 1024] and pay_bytes == out_bytes == 1024 + 392 * 256
    assert E.ragged_check(1024, items, 100_000) == (0, 0)
    assert E.ragged_check(1024, items, 392, reconstruct=True) == (0, 0)
