"""The systematic recovery's dispatch, ragged call and diagnostics (ec_amd.h
ECCR_AMD_systematic_*), what needs no GPU: the symbols, the kernel
ECCR_AMD_systematic_kernel names on both sides of every clause of
choose_systematic, the ragged kernel names, the workspace queries and every
rejection the ragged call makes on the host before it touches a device (the
addresses are made up: a launch would fault)."""
import pytest

import ecc_amd as E

T = E.Tag
NEW_SYMBOLS = ["ECCR_AMD_systematic_batch_ws", "ECCR_AMD_systematic_workspace_bytes", "ECCR_AMD_systematic_kernel",
               "ECCR_AMD_systematic_ragged", "ECCR_AMD_systematic_ragged_ws",
               "ECCR_AMD_systematic_ragged_workspace_bytes", "ECCR_AMD_systematic_ragged_kernel"]
W, G = "systematic_w", "systematic_g"


def test_symbols():
    L = E.lib()
    header = open(E.HEADERS[1]).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in header, name


# made-up addresses: the query dereferences nothing
SH, OUT, ITEMS, ST = 0x100000, 0x900000, 0x1100000, 0x1200000


def _name(nv, sh=SH, slen=64, ss_pad=0, batch=3, out=OUT, os_pad=0):
    k = E.code_params(nv)[1]
    return E.systematic_kernel(nv, sh, slen, 64 + ss_pad, batch, out, slen * k + os_pad)


def test_kernel_each_clause():
    assert E.code_params(45)[1] == 8 and E.code_params(46)[1] == 16
    # k >= 16
    assert _name(45) == G and _name(46) == W
    for nv in (46, 100, 1024, 1025, 5000, 40000):
        assert _name(nv) == W, nv
        # shard base, shard pitch, out base on 16 B
        assert _name(nv, sh=SH + 8) == G and _name(nv, ss_pad=8) == G and _name(nv, out=OUT + 8) == G, nv
        assert _name(nv, ss_pad=16) == W and _name(nv, os_pad=16) == W, nv
        # the out pitch only where it is applied
        assert _name(nv, os_pad=8, batch=2) == G and _name(nv, os_pad=8, batch=1) == W, nv
    for nv in (2, 6, 45):  # k < 16 whatever the layout
        assert _name(nv) == G and _name(nv, batch=1) == G, nv
    # an odd shard_len argument counts whole symbols
    assert _name(1024, slen=65, ss_pad=16) == W


def test_kernel_invalid_arguments():
    k = 256
    assert E.systematic_kernel(0, SH, 64, 64, 3, OUT, 64 * k) is None
    assert E.systematic_kernel(65537, SH, 64, 64, 3, OUT, 64 * k) is None
    assert E.systematic_kernel(1024, SH, 64, 64, 0, OUT, 64 * k) is None  # an empty batch
    assert E.systematic_kernel(1024, SH, 1, 64, 3, OUT, 64 * k) is None  # no whole symbol
    assert E.systematic_kernel(1024, SH, 64, 62, 3, OUT, 64 * k) is None  # pitch below the length
    assert E.systematic_kernel(1024, SH, 64, 64, 3, OUT, 64 * k - 2) is None  # out pitch below the output


@pytest.mark.parametrize("nv,name", [(6, "systematic_g_ragged"), (45, "systematic_g_ragged"),
                                     (46, "systematic_w_ragged"), (1024, "systematic_w_ragged"),
                                     (40000, "systematic_w_ragged")])
def test_ragged_kernel_names(nv, name):
    assert E.systematic_ragged_kernel(nv) == name


def test_ragged_kernel_name_invalid():
    for nv in (0, 1, 65537):
        assert E.systematic_ragged_kernel(nv) is None


@pytest.mark.parametrize("nv", [6, 45, 46, 1024, 5000, 40000])
def test_workspace_queries(nv):
    q = E.systematic_ragged_workspace_bytes
    assert q(nv, 1, 2) >= 512 and q(nv, 1, 2) % 256 == 0
    assert q(nv, 100_000, 2) >= 400_000  # 4 bytes per item of the plan
    sizes = [[q(nv, b, m) for m in (2, 1000, 1_000_000, 10_000_000)] for b in (1, 2, 97, 4096, 100_000)]
    for row in sizes:  # monotone in the maximum
        assert row == sorted(row), (nv, row)
    for col in zip(*sizes):  # monotone in the batch
        assert list(col) == sorted(col), (nv, col)
    assert q(nv, 0, 1000) == 0 and q(nv, 1 << 31, 1000) == 0 and q(nv, 3, 0) == 0
    u = E.systematic_workspace_bytes
    if E.code_params(nv)[1] >= 16:  # systematic_w's tile counter
        assert u(nv, 64, 3) > 0 and u(nv, 64, 3) % 256 == 0
    sizes = [[u(nv, m, b) for m in (2, 1000, 1_000_000)] for b in (1, 97, 4096)]
    for row in sizes + [list(c) for c in zip(*sizes)]:
        assert row == sorted(row), (nv, row)
    assert u(nv, 0, 3) == 0 and u(nv, 1, 3) == 0 and u(nv, 64, 0) == 0


def test_workspace_queries_invalid_nv():
    for bad_nv in (0, 1, 65537):
        assert E.systematic_ragged_workspace_bytes(bad_nv, 3, 1000) == 0
        assert E.systematic_workspace_bytes(bad_nv, 64, 3) == 0


def _rag(nv=1024, sh=SH, items=ITEMS, batch=4, mx=1000, out=OUT, st=ST, ws=None):
    L = E.lib()
    if ws is None:
        return T(L.ECCR_AMD_systematic_ragged(nv, sh, items, batch, mx, out, st, None).tag)
    return T(L.ECCR_AMD_systematic_ragged_ws(nv, sh, items, batch, mx, out, st, ws[0], ws[1], None).tag)


@pytest.mark.parametrize("nv", [6, 1024, 5000])
@pytest.mark.parametrize("ws", [None, (0x2000000, 1 << 30)], ids=["plain", "ws"])
def test_ragged_host_rejections_need_no_device(nv, ws):
    assert _rag(nv=1, ws=ws) == T.NOT_ENOUGH_VALIDATORS and _rag(nv=65537, ws=ws) == T.TOO_MANY_VALIDATORS
    # a NULL buffer
    for key in ("sh", "items", "out"):
        assert _rag(nv=nv, ws=ws, **{key: None}) == T.BAD_PAYLOAD and "NULL" in E.last_error(), key
    # a misaligned buffer
    assert _rag(nv=nv, sh=SH + 8, ws=ws) == T.BAD_PAYLOAD and "aligned" in E.last_error()
    assert _rag(nv=nv, out=OUT + 8, ws=ws) == T.BAD_PAYLOAD
    assert _rag(nv=nv, items=ITEMS + 4, ws=ws) == T.BAD_PAYLOAD and _rag(nv=nv, st=ST + 2, ws=ws) == T.BAD_PAYLOAD
    # batch 0 and 2^31
    assert _rag(nv=nv, batch=0, ws=ws) == T.BAD_PAYLOAD and "batch" in E.last_error()
    assert _rag(nv=nv, batch=1 << 31, ws=ws) == T.BAD_PAYLOAD
    # a maximum of 0
    assert _rag(nv=nv, mx=0, ws=ws) == T.NON_UNIFORM_CHUNKS and "maximum" in E.last_error()
    # more tiles than the 32-bit tickets hold
    assert _rag(nv=nv, batch=1 << 20, mx=1 << 40, ws=ws) == T.BAD_PAYLOAD and "2^32" in E.last_error()


def test_ragged_ticket_bound_counts_row_blocks():
    # k = 1024 (n_validators 5000): 64-column tiles in 4 row blocks each, so 2^18 items of
    # 2^12 column tiles reach 2^32 tickets; at k = 256 the same batch is 2^30 tickets
    assert E.code_params(5000)[1] == 1024
    ws = (0x2000000, 1 << 40)
    assert _rag(nv=5000, batch=1 << 18, mx=(1 << 12) * 64 * 2, ws=ws) == T.BAD_PAYLOAD and "2^32" in E.last_error()
    assert _rag(nv=5000, batch=1 << 18, mx=(1 << 12) * 64 * 2, ws=(0x2000000, 16)) == T.BAD_PAYLOAD
    need = E.systematic_ragged_workspace_bytes(1024, 1 << 18, (1 << 12) * 64 * 2)
    assert _rag(nv=1024, batch=1 << 18, mx=(1 << 12) * 64 * 2, ws=(0x2000000, need - 1)) == T.UNKNOWN_RECONSTRUCTION


def test_ragged_workspace_rejections_need_no_device():
    for nv in (6, 1024):
        need = E.systematic_ragged_workspace_bytes(nv, 4, 1000)
        assert _rag(nv=nv, ws=(0x2000000, need - 1)) == T.UNKNOWN_RECONSTRUCTION and "workspace" in E.last_error()
        assert _rag(nv=nv, ws=(None, 1 << 30)) == T.UNKNOWN_RECONSTRUCTION
        assert _rag(nv=nv, ws=(0x2000010, 1 << 30)) == T.UNKNOWN_RECONSTRUCTION  # not 256-B aligned
