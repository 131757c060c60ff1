"""Ragged device batches on the GPU (ECCR_AMD_encode_ragged /
ECCR_AMD_reconstruct_ragged and their _ws forms): every item of every batch
byte for byte against the oracle, items built to break the contract checked to
be untouched instead, and -- every buffer being carved out of one arena of
seeded noise (tests/layout_cases.py) -- nothing changed but the bytes the API
may write: row padding, the gaps between items, the guards, every input.

An encode case runs in one arena; its reconstruct runs in a second one whose
shard rows are the oracle's (the encode's were just checked against them),
absent rows left as noise.  Oracle results are computed once per distinct
(n_validators, length[, pattern]) and shared."""
import numpy as np
import pytest

import ecc_amd as E  # imports torch first
import layout_cases as L
import synth

pytestmark = pytest.mark.gpu
T = E.Tag


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()


def up16(x):
    return (x + 15) // 16 * 16


# ---- references ------------------------------------------------------------
_ENC, _PAT, _REC = {}, {}, {}


def ref_encode(oracle, nv, plen):
    """payload and its reference shard rows [nv][shard_len]"""
    if (nv, plen) not in _ENC:
        pay = synth.payload(7000 + nv + plen, plen)
        rows = np.frombuffer(b"".join(oracle.encode(nv, pay.tobytes())), np.uint8).reshape(nv, -1).copy()
        assert rows.shape[1] == E.shard_len(nv, plen)
        pay.setflags(write=False)
        rows.setflags(write=False)
        _ENC[(nv, plen)] = (pay, rows)
    return _ENC[(nv, plen)]


def pattern(oracle, nv, kind):
    """kind 0: a random threshold set; 1: every systematic row + parity up to the
    threshold; 2: a random set of exactly k rows; "P1" / "P2": the top and edge
    patterns of tests/nv_boundaries.py (P1 sets the flags of rows >= nv too, which
    stay erased: the locator is the one of the rows below nv).
    -> (present [n], locator mod 65535)"""
    if (nv, kind) not in _PAT:
        n, k, thr = E.code_params(nv)
        if kind in ("P1", "P2"):
            import nv_boundaries
            m = nv_boundaries.present(nv, kind)
        elif kind == 1:
            m = np.zeros(n, np.uint8)
            m[:k] = 1
            m[k + synth.present_set(10**6 + nv + 1, nv - k, thr - k)] = 1
        else:
            m = synth.present_mask(10**6 + nv + kind, nv, thr if kind == 0 else k, n)
        erased = m == 0
        erased[nv:] = True
        el = oracle.error_poly(erased.astype(np.uint8), n)[:n].astype(np.int64) % 65535
        m.setflags(write=False)
        _PAT[(nv, kind)] = (m, el)
    return _PAT[(nv, kind)]


def ref_reconstruct(oracle, nv, plen, kind):
    if (nv, plen, kind) not in _REC:
        pay, rows = ref_encode(oracle, nv, plen)
        m, _ = pattern(oracle, nv, kind)
        out = oracle.reconstruct(nv, [rows[i].tobytes() if m[i] else None for i in range(nv)])
        assert out[:plen] == pay.tobytes()
        _REC[(nv, plen, kind)] = np.frombuffer(out, np.uint8)
    return _REC[(nv, plen, kind)]


# ---- a batch: items of (payload length, pattern kind, pitch padding, defect) ----
class Item:
    def __init__(self, plen, kind=0, pad=0, bad=None):
        self.plen, self.kind, self.pad, self.bad = plen, kind, pad, bad


def layout(nv, items, gap=True):
    """offsets of every item's payload, shard rows and output, regions 16-B
    aligned with gaps of noise between them; -> per-item dicts and the three sizes"""
    _, k, _ = E.code_params(nv)
    lay, p, s, o = [], 0, 0, 0
    for i, it in enumerate(items):
        sl = E.shard_len(nv, it.plen)
        ss = up16(sl) + it.pad
        lay.append(dict(p=p, s=s, o=o, sl=sl, ss=ss))
        g = 16 * (1 + i % 3) if gap else 0
        p += up16(it.plen) + g
        s += nv * ss + g
        o += up16(sl * k) + g
    return lay, p, s, o


def item_rows(nv, items, lay, reconstruct, max_len):
    """the uint64 [batch][5] item array, defects applied"""
    a = np.zeros((len(items), 5), np.uint64)
    for i, (it, l) in enumerate(zip(items, lay)):
        a[i] = (l["o"] if reconstruct else l["p"], it.plen, l["s"], l["sl"], l["ss"])
        if it.bad == "len0":
            a[i, 3 if reconstruct else 1] = 0
        elif it.bad == "toolong":
            a[i, 3 if reconstruct else 1] = max_len + (2 if reconstruct else 1)
        elif it.bad == "shard_off+8":
            a[i, 2] += 8
        else:
            assert it.bad is None
    return a


def upload(arena):
    import torch
    dev = torch.from_numpy(arena.host).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev, dev.data_ptr()


def download(dev):
    import torch
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def strided(buf, base, rows, stride, used):
    return np.lib.stride_tricks.as_strided(buf[base:], (rows, used), (stride, 1))


def run_encode(oracle, nv, items, ws=False, ws_short=0, seed=1, gap=True, expect=T.OK, max_plen=None):
    """one ragged encode in an arena; checks shards, status and the arena"""
    B = len(items)
    lay, pbytes, sbytes, _ = layout(nv, items, gap)
    good = [i for i, it in enumerate(items) if it.bad is None]
    max_plen = max_plen or max(items[i].plen for i in good)
    need = E.ragged_workspace_bytes(nv, B, max_plen)[0]
    A = L.Arena(seed=seed * 7919 + nv)
    a_pay, a_sh = A.add("payloads", pbytes), A.add("shards", sbytes)
    a_it, a_st = A.add("items", B * 40), A.add("status", 8)
    a_ws = A.add("workspace", need - ws_short) if ws else None
    host = A.build()
    for it, l in zip(items, lay):
        host[a_pay + l["p"]: a_pay + l["p"] + it.plen] = ref_encode(oracle, nv, it.plen)[0]
    host[a_it: a_it + B * 40] = item_rows(nv, items, lay, False, max_plen).view(np.uint8).reshape(-1)
    if expect == T.OK:
        for i in good:
            A.allow_rows(a_sh + lay[i]["s"], nv, lay[i]["ss"], lay[i]["sl"])
        A.allow(a_st, 8)
        if ws:
            A.allow(a_ws, need)
    dev, base = upload(A)
    L_ = E.lib()
    if ws:
        r = L_.ECCR_AMD_encode_ragged_ws(nv, base + a_pay, base + a_it, B, max_plen, base + a_sh, base + a_st,
                                         base + a_ws, need - ws_short, E._stream(None))
    else:
        r = L_.ECCR_AMD_encode_ragged(nv, base + a_pay, base + a_it, B, max_plen, base + a_sh, base + a_st,
                                      E._stream(None))
    got = download(dev)
    assert T(r.tag) == expect, E.last_error()
    if expect == T.OK:
        for i in good:
            rows = strided(got, a_sh + lay[i]["s"], nv, lay[i]["ss"], lay[i]["sl"])
            assert np.array_equal(rows, ref_encode(oracle, nv, items[i].plen)[1]), (nv, i, items[i].plen)
        bad = [i for i in range(B) if i not in good]
        assert got[a_st: a_st + 8].view(np.uint32).tolist() == [len(bad), bad[0] if bad else 0]
    assert A.violations(got) == []
    return got, A, dict(pay=a_pay, sh=a_sh, lay=lay)


def run_reconstruct(oracle, nv, items, ws=False, ws_short=0, seed=2, gap=True, expect=T.OK, shared=None):
    """locator + one ragged reconstruct in an arena.  shared: the pattern rows
    (kinds) every item's d_pattern entry picks from, item i using row i % len(shared)"""
    n, k, _ = E.code_params(nv)
    B = len(items)
    lay, _, sbytes, obytes = layout(nv, items, gap)
    good = [i for i, it in enumerate(items) if it.bad is None]
    max_slen = max(lay[i]["sl"] for i in good)
    need = int(E.lib().ECCR_AMD_reconstruct_ragged_workspace_bytes(nv, B, max_slen))
    kinds = [shared[i % len(shared)] for i in range(B)] if shared else [it.kind for it in items]
    rows_pr = len(shared) if shared else B
    A = L.Arena(seed=seed * 7919 + nv)
    a_sh, a_pr, a_el = A.add("shards", sbytes), A.add("present", B * n), A.add("err_log", B * n * 2)
    a_out, a_it, a_st = A.add("out", obytes), A.add("items", B * 40), A.add("status", 8)
    a_pat = A.add("pattern", B * 4) if shared else None
    a_ws = A.add("workspace", need - ws_short) if ws else None
    host = A.build()
    for r in range(rows_pr):
        host[a_pr + r * n: a_pr + (r + 1) * n] = pattern(oracle, nv, shared[r] if shared else kinds[r])[0]
    for i, (it, l) in enumerate(zip(items, lay)):
        m = pattern(oracle, nv, kinds[i])[0][:nv].astype(bool)
        view = strided(host, a_sh + l["s"], nv, l["ss"], l["sl"])
        view[m] = ref_encode(oracle, nv, it.plen)[1][m]  # absent rows keep the noise
    host[a_it: a_it + B * 40] = item_rows(nv, items, lay, True, max_slen).view(np.uint8).reshape(-1)
    if shared:
        host[a_pat: a_pat + B * 4] = (np.arange(B, dtype=np.uint32) % len(shared)).view(np.uint8)
    A.allow(a_el, rows_pr * n * 2)  # (written by the locator call in either case)
    if expect == T.OK:
        for i in good:
            A.allow(a_out + lay[i]["o"], lay[i]["sl"] * k)
        A.allow(a_st, 8)
        if ws:
            A.allow(a_ws, need)
    dev, base = upload(A)
    E.error_locator(nv, base + a_pr, rows_pr, base + a_el)
    L_ = E.lib()
    pat = base + a_pat if shared else None
    if ws:
        r = L_.ECCR_AMD_reconstruct_ragged_ws(nv, base + a_sh, base + a_it, base + a_pr, base + a_el, pat, B,
                                              max_slen, base + a_out, base + a_st, base + a_ws, need - ws_short,
                                              E._stream(None))
    else:
        r = L_.ECCR_AMD_reconstruct_ragged(nv, base + a_sh, base + a_it, base + a_pr, base + a_el, pat, B,
                                           max_slen, base + a_out, base + a_st, E._stream(None))
    got = download(dev)
    assert T(r.tag) == expect, E.last_error()
    if expect == T.OK:
        for i in good:
            ref = ref_reconstruct(oracle, nv, items[i].plen, kinds[i])
            o = a_out + lay[i]["o"]
            assert np.array_equal(got[o: o + len(ref)], ref), (nv, i, items[i].plen)
            assert len(ref) == lay[i]["sl"] * k
        bad = [i for i in range(B) if i not in good]
        assert got[a_st: a_st + 8].view(np.uint32).tolist() == [len(bad), bad[0] if bad else 0]
    assert A.violations(got) == []
    return got, A, dict(sh=a_sh, out=a_out, lay=lay)


# ---- n_validators 766 .. 1024: 512-byte pieces, 64-piece / 64-column tiles ----
def mix9():
    """pieces 1 (15 B), 1 (512 B), 63, 64, 65, 129 (odd tail), 8, 4, 5, interleaved;
    a different pattern kind per item; tight and padded pitches"""
    plens = [15, 65 * 512, 512, 129 * 512 - 77, 8 * 512, 63 * 512, 4 * 512, 64 * 512, 5 * 512]
    return [Item(p, kind=i % 3, pad=48 if i % 2 else 0) for i, p in enumerate(plens)]


@pytest.mark.parametrize("nv", [1024, 800, 768])
def test_mixed_sizes(oracle, nv):
    assert E.encode_ragged_kernel(nv) == "encode_k256w_ragged"
    assert E.reconstruct_ragged_kernel(nv) == "reconstruct_n1024x_ragged"
    run_encode(oracle, nv, mix9())
    run_reconstruct(oracle, nv, mix9())


def test_shared_patterns(oracle):
    # two pattern rows for nine items, through d_pattern
    run_reconstruct(oracle, 1024, mix9(), shared=[2, 0])


def many():
    """540 items cycling five lengths of 1, 2, 2, 3 and 3 tiles: 1188 tiles, more
    than the encode's 2 x 256 and the reconstruct's 256 workgroups, so that one
    workgroup runs tiles of several different items"""
    pieces = [40, 65, 100, 129, 150]
    items = [Item(pieces[i % 5] * 512 - (i % 5) * 3, kind=(i % 5) % 3, pad=16 * (i % 2)) for i in range(540)]
    tiles = sum((E.shard_len(1024, it.plen) // 2 + 63) // 64 for it in items)
    assert tiles >= 1100
    return items


def test_more_tiles_than_workgroups_encode(oracle):
    run_encode(oracle, 1024, many(), gap=False)


def test_more_tiles_than_workgroups_reconstruct(oracle):
    run_reconstruct(oracle, 1024, many(), gap=False)


@pytest.mark.parametrize("nv,plen", [(1024, 70_001), (100, 20_001)])
def test_equal_lengths_match_the_uniform_calls(oracle, nv, plen):
    """a ragged batch laid out as a uniform one: the same bytes as
    ECCR_AMD_encode_batch / ECCR_AMD_reconstruct_batch write into the same arena"""
    import torch
    n, k, _ = E.code_params(nv)
    B, sl = 3, E.shard_len(nv, plen)
    ps, ss, os_ = up16(plen) + 16, up16(sl) + 32, up16(sl * k) + 16
    items = np.array([(b * ps, plen, b * nv * ss, sl, ss) for b in range(B)], np.uint64)
    A = L.Arena(seed=nv + plen)
    a_pay, a_sh, a_it = A.add("payloads", B * ps), A.add("shards", B * nv * ss), A.add("items", B * 40)
    a_pr, a_el, a_out, a_ito = A.add("present", B * n), A.add("err_log", B * n * 2), A.add("out", B * os_), A.add(
        "items_out", B * 40)
    host = A.build()
    pay, rows = ref_encode(oracle, nv, plen)
    for b in range(B):
        host[a_pay + b * ps: a_pay + b * ps + plen] = pay
        host[a_pr + b * n: a_pr + (b + 1) * n] = pattern(oracle, nv, b)[0]
    host[a_it: a_it + B * 40] = items.view(np.uint8).reshape(-1)
    items[:, 0] = [b * os_ for b in range(B)]
    host[a_ito: a_ito + B * 40] = items.view(np.uint8).reshape(-1)
    A.allow_rows(a_sh, B * nv, ss, sl)
    A.allow(a_el, B * n * 2)
    A.allow_rows(a_out, B, os_, sl * k)
    dev_r, br = upload(A)
    dev_u = torch.from_numpy(A.host).cuda()
    bu = dev_u.data_ptr()
    E.encode_ragged(nv, br + a_pay, br + a_it, B, plen, br + a_sh)
    E.encode_batch(nv, bu + a_pay, plen, ps, B, bu + a_sh, ss)
    for base, ragged in ((br, True), (bu, False)):
        E.error_locator(nv, base + a_pr, B, base + a_el)
        if ragged:
            E.reconstruct_ragged(nv, base + a_sh, base + a_ito, base + a_pr, base + a_el, B, sl, base + a_out)
        else:
            E.reconstruct_batch(nv, base + a_sh, sl, ss, base + a_pr, base + a_el, B, base + a_out, os_)
    got_r, got_u = download(dev_r), download(dev_u)
    assert np.array_equal(got_r, got_u)
    for b in range(B):
        assert np.array_equal(strided(got_r, a_sh + b * nv * ss, nv, ss, sl), rows)
        assert np.array_equal(got_r[a_out + b * os_:][:sl * k], ref_reconstruct(oracle, nv, plen, b))
    assert A.violations(got_r) == []


@pytest.mark.parametrize("nv", [1024, 100])
def test_invalid_items_among_valid_ones(oracle, nv):
    """length 0, a misaligned shard_off, a length above the maximum: those
    items' regions keep the arena's noise, the others are bit-exact, d_status =
    {3, lowest index}; an all-valid call afterwards gives {0, 0} (run_* checks both)"""
    unit = 512 if nv == 1024 else 64
    items = [Item(3 * unit), Item(70 * unit, kind=1, bad="len0"), Item(65 * unit + 5, kind=2),
             Item(9 * unit, bad="shard_off+8"), Item(unit, kind=1), Item(20 * unit, bad="toolong"),
             Item(130 * unit - 9, kind=2, pad=32)]
    run_encode(oracle, nv, items)
    run_reconstruct(oracle, nv, items)
    run_encode(oracle, nv, [it for it in items if it.bad is None])
    run_reconstruct(oracle, nv, [it for it in items if it.bad is None])


def test_offsets_above_4g(oracle):
    """two small items, one with payload_off, shard_off and the output offset
    above 2^32, in buffers that are allocated but not initialised beyond the items"""
    import torch
    nv = 1024
    n, k, _ = E.code_params(nv)
    plens, hi = [70 * 512 + 3, 5 * 512], (1 << 32) + 4096
    sls = [E.shard_len(nv, p) for p in plens]
    sss = [up16(s) + 16 for s in sls]
    offs = dict(p=[256, hi], s=[512, hi + 16], o=[1024, hi + 32])
    d_pay = torch.empty(hi + up16(plens[1]) + 256, dtype=torch.uint8, device="cuda")
    d_sh = torch.empty(hi + 16 + nv * sss[1] + 256, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(hi + 32 + sls[1] * k + 256, dtype=torch.uint8, device="cuda")
    for t in (d_pay, d_sh, d_out):
        assert t.data_ptr() % 16 == 0
    enc = np.array([(offs["p"][i], plens[i], offs["s"][i], 0, sss[i]) for i in range(2)], np.uint64)
    rec = np.array([(offs["o"][i], 0, offs["s"][i], sls[i], sss[i]) for i in range(2)], np.uint64)
    d_enc, d_rec = torch.from_numpy(enc.view(np.int64)).cuda(), torch.from_numpy(rec.view(np.int64)).cuda()
    d_st = torch.full((2,), 99, dtype=torch.int32, device="cuda")
    pres = np.stack([pattern(oracle, nv, i)[0] for i in range(2)])
    d_pr = torch.from_numpy(pres).cuda()
    d_el = torch.empty((2, n), dtype=torch.int16, device="cuda")
    for i in range(2):
        d_pay[offs["p"][i]: offs["p"][i] + plens[i]] = torch.from_numpy(ref_encode(oracle, nv, plens[i])[0].copy()).cuda()
        d_sh[offs["s"][i] - 64: offs["s"][i] + nv * sss[i] + 64] = 0x5A
        d_out[offs["o"][i] - 64: offs["o"][i] + sls[i] * k + 64] = 0xA5
    E.encode_ragged(nv, d_pay, d_enc, 2, max(plens), d_sh, d_status=d_st)
    torch.cuda.synchronize()
    assert d_st.tolist() == [0, 0]
    for i in range(2):
        blk = d_sh[offs["s"][i] - 64: offs["s"][i] + nv * sss[i] + 64].cpu().numpy()
        assert np.array_equal(strided(blk, 64, nv, sss[i], sls[i]), ref_encode(oracle, nv, plens[i])[1]), i
        pad = strided(blk, 64 + sls[i], nv, sss[i], sss[i] - sls[i])
        assert (pad[:-1] == 0x5A).all() and (blk[:64] == 0x5A).all() and (blk[-64:] == 0x5A).all(), i
    E.error_locator(nv, d_pr, 2, d_el)
    E.reconstruct_ragged(nv, d_sh, d_rec, d_pr, d_el, 2, max(sls), d_out, d_status=d_st)
    torch.cuda.synchronize()
    assert d_st.tolist() == [0, 0]
    for i in range(2):
        blk = d_out[offs["o"][i] - 64: offs["o"][i] + sls[i] * k + 64].cpu().numpy()
        assert np.array_equal(blk[64:-64], ref_reconstruct(oracle, nv, plens[i], i)), i
        assert (blk[:64] == 0xA5).all() and (blk[-64:] == 0xA5).all(), i


# ---- the generic kernels: every other n_validators ---------------------------
@pytest.mark.parametrize("nv,plens", [
    (6, [15, 300, 5000]),  # the reference's own shape; 4-byte pieces, 256 a block
    (100, [255 * 64, 1, 256 * 64, 257 * 64 - 3, 128 * 64 + 2, 129 * 64]),  # blocks of 256 pieces / 128 positions
    (2000, [31 * 1024, 32 * 1024, 33 * 1024 - 1, 8 * 1024, 9 * 1024, 7]),  # 32 pieces / 8 positions
    (5000, [3 * 2048, 4 * 2048, 5 * 2048 + 1, 16 * 2048, 17 * 2048]),  # n = 8192: global scratch; 16 / 4
], ids=lambda v: str(v) if isinstance(v, int) else None)
def test_generic_path(oracle, nv, plens):
    assert E.encode_ragged_kernel(nv) == "encode_g_ragged" and E.reconstruct_ragged_kernel(nv) == "reconstruct_g_ragged"
    items = [Item(p, kind=i % 3, pad=16 * (i % 2)) for i, p in enumerate(plens)]
    run_encode(oracle, nv, items, ws=(nv == 5000))
    run_reconstruct(oracle, nv, items, ws=(nv == 5000))


# ---- workspace and graph ------------------------------------------------------
@pytest.mark.parametrize("nv", [1024, 5000])
def test_workspace_exact_and_one_byte_short(oracle, nv):
    unit = 512 if nv == 1024 else 2048
    items = [Item(3 * unit), Item(70 * unit + 1, kind=1), Item(unit // 2, kind=2)]
    run_encode(oracle, nv, items, ws=True)
    run_reconstruct(oracle, nv, items, ws=True)
    # one byte less: UNKNOWN_*, nothing launched, the arena unchanged (nothing is allowed)
    run_encode(oracle, nv, items, ws=True, ws_short=1, expect=T.UNKNOWN_CODE_PARAM)
    run_reconstruct(oracle, nv, items, ws=True, ws_short=1, expect=T.UNKNOWN_RECONSTRUCTION)


@pytest.mark.parametrize("nv", [1024, 100])
def test_batch_of_one(oracle, nv):
    for plen in (15, 40_001):
        run_encode(oracle, nv, [Item(plen, kind=1)])
        run_reconstruct(oracle, nv, [Item(plen, kind=2)])


def test_graph_replay_with_changed_items(oracle):
    """encode_ws -> locator_ws -> reconstruct_ws captured once on one stream and
    replayed twice, the item array's contents (lengths, offsets, pitches: same
    batch and maxima) changed between the replays: a plan or counter that is
    not rebuilt on replay gives the second replay the first one's geometry"""
    import torch
    nv = 1024
    n, k, _ = E.code_params(nv)
    sets = [[Item(70 * 512 + 1, 0), Item(15, 1), Item(129 * 512, 2, pad=16), Item(5 * 512, 0)],
            [Item(4 * 512, 1, pad=32), Item(129 * 512, 2), Item(64 * 512, 0), Item(65 * 512 - 2, 1)]]
    B, max_plen = 4, 129 * 512
    max_slen = E.shard_len(nv, max_plen)
    lays = [layout(nv, s) for s in sets]
    pbytes, sbytes, obytes = (max(l[j] for l in lays) for j in (1, 2, 3))
    need = max(E.ragged_workspace_bytes(nv, B, max_plen) + (E.workspace_bytes(nv, max_plen, B)[1],))

    def arena(r):
        A = L.Arena(seed=31 + r)
        a = dict(pay=A.add("payloads", pbytes), sh=A.add("shards", sbytes), pr=A.add("present", B * n),
                 el=A.add("err_log", B * n * 2), out=A.add("out", obytes), ie=A.add("items_enc", B * 40),
                 ir=A.add("items_rec", B * 40), st=A.add("status", 16), ws=A.add("workspace", need))
        host = A.build()
        lay = lays[r][0]
        for i, (it, l) in enumerate(zip(sets[r], lay)):
            host[a["pay"] + l["p"]: a["pay"] + l["p"] + it.plen] = ref_encode(oracle, nv, it.plen)[0]
            host[a["pr"] + i * n: a["pr"] + (i + 1) * n] = pattern(oracle, nv, it.kind)[0]
            A.allow_rows(a["sh"] + l["s"], nv, l["ss"], l["sl"])
            A.allow(a["out"] + l["o"], l["sl"] * k)
        host[a["ie"]: a["ie"] + B * 40] = item_rows(nv, sets[r], lay, False, max_plen).view(np.uint8).reshape(-1)
        host[a["ir"]: a["ir"] + B * 40] = item_rows(nv, sets[r], lay, True, max_slen).view(np.uint8).reshape(-1)
        for name, nbytes in (("el", B * n * 2), ("st", 16), ("ws", need)):
            A.allow(a[name], nbytes)
        return A, a

    arenas = [arena(0), arena(1)]
    assert arenas[0][1] == arenas[1][1] and arenas[0][0].size == arenas[1][0].size
    a = arenas[0][1]
    dev, base = upload(arenas[0][0])
    ws = dev[a["ws"]: a["ws"] + need]

    def step():
        E.encode_ragged(nv, base + a["pay"], base + a["ie"], B, max_plen, base + a["sh"], d_status=base + a["st"], ws=ws)
        E.error_locator_ws(nv, base + a["pr"], B, base + a["el"], ws)
        E.reconstruct_ragged(nv, base + a["sh"], base + a["ir"], base + a["pr"], base + a["el"], B, max_slen,
                             base + a["out"], d_status=base + a["st"] + 8, ws=ws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # outside capture: kernel attributes, tables
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    for r in (1, 0):
        A, _ = arenas[r]
        dev.copy_(torch.from_numpy(A.host))
        g.replay()
        got = download(dev)
        for i, (it, l) in enumerate(zip(sets[r], lays[r][0])):
            rows = strided(got, a["sh"] + l["s"], nv, l["ss"], l["sl"])
            assert np.array_equal(rows, ref_encode(oracle, nv, it.plen)[1]), (r, i)
            ref = ref_reconstruct(oracle, nv, it.plen, it.kind)
            assert np.array_equal(got[a["out"] + l["o"]:][:len(ref)], ref), (r, i)
        assert got[a["st"]: a["st"] + 16].view(np.uint32).tolist() == [0, 0, 0, 0]
        assert A.violations(got) == []
