"""The systematic recovery on the GPU (ECCR_AMD_systematic_batch / _ws,
ECCR_AMD_systematic_ragged / _ws and the per-call ABI), byte for byte against
the oracle's reconstruct_from_systematic, every buffer carved out of one arena
of seeded noise (tests/layout_cases.py): nothing may change but the
shard_len * k output bytes of each payload -- not the row padding, the gaps,
the guards or any input.

The reference accepts arbitrary rows, so the k data rows are seeded noise (no
encode); rows y >= k keep the arena's noise and must not matter.  References
are computed once per (n_validators, columns) and shared."""
import numpy as np
import pytest

import ecc_amd as E  # imports torch first
import layout_cases as L

pytestmark = pytest.mark.gpu
T = E.Tag


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()


def up16(x):
    return (x + 15) // 16 * 16


def tile_cols(nv):
    """columns per tile of systematic_w: 16384 / min(k, 256)"""
    return 16384 // min(E.code_params(nv)[1], 256)


_REF = {}


def ref_rows(oracle, nv, cols, which=0):
    """k seeded rows of `cols` symbols and the reference's interleave of them"""
    key = (nv, cols, which)
    if key not in _REF:
        k = E.code_params(nv)[1]
        rows = np.random.default_rng(5000 + nv * 7 + cols * 3 + which).integers(0, 256, (k, 2 * cols), dtype=np.uint8)
        out = np.frombuffer(oracle.reconstruct_from_systematic(nv, [r.tobytes() for r in rows]), np.uint8)
        assert len(out) == 2 * cols * k
        rows.setflags(write=False)
        _REF[key] = (rows, out)
    return _REF[key]


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


# ---- the uniform call ----------------------------------------------------------
# "ws-misaligned": a workspace large enough but off the 256-B alignment runs the
# static schedule like a NULL or short one (no error, the workspace untouched)
FORMS = ["plain", "ws", "ws-null", "ws-misaligned"]


def run_uniform(oracle, nv, cols, pad, expect, sh_off=0, out_off=0, ss_odd=0, os_odd=0, batch=3, forms=FORMS):
    """one arena with the rows of `batch` payloads and one output region per
    form of the call; checks the kernel name, the bytes and the arena"""
    k = E.code_params(nv)[1]
    sl = 2 * cols
    ss, os_ = up16(sl) + pad + ss_odd, sl * k + (16 if pad else 0) + os_odd
    need = E.systematic_workspace_bytes(nv, sl, batch)
    A = L.Arena(seed=nv * 31 + cols)
    a_sh = A.add("shards", batch * nv * ss, sh_off)
    a_out = {f: A.add("out-" + f, batch * os_, out_off) for f in forms}
    a_ws = A.add("workspace", max(need, 256) + 128)  # (+ 128: the misaligned form's slice)
    host = A.build()
    for b in range(batch):
        strided(host, a_sh + b * nv * ss, k, ss, sl)[:] = ref_rows(oracle, nv, cols, b % 3)[0]
    for f in forms:
        A.allow_rows(a_out[f], batch, os_, sl * k)
    A.allow(a_ws, max(need, 256))
    dev, base = upload(A)
    for f in forms:
        args = (nv, base + a_sh, sl, ss, batch, base + a_out[f], os_)
        assert E.systematic_kernel(*args) == expect, (f, E.systematic_kernel(*args))
        if f == "plain":
            E.systematic_batch(*args)
        else:
            off = {"ws": 0, "ws-misaligned": 128}.get(f)
            E.systematic_batch_ws(*args, dev[a_ws + off: a_ws + off + need] if off is not None and need else None)
    got = download(dev)
    for f in forms:
        for b in range(batch):
            o = a_out[f] + b * os_
            assert np.array_equal(got[o: o + sl * k], ref_rows(oracle, nv, cols, b % 3)[1]), (f, b)
    assert A.violations(got) == []


UNIFORM_NV = [46, 100, 600, 1024, 1025, 1534, 4096, 5000, 12289]
UNIFORM_K = [16, 32, 128, 256, 256, 512, 1024, 1024, 4096]


def col_counts(nv):
    c = tile_cols(nv)
    return [1, c - 1, c, c + 1, 2 * c + 3, 9]  # 9 columns: a shard length = 2 mod 16


def test_uniform_shapes_are_the_intended_ones():
    assert [E.code_params(nv)[1] for nv in UNIFORM_NV] == UNIFORM_K
    assert [tile_cols(nv) for nv in UNIFORM_NV] == [1024, 512, 128, 64, 64, 64, 64, 64, 64]
    assert (2 * 9) % 16 == 2


@pytest.mark.parametrize("which", range(6), ids=["1", "C-1", "C", "C+1", "2C+3", "9"])
@pytest.mark.parametrize("nv", UNIFORM_NV)
def test_uniform(oracle, nv, which):
    cols = col_counts(nv)[which]
    for pad in (16, 48):
        run_uniform(oracle, nv, cols, pad, "systematic_w")


def test_uniform_tight_rows_and_batch_of_one(oracle):
    # no row padding at all, the out pitch = the output; one payload: its out pitch is not applied
    run_uniform(oracle, 1024, 64, 0, "systematic_w")
    run_uniform(oracle, 1024, 65, 0, "systematic_w", batch=1, os_odd=8)


def test_uniform_more_tiles_than_workgroups(oracle):
    """70 payloads of 3 columns at k = 4096: one column tile in 16 row blocks
    each, 1120 tiles, more than the four workgroups per CU of the launch, so
    the plain and the _ws form hand tiles out from the counter and the
    NULL-workspace form strides (a launch of fewer tiles needs no counter)"""
    import torch
    nv, batch = 12289, 70
    assert batch * 16 > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    run_uniform(oracle, nv, 3, 16, "systematic_w", batch=batch)


@pytest.mark.parametrize("name,kw", [("shard-pitch+8", dict(ss_odd=8)), ("out+8", dict(out_off=8))])
def test_layouts_that_fall_to_systematic_g(oracle, name, kw):
    run_uniform(oracle, 1024, 65, 16, "systematic_g", **kw)


# ---- the ragged call -----------------------------------------------------------
class Item:
    def __init__(self, cols, pad=0, bad=None):
        self.cols, self.pad, self.bad = cols, pad, bad


def layout(nv, items):
    """offsets of every item's rows and output: 16-B aligned, gaps of noise between them"""
    k = E.code_params(nv)[1]
    lay, s, o = [], 0, 0
    for i, it in enumerate(items):
        sl = 2 * it.cols
        ss = up16(sl) + it.pad
        lay.append(dict(s=s, o=o, sl=sl, ss=ss))
        g = 16 * (1 + i % 3)
        s += nv * ss + g
        o += up16(sl * k) + g
    return lay, s, o


def item_rows(items, lay, max_slen):
    a = np.zeros((len(items), 5), np.uint64)
    for i, (it, l) in enumerate(zip(items, lay)):
        a[i] = (l["o"], 0, l["s"], l["sl"], l["ss"])
        if it.bad == "len0":
            a[i, 3] = 0
        elif it.bad == "toolong":
            a[i, 3] = max_slen + 2
        elif it.bad == "odd":
            a[i, 3] -= 1
        elif it.bad == "shard_off+8":
            a[i, 2] += 8
        else:
            assert it.bad is None
    return a


def fill(oracle, nv, host, a_sh, items, lay):
    k = E.code_params(nv)[1]
    for i, (it, l) in enumerate(zip(items, lay)):
        strided(host, a_sh + l["s"], k, l["ss"], l["sl"])[:] = ref_rows(oracle, nv, it.cols, i % 3)[0]


def check(oracle, nv, got, a_out, a_st, items, lay):
    k = E.code_params(nv)[1]
    good = [i for i, it in enumerate(items) if it.bad is None]
    for i in good:
        o = a_out + lay[i]["o"]
        assert np.array_equal(got[o: o + lay[i]["sl"] * k], ref_rows(oracle, nv, items[i].cols, i % 3)[1]), (nv, i)
    bad = [i for i in range(len(items)) if i not in good]
    assert got[a_st: a_st + 8].view(np.uint32).tolist() == [len(bad), bad[0] if bad else 0]


def run_ragged(oracle, nv, items, ws):
    k = E.code_params(nv)[1]
    B = len(items)
    lay, sbytes, obytes = layout(nv, items)
    good = [i for i, it in enumerate(items) if it.bad is None]
    max_slen = max(lay[i]["sl"] for i in good)
    need = E.systematic_ragged_workspace_bytes(nv, B, max_slen)
    A = L.Arena(seed=nv * 13 + B)
    a_sh, a_out = A.add("shards", sbytes), A.add("out", obytes)
    a_it, a_st, a_ws = A.add("items", B * 40), A.add("status", 8), A.add("workspace", need)
    host = A.build()
    fill(oracle, nv, host, a_sh, items, lay)
    host[a_it: a_it + B * 40] = item_rows(items, lay, max_slen).view(np.uint8).reshape(-1)
    for i in good:
        A.allow(a_out + lay[i]["o"], lay[i]["sl"] * k)
    A.allow(a_st, 8)
    if ws:
        A.allow(a_ws, need)
    dev, base = upload(A)
    E.systematic_ragged(nv, base + a_sh, base + a_it, B, max_slen, base + a_out, d_status=base + a_st,
                        ws=dev[a_ws: a_ws + need] if ws else None)
    got = download(dev)
    check(oracle, nv, got, a_out, a_st, items, lay)
    assert A.violations(got) == []


def mix(nv, defects):
    c = tile_cols(nv) if E.code_params(nv)[1] >= 16 else 64
    items = [Item(1), Item(3 * c + 5, pad=48), Item(c - 1, pad=16), Item(c + 1)]
    if defects:
        items = [items[0], Item(c, bad="len0"), items[1], Item(7, bad="shard_off+8"), items[2],
                 Item(c + 2, pad=16, bad="toolong"), Item(5, bad="odd"), items[3]]
    return items


@pytest.mark.parametrize("defects", [False, True], ids=["valid", "defects"])
@pytest.mark.parametrize("nv", [6, 100, 1024, 4096])
def test_ragged(oracle, nv, defects):
    assert E.systematic_ragged_kernel(nv) == ("systematic_g_ragged" if nv == 6 else "systematic_w_ragged")
    run_ragged(oracle, nv, mix(nv, defects), ws=defects)


def test_ragged_defects_agree_with_the_host_check():
    nv = 1024
    items = mix(nv, True)
    lay, _, _ = layout(nv, items)
    max_slen = max(l["sl"] for it, l in zip(items, lay) if it.bad is None)
    assert E.ragged_check(nv, item_rows(items, lay, max_slen), max_slen, reconstruct=True) == (4, 1)


def test_ragged_more_tiles_than_workgroups(oracle):
    """1300 column tiles in 400 items of three lengths: more than the launch's
    workgroups, so one workgroup runs tiles of several items from the counter"""
    nv = 1024
    items = [Item([130, 200, 250][i % 3], pad=16 * (i % 2)) for i in range(400)]
    assert sum((it.cols + 63) // 64 for it in items) >= 1300
    run_ragged(oracle, nv, items, ws=False)


def test_ragged_graph_replay_with_changed_items(oracle):
    """one _ws call captured and replayed twice, the item array's contents
    changed between the replays (same batch and maximum): a plan or a counter
    that is not rebuilt on replay gives the second replay the first one's geometry"""
    import torch
    nv = 1024
    k = E.code_params(nv)[1]
    sets = [[Item(70), Item(1, pad=16), Item(197, pad=32), Item(64)],
            [Item(5, pad=48), Item(197), Item(63), Item(129, pad=16)]]
    B, max_slen = 4, 2 * 197
    lays = [layout(nv, s) for s in sets]
    sbytes, obytes = (max(l[j] for l in lays) for j in (1, 2))
    need = E.systematic_ragged_workspace_bytes(nv, B, max_slen)

    def arena(r):
        A = L.Arena(seed=77 + r)
        a = dict(sh=A.add("shards", sbytes), out=A.add("out", obytes), it=A.add("items", B * 40),
                 st=A.add("status", 8), ws=A.add("workspace", need))
        host = A.build()
        fill(oracle, nv, host, a["sh"], sets[r], lays[r][0])
        host[a["it"]: a["it"] + B * 40] = item_rows(sets[r], lays[r][0], max_slen).view(np.uint8).reshape(-1)
        for l in lays[r][0]:
            A.allow(a["out"] + l["o"], l["sl"] * k)
        A.allow(a["st"], 8)
        A.allow(a["ws"], need)
        return A, a

    arenas = [arena(0), arena(1)]
    assert arenas[0][1] == arenas[1][1] and arenas[0][0].size == arenas[1][0].size
    a = arenas[0][1]
    dev, base = upload(arenas[0][0])
    ws = dev[a["ws"]: a["ws"] + need]

    def step():
        E.systematic_ragged(nv, base + a["sh"], base + a["it"], B, max_slen, base + a["out"],
                            d_status=base + a["st"], ws=ws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # outside capture: kernel attributes
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
        check(oracle, nv, got, a["out"], a["st"], sets[r], lays[r][0])
        assert A.violations(got) == []


# ---- the per-call ABI ------------------------------------------------------------
def test_per_call_abi(oracle):
    """a 100 KB payload at n_validators 1024: 196 columns, more than one
    workgroup of either kernel; ECCR_reconstruct_from_systematic and
    ECCR_reconstruct from exactly the k systematic rows"""
    nv, plen = 1024, 100_000
    k = E.code_params(nv)[1]
    cols = E.shard_len(nv, plen) // 2
    assert cols == 196
    rows, ref = ref_rows(oracle, nv, cols)
    chunks = [(y, rows[y].tobytes()) for y in range(k)]
    assert E.reconstruct_from_systematic(nv, chunks) == ref.tobytes()
    full = oracle.reconstruct(nv, [rows[y].tobytes() if y < k else None for y in range(nv)])
    assert full == ref.tobytes()
    assert E.reconstruct(nv, chunks) == full
