"""Every persistent kernel past its first tile per workgroup.

The launchers size their grids as min(tiles, c x CUs); what a workgroup (a wave,
in the packed forms) does when it takes a SECOND tile - consuming the next
tile's prefetch, reloading per-payload tables or table image 0, the barrier for
the previous tile's readers, the "adjacent" mapping of the packed reconstruct,
the b += gridDim.y pass of the generic kernels - runs only with more tiles than
the grid has workgroups.  tests/tile_loops.py plans such shapes from the CU
count of the device; this module checks the plan without a device (for 64, 256
and 304 CUs) and runs every case of it on one.

Every payload of a batch is compared byte for byte with the oracle, cheaply:
the code is GF(2)-linear for a fixed length, so payload b is the XOR of the D = 5
basis payloads selected by the bits of b % 31 + 1 and its expected shards the
same XOR of oracle.encode of the basis (the linearity itself is pinned here
against the oracle, class by class).  Reconstruct inputs are those oracle
shards, never the GPU encode's, with the absent rows overwritten by 0x5C and
the patterns cycling over four kinds (period 4 against 3 tiles a payload); the
expected output is the zero-padded payload, which oracle.reconstruct is
asserted to return for the 5 basis payloads under each of the 4 patterns.
Shard rows and outputs sit in 0xAA-prefilled buffers with a gap after every row:
a skipped tile shows as prefill in a used region, a tile written for the wrong
payload as a wrong byte, a store past a row as a changed gap."""
import numpy as np
import pytest

import ecc_amd as E  # imports torch first
import nv_boundaries as NB
import synth
import tile_loops as TL

gpu = pytest.mark.gpu
CU_COUNTS = (64, 256, 304)
IDS = [TL.case_id(c) for c in TL.plan(256)]  # the same for every CU count (test_plan_ids_do_not_depend_on_the_cu_count)


# ================================================================== CPU: the plan
def test_plan_ids_do_not_depend_on_the_cu_count():
    assert len(set(IDS)) == len(IDS)
    for C in CU_COUNTS:
        assert [TL.case_id(c) for c in TL.plan(C)] == IDS


def test_plan_holds_every_kernel_and_class_of_the_table():
    p = TL.plan(256)
    by = {}
    for c in p:
        by.setdefault(c.kernel, []).append(c)
    assert set(by) == {"encode_kw", "encode_k512w", "encode_k256w", "encode_k1024", "encode_k256_packed",
                       "reconstruct_gen", "reconstruct_n4096", "reconstruct_n1024", "reconstruct_n1024_packed",
                       ("encode_g", "reconstruct_g", "systematic_g")}
    fast = [c for c in NB.classes() if NB.TINY_HI < c.lo <= NB.FAST_HI]
    assert {(c.n, c.k) for c in fast} == set(TL.ENC_QUEUE) and set(TL.REC_GEN) | set(TL.REC_N4096) | {(1024, 256)} == set(
        TL.ENC_QUEUE)
    assert sorted({c.nv for c in by["encode_kw"]}) == [63, 92, 127, 188, 255, 380, 511, 764, 1532]
    assert sorted({c.nv for c in by["reconstruct_gen"]}) == [63, 92, 127, 188, 255, 380, 511, 764]
    assert sorted({c.nv for c in by["reconstruct_n4096"]}) == [1532, 2047, 3068, 4095]
    # both forms of every queue encode; no one-tile shape at k = 256 (it would run packed)
    for name in ("encode_kw", "encode_k512w", "encode_k256w", "encode_k1024"):
        assert {c.form for c in by[name]} == {"ticket", "static"}
        for c in by[name]:
            assert c.tag.startswith("several") or E.code_params(c.nv)[1] != 256
    assert len(by["encode_kw"]) == 2 * (9 + 8) and len(by["encode_k512w"]) == 2 * (2 + 2)
    assert len(by["encode_k256w"]) == 2 and len(by["encode_k1024"]) == 4
    assert len(by["encode_k256_packed"]) == 16 and len(by["reconstruct_n4096"]) == 6
    assert len(by["reconstruct_n1024"]) == 4 and len(by["reconstruct_n1024_packed"]) == 12


@pytest.mark.parametrize("C", CU_COUNTS)
def test_every_case_names_its_kernel_and_meets_its_conditions(C):
    for c in TL.plan(C):
        assert TL.query(c) == c.kernel, TL.case_id(c)
        assert [w for w, ok in c.why.items() if not ok] == [], TL.case_id(c)
        second, third = TL.static_counts(c)
        assert second > 0, TL.case_id(c)  # somebody runs a second tile
        sl = E.shard_len(c.nv, c.plen)
        assert c.ss >= sl and c.os >= sl * E.code_params(c.nv)[1] and c.ps >= c.plen
        if c.kernel not in ("encode_k256_packed", "reconstruct_n1024_packed"):  # a gap after every row and output
            assert c.ss >= sl + 64 and c.os >= sl * E.code_params(c.nv)[1] + 64


def test_static_counts():
    """the coverage figures of three schedules, by hand"""
    mk = lambda T, units, sched: TL.Case(*([None] * 11), T, units, sched, None, None)
    assert TL.static_counts(mk(10, 4, "stride")) == (4, 2)  # 3 3 2 2
    assert TL.static_counts(mk(3, 4, "stride")) == (0, 0)
    assert TL.static_counts(mk(1278, 256, "range")) == (256, 256)  # ranges of 5, the last of 3
    assert TL.static_counts(mk(9, 4, "range")) == (3, 3)  # 3 3 3 0
    assert TL.span_ranges(2049, 256)[-1] == (7 * 257, 2049) and TL.span_ranges(2047, 256) is None
    assert TL.static_counts(mk(2049, 256, "spans")) == (256, 256)  # 257 (250 in the last span) tiles over 32 workgroups


def test_transitions_of_the_contiguous_ranges():
    per, seen = TL.range_transitions(1278, 256)
    assert per == 5 and len(seen) == 3
    per, seen = TL.range_transitions(12, 4)  # ranges of one payload each: never a payload change inside
    assert per == 3 and len(seen) == 2


def test_allocations_stay_under_one_gib():
    worst = max((max(TL.allocations(c).values()), TL.case_id(c)) for c in TL.plan(256))
    assert worst[0] < 1 << 30, worst
    for C in CU_COUNTS:  # (every count: the sum of a case's buffers fits a device many times over)
        assert max(sum(TL.allocations(c).values()) for c in TL.plan(C)) < 3 << 30


def test_the_code_is_linear(oracle):
    """What the expected bytes of every case rest on: for one small shape per class,
    oracle.encode(x ^ y) == oracle.encode(x) ^ oracle.encode(y), shard by shard."""
    nvs = sorted({c.nv for c in TL.plan(256)})
    assert {E.code_params(nv)[:2] for nv in nvs} >= set(TL.ENC_QUEUE) and {6, 20} <= set(nvs)
    for nv in nvs:
        _, k, _ = E.code_params(nv)
        plen = TL.pieces_len(k, 3) if k > 2 else 7
        x, y = synth.payload(500 + nv, plen), synth.payload(900 + nv, plen)
        ex, ey, exy = (oracle.encode(nv, p.tobytes()) for p in (x, y, x ^ y))
        assert len(exy) == nv
        for i in range(nv):
            assert exy[i] == (np.frombuffer(ex[i], np.uint8) ^ np.frombuffer(ey[i], np.uint8)).tobytes(), (nv, i)


# ================================================================== GPU
@pytest.fixture(scope="module")
def device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count  # the attribute prepare_kernel reads


_PLAN = {}


def case_of(C, cid):
    if C not in _PLAN:
        _PLAN[C] = {TL.case_id(c): c for c in TL.plan(C)}
    c = _PLAN[C][cid]
    failed = [w for w, ok in c.why.items() if not ok]
    assert failed == [], (cid, C, failed)
    return c


def patterns(nv):
    """the four flag rows [n]: P0, P1, P2 of nv_boundaries and a random exactly-k set"""
    n, k, _ = E.code_params(nv)
    return [NB.present(nv, kind) if kind != "K" else synth.present_mask(77_000 + nv, nv, k, n) for kind in TL.PATTERNS]


# references, computed once per (n_validators, payload length) and never modified
_REF = {}


def reference(oracle, nv, plen, reconstruct=False):
    """The D basis payloads [D][plen], their reference shard rows [D][nv][shard_len]
    and the expected outputs [D][shard_len * k] (the payloads, zero-padded).
    reconstruct: oracle.reconstruct is asserted, once, to return exactly those
    outputs for every basis payload under each of the four patterns."""
    key = (nv, plen)
    if key not in _REF:
        _, k, _ = E.code_params(nv)
        sl = E.shard_len(nv, plen)
        pay = np.stack([synth.payload(310_000 + 7 * nv + d, plen) for d in range(TL.D)])
        rows = np.stack([np.frombuffer(b"".join(oracle.encode(nv, p.tobytes())), np.uint8).reshape(nv, sl)
                         for p in pay])
        outs = np.zeros((TL.D, sl * k), np.uint8)
        outs[:, :plen] = pay
        for a in (pay, rows, outs):
            a.setflags(write=False)
        _REF[key] = [pay, rows, outs, False]
    ref = _REF[key]
    if reconstruct and not ref[3]:
        for kind, flags in zip(TL.PATTERNS, patterns(nv)):
            m = NB.effective(nv, flags)
            for d in range(TL.D):
                got = oracle.reconstruct(nv, [ref[1][d][i].tobytes() if m[i] else None for i in range(nv)])
                assert got == ref[2][d].tobytes(), (nv, plen, kind, d)
        ref[3] = True
    return ref[0], ref[1], ref[2]


def combos(basis):
    """[31][...]: entry c - 1 = the XOR of the basis entries selected by the bits of c (on the device)"""
    import torch
    d = torch.from_numpy(np.array(basis)).cuda()  # (a writable copy: the references are read-only)
    out = torch.zeros((TL.COMBOS,) + tuple(d.shape[1:]), dtype=torch.uint8, device="cuda")
    for c in range(1, TL.COMBOS + 1):
        for j in range(TL.D):
            if (c >> j) & 1:
                out[c - 1] ^= d[j]
    return out


def prefilled(nbytes):
    import torch
    return torch.full((nbytes,), 0xAA, dtype=torch.uint8, device="cuda")


def place(view, exp, used):
    """view[b, :, :used] = exp[b % 31] for every payload b"""
    for r in range(min(TL.COMBOS, view.shape[0])):
        view[r::TL.COMBOS, :, :used] = exp[r]


def wrong_payloads(view, exp, used):
    """indices of the payloads b whose rows view[b, :, :used] differ from exp[b % 31]
    or whose gaps view[b, :, used:] lost their 0xAA (one reduction per residue, one
    read-back)"""
    import torch
    bad = torch.zeros(view.shape[0], dtype=torch.bool, device="cuda")
    for r in range(min(TL.COMBOS, view.shape[0])):
        g = view[r::TL.COMBOS]
        b = (g[:, :, :used] != exp[r]).flatten(1).any(1)
        if view.shape[2] > used:
            b |= (g[:, :, used:] != 0xAA).flatten(1).any(1)
        bad[r::TL.COMBOS] = b
    return torch.nonzero(bad).flatten().tolist()


def check(c, what, view, exp, used, per_col):
    """Every payload; on a mismatch: n_validators, payload, tile, first wrong row and
    column.  per_col: bytes of one row that belong to one shard column."""
    wrong = wrong_payloads(view, exp, used)
    if not wrong:
        return
    b = wrong[0]
    have = view[b].cpu().numpy()
    want = exp[b % TL.COMBOS].cpu().numpy()
    diff = np.argwhere(have[:, :used] != want)
    if diff.size:
        row, byte = (int(x) for x in diff[0])
        col = byte // per_col
        if per_col > 2:  # an output: 2 k bytes a column, row y at 2 y
            row = byte % per_col // 2
        tile = (b * c.tile[0] + col) // c.tile[1]
        detail = dict(row=row, column=col, tile=tile, have=int(have[row if per_col == 2 else 0, byte]),
                      want=int(want[row if per_col == 2 else 0, byte]))
    else:
        row, byte = (int(x) for x in np.argwhere(have[:, used:] != 0xAA)[0])
        detail = dict(row=row, gap_byte=used + byte, have=int(have[row, used + byte]))
    raise AssertionError("%s %s: n_validators %d, %d of %d payloads wrong, the first: payload %d (pattern %s) %r"
                         % (TL.case_id(c), what, c.nv, len(wrong), c.batch, b, TL.PATTERNS[b % 4], detail))


def run_encode(oracle, c):
    import torch
    nv, plen, batch = c.nv, c.plen, c.batch
    sl = E.shard_len(nv, plen)
    pay, rows, _ = reference(oracle, nv, plen)
    d_buf = prefilled(c.off + batch * c.ps + 8)
    place(d_buf[c.off: c.off + batch * c.ps].view(batch, 1, c.ps), combos(pay).unsqueeze(1), plen)
    d_pay = d_buf[c.off:]
    d_sh = prefilled(batch * nv * c.ss)
    exp = combos(rows)
    args = (nv, d_pay, plen, c.ps, batch, d_sh, c.ss)
    want = c.kernel if c.op == "encode" else c.kernel[0]
    assert E.encode_kernel(*args) == want
    if c.form == "static":
        E.encode_batch_ws(*args, None)
    else:
        E.encode_batch(*args)
    torch.cuda.synchronize()
    check(c, "encode", d_sh.view(batch, nv, c.ss), exp, sl, 2)
    return exp


def erased_shards(c, exp):
    """[batch][nv][ss] in 0xAA: payload b's reference rows, the rows its pattern
    b % 4 lacks overwritten with 0x5C; and the flag rows [batch][n]"""
    import torch
    nv, batch = c.nv, c.batch
    sl = E.shard_len(nv, c.plen)
    d_sh = prefilled(batch * nv * c.ss)
    view = d_sh.view(batch, nv, c.ss)
    place(view, exp, sl)
    pats = patterns(nv)
    for j, flags in enumerate(pats):
        gone = np.flatnonzero(NB.effective(nv, flags)[:nv] == 0)
        assert gone.size
        view[j::4][:, torch.from_numpy(gone).cuda(), :sl] = 0x5C
    d_pr = torch.from_numpy(np.stack(pats)).cuda()[torch.arange(batch, device="cuda") % 4].contiguous()
    return d_sh, d_pr


def run_reconstruct(oracle, c, exp=None):
    import torch
    nv, batch = c.nv, c.batch
    n, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, c.plen)
    _, rows, outs = reference(oracle, nv, c.plen, reconstruct=True)
    d_sh, d_pr = erased_shards(c, combos(rows) if exp is None else exp)
    d_el = torch.zeros((batch, n), dtype=torch.int16, device="cuda")
    d_out = prefilled(batch * c.os)
    args = (nv, d_sh, sl, c.ss, d_pr, d_el, batch, d_out, c.os)
    want = c.kernel if c.op == "reconstruct" else c.kernel[1]
    assert E.reconstruct_kernel(*args) == want
    E.error_locator(nv, d_pr, batch, d_el)
    E.reconstruct_batch(*args)
    torch.cuda.synchronize()
    check(c, "reconstruct", d_out.view(batch, 1, c.os), combos(outs).unsqueeze(1), sl * k, 2 * k)


@gpu
@pytest.mark.parametrize("cid", [i for i in IDS if i.startswith("encode_")])
def test_encode(device, oracle, cid):
    """The tile-queue encodes with their ticket counter and, through
    encode_batch_ws without a workspace, on the static stride cur + gridDim.x: three
    tiles a payload (the last with waves that have no piece) and many one-tile
    payloads, both with more than two tiles per workgroup.  The packed encodes past
    two wave tasks per wave (n = 1024) and past two tiles per workgroup (n = 2048:
    every second tile reloads table image 0)."""
    run_encode(oracle, case_of(device, cid))


@gpu
@pytest.mark.parametrize("cid", [i for i in IDS if i.startswith("reconstruct_")])
def test_reconstruct(device, oracle, cid):
    """reconstruct_gen over contiguous ranges of five tiles (prefetch consumed, not
    made, tables reloaded: tile_loops.range_transitions), reconstruct_n4096 in its
    single-range regime and, at n = 2048, in its span regime, reconstruct_n1024 past
    two tiles a workgroup (tile_loops.reconstruct_n1024_cases on what an even grid
    cannot reach), reconstruct_n1024_packed in both mappings past one wave step."""
    run_reconstruct(oracle, case_of(device, cid))


@gpu
@pytest.mark.parametrize("cid", [i for i in IDS if i.startswith("generic")])
def test_generic_past_grid_y(device, oracle, cid):
    """encode_g, systematic_g and reconstruct_g with 65535 + 37 payloads: the last 37
    run in the second pass of b += gridDim.y"""
    import torch
    c = case_of(device, cid)
    nv, batch = c.nv, c.batch
    _, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, c.plen)
    exp = run_encode(oracle, c)
    _, _, outs = reference(oracle, nv, c.plen)
    oexp = combos(outs).unsqueeze(1)
    d_sh = prefilled(batch * nv * c.ss)  # the reference rows, none erased
    place(d_sh.view(batch, nv, c.ss), exp, sl)
    d_out = prefilled(batch * c.os)
    args = (nv, d_sh, sl, c.ss, batch, d_out, c.os)
    assert E.systematic_kernel(*args) == c.kernel[2]
    E.systematic_batch(*args)
    torch.cuda.synchronize()
    check(c, "systematic", d_out.view(batch, 1, c.os), oexp, sl * k, 2 * k)
    run_reconstruct(oracle, c, exp)
