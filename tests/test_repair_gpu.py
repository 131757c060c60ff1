"""The masked encode and the repair on the GPU (ec_amd.h "repair";
encode_k256w_missing, encode_g_missing).  Every buffer of a case is carved out
of one guard arena of seeded noise (layout_cases.Arena), so every shard row
starts as bytes that are not the codeword's.  After each call

* the wanted rows equal the oracle's;
* every other byte of the arena is what it was: present rows, the pad between
  shard_len and the pitch, the guards, every input;
* for the repair, d_out equals the oracle's reconstruct of the same inputs.

Expected bytes come from the oracle fixture only."""
import numpy as np
import pytest

import ecc_amd as E  # imports torch first
import layout_cases as L
import synth
import tile_loops as TL

pytestmark = pytest.mark.gpu

FAST, GENERIC = "encode_k256w_missing", "encode_g_missing"
# three tiles of 64 pieces at k = 256, the last with 35 pieces: waves 5 .. 7 of it have none
PLEN3 = 512 * (128 + 34) + 13
PHASES = ((0, 256), (256, 512), (512, 768), (768, 1024))  # systematic rows, cosets 256, 512, 768


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()


def _upload(arena):
    import torch
    dev = torch.from_numpy(arena.host).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev, dev.data_ptr()


def _download(dev):
    import torch
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def _workspace(nbytes):
    import torch
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


# references, computed once per (n_validators, payload length, payload) and never modified
_REF = {}


def reference(oracle, nv, plen, b):
    """payload b [plen] and its reference rows [nv][shard_len]"""
    key = (nv, plen, b)
    if key not in _REF:
        pay = synth.payload(40_000 + 31 * nv + b, plen)
        rows = np.frombuffer(b"".join(oracle.encode(nv, pay.tobytes())), np.uint8).reshape(nv, -1)
        pay.setflags(write=False)
        rows.setflags(write=False)
        _REF[key] = (pay, rows)
    return _REF[key]


def wanted_rows(nv, flags):
    return np.flatnonzero(np.asarray(flags[:nv]) == 0)


def run_encode_missing(oracle, nv, plen, ss, pres, pattern=None, kernel=None, use_ws=True, ps=None):
    """encode_missing_batch(_ws) of len(pattern or pres) payloads.  pres: rows of
    d_present [rows][n]; with `pattern`, only the rows it names are filled in,
    the others keep the arena's noise."""
    n, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    batch = len(pres) if pattern is None else len(pattern)
    ps = L.up(plen, 64) if ps is None else ps
    A = L.Arena(seed=nv * 977 + plen + ss)
    a_pay = A.add("payloads", batch * ps)
    a_sh = A.add("shards", batch * nv * ss)
    a_pr = A.add("present", len(pres) * n)
    a_pat = A.add("pattern", batch * 4) if pattern is not None else None
    host = A.build()
    refs = [reference(oracle, nv, plen, b) for b in range(batch)]
    for b in range(batch):
        host[a_pay + b * ps: a_pay + b * ps + plen] = refs[b][0]
    for r in (range(len(pres)) if pattern is None else sorted(set(pattern))):
        host[a_pr + r * n: a_pr + (r + 1) * n] = pres[r]
    if pattern is not None:
        host[a_pat: a_pat + batch * 4] = np.asarray(pattern, np.uint32).view(np.uint8)
    want = [wanted_rows(nv, pres[b if pattern is None else pattern[b]]) for b in range(batch)]
    for b in range(batch):
        for y in want[b]:
            A.allow(a_sh + (b * nv + int(y)) * ss, sl)
    dev, base = _upload(A)

    args = (nv, base + a_pay, plen, ps, batch, base + a_sh, ss)
    if kernel is not None:
        assert E.encode_missing_kernel(*args) == kernel
    pat = None if pattern is None else base + a_pat
    if use_ws:
        ws = _workspace(E.encode_missing_workspace_bytes(nv, plen, batch))
        E.encode_missing_batch_ws(*args, base + a_pr, ws, d_pattern=pat)
    else:
        E.encode_missing_batch(*args, base + a_pr, d_pattern=pat)
    got = _download(dev)

    for b in range(batch):
        for y in want[b]:
            r = a_sh + (b * nv + int(y)) * ss
            assert got[r: r + sl].tobytes() == refs[b][1][y].tobytes(), (nv, b, int(y))
    assert A.violations(got) == []
    return want


# ---------------------------------------------------------------- 1. every flag combination
def subset_patterns(nv, seed):
    """16 present rows [n]: payload s wants rows of exactly the phases in the bits
    of s (those that have rows below nv), random ones inside a wanted phase, a
    single row per phase for the payloads 1, 2, 4, 8 and 15; everything else present"""
    n = E.code_params(nv)[0]
    rng = np.random.default_rng(seed)
    pres = np.ones((16, n), np.uint8)
    for s in range(16):
        for j, (lo, hi) in enumerate(PHASES):
            hi = min(hi, nv)
            if not (s >> j) & 1 or lo >= hi:
                continue
            count = 1 if s in (1, 2, 4, 8, 15) else int(rng.integers(1, hi - lo + 1))
            pres[s, rng.choice(np.arange(lo, hi), count, replace=False)] = 0
    return pres


@pytest.mark.parametrize("ss", [336, 328], ids=["pitch16", "pitch8"])
@pytest.mark.parametrize("nv", [1024, 769, 766])
def test_every_flag_combination(oracle, nv, ss):
    """One payload per subset of {systematic rows, coset 256, coset 512, coset 768}:
    every combination of skipped phases, three tiles each, the last with idle
    waves.  ss 336: the 16-B streaming stores; 328: rows off 16 B, the 8-B path."""
    assert E.shard_len(nv, PLEN3) == 2 * 163 <= ss and ss % 8 == 0 and (ss % 16 == 0) == (ss == 336)
    pres = subset_patterns(nv, nv)
    want = run_encode_missing(oracle, nv, PLEN3, ss, pres, kernel=FAST)
    assert len(want[0]) == 0 and all(len(w) for w in want[1:4])
    # the subsets are what they are meant to be: the phases wanted by payload s
    for s in range(16):
        have = {j for j, (lo, hi) in enumerate(PHASES) if ((want[s] >= lo) & (want[s] < hi)).any()}
        assert have == {j for j in range(4) if (s >> j) & 1 and PHASES[j][0] < nv}, (nv, s)


# ---------------------------------------------------------------- 2. flags at or above n_validators
def test_present_bytes_at_or_above_n_validators(oracle):
    """rows 766 .. 1023 do not exist at n_validators 766: their present bytes are 0
    here and nothing is written past row 765 (the next payload's rows and, behind
    the last payload, the guard)"""
    nv = 766
    pres = subset_patterns(nv, 5)[[3, 6, 0, 15]]
    pres[:, nv:] = 0
    run_encode_missing(oracle, nv, PLEN3, 336, pres, kernel=FAST)


# ---------------------------------------------------------------- 3. shared patterns
def test_shared_patterns(oracle):
    """16 payloads on 3 rows of d_present through d_pattern; the other rows hold noise"""
    nv = 1024
    pres = subset_patterns(nv, 11)
    leaders = (0, 5, 9)
    pres[0] = pres[7]  # (row 0 wants nothing in subset_patterns)
    pattern = [leaders[b % 3] for b in range(16)]
    shared = run_encode_missing(oracle, nv, PLEN3, 336, pres, pattern=pattern, kernel=FAST)
    own = run_encode_missing(oracle, nv, PLEN3, 336, pres[pattern], kernel=FAST)
    assert all((a == b).all() for a, b in zip(shared, own))


def test_fewer_rows_than_payloads(oracle):
    """The reconstruct's shared-pattern layout: d_present (and a repair's d_err_log)
    of exactly P rows, each directly in front of a guard, serving 12 payloads
    through d_pattern, and ONE row serving them all.  Only the named rows may be
    read.  (A read past the buffer cannot be seen from here; what is pinned is
    that the calls take the layout and give the right bytes from it.)"""
    nv = 1024
    pres = subset_patterns(nv, 17)[[6, 9, 13]]
    n, k, thr = E.code_params(nv)
    for rows, pattern in ((pres, [b % 3 for b in range(12)]), (pres[1:2], [0] * 12)):
        run_encode_missing(oracle, nv, PLEN3, 336, rows, pattern=pattern, kernel=FAST)
    rep = np.stack([synth.present_mask(300 + r, nv, (k, thr, thr + 40)[r], n) for r in range(3)])
    for rows, pattern in ((rep, [(b * 2) % 3 for b in range(12)]), (rep[2:3], [0] * 12)):
        run_repair(oracle, nv, PLEN3, 336, rows, pattern=pattern, kernel=FAST)
    small = random_patterns(100, 2, 4_100)
    run_encode_missing(oracle, 100, 3_001, 104, small, pattern=[0, 1, 1, 0, 1], kernel=GENERIC)
    run_repair(oracle, 100, 3_001, 104, small, pattern=[1, 0, 0, 1, 1], kernel=GENERIC)


# ---------------------------------------------------------------- 4. the tile loop
def test_tile_loop(oracle):
    """Every workgroup of the 2 x CUs grid takes a second and a third tile; the
    pattern of payload b cycles with period 4 over three-tile payloads."""
    import torch
    from test_tile_loops import combos, place, prefilled, reference as tl_reference
    C = torch.cuda.get_device_properties(0).multi_processor_count
    nv, tile, S = 1023, 64, 2 * C
    pieces = 2 * tile + tile // 2 + 1
    plen = TL.pieces_len(256, pieces)
    batch = TL.next_batch(S + 1, lambda b: (3 * b) % S != 0)
    T = 3 * batch
    why = {
        "three tiles per payload": E.shard_len(nv, plen) == 2 * pieces and -(-pieces // tile) == 3,
        "the last tile has populated and empty waves": 1 <= -(-(tile // 2 + 1) // 8) < 8,
        "every workgroup runs three tiles": T >= 3 * S,
        "some run one more": T % S != 0,
        "the pattern's period is coprime to the tiles per payload": np.gcd(4, 3) == 1,
    }
    assert all(why.values()), why
    ps, ss, _ = TL.guard_pitches(nv, plen)
    sl = E.shard_len(nv, plen)
    pay, rows, _ = tl_reference(oracle, nv, plen)
    pres4 = subset_patterns(nv, 23)[[15, 8, 0, 5]]  # -> every row / one row of coset 768 / nothing / two phases
    pres4[0] = 0  # (the flags at and above n_validators too)
    d_buf = prefilled(batch * ps + 8)
    place(d_buf[: batch * ps].view(batch, 1, ps), combos(pay).unsqueeze(1), plen)
    d_sh = prefilled(batch * nv * ss)
    d_pr = torch.from_numpy(pres4).cuda()[torch.arange(batch, device="cuda") % 4].contiguous()
    args = (nv, d_buf, plen, ps, batch, d_sh, ss)
    assert E.encode_missing_kernel(*args) == FAST
    E.encode_missing_batch(*args, d_pr)
    torch.cuda.synchronize()

    exp = prefilled(batch * nv * ss).view(batch, nv, ss)
    place(exp, combos(rows), sl)
    for j in range(4):
        kept = torch.from_numpy(np.flatnonzero(pres4[j][:nv] != 0)).cuda()
        exp[j::4][:, kept, :] = 0xAA
    bad = (d_sh.view(batch, nv, ss) != exp).flatten(1).any(1)
    wrong = torch.nonzero(bad).flatten().tolist()
    assert wrong == [], "%d of %d payloads wrong, the first: %d (pattern %d)" % (len(wrong), batch, wrong[0], wrong[0] % 4)


# ---------------------------------------------------------------- repair
def run_repair(oracle, nv, plen, ss, pres, wrong=None, kernel=None, use_ws=True, os_pad=64, pattern=None):
    """repair_batch(_ws) of len(pattern or pres) payloads.  wrong: (payload, row)
    -> that present row holds bytes that are not the codeword's.  pattern:
    d_present and d_err_log hold exactly the len(pres) rows it names."""
    n, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    rows = len(pres)
    batch = rows if pattern is None else len(pattern)
    if pattern is not None:
        assert sorted(set(pattern)) == list(range(rows)) and rows < batch
        row_flags, pres = pres, [pres[r] for r in pattern]
    else:
        row_flags = pres
    os_ = L.up(sl * k, 64) + os_pad
    A = L.Arena(seed=nv * 613 + plen + ss)
    a_sh = A.add("shards", batch * nv * ss)
    a_pr = A.add("present", rows * n)
    a_el = A.add("err_log", rows * n * 2)
    a_out = A.add("out", batch * os_)
    a_pat = A.add("pattern", batch * 4) if pattern is not None else None
    host = A.build()
    for r in range(rows):
        host[a_pr + r * n: a_pr + (r + 1) * n] = row_flags[r]
    if pattern is not None:
        host[a_pat: a_pat + batch * 4] = np.asarray(pattern, np.uint32).view(np.uint8)
    refs = [reference(oracle, nv, plen, b) for b in range(batch)]
    exp_out, exp_rows = [], []
    for b in range(batch):
        have = [None] * nv
        for y in np.flatnonzero(np.asarray(pres[b][:nv]) != 0):
            row = refs[b][1][y]
            if wrong is not None and wrong == (b, int(y)):
                row = row ^ np.uint8(0x5A)
            have[int(y)] = row.tobytes()
            r = a_sh + (b * nv + int(y)) * ss
            host[r: r + sl] = np.frombuffer(have[int(y)], np.uint8)
        if sum(h is not None for h in have) >= k:
            out = oracle.reconstruct(nv, have)
            assert len(out) == sl * k
            exp_out.append(out)
            # the missing rows are the encode of what the reconstruct gave
            exp_rows.append(refs[b][1] if wrong is None or wrong[0] != b else np.frombuffer(
                b"".join(oracle.encode(nv, out)), np.uint8).reshape(nv, sl))
        else:
            exp_out.append(None)
            exp_rows.append(None)
    want = [wanted_rows(nv, pres[b]) for b in range(batch)]
    for b in range(batch):
        for y in want[b]:
            A.allow(a_sh + (b * nv + int(y)) * ss, sl)
    A.allow(a_el, rows * n * 2)
    A.allow_rows(a_out, batch, os_, sl * k)
    dev, base = _upload(A)

    if kernel is not None:
        assert E.encode_missing_kernel(nv, base + a_out, sl * k, os_, batch, base + a_sh, ss) == kernel
    E.error_locator(nv, base + a_pr, rows, base + a_el)
    args = (nv, base + a_sh, sl, ss, base + a_pr, base + a_el, batch, base + a_out, os_)
    pat = None if pattern is None else base + a_pat
    if use_ws:
        E.repair_batch_ws(*args, _workspace(E.repair_workspace_bytes(nv, sl, batch)), d_pattern=pat)
    else:
        E.repair_batch(*args, d_pattern=pat)
    got = _download(dev)

    for b in range(batch):
        if exp_out[b] is None:  # too few rows: unspecified bytes, only the bounds are checked
            continue
        assert got[a_out + b * os_: a_out + b * os_ + sl * k].tobytes() == exp_out[b], (nv, b)
        for y in want[b]:
            r = a_sh + (b * nv + int(y)) * ss
            assert got[r: r + sl].tobytes() == exp_rows[b][y].tobytes(), (nv, b, int(y))
    assert A.violations(got) == []


@pytest.mark.parametrize("nv", [1024, 800])
def test_repair_fast_path(oracle, nv):
    """exactly k random rows / threshold-many random with one present row of wrong
    bytes at an index >= k / all present / only rows >= k / rows 0 .. 255 only"""
    n, k, thr = E.code_params(nv)
    assert k == 256 and thr > k + 1
    pres = np.zeros((5, n), np.uint8)
    pres[0] = synth.present_mask(7_000 + nv, nv, k, n)
    pres[1] = synth.present_mask(7_001 + nv, nv, thr, n)
    pres[2, :nv] = 1
    pres[3, k:nv] = 1
    pres[4, :k] = 1
    bad_row = int(np.flatnonzero(pres[1][k:nv])[3]) + k
    assert pres[1][bad_row] and bad_row >= k and pres[1].sum() - 1 > k
    for use_ws in (True, False):
        run_repair(oracle, nv, PLEN3, 336, pres, wrong=(1, bad_row), kernel=FAST, use_ws=use_ws)


# ---------------------------------------------------------------- 6. the generic path
def random_patterns(nv, batch, seed):
    n, k, thr = E.code_params(nv)
    counts = [k, thr, min(nv, thr + 3)]
    return np.stack([synth.present_mask(seed + b, nv, counts[b % 3], n) for b in range(batch)])


@pytest.mark.parametrize("nv", [6, 100, 1500, 4096, 5000])
def test_generic_path(oracle, nv):
    plen = 3_001 if nv > 6 else 45
    sl = E.shard_len(nv, plen)
    ss = sl + 1 if nv == 6 else L.up(sl, 8) + 8
    pres = random_patterns(nv, 3, 50_000 + nv)
    assert plen % 2 == 1 and all(len(wanted_rows(nv, p)) for p in pres)
    run_encode_missing(oracle, nv, plen, ss, pres, kernel=GENERIC, ps=plen + 3)
    run_encode_missing(oracle, nv, plen, ss, pres, kernel=GENERIC, use_ws=False)
    run_repair(oracle, nv, plen, ss, pres, kernel=GENERIC, os_pad=1 if nv == 6 else 64)
    run_repair(oracle, nv, plen, ss, pres, kernel=GENERIC, use_ws=False)


def test_generic_below_one_tile_of_pieces(oracle):
    """k = 256 with 127 pieces per payload: the plain encode runs packed there, the
    masked one the generic kernel"""
    nv, plen = 1024, 512 * 127 - 3
    assert E.encode_kernel(nv, 0x7F00_0000_0000, plen, L.up(plen, 64), 3, 0x7E00_0000_0000, 256) == "encode_k256_packed"
    pres = subset_patterns(nv, 3)[[9, 15, 4]]
    run_encode_missing(oracle, nv, plen, 256, pres, kernel=GENERIC)
    run_repair(oracle, nv, plen, 256, random_patterns(nv, 3, 99), kernel=GENERIC)


# ---------------------------------------------------------------- 7. graph capture
def test_graph_capture_repair_ws(oracle):
    """repair_batch_ws captured on one stream and replayed twice; d_present and
    d_err_log change between the replays (the plan is rebuilt by a kernel each time)"""
    import torch
    nv, plen, batch = 1024, PLEN3, 4
    n, k, thr = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    ss, os_ = 336, sl * k + 64
    ws = _workspace(E.repair_workspace_bytes(nv, sl, batch))
    refs = [reference(oracle, nv, plen, b) for b in range(batch)]
    full = np.stack([np.pad(r[1], ((0, 0), (0, ss - sl)), constant_values=0xEE) for r in refs])
    d_sh = torch.empty((batch, nv, ss), dtype=torch.uint8, device="cuda")
    d_pr = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    d_el = torch.empty((batch, n), dtype=torch.int16, device="cuda")
    d_out = torch.empty((batch, os_), dtype=torch.uint8, device="cuda")

    def damage(seed):
        pres = np.stack([synth.present_mask(seed * 100 + b, nv, (k, thr)[(seed + b) % 2], n) for b in range(batch)])
        if seed == 3:
            pres[0, :nv] = 1
            pres[0, 900:910] = 0  # a coset-768-only repair
        sh = full.copy()
        for b in range(batch):
            sh[b, wanted_rows(nv, pres[b]), :sl] = 0x33
        d_sh.copy_(torch.from_numpy(sh))
        d_pr.copy_(torch.from_numpy(pres))
        d_out.fill_(0xAA)
        E.error_locator(nv, d_pr, batch, d_el)
        return pres

    def step():
        E.repair_batch_ws(nv, d_sh, sl, ss, d_pr, d_el, batch, d_out, os_, ws)

    damage(1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # outside capture: kernel attributes, tables
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    for seed in (2, 3):
        pres = damage(seed)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (d_sh.cpu().numpy() == full).all(), seed  # every row back, pads untouched
        out = d_out.cpu().numpy()
        for b in range(batch):
            exp = oracle.reconstruct(nv, [refs[b][1][y].tobytes() if pres[b][y] else None for y in range(nv)])
            assert out[b, : sl * k].tobytes() == exp and (out[b, sl * k:] == 0xAA).all(), (seed, b)


# ---------------------------------------------------------------- 8. too few rows
def test_too_few_rows_stay_in_bounds(oracle):
    """k - 1 present rows: OK, unspecified bytes in d_out and the missing rows
    (nothing is asserted about them), and nothing else touched"""
    nv = 1024
    n, k, _ = E.code_params(nv)
    pres = np.stack([synth.present_mask(123 + b, nv, k - 1, n) for b in range(2)])
    assert all(int(p[:nv].sum()) == k - 1 for p in pres)
    run_repair(oracle, nv, PLEN3, 336, pres, kernel=FAST)
