"""The erasure-pattern stage at batch scale: the dedup hash table past its
first block and its first probe, leader-only locators, the workgroup locator
at both ends of its range, degenerate patterns, the locator workspace at its
exact size, the documented composition dedup -> error_locator_patterns ->
reconstruct_batch_patterns end to end, and the per-call locator cache across n.

tests/pattern_cases.py holds the inputs and the contract.  Pattern indices are
compared with pattern_cases.leaders() only; locator rows with the oracle's
error_poly(erased, n)[:n], both sides mod 65535, positions >= n_validators
erased; reconstruct outputs byte for byte with oracle.reconstruct.

Not covered: the `differ` branch of pattern_resolve (two different patterns
with one 64-bit hash cannot be constructed: pattern_cases' docstring)."""
import numpy as np
import pytest

import pattern_cases as PC
import test_locator_contract as LC

import ecc_amd as E  # (imports torch first)
import synth

gpu = pytest.mark.gpu


# ================================================================== CPU tests
def test_mix64_is_the_splitmix64_finaliser():
    def mix(x):  # csrc/ec_kernels.hip mix64
        x = (x + 0x9E3779B97F4A7C15) & PC.M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & PC.M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & PC.M64
        return x ^ (x >> 31)
    for i in (0, 1, 19, 255, 256, 999, 4999, 65535):
        assert PC.mix64(i) == mix(i)
    assert PC.mask_hash(0b1011) == (mix(0) + mix(1) + mix(3)) & PC.M64
    assert PC.row_hashes(np.zeros((1, 32), np.uint8), 20) == [1]  # an empty row: 0 -> 1
    assert [PC.table_cap(b) for b in (1, 24, 32, 33, 257, 1000, 3000)] == [64, 64, 64, 128, 1024, 2048, 8192]


def test_leaders_and_the_right_table_agree():
    """the restated table, run in row order, gives the contract on every named
    input (so what it reports about probing is about a table that works)"""
    for name in PC.NAMES:
        nv, pr = PC.case(name)
        assert PC.simulate(nv, pr).resolve(pr, nv) == PC.leaders(pr, nv), name


@pytest.mark.parametrize("name", PC.NAMES)
def test_named_input_shape_and_repeats(name):
    nv, pr = PC.case(name)
    lead = PC.leaders(pr, nv)
    B, n = pr.shape
    distinct = len(set(lead))
    want_shape = dict(one=(1, 32), block_edge=(257, 32), distinct=(1000, 32), few_late=(3000, 32),
                      single=(3000, 32), wrap=(24, 32), wide=(300, 1024), huge=(64, 8192))[name]
    assert (B, n) == want_shape and nv == dict(wide=1000, huge=5000).get(name, 20)
    assert pr.dtype == np.uint8 and not pr.flags.writeable
    # what must not matter is varied: other present bytes than 1, flags at positions >= nv
    assert B == 1 or len(np.unique(pr[:, :nv])) > 2
    assert pr[:, nv:].any()
    if name == "one":
        assert lead == [0]
    elif name == "block_edge":
        assert lead == list(range(255)) + [3, 0]
    elif name == "distinct":
        assert lead == list(range(1000))
    elif name == "few_late":
        assert distinct == 7
        late = [l for l in set(lead) if l >= 2900]
        assert len(late) == 1 and lead.count(late[0]) >= 2, "one pattern first seen at a row >= 2900, repeated"
        assert min(lead.count(l) for l in set(lead) if l < 2900) > 300
    elif name == "single":
        assert lead == [0] * 3000
    elif name == "wrap":
        assert lead == list(range(12)) + list(range(8)) + list(range(20, 24))
        home = PC.simulate(nv, pr).home
        assert all(h >= PC.WRAP_HOME for h in home[:8]) and home[8:12] == [0, 1, 2, 3]
        assert all(4 <= h < PC.WRAP_HOME for h in home[20:])
    else:
        spec = PC.WIDE if name == "wide" else PC.HUGE
        _, rows = PC.edge_rows(**spec)
        E_ = len(spec["edges"])
        assert [lead[r] for r in rows["same"]] == [0, 0, 0, 0]
        assert [lead[r] for r in rows["edges"]] == rows["edges"], "each edge position makes a pattern of its own"
        assert [lead[r] for r in rows["empty"]] == [E_ + 3, E_ + 3]
        assert lead[rows["random_from"]:] == list(range(rows["random_from"], B)), "the random rows are distinct"
        for j, pos in enumerate(spec["edges"]):  # one byte apart from the base, at the edge
            assert np.flatnonzero(pr[1 + j] != pr[0]).tolist() == [pos]
        assert np.flatnonzero(pr[E_ + 1] != pr[0]).tolist() == list(range(nv, n))
        assert np.flatnonzero(pr[E_ + 5] != pr[0]).tolist() == [nv]
        assert set(np.unique(pr[E_ + 2][pr[0] != 0])) == {2, 0x80, 0xFF}
        assert nv > 256, "the hash and compare loops iterate"


def test_distinct_probes():
    """a condition on the input, not a measurement of the kernel: at least 100 of
    the 1000 rows end up outside their home slot"""
    nv, pr = PC.case("distinct")
    t = PC.simulate(nv, pr)
    print(f"distinct: cap {t.cap}, {t.displaced} rows displaced, longest probe {t.longest}, {t.wraps} wraps")
    assert t.cap == 2048 and t.displaced >= 100 and t.longest >= 2


def test_wrap_wraps():
    nv, pr = PC.case("wrap")
    t = PC.simulate(nv, pr)
    print(f"wrap: cap {t.cap}, {t.displaced} rows displaced, longest probe {t.longest}, {t.wraps} wraps")
    assert t.cap == 64 and t.wraps >= 1 and t.displaced >= 4


def test_block_edge_reaches_the_second_insert_block():
    nv, pr = PC.case("block_edge")
    assert len(pr) > 256 and PC.leaders(pr, nv)[256] == 0


@pytest.mark.parametrize("model", PC.WRONG_MODELS)
def test_wrong_tables_are_told_apart(model):
    caught = []
    for name in PC.NAMES:
        nv, pr = PC.case(name)
        if PC.simulate(nv, pr, model).resolve(pr, nv) != PC.leaders(pr, nv):
            caught.append(name)
    print(f"{model}: differs from leaders() on {caught}")
    assert caught, model
    if model == "stop_at_last_slot":
        assert "wrap" in caught
    if model == "drop_rows_from_256":
        assert "few_late" in caught


def test_locator_pattern_sets():
    for nv, n in ((3, 4), (20, 32), (1000, 1024), (16384, 16384)):
        d = PC.degenerate_rows(nv, n)
        assert d[:, :nv].sum(axis=1).tolist() == [nv, 0, 1, nv - 1] and not d[:, nv:].any()
    small = PC.small_batch(20, 32)
    assert small.shape == (300, 32) and len({r.tobytes() for r in small}) <= 40
    assert {r.tobytes() for r in PC.degenerate_rows(20, 32)} <= {r.tobytes() for r in small}
    for b in PC.large_batches(5000, 8192, 1024, 1667):
        assert b.shape == (9, 8192) and PC.leaders(b, 5000) == [0, 1, 2, 0, 4, 1, 4, 2, 0]
    late = PC.late_leaders(PC.LEADER_DEAL)
    assert late == [10, 9, 10, 7, 9, 8, 10, 7, 8, 9, 10]
    assert all(late[l] == l for l in late) and any(l > b for b, l in enumerate(late))


# ================================================================== GPU tests
@pytest.fixture(scope="module")
def device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()


_ROW = {}


def oracle_rows(oracle, flags, nv):
    """error_poly(erased, n)[:n] mod 65535 per row of flags [B][n], once per pattern"""
    n = flags.shape[1]
    out = np.empty(flags.shape, np.int64)
    for b, row in enumerate(flags):
        key = (nv, n, row[:nv].tobytes())
        if key not in _ROW:
            erased = np.ones(n, np.uint8)
            erased[:nv] = ~row[:nv]
            _ROW[key] = oracle.error_poly(erased, n)[:n].astype(np.int64) % 65535
        out[b] = _ROW[key]
    return out


def mod(rows):
    return rows.view(np.uint16).astype(np.int64) % 65535


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def wrong_rows(got, want):
    return np.flatnonzero((got != want).any(axis=1)).tolist()


FILL = 0x1234


def err_log(batch, n, fill=FILL):
    """batch + 1 rows of d_err_log, prefilled"""
    import torch
    return torch.full((batch + 1, n), fill, dtype=torch.int16, device="cuda")


@gpu
@pytest.mark.parametrize("name", PC.NAMES)
def test_dedup(device, name):
    import torch
    nv, pr = PC.case(name)
    B = len(pr)
    d_pat = torch.full((B + 1,), 0x7EADBEEF, dtype=torch.int32, device="cuda")
    E.dedup_patterns(nv, cuda(pr), B, d_pat)
    torch.cuda.synchronize()
    got = d_pat.cpu().tolist()
    want = PC.leaders(pr, nv)
    bad = [(b, got[b], want[b]) for b in range(B) if got[b] != want[b]]
    assert not bad, f"{name}: {len(bad)} rows, (row, device, leaders()) {bad[:8]}"
    assert got[B] == 0x7EADBEEF, "written past the batch"


LEADER_SHAPES = [(64, 50), (128, 100), (256, 200), (512, 300), (1024, 1000), (2048, 1500), (4096, 3000),
                 (32, 20), (8192, 5000)]


@gpu
@pytest.mark.parametrize("n,nv", LEADER_SHAPES, ids=[f"n{n}-nv{nv}" for n, nv in LEADER_SHAPES])
def test_leader_only_locators(oracle, device, n, nv):
    """ECCR_AMD_error_locator_patterns with a d_pattern: the leaders' rows, every
    other row untouched -- with the device's own d_pattern and with one whose
    followers point to a later row"""
    import torch
    n_, k, thr = E.code_params(nv)
    assert n_ == n
    deal = list(PC.LEADER_DEAL)
    B = len(deal)
    flags = PC.count_patterns(nv, n, k, thr)[deal]
    pr = PC.dress(flags, nv, 40 + nv)
    want = oracle_rows(oracle, flags, nv)
    d_pr = cuda(pr)
    d_pat = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    E.dedup_patterns(nv, d_pr, B, d_pat)
    torch.cuda.synchronize()
    first = d_pat.cpu().tolist()
    assert first == PC.leaders(pr, nv) == [0, 1, 0, 3, 1, 5, 0, 3, 5, 1, 0]
    for pat, d_p in ((first, d_pat), (PC.late_leaders(deal), None)):
        if d_p is None:
            d_p = torch.tensor(pat, dtype=torch.int32, device="cuda")
        d_el = err_log(B, n)
        E.error_locator_patterns(nv, d_pr, d_p, B, d_el)
        torch.cuda.synchronize()
        el = d_el.cpu().numpy()
        lead = sorted(set(pat))
        rest = [b for b in range(B + 1) if b not in lead]
        assert not wrong_rows(mod(el[lead]), want[lead]), (pat, "leader rows")
        touched = [b for b in rest if (el[b] != FILL).any()]
        assert not touched, (pat, "rows written that lead nothing", touched)


def run_locator(nv, pr):
    """ECCR_AMD_error_locator on present [B][n] -> rows [B][n], the row past the batch"""
    import torch
    B, n = pr.shape
    d_el = err_log(B, n, 0x5A5A)
    E.error_locator(nv, cuda(pr), B, d_el)
    torch.cuda.synchronize()
    el = d_el.cpu().numpy()
    return el[:B], el[B]


def check_locator(oracle, nv, flags, seed):
    pr = PC.dress(flags, nv, seed)
    el, past = run_locator(nv, pr)
    bad = wrong_rows(mod(el), oracle_rows(oracle, flags, nv))
    assert not bad, f"nv {nv}: rows {bad[:10]} of {len(flags)} differ from error_poly"
    assert (past == 0x5A5A).all(), "written past the batch"


@gpu
@pytest.mark.parametrize("nv,n", [(3, 4), (6, 8), (12, 16), (20, 32)])
def test_locator_small_n(oracle, device, nv, n):
    """the workgroup form below the wave form: 300 rows from <= 40 patterns
    through dedup, leader compute and broadcast"""
    assert E.code_params(nv)[0] == n
    check_locator(oracle, nv, PC.small_batch(nv, n), 60 + nv)


@gpu
@pytest.mark.parametrize("nv,n", [(5000, 8192), (16384, 16384), (30000, 32768), (65536, 65536)])
def test_locator_large_n(oracle, device, nv, n):
    """the workgroup form above the wave form (16 .. 128 KB of dynamic LDS): 9
    rows over 4 patterns, ordinary ones and the degenerate ones"""
    n_, k, thr = E.code_params(nv)
    assert n_ == n
    for j, flags in enumerate(PC.large_batches(nv, n, k, thr)):
        check_locator(oracle, nv, flags, 70 + nv + j)


@gpu
@pytest.mark.parametrize("nv", [64, 1000, 4096])
def test_locator_wave_degenerate(oracle, device, nv):
    n = E.code_params(nv)[0]
    check_locator(oracle, nv, PC.degenerate_rows(nv, n), 80 + nv)


def ws_inputs(which):
    if which == "nv20":
        nv, pr = PC.case("block_edge")
        return nv, pr, pr[:, :nv] != 0
    nv, n, k, thr = 5000, 8192, 1024, 1667
    flags = PC.large_batches(nv, n, k, thr)[0]
    return nv, PC.dress(flags, nv, 90), flags[:, :nv]


@gpu
@pytest.mark.parametrize("which", ["nv20", "nv5000"])
def test_locator_workspace_exact(oracle, device, which):
    """ECCR_AMD_error_locator_ws on exactly the queried bytes, 256-B aligned,
    inside a larger buffer of 0xA5: the oracle's rows, nothing written outside;
    one byte less: an error, nothing written at all"""
    import torch
    nv, pr, fl = ws_inputs(which)
    B, n = pr.shape
    assert (nv, B) in ((20, 257), (5000, 9)) and E.code_params(nv)[0] == n
    flags = np.zeros(pr.shape, bool)
    flags[:, :nv] = fl
    need = int(E.lib().ECCR_AMD_error_locator_workspace_bytes(nv, B))
    cap = PC.table_cap(B)
    assert need == (B * 4 + 255) // 256 * 256 + B * 8 + cap * 8 + cap * 4
    buf = torch.full((need + 1024,), 0xA5, dtype=torch.uint8, device="cuda")
    off = 256 + (-buf.data_ptr()) % 256
    ws = buf[off: off + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    d_pr = cuda(pr)
    d_el = err_log(B, n)
    E.error_locator_ws(nv, d_pr, B, d_el, ws)
    torch.cuda.synchronize()
    el = d_el.cpu().numpy()
    assert not wrong_rows(mod(el[:B]), oracle_rows(oracle, flags, nv))
    assert (el[B] == FILL).all()
    h = buf.cpu().numpy()
    assert (h[:off] == 0xA5).all(), "written before the workspace"
    assert (h[off + need:] == 0xA5).all(), "written past the queried size"
    d_el = err_log(B, n)
    with pytest.raises(E.ECError):
        E.error_locator_ws(nv, d_pr, B, d_el, ws[: need - 1])
    torch.cuda.synchronize()
    assert (d_el.cpu().numpy() == FILL).all(), "a refused call wrote locator rows"


COMPOSE = [("reconstruct_g", 20, None), ("reconstruct_gen", 300, None), ("reconstruct_n1024x", 1024, 12),
           ("reconstruct_n4096", 2500, None)]
COMPOSE_DEAL = (0, 1, 0, 1, 2, 0, 2, 1, 2, 0, 1, 2)  # first occurrences at rows 0, 1 and 4


def compose_case(kernel, nv, waves):
    (c,) = [c for c in LC.CASES if (c.kernel, c.nv, c.waves) == (kernel, nv, waves) and not c.pr_off]
    return c


def test_compose_shapes():
    for kernel, nv, waves in COMPOSE:
        c = compose_case(kernel, nv, waves)
        assert LC.named_kernel(c, len(COMPOSE_DEAL)) == kernel
    c = compose_case("reconstruct_g", 20, None)
    assert c.cols == (9,) and c.tight
    assert compose_case("reconstruct_gen", 300, None).cols == (LC.gen_cols(300),)
    assert compose_case("reconstruct_n1024x", 1024, 12).cols == (50,)
    assert compose_case("reconstruct_n4096", 2500, None).cols == (70,)
    assert PC.leaders(np.array(COMPOSE_DEAL)[:, None] == np.arange(3)[None, :], 3) == [0, 1, 0, 1, 4, 0, 4, 1, 4, 0, 1, 4]


@gpu
@pytest.mark.parametrize("kernel,nv,waves", COMPOSE, ids=[f"{k.replace('reconstruct_', '')}-nv{nv}" for k, nv, _ in COMPOSE])
def test_documented_composition(oracle, device, kernel, nv, waves):
    """dedup_patterns -> error_locator_patterns(d_pattern) ->
    reconstruct_batch_patterns(d_pattern): the follower rows of d_err_log are
    never written (they keep their noise) and never read"""
    import torch
    c = compose_case(kernel, nv, waves)
    n, k, thr = E.code_params(nv)
    deal = list(COMPOSE_DEAL)
    B = len(deal)
    masks = [synth.present_mask(7100 + nv + j, nv, thr, n) for j in range(3)]
    pres = np.stack([masks[j] for j in deal])
    noise = synth.splitmix64_words(7200 + nv, B * n).astype(np.uint16).reshape(B, n)
    d_pr = cuda(pres)
    d_pat = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    d_el = cuda(noise.view(np.int16))
    E.dedup_patterns(nv, d_pr, B, d_pat)
    E.error_locator_patterns(nv, d_pr, d_pat, B, d_el)
    torch.cuda.synchronize()
    pat = d_pat.cpu().tolist()
    assert pat == PC.leaders(pres, nv) == [0, 1, 0, 1, 4, 0, 4, 1, 4, 0, 1, 4]
    el = d_el.cpu().numpy().view(np.uint16)
    followers = [b for b in range(B) if pat[b] != b]
    assert (el[followers] == noise[followers]).all(), "follower rows of d_err_log were written"
    shard_rows, want = {}, {}
    for j in range(3):
        both = [LC.ref_data(oracle, nv, cols, masks[j], ("stage", j)) for cols in c.cols]
        shard_rows[j], want[j] = [x[0] for x in both], [x[1] for x in both]
    out = LC.launch(c, pres, el, deal, shard_rows, pattern=pat)
    for b in range(B):
        assert np.array_equal(out[b][0], want[deal[b]][0]), (c.id, "payload", b)


# ------------------------------------------------------------------ the per-call locator cache
_SH = {}


def cached_call(oracle, nv, keep):
    """ECCR_reconstruct of one small payload per n_validators from the shards
    `keep`, compared with the oracle"""
    if nv not in _SH:
        k = E.code_params(nv)[1]
        pay = synth.payload(8100 + nv, 2 * k * 3 - 1).tobytes()
        _SH[nv] = oracle.encode(nv, pay)
    sh = _SH[nv]
    keep = sorted(int(i) for i in keep)
    got = E.reconstruct(nv, [(i, sh[i]) for i in keep])
    have = set(keep)
    assert got == oracle.reconstruct(nv, [sh[i] if i in have else None for i in range(nv)]), (nv, keep[:4])


def keep_sets(seed, nv, count):
    thr = E.code_params(nv)[2]
    masks = synth.present_masks([880_000 + seed + j for j in range(count)], nv, thr)
    assert len({m.tobytes() for m in masks}) == count
    return [np.flatnonzero(m) for m in masks]


def stats_delta(since):
    h, m = E.locator_cache_stats()
    return h - since[0], m - since[1]


@gpu
def test_locator_cache_keys_n_validators(oracle, device):
    """(a) the same present bytes (n = 1024) at n_validators 800 and 1024 are two entries"""
    keep = np.flatnonzero(synth.present_masks([881_234], 800, 400)[0])
    s0 = E.locator_cache_stats()
    cached_call(oracle, 800, keep)
    cached_call(oracle, 1024, keep)
    assert stats_delta(s0) == (0, 2)
    cached_call(oracle, 800, keep)
    cached_call(oracle, 1024, keep)
    assert stats_delta(s0) == (2, 2)


@gpu
def test_locator_cache_recycles_larger_entries(oracle, device):
    """(b) a full cache of n = 4096 entries, then n = 128 patterns: they take
    over the least recent entries' (larger) buffers.  Whatever the process-wide
    cache held before, after the 64 misses of the fill every entry is one of
    the fill's, with buffers of at least 4096 positions (new, taken over from
    an entry at least as large, or put in the place of a smaller one)."""
    big, small = keep_sets(1000, 4096, 64), keep_sets(2000, 100, 3)
    s0 = E.locator_cache_stats()
    for keep in big:
        cached_call(oracle, 4096, keep)
    assert stats_delta(s0) == (0, 64)
    for keep in small:
        cached_call(oracle, 100, keep)
    assert stats_delta(s0) == (0, 67)
    for keep in small:
        cached_call(oracle, 100, keep)
    assert stats_delta(s0) == (3, 67)
    cached_call(oracle, 4096, big[0])  # evicted by the first n = 128 pattern
    assert stats_delta(s0) == (3, 68)


def replace_smaller_sequence(oracle):
    """(c), for a process whose cache is EMPTY: 64 patterns at n_validators 100
    are then 64 new entries with buffers of 128 positions; the 2 patterns at
    n_validators 1024 evict two of them, whose buffers are too small and must be
    replaced; afterwards the 62 surviving small entries and the 2 large ones
    still give the oracle's bytes (every call is compared).
    -> the (hits, misses) deltas after each step"""
    small, big = keep_sets(3000, 100, 64), keep_sets(4000, 1024, 2)
    s0 = E.locator_cache_stats()
    steps = [s0]
    for keep in small:
        cached_call(oracle, 100, keep)
    steps.append(stats_delta(s0))
    for keep in big:
        cached_call(oracle, 1024, keep)
    steps.append(stats_delta(s0))
    for keep in big + small[2:]:
        cached_call(oracle, 1024 if len(keep) > 100 else 100, keep)
    steps.append(stats_delta(s0))
    return [list(x) for x in steps]


REPLACE_CHILD = """
import json, sys
sys.path[:0] = [{tests!r}, {orc!r}, {pkg!r}]
import test_pattern_stage as T
import oracle
assert T.E.lib().ECCR_AMD_init_device().tag == 0, T.E.last_error()
print("STEPS " + json.dumps(T.replace_smaller_sequence(oracle.Checker.default())))
"""


@gpu
def test_locator_cache_replaces_smaller_entries(device):
    """(c) in a fresh child process, because the cache belongs to the process
    and an entry keeps the capacity it was allocated with: in this process the
    entries may all be large already (after (b) they are), and the evicted
    ones would be taken over, not replaced.  The child starts with no entry
    (asserted: no hit and no miss before the first call)."""
    import json
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    code = REPLACE_CHILD.format(tests=tests, orc=os.path.join(root, "oracle"),
                                pkg=os.path.join(root, "erasure-coding-crust_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    (line,) = [x for x in r.stdout.splitlines() if x.startswith("STEPS ")]
    start, filled, replaced, again = json.loads(line[6:])
    assert start == [0, 0], "the child's cache was not empty"
    assert (filled, replaced, again) == ([0, 64], [0, 66], [64, 66])
