"""Every kernel on both sides of its n_validators boundaries.

The kernels branch on n_validators by hand (coset counts, the last partial
coset, the quarters of reconstruct_n4096, the `row < nv` masks), nearly always
at a multiple of k or of 1024.  tests/nv_boundaries.py computes those values
from the code parameters; this module checks the table without a device and
runs every entry of it on one:

  * the uniform device batch, in an aligned and a narrow-pitch layout, with
    three erasure patterns of which two are built around the last row;
  * the packed kernels, the ragged calls and the per-call C ABI at the
    boundaries they have.

Everything is compared byte for byte with the oracle, in arenas of seeded
noise (tests/layout_cases.py) in which only the nv x shard_len shard bytes, the
locator rows and the shard_len * k output bytes may change: a store to row nv
lands in the next payload's rows or in a guard, and absent rows keep the noise."""
import numpy as np
import pytest

import ecc_amd as E  # imports torch first
import layout_cases as L
import nv_boundaries as NB
import synth
import test_dispatch as D
import test_ragged_gpu as RG

gpu = pytest.mark.gpu
TABLE = NB.table()
K256 = [nv for nv in TABLE if E.code_params(nv)[1] == 256]  # 766 .. 1533
CAPI = [nv for nv in TABLE if E.code_params(nv)[1] >= 256]  # 766 .. 8193


def uniform_cases():
    return [(nv, cols, lay) for nv in TABLE for cols in NB.column_counts(nv) for lay in NB.LAYOUTS]


def uniform_id(case):
    return "nv%d-%dcols-%s" % case


# ================================================================== CPU: the table
def test_table_holds_the_values_no_test_ran_before():
    assert set(TABLE) >= {766, 767, 768, 769, 1023, 1024, 1025, 3069, 3070, 3071, 3072, 3073, 4095, 4096, 4097}
    assert TABLE == sorted(set(TABLE))
    assert set(TABLE) >= set(range(2, 46))
    assert [v for v in TABLE if v > 4096] == [4097, 6141, 6142, 8192, 8193]


def test_table_holds_the_hand_written_lists():
    hand = NB.hand_listed()
    # (spot values of the two lists, so that a change of how they are read shows)
    assert {46, 47, 64, 65, 381, 765, 1025, 1280, 1281, 1533, 1534, 2048, 2049, 2560, 2561, 3069} <= set(hand)
    assert set(hand) <= set(TABLE)


def test_thirteen_fast_classes():
    cl = [c for c in NB.classes() if NB.TINY_HI < c.lo <= NB.FAST_HI]
    assert len(cl) == 13 and cl[0].lo == 46 and cl[-1].hi == 4096
    for c in cl:
        assert (c.n, c.k) in NB.CLASSES
        b = NB.boundaries(c)
        assert b[0] == c.lo and b[-1] == c.hi and set(b) <= set(TABLE)
    # the classes are the ranges tests/test_dispatch.py TABLE is written in
    edges = sorted({c.lo for c in cl} | {c.hi for c in cl})
    assert {nv for nv, _, _ in D.TABLE if 46 <= nv <= 4096} <= set(edges)


@pytest.mark.parametrize("nv", TABLE)
def test_code_params_equal_the_restatement(restatement, nv):
    n, k, thr = E.code_params(nv)
    assert (n, k) == restatement.params(nv) and thr == restatement.threshold(nv)
    assert k < nv  # every entry has a row to erase below k (nv_boundaries.present)


def _dispatch_names(nv):
    """the aligned-layout names of tests/test_dispatch.py TABLE for the class of nv"""
    rows = sorted(D.TABLE)
    for (lo, e0, r0), (hi, e1, r1) in zip(rows[::2], rows[1::2]):
        if lo <= nv <= hi:
            assert (e0, r0) == (e1, r1)
            return e0, r0
    raise AssertionError(nv)


def _query(nv, cols, lay, base=0x7F00_0000_0000):
    _, k, _ = E.code_params(nv)
    plen = NB.payload_len(nv, cols)
    sl = E.shard_len(nv, plen)
    ps, ss = NB.pitches(lay, plen, sl)
    pay, sh, pr, el, out = (base + (i << 40) for i in range(5))
    return (E.encode_kernel(nv, pay, plen, ps, NB.BATCH, sh, ss),
            E.reconstruct_kernel(nv, sh, sl, ss, pr, el, NB.BATCH, out, sl * k))


@pytest.mark.parametrize("nv", TABLE)
def test_boundary_cases_run_the_fast_kernels(nv):
    """No entry silently runs the generic kernel: with the column count that
    reaches it (129 at k = 256, whose fast encode starts at 128 pieces, 97
    elsewhere), the aligned layout names what test_dispatch.TABLE gives for the
    class; every other (columns, layout) names the literal of nv_boundaries."""
    _, k, _ = E.code_params(nv)
    fast_cols = NB.COLS_K256 if NB.COLS_K256 in NB.column_counts(nv) else NB.COLS
    assert _query(nv, fast_cols, "aligned") == _dispatch_names(nv)
    for cols in NB.column_counts(nv):
        sl = E.shard_len(nv, NB.payload_len(nv, cols))
        assert sl == 2 * cols or (k == 1 and sl == 2 * cols - 2)  # k = 1: the tail takes a column off
        nm = NB.names(nv, cols)
        assert _query(nv, cols, "aligned") == (nm.enc, nm.rec), cols
        assert _query(nv, cols, "narrow") == (nm.enc_narrow, nm.rec_narrow), cols
        ps, ss = NB.pitches("narrow", NB.payload_len(nv, cols), sl)
        assert ss % 16 == 8 and ss >= sl and ps % 64 == 0


def _packed_layout(nv):
    """the "odd" layout of test_packed_small_batches: (plen, batch, payload base
    offset, payload pitch, shard pitch)"""
    plen = 300
    return plen, 7, 1, plen + 3, E.shard_len(nv, plen) + 2


def _packed_names(nv):
    n, _, _ = E.code_params(nv)
    return "encode_k256_packed", ("reconstruct_n1024_packed" if n == 1024 else "reconstruct_g")


RAGGED_FAST = [766, 767, 769, 1023]
RAGGED_GENERIC = [765, 1025, 3072, 3073]


def test_every_kernel_has_a_full_and_a_partial_coset_entry():
    """every kernel name the queries can return runs at some entry whose last
    coset is whole (nv a multiple of k) and at some entry where it is not"""
    seen = {}
    for nv, cols, lay in uniform_cases():
        nm = NB.names(nv, cols)
        for name in ((nm.enc, nm.rec) if lay == "aligned" else (nm.enc_narrow, nm.rec_narrow)):
            seen.setdefault(name, set()).add(NB.is_full_coset(nv))
    for nv in K256:
        for name in _packed_names(nv):
            seen.setdefault(name, set()).add(NB.is_full_coset(nv))
    assert set(seen) == set(L.KERNELS)
    assert {name: sides for name, sides in seen.items() if sides != {True, False}} == {}


def test_packed_and_ragged_cases_name_their_kernels():
    for nv in K256:
        plen, batch, off, ps, ss = _packed_layout(nv)
        _, k, _ = E.code_params(nv)
        sl = E.shard_len(nv, plen)
        base = 0x7F00_0000_0000
        assert sl == 2 and ss == 4
        assert E.encode_kernel(nv, base + off, plen, ps, batch, base + (1 << 40), ss) == _packed_names(nv)[0]
        assert E.reconstruct_kernel(nv, base + (1 << 40), sl, ss, base + (2 << 40), base + (3 << 40), batch,
                                    base + (4 << 40), sl * k) == _packed_names(nv)[1]
    assert set(RAGGED_FAST + RAGGED_GENERIC) <= set(TABLE)
    for nv in RAGGED_FAST:
        assert (E.encode_ragged_kernel(nv), E.reconstruct_ragged_kernel(nv)) == (
            "encode_k256w_ragged", "reconstruct_n1024x_ragged")
    for nv in RAGGED_GENERIC:
        assert (E.encode_ragged_kernel(nv), E.reconstruct_ragged_kernel(nv)) == (
            "encode_g_ragged", "reconstruct_g_ragged")


@pytest.mark.parametrize("nv", [2, 3, 5, 46, 769, 1024, 3073, 8193])
def test_patterns(nv):
    n, k, thr = E.code_params(nv)
    p0, p1, p2 = (NB.present(nv, kind) for kind in NB.KINDS)
    for m in (p0, p1, p2):
        assert m.shape == (n,) and NB.effective(nv, m).sum() >= k
    assert not p0[nv:].any() and p0.sum() == thr
    assert p1[nv:].all() and p1[nv - k: nv].all() and not p1[:nv - k].any()
    assert NB.effective(nv, p1).sum() == k and not NB.effective(nv, p1)[nv:].any()
    assert p2.sum() == k and p2[nv - 1] and not p2[k - 1: nv - 1].any()


# per-call C ABI: which staging path a call takes (capi.cpp: kDirectBytes = 64 KiB
# over the payload plus nv rows of dev_pitch(shard_len) = shard_len rounded up to 16)
def _capi_direct(nv, plen):
    _, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    rows = nv * NB.up(sl, 16)
    return plen + rows <= 64 << 10, rows + sl * k <= 64 << 10


def test_capi_payloads_take_both_staging_paths():
    """3 columns: direct (kernels on the pinned buffers) wherever a call of that
    n_validators can be; 97 columns: staged everywhere.  From 4095 up nv rows
    of 16 bytes fill the 64 KiB alone: whatever is longer than 16 bytes is staged."""
    for nv in CAPI:
        assert _capi_direct(nv, NB.payload_len(nv, 3)) == ((True, True) if nv <= 3073 else (False, False)), nv
        assert _capi_direct(nv, NB.payload_len(nv, NB.COLS)) == (False, False), nv
        if nv > 3073:
            assert nv >= 4095 and nv * 16 + 17 > 64 << 10
    assert sum(nv <= 3073 for nv in CAPI) >= 25


# ================================================================== GPU
@pytest.fixture(scope="module")
def device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()


# references, computed once per (n_validators, payload length) and never modified
_REF = {}


def reference(oracle, nv, plen, batch=NB.BATCH, kinds=NB.KINDS):
    """`batch` payloads, their reference shard rows [nv][shard_len], the flag
    rows of patterns P0 / P1 / P2 cycling, the reference locators mod 65535 of
    what those rows mean and the reference outputs"""
    key = (nv, plen, batch)
    if key not in _REF:
        n, k, _ = E.code_params(nv)
        pay = [synth.payload(40_000 + nv + b, plen) for b in range(batch)]
        rows = [np.frombuffer(b"".join(oracle.encode(nv, p.tobytes())), np.uint8).reshape(nv, -1) for p in pay]
        flags, elog, out = [], [], []
        for b in range(batch):
            f = NB.present(nv, kinds[b % len(kinds)])
            m = NB.effective(nv, f)
            assert m.sum() >= k, (nv, b)  # a pattern the oracle cannot decode is a fault of the table
            flags.append(f)
            elog.append(oracle.error_poly((m == 0).astype(np.uint8), n)[:n].astype(np.int64) % 65535)
            out.append(oracle.reconstruct(nv, [rows[b][i].tobytes() if m[i] else None for i in range(nv)]))
            assert out[b][:plen] == pay[b].tobytes()
        for a in pay + rows + flags + elog:
            a.setflags(write=False)
        _REF[key] = (pay, rows, flags, elog, out)
    return _REF[key]


def _encode_in_arena(oracle, nv, plen, batch, pay_off, ps, ss, want, seed):
    sl = E.shard_len(nv, plen)
    pay, rows, _, _, _ = reference(oracle, nv, plen, batch)
    A = L.Arena(seed=seed)
    a_pay = A.add("payloads", batch * ps, pay_off)
    a_sh = A.add("shards", batch * nv * ss)
    host = A.build()
    for b in range(batch):
        host[a_pay + b * ps: a_pay + b * ps + plen] = pay[b]
    A.allow_rows(a_sh, batch * nv, ss, sl)
    dev, base = RG.upload(A)
    args = (nv, base + a_pay, plen, ps, batch, base + a_sh, ss)
    assert E.encode_kernel(*args) == want
    E.encode_batch(*args)
    got = RG.download(dev)
    wrong = []  # (payload, the first shard rows that differ)
    for b in range(batch):
        have = RG.strided(got, a_sh + b * nv * ss, nv, ss, sl)
        bad = np.flatnonzero((have != rows[b]).any(axis=1))
        if bad.size:
            wrong.append((b, bad[:8].tolist()))
    assert wrong == [], (nv, "shard rows", wrong)
    assert A.violations(got) == []


def _reconstruct_in_arena(oracle, nv, plen, batch, ss, want, seed):
    n, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    pay, rows, flags, elog, out = reference(oracle, nv, plen, batch)
    os_ = sl * k
    A = L.Arena(seed=seed)
    a_sh = A.add("shards", batch * nv * ss)
    a_pr = A.add("present", batch * n)
    a_el = A.add("err_log", batch * n * 2)
    a_out = A.add("out", batch * os_)
    host = A.build()
    for b in range(batch):
        host[a_pr + b * n: a_pr + (b + 1) * n] = flags[b]
        m = NB.effective(nv, flags[b])[:nv].astype(bool)
        view = RG.strided(host, a_sh + b * nv * ss, nv, ss, sl)
        view[m] = rows[b][m]  # absent rows keep the noise
    A.allow(a_el, batch * n * 2)
    A.allow_rows(a_out, batch, os_, sl * k)
    dev, base = RG.upload(A)
    args = (nv, base + a_sh, sl, ss, base + a_pr, base + a_el, batch, base + a_out, os_)
    assert E.reconstruct_kernel(*args) == want
    E.error_locator(nv, base + a_pr, batch, base + a_el)
    E.reconstruct_batch(*args)
    got = RG.download(dev)
    wrong = []  # every payload is looked at: (payload, its pattern, what differs, where)
    for b in range(batch):
        kind = NB.KINDS[b % len(NB.KINDS)]
        el = got[a_el + b * n * 2: a_el + (b + 1) * n * 2].copy().view(np.uint16).astype(np.int64) % 65535
        bad = np.flatnonzero(el != elog[b])
        if bad.size:
            wrong.append((b, kind, "locator rows", bad[:4].tolist()))
        have = got[a_out + b * os_: a_out + (b + 1) * os_]
        bad = np.flatnonzero(have != np.frombuffer(out[b], np.uint8))
        if bad.size:
            wrong.append((b, kind, "output bytes", bad[:4].tolist()))
        elif have[:plen].tobytes() != pay[b].tobytes():
            wrong.append((b, kind, "payload", []))
    assert wrong == [], (nv, wrong)
    assert A.violations(got) == []


# ---------------------------------------------------------------- uniform device batch
@gpu
@pytest.mark.parametrize("case", uniform_cases(), ids=uniform_id)
def test_uniform_encode(device, oracle, case):
    nv, cols, lay = case
    plen = NB.payload_len(nv, cols)
    ps, ss = NB.pitches(lay, plen, E.shard_len(nv, plen))
    nm = NB.names(nv, cols)
    _encode_in_arena(oracle, nv, plen, NB.BATCH, 0, ps, ss, nm.enc if lay == "aligned" else nm.enc_narrow,
                     seed=nv * 1000 + cols)


@gpu
@pytest.mark.parametrize("case", uniform_cases(), ids=uniform_id)
def test_uniform_reconstruct(device, oracle, case):
    """payload 0: P0, payload 1: P1 "top", payload 2: P2 "edge" (nv_boundaries.present)"""
    nv, cols, lay = case
    plen = NB.payload_len(nv, cols)
    _, ss = NB.pitches(lay, plen, E.shard_len(nv, plen))
    nm = NB.names(nv, cols)
    _reconstruct_in_arena(oracle, nv, plen, NB.BATCH, ss, nm.rec if lay == "aligned" else nm.rec_narrow,
                          seed=nv * 1000 + cols + 1)


# ---------------------------------------------------------------- packed kernels
@gpu
@pytest.mark.parametrize("nv", K256)
def test_packed(device, oracle, nv):
    """300-byte payloads (one column), odd payload base and pitch, shard pitch
    = shard_len + 2: encode_k256_packed at every k = 256 entry, the packed n =
    1024 reconstruct up to 1024 and reconstruct_g above (2-byte rows off 16)"""
    plen, batch, off, ps, ss = _packed_layout(nv)
    enc, rec = _packed_names(nv)
    _encode_in_arena(oracle, nv, plen, batch, off, ps, ss, enc, seed=nv * 1000 + 7)
    _reconstruct_in_arena(oracle, nv, plen, batch, ss, rec, seed=nv * 1000 + 8)


# ---------------------------------------------------------------- ragged calls
@gpu
@pytest.mark.parametrize("nv", RAGGED_FAST + RAGGED_GENERIC)
def test_ragged(device, oracle, nv):
    """items of 15 bytes, 65 pieces and 64 pieces - 3 bytes (a piece = 2 k
    bytes), patterns P1, P2 and a random threshold set among them"""
    _, k, _ = E.code_params(nv)
    fast = nv in RAGGED_FAST
    assert E.encode_ragged_kernel(nv) == ("encode_k256w_ragged" if fast else "encode_g_ragged")
    assert E.reconstruct_ragged_kernel(nv) == ("reconstruct_n1024x_ragged" if fast else "reconstruct_g_ragged")
    plens = [15, 65 * 2 * k, 64 * 2 * k - 3]
    kinds = ["P1", "P2", 0, "P2", 0, "P1", 0, "P1", "P2"]  # every length with every pattern
    items = [RG.Item(plens[i % 3], kind=kinds[i], pad=16 * (i % 2)) for i in range(9)]
    assert {(it.plen, it.kind) for it in items} == {(p, kd) for p in plens for kd in ("P1", "P2", 0)}
    RG.run_encode(oracle, nv, items, seed=11)
    RG.run_reconstruct(oracle, nv, items, seed=12)


# ---------------------------------------------------------------- per-call C ABI
@gpu
@pytest.mark.parametrize("nv", CAPI)
def test_capi(device, oracle, nv):
    """ECCR_obtain_chunks / ECCR_reconstruct: a 3-column payload (the direct
    pinned-memory path up to n_validators 3073) and the 97-column one (staged
    copies), reconstructed from P2's chunk set"""
    keep = np.flatnonzero(NB.present(nv, "P2"))
    for cols in (3, NB.COLS):
        plen = NB.payload_len(nv, cols)
        pay, rows, _, _, _ = reference(oracle, nv, plen, 1)
        shards = E.obtain_chunks(nv, pay[0].tobytes())
        assert len(shards) == nv
        bad = [i for i in range(nv) if shards[i] != rows[0][i].tobytes()]
        assert bad == [], (nv, cols, bad[:8])
        got = E.reconstruct(nv, [(int(i), shards[i]) for i in keep])
        have = set(int(i) for i in keep)
        assert got == oracle.reconstruct(nv, [shards[i] if i in have else None for i in range(nv)]), (nv, cols)
        assert got[:plen] == pay[0].tobytes()
