"""Buffer layouts of the device- and host-batch API: the kernel a call runs is
decided by the alignment of every base and pitch (choose_encode /
choose_reconstruct), so each case here moves one base or one pitch of the
all-64-byte control and asserts, in this order,

1. the kernel the query names, against a literal (tests/layout_cases.py);
2. the outputs, byte for byte against the oracle;
3. that nothing but the bytes the API may write changed: every buffer is
   carved out of one arena of seeded noise and the whole arena is compared
   with its host copy afterwards (row padding, the [used, pitch) gaps of out
   rows, 256 bytes before each base and after each end, every input buffer).

Absent shard rows of the reconstruct cases keep the arena's noise."""
import numpy as np
import pytest

import ecc_amd as E  # imports torch first
import layout_cases as L
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    r = E.lib().ECCR_AMD_init_device()
    assert r.tag == 0, E.last_error()


def _upload(arena):
    import torch
    dev = torch.from_numpy(arena.host).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev, dev.data_ptr()


def _download(dev):
    import torch
    torch.cuda.synchronize()
    return dev.cpu().numpy()


# references, computed once per (n_validators, payload length) and never modified
_REF = {}


def ref_case(oracle, nv, plen):
    """3 payloads, their reference shards, 3 erasure patterns (random threshold
    set / all systematic rows + parity up to the threshold / random k rows),
    the reference locators mod 65535 and the reference reconstructions"""
    key = (nv, plen)
    if key not in _REF:
        n, k, thr = E.code_params(nv)
        pay = [synth.payload(9000 + nv + b, plen) for b in range(3)]
        shards = [oracle.encode(nv, p.tobytes()) for p in pay]
        pres = [synth.present_mask(10**6 + nv, nv, thr, n), np.zeros(n, np.uint8),
                synth.present_mask(10**6 + nv + 2, nv, k, n)]
        parity = k + synth.present_set(10**6 + nv + 1, nv - k, thr - k)
        pres[1][:k] = 1
        pres[1][parity] = 1
        elog = [oracle.error_poly((m == 0).astype(np.uint8), n)[:n].astype(np.int64) % 65535 for m in pres]
        out = [oracle.reconstruct(nv, [shards[b][i] if pres[b][i] else None for i in range(nv)])
               for b in range(3)]
        for a in pay + pres + elog:
            a.setflags(write=False)
        _REF[key] = (pay, shards, pres, elog, out)
    return _REF[key]


# ---------------------------------------------------------------- encode
@pytest.mark.parametrize("case", L.enc_cases(), ids=L.case_id)
def test_encode_layout(oracle, case):
    shape, var = case
    nv, plen, batch = shape.nv, shape.plen, var.batch
    sl = E.shard_len(nv, plen)
    pay_off, ps, sh_off, ss = L.enc_layout(shape, var, sl)
    pay, shards, _, _, _ = ref_case(oracle, nv, plen)
    A = L.Arena(seed=nv * 1000 + plen)
    a_pay = A.add("payloads", batch * ps, pay_off)
    a_sh = A.add("shards", batch * nv * ss, sh_off)
    host = A.build()
    for b in range(batch):
        host[a_pay + b * ps: a_pay + b * ps + plen] = pay[b]
    A.allow_rows(a_sh, batch * nv, ss, sl)
    dev, base = _upload(A)

    args = (nv, base + a_pay, plen, ps, batch, base + a_sh, ss)
    assert E.encode_kernel(*args) == getattr(shape, var.cls)
    E.encode_batch(*args)
    got = _download(dev)

    rows = np.lib.stride_tricks.as_strided(got[a_sh:], (batch, nv, sl), (nv * ss, ss, 1))
    for b in range(batch):
        assert rows[b].tobytes() == b"".join(shards[b]), b
    assert A.violations(got) == []


# ---------------------------------------------------------------- reconstruct
@pytest.mark.parametrize("case", L.rec_cases(), ids=L.case_id)
def test_reconstruct_layout(oracle, case):
    shape, var = case
    nv, plen, batch = shape.nv, shape.plen, var.batch
    n, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    sh_off, ss, pr_off, el_off, out_off, os_ = L.rec_layout(shape, var, sl, k)
    _, shards, pres, elog, out = ref_case(oracle, nv, plen)
    A = L.Arena(seed=nv * 1000 + plen + 1)
    a_sh = A.add("shards", batch * nv * ss, sh_off)
    a_pr = A.add("present", batch * n, pr_off)
    a_el = A.add("err_log", batch * n * 2, el_off)
    a_out = A.add("out", batch * os_, out_off)
    host = A.build()
    for b in range(batch):
        host[a_pr + b * n: a_pr + (b + 1) * n] = pres[b]
        for i in np.flatnonzero(pres[b][:nv]):  # absent rows keep the noise
            r = a_sh + (b * nv + int(i)) * ss
            host[r: r + sl] = np.frombuffer(shards[b][i], np.uint8)
    A.allow(a_el, batch * n * 2)
    A.allow_rows(a_out, batch, os_, sl * k)
    dev, base = _upload(A)

    args = (nv, base + a_sh, sl, ss, base + a_pr, base + a_el, batch, base + a_out, os_)
    assert E.reconstruct_kernel(*args) == getattr(shape, var.cls)
    E.error_locator(nv, base + a_pr, batch, base + a_el)
    E.reconstruct_batch(*args)
    got = _download(dev)

    for b in range(batch):
        el = got[a_el + b * n * 2: a_el + (b + 1) * n * 2].copy().view(np.uint16).astype(np.int64) % 65535
        assert (el == elog[b]).all(), b
        assert got[a_out + b * os_: a_out + b * os_ + sl * k].tobytes() == out[b], b
    assert A.violations(got) == []


# ---------------------------------------------------------------- error locator
@pytest.mark.parametrize("nv", L.LOCATOR_N)
@pytest.mark.parametrize("pr_off,el_off", [(0, 0), (1, 0), (0, 2), (1, 2)])
def test_error_locator_layout(oracle, nv, pr_off, el_off):
    n, k, thr = E.code_params(nv)
    assert n == nv
    batch = 5  # two rows share a pattern (the dedup of n > 4096)
    pres = [synth.present_mask(77 + nv + (b % 3), nv - 3, thr if b else k, n) for b in range(batch)]
    A = L.Arena(seed=nv)
    a_pr = A.add("present", batch * n, pr_off)
    a_el = A.add("err_log", batch * n * 2, el_off)
    host = A.build()
    for b in range(batch):
        host[a_pr + b * n: a_pr + (b + 1) * n] = pres[b] * (1 + b)  # any non-zero byte = present
    A.allow(a_el, batch * n * 2)
    dev, base = _upload(A)
    E.error_locator(nv, base + a_pr, batch, base + a_el)
    got = _download(dev)
    for b in range(batch):
        el = got[a_el + b * n * 2: a_el + (b + 1) * n * 2].copy().view(np.uint16).astype(np.int64) % 65535
        ep = oracle.error_poly((pres[b] == 0).astype(np.uint8), n)[:n].astype(np.int64) % 65535
        assert (el == ep).all(), b
    assert A.violations(got) == []


# ---------------------------------------------------------------- systematic
@pytest.mark.parametrize("nv", L.SYSTEMATIC_NV)
@pytest.mark.parametrize("name,sh_off,ss_pad,out_off,os_pad,odd_len", [
    ("control", 0, 0, 0, 0, 0), ("padded", 0, 24, 0, 40, 0), ("ss-odd", 0, 1, 0, 0, 0),
    ("os-odd", 0, 0, 0, 3, 0), ("out+1", 0, 0, 1, 0, 0), ("sh+1", 1, 0, 0, 0, 0),
    ("odd-shard_len", 0, 8, 0, 8, 1)])
def test_systematic_layout(oracle, nv, name, sh_off, ss_pad, out_off, os_pad, odd_len):
    n, k, _ = E.code_params(nv)
    plen, batch = 3_001, 3
    sl = E.shard_len(nv, plen)
    pay, shards, _, _, _ = ref_case(oracle, nv, plen)
    ss, os_ = L.up(sl, 64) + ss_pad, sl * k + os_pad
    A = L.Arena(seed=nv + 5)
    a_sh = A.add("shards", batch * nv * ss, sh_off)
    a_out = A.add("out", batch * os_, out_off)
    host = A.build()
    for b in range(batch):
        for i in range(k):  # rows >= k keep the noise
            r = a_sh + (b * nv + i) * ss
            host[r: r + sl] = np.frombuffer(shards[b][i], np.uint8)
    A.allow_rows(a_out, batch, os_, sl * k)
    dev, base = _upload(A)
    # an odd shard_len argument counts whole 2-byte symbols only
    E.systematic_batch(nv, base + a_sh, sl + odd_len, ss, batch, base + a_out, os_)
    got = _download(dev)
    for b in range(batch):
        ref = oracle.reconstruct_from_systematic(nv, shards[b][:k])
        assert got[a_out + b * os_:][:sl * k].tobytes() == ref, b
        assert ref[:plen] == pay[b].tobytes()
    assert A.violations(got) == []


# ---------------------------------------------------------------- host batches
def _host_arena(arena):
    """a 256-byte aligned numpy copy of the arena for the API to work in"""
    raw = np.empty(arena.size + 256, np.uint8)
    o = (-raw.ctypes.data) % 256
    buf = raw[o: o + arena.size]
    buf[:] = arena.host
    return buf


@pytest.mark.parametrize("nv,plen,pad,opad", L.HOST_CASES)
def test_host_batch_layout(oracle, nv, plen, pad, opad):
    """numpy arenas, padded pitches.  The pipeline copies rows back in one
    piece, row by row, or re-pitched, by the pitch mod 8 and the row length
    (host_pipeline.hip): ostride = used + 3 with rows of at least 256 bytes is
    the re-pitched leg of the out copy, + 64 the row-by-row one, rows under 256
    bytes (2-byte shard rows; the nv = 100 out rows) the one-piece one"""
    n, k, thr = E.code_params(nv)
    batch, chunk = 3, 2
    sl = E.shard_len(nv, plen)
    pay, shards, pres, _, out = ref_case(oracle, nv, plen)
    ps, ss, os_ = plen + pad, sl + pad, sl * k + opad
    assert sl * k >= 256 or nv == 100

    A = L.Arena(seed=nv + plen + pad)
    a_pay = A.add("payloads", batch * ps)
    a_sh = A.add("shards", batch * nv * ss)
    host = A.build()
    for b in range(batch):
        host[a_pay + b * ps: a_pay + b * ps + plen] = pay[b]
    A.allow_rows(a_sh, batch * nv, ss, sl)
    buf = _host_arena(A)
    E.encode_host_batch(nv, buf[a_pay:], plen, ps, batch, buf[a_sh:], ss, chunk)
    rows = np.lib.stride_tricks.as_strided(buf[a_sh:], (batch, nv, sl), (nv * ss, ss, 1))
    for b in range(batch):
        assert rows[b].tobytes() == b"".join(shards[b]), b
    assert A.violations(buf) == []

    cnt = [int(m.sum()) for m in pres]
    cmin = min(cnt)  # the compacted form has one count per call
    A = L.Arena(seed=nv + plen + pad + 1)
    a_comp = A.add("shards", batch * cmin * ss)
    a_idx = A.add("index", batch * cmin * 2)
    a_out = A.add("out", batch * os_)
    host = A.build()
    refs = []
    for b in range(batch):
        idx = np.flatnonzero(pres[b][:nv])[:cmin].astype(np.uint16)
        assert (idx[:k] < nv).all() and len(idx) == cmin >= k
        host[a_idx + b * cmin * 2: a_idx + (b + 1) * cmin * 2] = idx.view(np.uint8)
        for j, i in enumerate(idx):
            r = a_comp + (b * cmin + j) * ss
            host[r: r + sl] = np.frombuffer(shards[b][int(i)], np.uint8)
        keep = set(int(i) for i in idx)
        refs.append(out[b] if cmin == cnt[b] else
                    oracle.reconstruct(nv, [shards[b][i] if i in keep else None for i in range(nv)]))
    A.allow_rows(a_out, batch, os_, sl * k)
    buf = _host_arena(A)
    E.reconstruct_host_batch(nv, buf[a_comp:], sl, ss, buf[a_idx:].view(np.uint16), cmin, batch,
                             buf[a_out:], os_, chunk)
    for b in range(batch):
        assert buf[a_out + b * os_: a_out + b * os_ + sl * k].tobytes() == refs[b], b
    assert A.violations(buf) == []
