"""The locator-to-reconstruct contract, on every reconstruct kernel.

ECCR_AMD_reconstruct_batch (and its _ws / _patterns / _ragged forms) takes the
erasure locator as an input: d_err_log (uint16 logs) next to d_present, and
every reconstruct kernel decodes the two arrays itself.  What this module pins
(include/erasure_coding/ec_amd.h, "Layouts"):

  * a log is a residue mod 65535: 0 and 65535 both mean "multiply by one", a
    row produced by the locator may hold either, and the kernels (where the raw
    value 65535 also indexes the multiply-by-zero table and marks absent rows
    of the gather order) must take both -- csrc/ec_device.hpp mul_index();
  * any non-zero present byte means present, flags at rows >= n_validators are
    ignored;
  * locator entries at erased rows >= k and at rows >= n_validators are not
    part of the result.

About one used locator entry in 65535 is == 0, so tests/golden/locator_zero.json
(tests/golden/make_locator_zero.py) holds, per n_validators, a present mask P
with such an entry at a present row (and an erased row below k, so that the
scaled symbols reach the output) and a mask S with one at an erased row below k.  Everything is compared byte for byte with the oracle at the smallest
shapes that reach each kernel (CASES; asserted by kernel name)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_locator_zero as Z  # noqa: E402

import ecc_amd as E  # noqa: E402  (imports torch first)
import synth  # noqa: E402

gpu = pytest.mark.gpu
KINDS = Z.KINDS


def up16(x):
    return (x + 15) // 16 * 16


# ------------------------------------------------------------------ the fixture
_FX = None


def fixture_file():
    global _FX
    if _FX is None:
        with open(Z.OUT) as f:
            _FX = json.load(f)["cases"]
    return _FX


def fx_mask(nv, kind):
    """(present mask [n] of 0 / 1, the listed zero-log rows) -- a missing entry is a KeyError"""
    c = fixture_file()[str(nv)]
    return Z.mask_from_hex(c[kind]["present"], c["n"]), list(c[kind]["zero"])


# ------------------------------------------------------------------ the shape table
class Case:
    """kernel: the name ECCR_AMD_reconstruct_kernel / _ragged_kernel must give.
    cols: shard columns (2-byte symbols per shard) of each payload: one count
    for a uniform call, several for the items of one ragged call.  tight: shard
    pitch = shard length (else rounded up to 16).  pr_off: bytes d_present is
    based off 16-B alignment.  waves: reconstruct_n1024x's form."""

    def __init__(self, kernel, nv, cols, tight=False, pr_off=0, waves=None, tag=""):
        self.kernel, self.nv, self.tight, self.pr_off, self.waves = kernel, nv, tight, pr_off, waves
        self.cols = tuple(cols) if isinstance(cols, (tuple, list)) else (cols,)
        self.ragged = kernel.endswith("_ragged")
        self.id = f"{kernel.replace('reconstruct_', '')}{tag}-nv{nv}"

    def pitch(self, c):
        return 2 * c if self.tight else up16(2 * c)


def gen_cols(nv):
    """reconstruct_gen: a tile is TC = WAVES * 4 * INST = 8 * 4 * (1024 / n) shard
    columns (csrc/dec_gen.hip); 70 columns, or the smallest count with a whole
    tile and a partial one where 70 is not more than a tile"""
    n, _, _ = E.code_params(nv)
    tc = 8 * 4 * (1024 // n)
    return max(70, tc + 1)


N4096_COLS = 70  # reconstruct_n4096: COLS = 4 * WAVES = 32 columns per tile (csrc/dec_n4096.hip)

CASES = (
    [Case("reconstruct_g", nv, 9, tight=True) for nv in (6, 20, 5000)]
    + [Case("reconstruct_g", 1024, 50, pr_off=1, tag="@n1024,pr+1")]
    + [Case("reconstruct_gen", nv, gen_cols(nv)) for nv in (46, 100, 300, 600, 765)]
    + [Case("reconstruct_n1024_packed", nv, 5) for nv in (800, 1024)]
    + [Case("reconstruct_n1024", nv, 40) for nv in (800, 1024)]
    + [Case("reconstruct_n1024x", nv, 50, waves=12, tag="@12") for nv in (766, 1024)]
    + [Case("reconstruct_n1024x", nv, 150, waves=16, tag="@16") for nv in (800, 1024)]
    # (NQ, K) = (2, 256), (2, 512), (4, 512), (4, 1024), (4, 1024) with nv < n
    + [Case("reconstruct_n4096", nv, N4096_COLS) for nv in (1500, 2048, 2500, 4096, 3070)]
    + [Case("reconstruct_n1024x_ragged", nv, (5, 50, 150)) for nv in (800, 1024)]
    + [Case("reconstruct_g_ragged", 600, (5, 70))]
)
CASE_IDS = [c.id for c in CASES]
VARIANTS = ("device", "zero", "65535", "oracle")  # the four d_err_log spellings of (b)
FILLS = ("asis", "ffff", "random")                # (c): what the unused entries hold
ROWS = [(kind, var, fill) for kind in KINDS for var in VARIANTS for fill in FILLS]
HALF = len(ROWS) // 2
# payload b reads pattern row PERM[b]: the rows of its own kind in reverse order
PERM = [HALF - 1 - b if b < HALF else 3 * HALF - 1 - b for b in range(len(ROWS))]
assert all(ROWS[PERM[b]][0] == ROWS[b][0] for b in range(len(ROWS))) and sorted(PERM) == list(range(len(ROWS)))


# ================================================================== CPU tests
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nv", Z.NVS)
def test_fixture_entry(restatement, nv, kind):
    """every n_validators of the table has both kinds (a missing entry fails,
    nothing skips); the listed rows are exactly the used rows with log == 0"""
    n, k = restatement.params(nv)
    c = fixture_file()[str(nv)]
    assert (c["n"], c["k"]) == (n, k)
    mask, listed = fx_mask(nv, kind)
    assert mask.shape == (n,) and not mask[nv:].any() and int(mask[:nv].sum()) >= k
    zp, zs = Z.zero_rows(mask, Z.locator(restatement, mask, nv, n), nv, k)
    assert sorted(zp + zs) == listed
    assert len(zp if kind == "P" else zs) >= 1, "no zero log at a " + (
        "present row" if kind == "P" else "erased row below k")
    if kind == "P":  # else the output copies the received rows and E[v] reaches no byte of it
        assert not mask[:k].all(), "P needs an erased row below k"


def test_fixture_covers_the_shape_table():
    assert sorted(int(x) for x in fixture_file()) == sorted(Z.NVS)
    assert {c.nv for c in CASES} <= set(Z.NVS)


SH, PR, EL, OUT = (0x7F00_0000_0000 + i * 0x1000_0000_0000 for i in range(4))  # made-up, 4 KiB aligned


def out_pitch(c, nv, cols):
    _, k, _ = E.code_params(nv)
    return up16(2 * cols * k) + 32  # 32 guard bytes after every output


def named_kernel(c, batch, sh=SH, pr=None, el=EL, out=OUT):
    if c.ragged:
        return E.reconstruct_ragged_kernel(c.nv)
    sl = 2 * c.cols[0]
    return E.reconstruct_kernel(c.nv, sh, sl, c.pitch(c.cols[0]), PR + c.pr_off if pr is None else pr, el,
                                batch, out, out_pitch(c, c.nv, c.cols[0]))


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_dispatch_of_the_shape_table(c):
    """every row of the table selects the kernel it names, at the batch sizes
    the GPU tests run (made-up addresses); a dispatch change cannot empty a row
    without failing here"""
    for batch in (len(ROWS), 4):
        assert named_kernel(c, batch) == c.kernel
    if c.waves:
        assert E.reconstruct_n1024x_waves(2 * c.cols[0]) == c.waves
    if c.kernel == "reconstruct_gen":
        n, _, _ = E.code_params(c.nv)
        tc = 32 * 1024 // n
        assert tc < c.cols[0] and c.cols[0] % tc, "a whole tile and a partial one"
    if c.kernel == "reconstruct_n4096":
        assert c.cols[0] > 32 and c.cols[0] % 32
    if c.pr_off:  # the clause under test: aligned, the same shape runs a fast kernel
        assert named_kernel(c, 4, pr=PR) == "reconstruct_n1024x"


def test_dispatch_covers_every_reconstruct_kernel():
    forms = {(c.kernel, c.waves) for c in CASES}
    for name in ("reconstruct_g", "reconstruct_gen", "reconstruct_n1024_packed", "reconstruct_n1024",
                 "reconstruct_n4096", "reconstruct_n1024x_ragged", "reconstruct_g_ragged"):
        assert (name, None) in forms
    assert ("reconstruct_n1024x", 12) in forms and ("reconstruct_n1024x", 16) in forms
    # the n4096 instantiations (NQ, K)
    assert {E.code_params(c.nv)[:2] for c in CASES if c.kernel == "reconstruct_n4096"} == {
        (2048, 256), (2048, 512), (4096, 512), (4096, 1024)}
    assert any(c.kernel == "reconstruct_n4096" and c.nv < E.code_params(c.nv)[0] and
               E.code_params(c.nv)[1] == 1024 for c in CASES)


# ================================================================== GPU tests
@pytest.fixture(scope="module")
def device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()


_REF, _LOC, _RUN = {}, {}, {}


def ref_data(oracle, nv, cols, mask, key, seed=0):
    """(reference shard rows [nv][2 cols], the oracle's reconstruct of the rows
    `mask` keeps), once per (n_validators, columns, pattern, payload)"""
    if (nv, cols, seed) not in _REF:
        _, k, _ = E.code_params(nv)
        plen = 2 * k * cols - min(5, 2 * k - 1)  # a ragged tail (k = 2: 5 bytes would be a whole column)
        assert E.shard_len(nv, plen) == 2 * cols
        pay = synth.payload(31_000 + nv + 7 * cols + seed, plen)
        rows = np.frombuffer(b"".join(oracle.encode(nv, pay.tobytes())), np.uint8).reshape(nv, 2 * cols).copy()
        rows.setflags(write=False)
        _REF[(nv, cols, seed)] = (pay, rows)
    pay, rows = _REF[(nv, cols, seed)]
    if (nv, cols, seed, key) not in _REF:
        want = oracle.reconstruct(nv, [rows[i].tobytes() if mask[i] else None for i in range(nv)])
        assert want[: len(pay)] == pay.tobytes() and not any(want[len(pay):])
        _REF[(nv, cols, seed, key)] = np.frombuffer(want, np.uint8)
    return rows, _REF[(nv, cols, seed, key)]


def locators(oracle, nv):
    """the P and S masks of n_validators, the oracle's locator rows and the rows
    ECCR_AMD_error_locator emits for them (raw uint16), once per n_validators"""
    if nv not in _LOC:
        import torch
        n, k, _ = E.code_params(nv)
        masks = np.stack([fx_mask(nv, kind)[0] for kind in KINDS])
        orc = np.stack([Z.locator(oracle, m, nv, n) for m in masks])
        d_pr = torch.from_numpy(masks).cuda()
        d_el = torch.full((len(KINDS), n), 0x5A5A, dtype=torch.int16, device="cuda")
        E.error_locator(nv, d_pr, len(KINDS), d_el)
        torch.cuda.synchronize()
        _LOC[nv] = (masks, orc, d_el.cpu().numpy().view(np.uint16))
    return _LOC[nv]


def launch(c, present, err_log, kinds, shard_rows, pattern=None, spare_rows=0):
    """One reconstruct call of case c.  present [R][n] uint8 and err_log [R][n]
    uint16 are the pattern rows; payload b reads row pattern[b] (None: row b,
    the plain call) and its shards are shard_rows[kinds[row]][ci] with the
    absent rows (flags of positions < n_validators that are 0) overwritten with
    0x5C, pitch padding 0xAA.  A ragged case runs every payload at each of its
    column counts as one item each, all in one call.  Outputs are prefilled
    with 0xAA and have 32 guard bytes each, which must come back untouched.
    -> out[b][ci]: the shard_len * k output bytes."""
    import torch
    nv = c.nv
    n, k, _ = E.code_params(nv)
    R = len(present)
    B = R if pattern is None else len(pattern)
    row_of = list(range(R)) if pattern is None else list(pattern)
    lay, soff, ooff = [], 0, 0
    for b in range(B):
        for ci, cols in enumerate(c.cols):
            ss = c.pitch(cols)
            lay.append((b, ci, cols, ss, soff, ooff))
            soff += nv * ss
            ooff += out_pitch(c, nv, cols)
    h_sh = np.full(soff + spare_rows * c.pitch(c.cols[-1]), 0xAA, np.uint8)
    h_sh[soff:] = 0x3D  # spare rows past the last payload: defined bytes, never to be read
    for b, ci, cols, ss, so, _ in lay:
        view = np.lib.stride_tricks.as_strided(h_sh[so:], (nv, 2 * cols), (ss, 1))
        have = np.asarray(present[row_of[b]][:nv]) != 0
        view[have] = shard_rows[kinds[row_of[b]]][ci][have]
        view[~have] = 0x5C
    d_sh = torch.from_numpy(h_sh).cuda()
    d_prb = torch.zeros(R * n + 16, dtype=torch.uint8, device="cuda")
    d_pr = d_prb[c.pr_off: c.pr_off + R * n]
    d_pr.copy_(torch.from_numpy(np.ascontiguousarray(present, np.uint8).reshape(-1)))
    d_el = torch.from_numpy(np.ascontiguousarray(err_log, np.uint16).view(np.int16)).cuda()
    d_out = torch.full((ooff,), 0xAA, dtype=torch.uint8, device="cuda")
    d_pat = None if pattern is None else torch.tensor(row_of, dtype=torch.int32, device="cuda")
    for t in (d_sh, d_prb, d_el, d_out):
        assert t.data_ptr() % 16 == 0
    assert d_pr.data_ptr() % 16 == c.pr_off
    if c.ragged:
        assert E.reconstruct_ragged_kernel(nv) == c.kernel
        items = np.array([(oo, 0, so, 2 * cols, ss) for _, _, cols, ss, so, oo in lay], np.uint64)
        d_items = torch.from_numpy(items.view(np.int64)).cuda()
        d_status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
        # an item's pattern row: d_pattern is per item
        d_ipat = torch.tensor([row_of[b] for b, *_ in lay], dtype=torch.int32, device="cuda")
        E.reconstruct_ragged(nv, d_sh, d_items, d_pr, d_el, len(lay), 2 * max(c.cols), d_out,
                             d_status=d_status, d_pattern=d_ipat)
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [0, 0]
    else:
        cols = c.cols[0]
        sl, ss, op = 2 * cols, c.pitch(cols), out_pitch(c, nv, cols)
        assert E.reconstruct_kernel(nv, d_sh, sl, ss, d_pr, d_el, B, d_out, op) == c.kernel
        if c.waves:
            assert E.reconstruct_n1024x_waves(sl) == c.waves
        if pattern is None:
            E.reconstruct_batch(nv, d_sh, sl, ss, d_pr, d_el, B, d_out, op)
        else:
            E.reconstruct_batch_patterns(nv, d_sh, sl, ss, d_pr, d_el, d_pat, B, d_out, op)
        torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    out = [[None] * len(c.cols) for _ in range(B)]
    for b, ci, cols, _, _, oo in lay:
        used = 2 * cols * k
        guard = got[oo + used: oo + out_pitch(c, nv, cols)]
        assert (guard == 0xAA).all(), f"{c.id}: payload {b}, {cols} columns: written past shard_len * k"
        out[b][ci] = got[oo: oo + used]
    return out


def variant_rows(c, oracle):
    """the pattern rows of (b) and (c), in ROWS order: present [R][n], err_log [R][n]"""
    nv = c.nv
    n, k, _ = E.code_params(nv)
    masks, orc, dev = locators(oracle, nv)
    pres, logs = [], []
    for r, (kind, var, fill) in enumerate(ROWS):
        i = KINDS.index(kind)
        m, d = masks[i], dev[i]
        zero = d.astype(np.int64) % 65535 == 0
        el = {"device": d, "zero": np.where(zero, 0, d), "65535": np.where(zero, 65535, d),
              "oracle": orc[i]}[var].astype(np.uint16)
        v = np.arange(n)
        unused = ((m == 0) & (v >= k)) | (v >= nv)  # what decode_main never reads
        if fill == "ffff":
            el = np.where(unused, 0xFFFF, el).astype(np.uint16)
        elif fill == "random":
            noise = synth.splitmix64_words(900 + 131 * nv + r, n).astype(np.uint16)
            el = np.where(unused, noise, el).astype(np.uint16)
        pres.append(m)
        logs.append(el)
    return np.stack(pres), np.stack(logs)


def run_case(c, oracle):
    """the calls of (b) and (c) for case c, run once: every row of ROWS as a
    payload of one _patterns call (payload b reading row PERM[b]) and, uniform
    shapes only, of one plain call (payload b reading row b).
    -> {"want": {kind: [per column count]}, "patterns": {row: [...]}, "plain": {row: [...]} or None}"""
    if c.id not in _RUN:
        try:
            masks, _, _ = locators(oracle, c.nv)
            shard_rows, want = {}, {}
            for i, kind in enumerate(KINDS):
                both = [ref_data(oracle, c.nv, cols, masks[i], kind) for cols in c.cols]
                shard_rows[kind], want[kind] = [x[0] for x in both], [x[1] for x in both]
            pres, logs = variant_rows(c, oracle)
            kinds = [r[0] for r in ROWS]
            res = dict(want=want, plain=None)
            out = launch(c, pres, logs, kinds, shard_rows, pattern=PERM)
            res["patterns"] = {ROWS[PERM[b]]: out[b] for b in range(len(ROWS))}
            if not c.ragged:
                out = launch(c, pres, logs, kinds, shard_rows)
                res["plain"] = {ROWS[b]: out[b] for b in range(len(ROWS))}
            _RUN[c.id] = res
        except BaseException as e:  # not run again by the other tests of the case
            _RUN[c.id] = e
            raise
    if isinstance(_RUN[c.id], BaseException):
        raise AssertionError(f"{c.id}: the case's calls failed earlier: {_RUN[c.id]!r}")
    return _RUN[c.id]


def spelling(raw):
    return {0: "0", 65535: "65535"}.get(int(raw), f"?{int(raw)}")


@gpu
@pytest.mark.parametrize("nv", Z.NVS)
def test_locator_rows(oracle, device, nv):
    """(a) ECCR_AMD_error_locator on the P and S masks: the oracle's residues,
    and 0 or 65535 -- printed: the spelling the real pipeline feeds the
    reconstruct kernels -- at the zero-log rows"""
    masks, orc, dev = locators(oracle, nv)
    for i, kind in enumerate(KINDS):
        assert ((dev[i].astype(np.int64) % 65535) == (orc[i].astype(np.int64) % 65535)).all(), kind
        rows = fx_mask(nv, kind)[1]
        assert rows and all(int(dev[i][v]) in (0, 65535) for v in rows), (kind, [int(dev[i][v]) for v in rows])
        print(f"locator spelling nv {nv} {kind}: " + ", ".join(
            f"row {v} ({'present' if masks[i][v] else 'erased'}) device {spelling(dev[i][v])} "
            f"oracle {spelling(orc[i][v])}" for v in rows))


@gpu
@pytest.mark.parametrize("var", VARIANTS)
@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_both_spellings(oracle, device, c, var):
    """(b) the locator as the device emitted it, with every == 0 entry spelled
    0, spelled 65535, and the oracle's own row: the oracle's bytes each time,
    through d_pattern and as rows of the plain call"""
    res = run_case(c, oracle)
    bad = []
    for form in ("patterns", "plain"):
        if res[form] is None:
            continue
        for kind in KINDS:
            for ci, cols in enumerate(c.cols):
                got, want = res[form][(kind, var, "asis")][ci], res["want"][kind][ci]
                if not np.array_equal(got, want):
                    bad.append((form, kind, cols, int((got != want).sum())))
    assert not bad, f"{c.id} err_log '{var}': (call, pattern, columns, wrong bytes) {bad}"


@gpu
@pytest.mark.parametrize("fill", FILLS[1:])
@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_unused_entries_are_not_read(oracle, device, c, fill):
    """(c) entries at erased rows >= k and at rows >= n_validators overwritten
    with 0xFFFF / with noise: the bytes of (b)"""
    res = run_case(c, oracle)
    bad = []
    for form in ("patterns", "plain"):
        if res[form] is None:
            continue
        for kind in KINDS:
            for var in VARIANTS:
                for ci, cols in enumerate(c.cols):
                    if not np.array_equal(res[form][(kind, var, fill)][ci], res[form][(kind, var, "asis")][ci]):
                        bad.append((form, kind, var, cols))
    assert not bad, f"{c.id} unused entries '{fill}': (call, pattern, err_log, columns) {bad}"


@gpu
@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_present_byte_encodings(oracle, device, c):
    """(d) present bytes drawn from {1, 2, 0x80, 0xFF} and every flag in
    [n_validators, n) set to 0xFF: the locator (mod 65535), the dedup leader and
    the reconstruct output of the canonical 0 / 1 mask.  The P pattern and an
    ordinary threshold pattern; the shard buffer ends in n - n_validators spare,
    initialised rows, so a kernel that honoured a flag past n_validators would
    read defined bytes and fail the comparison."""
    import torch
    nv = c.nv
    n, k, thr = E.code_params(nv)
    canon = {"P": fx_mask(nv, "P")[0], "T": synth.present_mask(4242 + nv, nv, thr, n)}
    rows, kinds = [], []
    for j, (name, m) in enumerate(canon.items()):
        alt = np.array([1, 2, 0x80, 0xFF], np.uint8)[(synth.splitmix64_words(77 + nv + j, n) % np.uint64(4))
                                                     .astype(np.int64)]
        alt = np.where(m != 0, alt, 0).astype(np.uint8)
        alt[nv:] = 0xFF
        assert set(np.unique(alt[:nv][m[:nv] != 0])) <= {1, 2, 0x80, 0xFF}
        rows += [m, alt]
        kinds += [name, name]
    pres = np.stack(rows)
    R = len(pres)
    d_prb = torch.zeros(R * n + 16, dtype=torch.uint8, device="cuda")
    d_pr = d_prb[c.pr_off: c.pr_off + R * n]
    d_pr.copy_(torch.from_numpy(pres.reshape(-1)))
    d_el = torch.full((R, n), 0x5A5A, dtype=torch.int16, device="cuda")
    E.error_locator_patterns(nv, d_pr, None, R, d_el)  # every row computed from its own flags
    d_pat = torch.full((R,), 99, dtype=torch.int32, device="cuda")
    E.dedup_patterns(nv, d_pr, R, d_pat)
    torch.cuda.synchronize()
    el = d_el.cpu().numpy().view(np.uint16)
    assert d_pat.cpu().tolist() == [0, 0, 2, 2]
    for r in range(R):
        orc = Z.locator(oracle, canon[kinds[r]], nv, n).astype(np.int64) % 65535
        assert ((el[r].astype(np.int64) % 65535) == orc).all(), r
    shard_rows, want = {}, {}
    for name, m in canon.items():
        both = [ref_data(oracle, nv, cols, m, name) for cols in c.cols]
        shard_rows[name], want[name] = [x[0] for x in both], [x[1] for x in both]
    out = launch(c, pres, el, kinds, shard_rows, spare_rows=n - nv)
    for r in range(R):
        for ci, cols in enumerate(c.cols):
            assert np.array_equal(out[r][ci], want[kinds[r]][ci]), (c.id, kinds[r], "alt" if r % 2 else "canon", cols)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nv", [6, 600, 1024, 2500])
def test_host_entry_points(oracle, device, nv, kind):
    """(e) ECCR_reconstruct (twice: the second call takes the locator from the
    cache) and ECCR_AMD_reconstruct_host_batch on the shards of the P and S
    patterns: these build `present` themselves and use whatever spelling the
    device locator emits"""
    n, k, _ = E.code_params(nv)
    cols = 50
    mask = fx_mask(nv, kind)[0]
    idx = np.flatnonzero(mask[:nv])
    data = [ref_data(oracle, nv, cols, mask, kind, seed=s) for s in (0, 1)]
    h0, m0 = E.locator_cache_stats()
    for rep in range(2):
        rows, want = data[rep]
        got = E.reconstruct(nv, [(int(i), rows[i].tobytes()) for i in idx])
        assert got == want.tobytes(), (nv, kind, rep)
    h1, m1 = E.locator_cache_stats()
    assert h1 - h0 >= 1 and m1 - m0 <= 1, "the second call is a cache hit"
    sl = 2 * cols
    comp = np.stack([rows[idx] for rows, _ in data])
    out = np.full((2, sl * k + 32), 0xAA, np.uint8)
    E.reconstruct_host_batch(nv, comp, sl, sl, np.stack([idx, idx]).astype(np.uint16), len(idx), 2, out,
                             sl * k + 32, 0)
    for b, (_, want) in enumerate(data):
        assert np.array_equal(out[b, : sl * k], want), (nv, kind, b)
        assert (out[b, sl * k:] == 0xAA).all()
