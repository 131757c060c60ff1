"""reconstruct_n1024x's 16-wave form (dec_n1024x.hip, reconstruct_n1024x<16>:
four waves per SIMD, 64-column tiles, phase 5's received rows read from the
shards): its register budget from the compiled code, the host query that
tells which form a shard length runs, and byte parity with the oracle at the
shapes around its tile edges, for every present pattern phase 5 and the
gather tell apart, with the 12-wave form (ECCR_AMD_RECON_WAVES=12, a fresh
process) giving the same bytes on the same inputs."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ecc_amd as E  # noqa: E402  (imports torch first)
import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasure-coding-crust_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
TILE = 64      # columns per tile of the 16-wave form
CUTOFF = 145   # kN1024x16MinCols: fewest columns the 16-wave form takes
NVS = (766, 800, 1024)
# at the cutoff: a last tile with a single-column, a partial and a whole last
# group; the exact fit and the off-by-one cases around two tiles (below the
# cutoff: the 12-wave form) and around three (the 16-wave form)
COLS = (CUTOFF, CUTOFF + 1, CUTOFF + 3, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1,
        3 * TILE - 1, 3 * TILE, 3 * TILE + 1)
PATTERNS = ("k", "threshold", "all", "parity_only", "systematic_only")


# ------------------------------------------------------------- CPU: the code

def _resources(text):
    """{waves: {NumVgprs, ScratchSize, Occupancy}} of the reconstruct_n1024x
    instantiations in a gfx950 assembly listing."""
    out = {}
    for m in re.finditer(r"^_ZN5ecamd18reconstruct_n1024xILi(\d+)EEE\w*:", text, re.M):
        tail = text[m.end():]
        out[int(m.group(1))] = {key: int(re.search(r";\s*" + key + r":\s+(\d+)", tail).group(1))
                                for key in ("NumVgprs", "ScratchSize", "Occupancy")}
    return out


def test_register_budget(tmp_path):
    """Four waves per SIMD need <= 128 VGPRs and no scratch (launch bounds
    1024); the 12-wave form keeps its <= 168 without scratch."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    mk = open(os.path.join(ROOT, "erasure-coding-crust_amd", "Makefile")).read()
    m = re.search(r"^SCHED_dec_n1024x\.hip\s*\??=\s*(.*)$", mk, re.M)
    out = tmp_path / "dec_n1024x.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    *(m.group(1).split() if m else []), "-o", str(out), os.path.join(CSRC, "dec_n1024x.hip")],
                   check=True, capture_output=True)
    res = _resources(out.read_text())
    assert set(res) == {12, 16}, res
    assert res[16]["NumVgprs"] <= 128 and res[16]["ScratchSize"] == 0 and res[16]["Occupancy"] == 4, res
    assert res[12]["NumVgprs"] <= 168 and res[12]["ScratchSize"] == 0, res


# ----------------------------------------------------- CPU: the host queries

def _plen(nv, cols):
    """A payload length (not a multiple of the row) whose shards have `cols` columns."""
    n, k, thr = E.code_params(nv)
    plen = 2 * k * cols - 5
    assert E.shard_len(nv, plen) == 2 * cols
    return plen


_B = 0x7F0000000000


def _kernel(nv, cols):
    return E.reconstruct_kernel(nv, _B, 2 * cols, (2 * cols + 15) // 16 * 16, _B + (1 << 40), _B + (2 << 40), 3,
                                _B + (3 << 40), 512 * cols)


@pytest.mark.parametrize("nv", NVS)
def test_waves_query(nv):
    """12 waves below the cutoff, 16 at and above it; the kernel class is
    reconstruct_n1024x on both sides."""
    for cols in (48, 49, 2 * TILE, CUTOFF - 1, CUTOFF, CUTOFF + 1, 3 * TILE, 1954, 19532):
        sl = E.shard_len(nv, _plen(nv, cols))
        assert E.reconstruct_n1024x_waves(sl) == (16 if cols >= CUTOFF else 12), cols
        assert _kernel(nv, cols) == "reconstruct_n1024x", cols


_QUERY = """
import sys
sys.path[:0] = [{pkg!r}]
import ecc_amd as E
B = 0x7F0000000000
for cols in (10, 40, 59, 64, 144, 145, 192, 1954):
    k = E.reconstruct_kernel(1024, B, 2 * cols, (2 * cols + 15) // 16 * 16, B + (1 << 40), B + (2 << 40), 3,
                             B + (3 << 40), 512 * cols)
    print(cols, k, E.reconstruct_n1024x_waves(2 * cols))
"""


def _query(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ECCR_AMD_RECON_")}
    r = subprocess.run([sys.executable, "-c", _QUERY.format(pkg=os.path.dirname(E.__file__))],
                       env={**clean, **env}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [line.split() for line in r.stdout.strip().split("\n")]


def test_waves_override_12():
    """ECCR_AMD_RECON_WAVES=12, read once per process: the 12-wave form
    everywhere, the kernel classes as without it."""
    for cols, kern, waves in _query({"ECCR_AMD_RECON_WAVES": "12"}):
        want = ("reconstruct_n1024_packed" if int(cols) < 32 else
                "reconstruct_n1024" if int(cols) < 48 else "reconstruct_n1024x")
        assert (kern, waves) == (want, "12"), cols


def test_waves_override_8_unchanged():
    """ECCR_AMD_RECON_WAVES=8 still selects the 8-wave kernel wherever
    reconstruct_n1024x would run."""
    for cols, kern, waves in _query({"ECCR_AMD_RECON_WAVES": "8"}):
        assert kern == ("reconstruct_n1024_packed" if int(cols) < 32 else "reconstruct_n1024"), cols


# ------------------------------------------------------------ GPU: parity

def _masks(nv, seed):
    """The present patterns: exactly k rows; the threshold count; every row
    (every gather thread multiplies, every data output is a raw re-read); no
    data row (no re-read at all); the 256 data rows and nothing else."""
    n, k, thr = E.code_params(nv)
    rng = np.random.default_rng(seed)

    def mask(idx):
        m = np.zeros(n, dtype=np.uint8)
        m[np.asarray(sorted(int(x) for x in idx), dtype=np.int64)] = 1
        return m

    return {"k": mask(rng.permutation(nv)[:k]), "threshold": mask(rng.permutation(nv)[:thr]),
            "all": mask(range(nv)), "parity_only": mask(k + rng.permutation(nv - k)[:k]),
            "systematic_only": mask(range(k))}


def _inputs(nv, cols):
    plen = _plen(nv, cols)
    masks = _masks(nv, nv * 1000 + cols)
    pay = np.stack([synth.payload(5000 + nv + cols + i, plen) for i in range(len(PATTERNS))])
    pres = np.stack([masks[p] for p in PATTERNS])
    return plen, pay, pres


def _run(nv, plen, pay, pres, pad, extra):
    """Encode and reconstruct the batch (pay[i], pres[i]) on the device: shard
    pitch = the shard length rounded up to `pad`, row padding 0xAA and absent
    rows 0x5C, output prefilled with 0xAA at a pitch of `extra` bytes more than
    the row.  Returns (encoded shards, output incl. the pitch bytes)."""
    import torch
    n, k, thr = E.code_params(nv)
    batch = len(pay)
    sl = E.shard_len(nv, plen)
    ss = (sl + pad - 1) // pad * pad
    d_pay = torch.from_numpy(np.ascontiguousarray(pay)).cuda()
    d_sh = torch.full((batch, nv, ss), 0xAA, dtype=torch.uint8, device="cuda")
    d_pr = torch.from_numpy(np.ascontiguousarray(pres)).cuda()
    d_el = torch.zeros((batch, n), dtype=torch.int16, device="cuda")
    ostride = sl * k + extra
    d_out = torch.full((batch, ostride), 0xAA, dtype=torch.uint8, device="cuda")
    E.encode_batch(nv, d_pay, plen, plen, batch, d_sh, ss)
    torch.cuda.synchronize()
    sh = d_sh.cpu().numpy()
    for b in range(batch):
        gone = np.where(pres[b][:nv] == 0)[0]
        if len(gone):
            d_sh[b, torch.from_numpy(gone).cuda()] = 0x5C
    assert E.reconstruct_kernel(nv, d_sh, sl, ss, d_pr, d_el, batch, d_out, ostride) == "reconstruct_n1024x"
    E.error_locator(nv, d_pr, batch, d_el)
    E.reconstruct_batch(nv, d_sh, sl, ss, d_pr, d_el, batch, d_out, ostride)
    torch.cuda.synchronize()
    return sh, d_out.cpu().numpy()


# (patterns of the call, shard pitch rounding, output pitch beyond the row):
# batch 3 twice, covering the five patterns and both pitches, and batch 1
CALLS = (((0, 1, 2), 16, 0), ((3, 4, 2), 64, 8), ((3,), 16, 8), ((2,), 64, 0))


def _outputs(nv, cols):
    """Every call of CALLS at this shape: [(patterns, shards, output, plen)]."""
    plen, pay, pres = _inputs(nv, cols)
    got = []
    for pats, pad, extra in CALLS:
        idx = list(pats)
        sh, out = _run(nv, plen, pay[idx], pres[idx], pad, extra)
        got.append((pats, sh, out, plen))
    return pay, pres, got


def digest(nv, cols):
    """sha256 over the outputs of every call at this shape (the child-process
    comparison of the two forms)."""
    h = hashlib.sha256()
    for _, _, out, _ in _outputs(nv, cols)[2]:
        h.update(out.tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def _device():
    assert E.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("nv", NVS)
def test_parity_tile_edges(oracle, _device, nv, cols):
    n, k, thr = E.code_params(nv)
    assert E.reconstruct_n1024x_waves(2 * cols) == (16 if cols >= CUTOFF else 12)
    pay, pres, got = _outputs(nv, cols)
    want = {}
    for pats, sh, out, plen in got:
        sl = 2 * cols
        for j, p in enumerate(pats):
            if p not in want:  # one oracle run per pattern, shared by the calls
                shards = [sh[j, i, :sl].tobytes() if pres[p][i] else None for i in range(nv)]
                want[p] = oracle.reconstruct(nv, shards)
                assert want[p][:plen] == pay[p].tobytes(), (PATTERNS[p], "oracle round trip")
            assert out[j, :sl * k].tobytes() == want[p], (PATTERNS[p], pats)
            assert (out[j, sl * k:] == 0xAA).all(), (PATTERNS[p], pats, "bytes past the row written")


@pytest.mark.gpu
def test_parity_more_tiles_than_cus(oracle, _device):
    """389 columns x batch 40 = 280 tiles, more than the CUs: the tiles past a
    workgroup's first come from the ticket counter.  Five distinct (payload,
    pattern) pairs, eight times each."""
    nv, cols, reps = 1024, 389, 8
    n, k, thr = E.code_params(nv)
    plen, pay, pres = _inputs(nv, cols)
    idx = [i % len(PATTERNS) for i in range(len(PATTERNS) * reps)]
    sh, out = _run(nv, plen, pay[idx], pres[idx], 64, 8)
    sl = 2 * cols
    want = {}
    for j, p in enumerate(idx):
        if p not in want:
            want[p] = oracle.reconstruct(nv, [sh[j, i, :sl].tobytes() if pres[p][i] else None for i in range(nv)])
            assert want[p][:plen] == pay[p].tobytes()
        assert out[j, :sl * k].tobytes() == want[p], (j, PATTERNS[p])
        assert (out[j, sl * k:] == 0xAA).all(), j


_CHILD = """
import sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import ecc_amd as E
assert E.lib().ECCR_AMD_init_device().tag == 0
import test_n1024x_waves16 as T
for nv, cols in {cases!r}:
    assert E.reconstruct_n1024x_waves(2 * cols) == 12
    print(nv, cols, T.digest(nv, cols))
"""


@pytest.mark.gpu
def test_twelve_wave_form_gives_the_same_bytes(_device):
    """The same inputs through the 12-wave form (ECCR_AMD_RECON_WAVES=12 in a
    fresh process): byte-identical outputs."""
    cases = [(1024, CUTOFF + 3), (800, 3 * TILE + 1)]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ECCR_AMD_RECON_")}
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)),
                                                            pkg=os.path.dirname(E.__file__), cases=cases)],
                       env={**clean, "ECCR_AMD_RECON_WAVES": "12"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line.split() for line in r.stdout.strip().split("\n")]
    assert [(int(a), int(b)) for a, b, _ in lines] == cases
    for (nv, cols), (_, _, h) in zip(cases, lines):
        assert E.reconstruct_n1024x_waves(2 * cols) == 16
        assert digest(nv, cols) == h, (nv, cols)
