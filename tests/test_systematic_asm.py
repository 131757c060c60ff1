"""Static checks of systematic_w and systematic_w_ragged (sys_w.hip, one body:
sys_w_body.inc), as tests/test_ragged_asm.py makes them for the other ragged
kernels: no scratch, and at most 128 VGPRs -- the file is written for four
4-wave workgroups per CU (32 KB of LDS each), i.e. four waves per SIMD.  The
exchange the DESIGN.md §5.10 account counts is there: per tile and lane 32
ds_write_b32, 8 ds_read_b128 and 8 streaming 16-B stores.  CPU only: hipcc -S
for gfx950 with the Makefile's per-source flags."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasure-coding-crust_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NAME = "sys_w.hip"


def _sched_flags(name):
    mk = open(os.path.join(ROOT, "erasure-coding-crust_amd", "Makefile")).read()
    m = re.search(r"^SCHED_" + re.escape(name) + r"\s*\??=\s*(.*)$", mk, re.M)
    return m.group(1).split() if m else []


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("asm") / (NAME + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    *_sched_flags(NAME), "-o", str(out), os.path.join(CSRC, NAME)], check=True, capture_output=True)
    return out.read_text()


def _body(text, kernel):
    """the code of the one kernel whose symbol ends in `kernel` + its arguments, up to its s_endpgm"""
    names = re.findall(r"^(_ZN5ecamd\d+" + kernel + r"E\w*):", text, re.M)
    assert len(names) == 1, names
    block = text[text.index("\n" + names[0] + ":"):]
    return block, block[:block.index("s_endpgm")]


@pytest.mark.parametrize("kernel", ["systematic_w", "systematic_w_ragged"])
def test_resources(asm, kernel):
    block, _ = _body(asm, kernel)
    res = {key: int(re.search(r";\s+" + key + r":\s+(\d+)", block).group(1))
           for key in ("NumVgprs", "ScratchSize", "Occupancy")}
    assert res["ScratchSize"] == 0 and res["NumVgprs"] <= 128 and res["Occupancy"] >= 4, res


@pytest.mark.parametrize("kernel", ["systematic_w", "systematic_w_ragged"])
def test_exchange_instructions(asm, kernel):
    _, code = _body(asm, kernel)
    count = lambda pat: len(re.findall(r"^\s+" + pat, code, re.M))
    assert count(r"ds_write_b32 ") == 32 and count(r"ds_read_b128 ") == 8, kernel
    assert count(r"global_store_dwordx4 .* nt\b") == 8, kernel
    # 16-B loads: the first tile's and the next tile's, 8 each (the ragged
    # form also loads item records, 40 B, where it resolves a ticket)
    loads = count(r"global_load_dwordx4 ")
    assert loads == 16 if kernel == "systematic_w" else 16 <= loads <= 20, (kernel, loads)
    assert count(r"scratch_") == 0, kernel


def test_in_the_makefile():
    mk = open(os.path.join(ROOT, "erasure-coding-crust_amd", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bsys_w\.hip\b", mk, re.M)
