"""Static checks of the masked encode's code (enc_k256w_missing.hip), as
tests/test_ragged_asm.py makes them for the ragged kernel on the same body: no
scratch and at most 128 VGPRs (two 8-wave workgroups per CU), compiled with the
Makefile's per-source flags, which are encode_k256w's.  Resources only: under a
row mask the compiler is free to lay the stores out as it likes.  CPU only:
hipcc -S for gfx950."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasure-coding-crust_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "enc_k256w_missing.hip"


def _sched_flags(name):
    mk = open(os.path.join(ROOT, "erasure-coding-crust_amd", "Makefile")).read()
    m = re.search(r"^SCHED_" + re.escape(name) + r"\s*\??=\s*(.*)$", mk, re.M)
    return m.group(1).split() if m else []


def test_sched_flags_are_encode_k256ws():
    assert _sched_flags(SRC) == _sched_flags("enc_k256w.hip") != []


def test_the_source_is_built():
    mk = open(os.path.join(ROOT, "erasure-coding-crust_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1)
    assert SRC in srcs and "row_mask.hip" in srcs


def test_encode_k256w_missing_resources(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path / (SRC + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    *_sched_flags(SRC), "-o", str(out), os.path.join(CSRC, SRC)], check=True, capture_output=True)
    text = out.read_text()
    names = re.findall(r"^(_Z\w*encode_k256w_missing\w*):", text, re.M)
    assert len(names) == 1, names
    block = text[text.index("\n" + names[0] + ":"):]
    res = {key: int(re.search(r";\s+" + key + r":\s+(\d+)", block).group(1)) for key in ("NumVgprs", "ScratchSize")}
    assert res["ScratchSize"] == 0 and res["NumVgprs"] <= 128, res
