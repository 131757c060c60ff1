"""Static checks of the ragged kernels' code (enc_k256w_ragged.hip,
dec_n1024x_ragged.hip), as tests/test_asm_checks.py makes them for the uniform
kernels whose bodies they share: no scratch, at most 128 VGPRs (the occupancy
both bodies are written for: two 8-wave workgroups / one 16-wave workgroup per
CU), and the encode's fast store path still issuing 4 streaming stores per lane
and phase, which the compiler's vmcnt(4) before the next tile's transposes
relies on.  CPU only: hipcc -S for gfx950 with the Makefile's per-source flags."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasure-coding-crust_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _sched_flags(name):
    mk = open(os.path.join(ROOT, "erasure-coding-crust_amd", "Makefile")).read()
    m = re.search(r"^SCHED_" + re.escape(name) + r"\s*\??=\s*(.*)$", mk, re.M)
    return m.group(1).split() if m else []


_ASM = {}


def _asm(name, tmp_path_factory):
    if name not in _ASM:
        if not os.path.exists(HIPCC):
            pytest.skip("no hipcc")
        out = tmp_path_factory.mktemp("asm") / (name + ".s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        *_sched_flags(name), "-o", str(out), os.path.join(CSRC, name)], check=True,
                       capture_output=True)
        _ASM[name] = out.read_text()
    return _ASM[name]


def _summary(text, kernel):
    """{NumVgprs, ScratchSize} of the one kernel of the file whose symbol contains `kernel`"""
    names = re.findall(r"^(_Z\w*" + kernel + r"\w*):", text, re.M)
    assert len(names) == 1, names
    block = text[text.index("\n" + names[0] + ":"):]
    return {key: int(re.search(r";\s+" + key + r":\s+(\d+)", block).group(1)) for key in ("NumVgprs", "ScratchSize")}


def _nt_store_blocks(text, kernel):
    """Streaming (nt) global stores per basic block of `kernel` (the fast store
    paths are the only nt stores); tests/test_asm_checks.py counts the same"""
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and kernel in l.split(":")[0] and ":" in l)
    counts, cur = [], 0
    for l in lines[start + 1:]:
        if re.match(r"^(\.LBB\w+|_Z\w+):", l) or "s_endpgm" in l:
            if cur:
                counts.append(cur)
            cur = 0
            if "s_endpgm" in l:
                break
            continue
        if re.match(r"\s+global_store_dwordx4 .* nt\b", l):
            cur += 1
    return counts


def test_sched_flags_are_the_shared_bodies():
    assert _sched_flags("enc_k256w_ragged.hip") == _sched_flags("enc_k256w.hip") != []
    assert _sched_flags("dec_n1024x_ragged.hip") == _sched_flags("dec_n1024x.hip") == []


def test_encode_k256w_ragged_resources(tmp_path_factory):
    res = _summary(_asm("enc_k256w_ragged.hip", tmp_path_factory), "encode_k256w_ragged")
    assert res["ScratchSize"] == 0 and res["NumVgprs"] <= 128, res


def test_encode_k256w_ragged_fast_store_count(tmp_path_factory):
    blocks = _nt_store_blocks(_asm("enc_k256w_ragged.hip", tmp_path_factory), "encode_k256w_ragged")
    assert blocks and all(c == 4 for c in blocks), blocks


def test_reconstruct_n1024x_ragged_resources(tmp_path_factory):
    res = _summary(_asm("dec_n1024x_ragged.hip", tmp_path_factory), "reconstruct_n1024x_ragged")
    assert res["ScratchSize"] == 0 and res["NumVgprs"] <= 128, res
