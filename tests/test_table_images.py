"""The device table images (csrc/table_images.hpp), CPU only: builds
tests/cpp/table_images_check.cpp against the library's host field code and
image builders with plain g++ and runs it.  Every image's length and SHA-256
must equal tests/golden/table_images.json (recorded from the upload loops the
builders replaced, not from the builders), and entries of the tower images read
back from their LdsTabs slots must be the tables the tower_sub_min rule names."""
import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "erasure-coding-crust_amd" / "csrc"
# fixed by the layout constants
LENGTHS = {"tower": 4 * 81920, "f9": 2 * 81920, "compact": 32768, "eimg512": 7 * 35840,
           "eimg256": 4 * 10240, "mslot": 65535 * 80}


def test_table_images(tmp_path):
    exe = tmp_path / "table_images_check"
    subprocess.run(["g++", "-std=c++17", "-O2", f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "table_images_check.cpp"),
                    str(CSRC / "gf_field.cpp"), str(CSRC / "table_images.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tower slots ok" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        if line.startswith("image "):
            _, name, nbytes, digest = line.split()
            got[name] = {"bytes": int(nbytes), "sha256": digest}
    golden = json.loads((ROOT / "tests" / "golden" / "table_images.json").read_text())
    assert {k: v["bytes"] for k, v in golden.items()} == LENGTHS
    assert got == golden
