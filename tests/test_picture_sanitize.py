"""Sanitizer + fuzz gate of the HIP-free host code of the picture layer (CPU suite): csrc/picture_host.cpp and the stand-alone program
tests/sanitize/fuzz_picture.cpp, built with gcc's ASan + UBSan the way test_image_sanitize.py builds its binary.  Nothing here is
loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_picture_fuzz_under_asan_ubsan(tmp_path):
    """600 seeded cases: random options (some out of range: refused with a text), masks, 0 .. 5 strip rows, grey and colour, random
    selections, pieces of 0 .. 6 rows, every buffer exactly as long as the interface says: no sanitizer report, every accepted
    result within the rules, the pieces equal to one batch."""
    exe = tmp_path / "fuzz_picture"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_picture.cpp"),
                        str(CSRC / "picture_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "600", "11"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 600 and rep["bad"] == 0
    # the draw covers refused options, empty pictures, both plane counts, identity and stretched tables, and maps of many widths
    assert rep["refused"] > 40 and rep["empty"] > 30 and rep["grey"] > 100 and rep["colour"] > 100 and rep["stretched"] > 100 and rep["identity"] > 50, rep
    assert rep["widths"] > 50 and rep["pieces"] > 300, rep
