"""Sanitizer + fuzz gate of the HIP-free host code of the equalise layer (CPU suite): csrc/equalise_host.cpp and the stand-alone
program tests/sanitize/fuzz_equalise.cpp, built with gcc's ASan + UBSan the way test_jpeg_sanitize.py builds its binary.  Nothing here
is loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_equalise_fuzz_under_asan_ubsan(tmp_path):
    """400 seeded cases: pictures of random sizes, masks, tiles, clips, amounts and modes (some out of range) through the model's
    tables and its apply, out of place and in place; every buffer exactly as long as the interface says: no sanitizer report, every
    refusal with its code and text and nothing written, the counts add up, the tables rise to 255, uncounted pixels stay."""
    exe = tmp_path / "fuzz_equalise"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_equalise.cpp"), str(CSRC / "equalise_host.cpp"),
                        str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "400", "37"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 400 and rep["bad"] == 0
    # the draw covers refusals, masks of both steps, both layouts, the widest line and empty tiles
    assert rep["refused"] > 40 and rep["accepted"] > 250 and rep["masked"] > 150 and rep["step8"] > 50 and rep["colour"] > 100, rep
    assert rep["wide"] > 10 and rep["tiles"] > 5000 and rep["empty"] > 100 and rep["pixels"] > 500000, rep
