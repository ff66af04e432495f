"""Sanitizer + fuzz gate of the HIP-free host code of the PNG encoder (CPU suite): csrc/png_host.cpp and the stand-alone program
tests/sanitize/fuzz_png.cpp, built with gcc's ASan + UBSan the way test_jpeg_sanitize.py builds its binary.  Nothing here is
loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_png_fuzz_under_asan_ubsan(tmp_path):
    """300 seeded cases: pictures of random sizes, masks, filters and segments (some out of range) through the model's filter and its
    whole file, and arrays of any bytes through its deflate stage; every buffer exactly as long as the interface says, out_room from 0
    to the bound: no sanitizer report, every refusal with its code and text, too little room answered with the bytes needed and
    nothing written, and every accepted stream inflates back, by the program's own inflater, to the bytes that went in."""
    exe = tmp_path / "fuzz_png"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_png.cpp"), str(CSRC / "png_host.cpp"),
                        str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "300", "31"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 300 and rep["bad"] == 0
    # the draw covers refusals, both entries, rooms that are too small, stored and dynamic segments, matches, masks, and long codes
    assert rep["refused"] > 30 and rep["accepted"] > 200 and rep["pictures"] == 150 and rep["arrays"] == 150, rep
    assert rep["short_rooms"] > 400 and rep["wild_segments"] > 5 and rep["masks"] > 40, rep
    assert rep["stored"] > 100 and rep["dynamic"] > 300 and rep["matches"] > 1000 and rep["max_bits"] >= 12, rep
