"""Sanitizer + fuzz gate of the HIP-free host code of the overlay layer (CPU suite): csrc/overlay_host.cpp and the stand-alone program
tests/sanitize/fuzz_overlay.cpp, built with gcc's ASan + UBSan the way test_mosaic_sanitize.py builds its binary.  Nothing here is
loaded into python, and nothing is preloaded; the binary and its vector files land in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_overlay_fuzz_under_asan_ubsan(tmp_path):
    """300 seeded cases: a shapefile or a text file, two in three hostile (truncated, lying lengths, part indices out of order, NaN,
    stray bytes), through the reader; polylines of any int32 vertices through the cut, the bins and the model, over every piece and
    tile by tile; polylines in degrees and a graticule through the whole-picture entry's model path in bands of 32 .. 96 lines against
    one batch; every buffer exactly as long as the interface says: no sanitizer report, every accepted result within the rules."""
    exe = tmp_path / "fuzz_overlay"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_overlay.cpp"), str(CSRC / "overlay_host.cpp"),
                        str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "300", "29", str(tmp_path)], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 300 and rep["bad"] == 0
    # the draw covers refused and accepted files of both formats, the cut with far vertices, and the bands
    assert rep["refused"] > 60 and rep["accepted"] > 100 and rep["shp"] > 30 and rep["txt"] > 30 and rep["banded"] == 300, rep
    assert rep["cut"] == 300 and rep["pieces"] > 1000 and rep["wild"] > 60 and rep["drawn"] > 10000, rep
