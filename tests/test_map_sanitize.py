"""Sanitizer + fuzz gate of the HIP-free host code of the map layer (CPU suite): csrc/map_host.cpp and the stand-alone program
tests/sanitize/fuzz_map.cpp, built with gcc's ASan + UBSan the way test_picture_sanitize.py builds its binary.  Nothing here is
loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_map_fuzz_under_asan_ubsan(tmp_path):
    """300 seeded cases: the TLE parser on mutated text, random placements and stamps through the time fit, random options (some out
    of range: refused with a text), grids of passes of 1 .. 6 strip rows anywhere on the orbit (polar ones refused), every node
    back through the forward function, the model warp (sometimes through nodes of any int32), bands of 16 .. 96 lines against one
    batch, every buffer exactly as long as the interface says: no sanitizer report, every accepted result within the rules."""
    exe = tmp_path / "fuzz_map"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_map.cpp"), str(CSRC / "map_host.cpp"),
                        str(CSRC / "picture_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "300", "17", str(GOLDEN / "map_tle.txt")], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 300 and rep["bad"] == 0
    # the draw covers accepted and refused element sets, refused options, polar passes, both plane counts, present and missing nodes
    assert rep["tle_ok"] > 100 and rep["tle_refused"] > 1000 and rep["refused"] > 30 and rep["polar"] > 10 and rep["grids"] > 100, rep
    assert rep["grey"] > 30 and rep["colour"] > 30 and rep["bands"] > 100 and rep["nodes_there"] > 1000 and rep["nodes_missing"] > 100, rep
