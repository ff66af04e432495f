"""Sanitizer + fuzz gate of the HIP-free host code of the sun layer (CPU suite): csrc/sun_host.cpp over csrc/map_host.cpp and the
stand-alone program tests/sanitize/fuzz_sun.cpp, built with gcc's ASan + UBSan the way test_equalise_sanitize.py builds its binary.
Nothing here is loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_sun_fuzz_under_asan_ubsan(tmp_path):
    """300 seeded cases: passes of random sizes, dates, scan angles and sun options (some out of range) through the nodes, gain
    tables with missing nodes through the model's apply under every slot mask (some out of range), out of place and in place, and the
    host entry's model with random APIDs; every buffer exactly as long as the interface says: no sanitizer report, every refusal
    with its code and text and nothing written, the counts and the copied cells as the header says."""
    exe = tmp_path / "fuzz_sun"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_sun.cpp"), str(CSRC / "sun_host.cpp"),
                        str(CSRC / "map_host.cpp"), str(CSRC / "picture_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "300", "23", str(GOLDEN / "map_tle.txt")], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 300 and rep["bad"] == 0
    # the draw covers refusals of every kind, tables with missing nodes, every mask, in place, and passes with nodes off the Earth
    assert rep["refused"] > 40 and rep["accepted"] > 180 and rep["missing_tables"] > 50 and rep["in_place"] > 60 and min(rep["masks"]) > 10, rep
    assert rep["node_tables"] > 100 and rep["nodes_off_earth"] > 0 and rep["hosts"] > 50 and rep["pixels"] > 5000000 and rep["saturated"] > 100000, rep
