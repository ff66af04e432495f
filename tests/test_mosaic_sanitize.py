"""Sanitizer + fuzz gate of the HIP-free host code of the mosaic layer (CPU suite): csrc/mosaic_host.cpp over csrc/map_host.cpp and
the stand-alone program tests/sanitize/fuzz_mosaic.cpp, built with gcc's ASan + UBSan the way test_map_sanitize.py builds its
binary.  Nothing here is loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_mosaic_fuzz_under_asan_ubsan(tmp_path):
    """300 seeded cases: 1 .. 8 passes of 1 .. 6 strip rows anywhere on the orbit, random options (some out of range: refused with a
    text), the common grid (polar passes and passes with nothing placed refused), the model blend through the grid's nodes and through
    nodes of any int32, one pass against the map layer's warp, bands of 16 .. 96 lines against one batch, every buffer exactly as long
    as the interface says: no sanitizer report, every accepted result within the rules."""
    exe = tmp_path / "fuzz_mosaic"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_mosaic.cpp"), str(CSRC / "mosaic_host.cpp"),
                        str(CSRC / "map_host.cpp"), str(CSRC / "picture_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "300", "23", str(GOLDEN / "map_tle.txt")], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 300 and rep["bad"] == 0
    # the draw covers refused options, refused grids, every count of passes, both plane counts and modes, wild nodes, overlapping passes
    assert rep["refused"] > 15 and rep["grid_refused"] > 15 and rep["grids"] > 100 and rep["most"] == 8 and rep["passes"] > 2 * rep["grids"], rep
    assert rep["grey"] > 30 and rep["colour"] > 30 and rep["feather"] > 30 and rep["best"] > 30 and rep["bands"] > 100 and rep["wild"] > 20, rep
    assert rep["single"] > 5 and rep["overlap"] > 1000, rep
