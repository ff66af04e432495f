"""Sanitizer + fuzz gate of the HIP-free host code of the polar layer (CPU suite): csrc/polar_host.cpp over csrc/mosaic_host.cpp and
csrc/map_host.cpp and the stand-alone program tests/sanitize/fuzz_polar.cpp, built with gcc's ASan + UBSan the way
test_mosaic_sanitize.py builds its binary.  Nothing here is loaded into python, and nothing is preloaded; the binary lands in a
temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_polar_fuzz_under_asan_ubsan(tmp_path):
    """300 seeded cases: 1 .. 4 passes of 1 .. 6 strip rows anywhere on the orbit, both poles, options in and out of range (refused
    with a text), frames with host nodes through both entries, the projection, the texts into buffers that just fit, graticules,
    vertices of random polylines, bands of 16 .. 96 lines against one batch: no sanitizer report, every accepted result within the
    rules."""
    exe = tmp_path / "fuzz_polar"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_polar.cpp"), str(CSRC / "polar_host.cpp"),
                        str(CSRC / "mosaic_host.cpp"), str(CSRC / "map_host.cpp"), str(CSRC / "picture_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "300", "29", str(GOLDEN / "map_tle.txt")], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 300 and rep["bad"] == 0
    # the draw covers refused options, refused frames (a pass across the equator, a forced pole on the other side), both poles, every
    # count of passes, nodes, bands, graticules and vertices
    assert rep["refused"] > 15 and rep["frame_refused"] > 15 and rep["frames"] > 100 and rep["north"] > 30 and rep["south"] > 30 and rep["most"] == 4, rep
    assert rep["passes"] > 2 * rep["frames"] and rep["nodes"] > 1000 and rep["bands"] == rep["frames"] and rep["graticules"] == rep["frames"], rep
    assert rep["lines"] > 50 and rep["vertices"] > 1000, rep
