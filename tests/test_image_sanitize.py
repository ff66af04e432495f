"""Sanitizer + fuzz gate of the HIP-free host code of the image layer (CPU suite): csrc/image_host.cpp and the stand-alone program
tests/sanitize/fuzz_image.cpp, built with gcc's ASan + UBSan the way test_interleave_sanitize.py builds its binary.  Nothing here is
loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_image_fuzz_under_asan_ubsan(tmp_path):
    """2 000 seeded cases: VCDU batches as sent, mutated and random, the descriptors found in them and descriptors drawn at random,
    random options, the pieces of the host entry's model path and the placement, every buffer exactly as long as the interface says:
    no sanitizer report, every accepted result within the rules, every refusal MDEMOD_ERR_PARAM with a text."""
    exe = tmp_path / "fuzz_image"
    r = subprocess.run(["g++", "-std=c++17", *ASAN, "-I", str(ROOT / "include"), str(ROOT / "tests" / "sanitize" / "fuzz_image.cpp"),
                        str(CSRC / "image_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "2000", "11"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["cases"] == 2000 and rep["bad"] == 0
    # the draw covers accepted packets, refused options, truncated strips, descriptors outside the batch and clean strips
    assert rep["accepted"] > 10000 and rep["refused"] > 100 and rep["truncated"] > 200 and rep["outside"] > 2000 and rep["decoded"] > 5000, rep
    assert rep["placed"] > 2000 and rep["pieces"] > 1000, rep
