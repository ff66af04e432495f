"""Sanitizer gate of the buffer set of the device entries (CPU suite): csrc/buffers.h alone, through the stand-alone program
tests/sanitize/buffers_test.cpp, built with gcc's ASan + UBSan the way test_png_sanitize.py builds its binary.  The header needs no
GPU runtime: g++ compiles it.  Nothing here is loaded into python, and nothing is preloaded; the binary lands in a temporary directory."""
from __future__ import annotations

import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
ASAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(120)
def test_buffer_set_under_asan_ubsan(tmp_path):
    """An output against an input and against a second output (refused), inputs that alias (accepted), NULL and empty ranges (they
    join nothing), ranges that only touch (accepted), one byte of overlap at either end (refused), and sets of 64 inputs with an
    output on the last byte of each in turn: every answer as the rule says, and no sanitizer report."""
    exe = tmp_path / "buffers_test"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *ASAN, "-I", str(CSRC), str(ROOT / "tests" / "sanitize" / "buffers_test.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["ok"] and rep["bad"] == 0 and rep["checks"] == 25 + 65 + 64 + 2
