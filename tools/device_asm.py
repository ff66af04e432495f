#!/usr/bin/env python3
"""Device assembly of every unit of the product library that holds kernels, for comparing two trees (needs no GPU).

    python tools/device_asm.py OUTDIR [TREE]

compiles each unit of TREE (default: this tree) with the flags of its `meteor_demod_amd/build.py` to gfx950 assembly
(`--offload-device-only -S`) and writes OUTDIR/<unit>.s without the `__hip_cuid_` lines, which differ from compile to
compile.  Run it for two trees and `diff -r` the directories: a host-side refactor leaves every file identical.
"""
import importlib.util
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

out = Path(sys.argv[1])
tree = Path(sys.argv[2] if len(sys.argv) > 2 else Path(__file__).resolve().parent.parent).resolve()
spec = importlib.util.spec_from_file_location("tree_build", tree / "meteor_demod_amd" / "build.py")
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)

UNITS = {"demod_kernel": [], "demod_kernel_rot": b.ROT_FLAGS, "demod_kernel_rotp": b.ROTP_FLAGS,
         "demod_kernel_gat": ["-fno-slp-vectorize"],
         "demod_kernel_lat": ["-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=max-ilp"],
         "demod_aux": [], "recording": [], "frontend": [], "survey": []}


def one(item):
    stem, extra = item
    text = subprocess.run([b._hipcc(), *b.COMMON, *extra, "-x", "hip", "--offload-device-only", "-S",
                           str(b.CSRC / (stem + ".hip")), "-o", "-"], capture_output=True, text=True, check=True).stdout
    (out / (stem + ".s")).write_text("".join(l for l in text.splitlines(True) if "__hip_cuid_" not in l))
    return stem


out.mkdir(parents=True, exist_ok=True)
with ThreadPoolExecutor(4) as pool:
    for stem in pool.map(one, UNITS.items()):
        print(stem, flush=True)
