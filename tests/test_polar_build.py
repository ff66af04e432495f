"""What the compiler makes of csrc/polar.hip for gfx950 (CPU suite: hipcc cross-compiles, no GPU needed): one kernel, polar_nodes,
whose LDS, register and scratch figures are the ones profiles/polar.md records.  Only the kernel's metadata is read."""
from __future__ import annotations

import re
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_polar_nodes_compiles_to_what_the_profile_records(tmp_path):
    from meteor_demod_amd import build
    assert "-ffp-contract=off" in build.COMMON                                   # the Newton loop does not depend on what would be fused
    out = tmp_path / "polar.s"
    r = subprocess.run([build._hipcc(), *build.COMMON, "-x", "hip", "--offload-device-only", "-S", str(build.CSRC / "polar.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)"
                         r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        seen[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sgprs=int(m.group(4)), vgprs=int(m.group(5)))
    print(seen)
    assert len(seen) == 1 and "polar_nodes" in next(iter(seen))
    got = next(iter(seen.values()))
    line = re.search(r"polar_nodes: LDS (\d+) bytes, (\d+) VGPRs, (\d+) SGPRs, scratch (\d+) bytes", (ROOT / "profiles" / "polar.md").read_text())
    assert line, "profiles/polar.md does not record the kernel's figures"
    want = dict(zip(("lds", "vgprs", "sgprs", "scratch"), map(int, line.groups())))
    print(f"profiles/polar.md: {want}")
    assert got == want
    # a scratch segment would have to be explained there; double-precision functions are inlined: no call, no stack
    assert got["scratch"] == 0 and got["lds"] == 0 and "s_swappc" not in text and got["vgprs"] <= 256
