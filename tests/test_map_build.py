"""What the compiler makes of csrc/map.hip for gfx950 (CPU suite: hipcc cross-compiles, no GPU needed): neither instance of map_warp has
a scratch segment, and LDS and VGPRs stay within the figures of profiles/map.md.  Only the kernels' metadata is read."""
from __future__ import annotations

import re
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_map_kernels_have_no_scratch(tmp_path):
    from meteor_demod_amd import build
    out = tmp_path / "map.s"
    r = subprocess.run([build._hipcc(), *build.COMMON, "-x", "hip", "--offload-device-only", "-S", str(build.CSRC / "map.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        seen[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)))
    print(seen)
    colour = next(v for k, v in seen.items() if "map_warpILi3E" in k)
    grey = next(v for k, v in seen.items() if "map_warpILi1E" in k)
    assert len(seen) == 2 and all(v["scratch"] == 0 for v in seen.values())
    # profiles/map.md: LDS holds the tables and nothing else; registers for 8 waves per SIMD (64 VGPRs)
    assert colour["lds"] == 768 and grey["lds"] == 256 and colour["vgprs"] <= 64 and grey["vgprs"] <= 64
    # and no more of them than before the sampling code moved to csrc/warp_device.h (profiles/map.md, "One warp sampler")
    assert colour["vgprs"] <= 46 and grey["vgprs"] <= 28
