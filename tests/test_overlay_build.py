"""What the compiler makes of csrc/overlay.hip for gfx950 (CPU suite: hipcc cross-compiles, no GPU needed): neither instance of
overlay_draw has a scratch segment, LDS holds one chunk of 256 records of 32 bytes and nothing else, and the registers leave room for
four waves per SIMD (profiles/overlay.md has the figures).  Only the kernels' metadata is read."""
from __future__ import annotations

import re
import subprocess

import pytest


@pytest.mark.timeout(300)
def test_overlay_kernels_have_no_scratch(tmp_path):
    from meteor_demod_amd import build
    out = tmp_path / "overlay.s"
    r = subprocess.run([build._hipcc(), *build.COMMON, "-x", "hip", "--offload-device-only", "-S", str(build.CSRC / "overlay.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)"
                         r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        seen[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sgprs=int(m.group(4)), vgprs=int(m.group(5)))
    print(seen)
    colour = next(v for k, v in seen.items() if "overlay_drawILi3E" in k)
    grey = next(v for k, v in seen.items() if "overlay_drawILi1E" in k)
    assert len(seen) == 2 and all(v["scratch"] == 0 for v in seen.values())
    assert colour["lds"] == 256 * 32 and grey["lds"] == 256 * 32
    assert colour["vgprs"] <= 128 and grey["vgprs"] <= 128                          # four waves per SIMD
