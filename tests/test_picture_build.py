"""What the compiler makes of csrc/picture.hip for gfx950 (CPU suite: hipcc cross-compiles, no GPU needed): neither kernel has a
scratch segment, and LDS and VGPRs stay within the figures of profiles/picture.md.  Only the kernels' metadata is read."""
from __future__ import annotations

import re
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_picture_kernels_have_no_scratch(tmp_path):
    from meteor_demod_amd import build
    out = tmp_path / "picture.s"
    r = subprocess.run([build._hipcc(), *build.COMMON, "-x", "hip", "--offload-device-only", "-S", str(build.CSRC / "picture.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        seen[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)))
    print(seen)
    hist = next(v for k, v in seen.items() if "picture_histogram" in k)
    colour = next(v for k, v in seen.items() if "picture_renderILi3E" in k)
    grey = next(v for k, v in seen.items() if "picture_renderILi1E" in k)
    assert len(seen) == 3 and all(v["scratch"] == 0 for v in seen.values())
    # profiles/picture.md: the histogram's bins; 8 lines of 3 (1) slots, the tables and the masks; four blocks of the colour kernel
    # on a CU's 160 KB, and registers for 8 waves per SIMD (64 VGPRs)
    assert hist["lds"] == 3 * 256 * 4 and hist["vgprs"] <= 32
    assert 3 * 8 * 1568 + 768 <= colour["lds"] <= 40 * 1024 and colour["vgprs"] <= 64
    assert 8 * 1568 + 256 <= grey["lds"] <= 14 * 1024 and grey["vgprs"] <= 64
