"""What the compiler makes of csrc/image.hip for gfx950 (CPU suite: hipcc cross-compiles, no GPU needed): image_decode keeps its
64-entry arrays in LDS, so it has no scratch segment; the figures are those of profiles/image.md."""
from __future__ import annotations

import re
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_image_decode_has_no_scratch(tmp_path):
    from meteor_demod_amd import build
    out = tmp_path / "image.s"
    r = subprocess.run([build._hipcc(), *build.COMMON, "-x", "hip", "--offload-device-only", "-S", str(build.CSRC / "image.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        seen[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)))
    print(seen)
    decode = next(v for k, v in seen.items() if "image_decode" in k)
    assert decode["scratch"] == 0 and 16384 + 8192 <= decode["lds"] <= 32768 and decode["vgprs"] <= 256
    assert {k for k in seen if "packets_" in k} and all(v["scratch"] == 0 for v in seen.values())
