"""What the compiler makes of csrc/sun.hip for gfx950 (CPU suite: hipcc cross-compiles, no GPU needed): one kernel, sun_apply, whose
LDS, register and scratch figures are the ones profiles/sun.md records.  Only the kernel's metadata is read."""
from __future__ import annotations

import re
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_sun_kernel_compiles_to_what_the_profile_records(tmp_path):
    from meteor_demod_amd import build
    out = tmp_path / "sun.s"
    r = subprocess.run([build._hipcc(), *build.COMMON, "-x", "hip", "--offload-device-only", "-S", str(build.CSRC / "sun.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)"
                         r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        seen[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sgprs=int(m.group(4)), vgprs=int(m.group(5)))
    print(seen)
    # mangled name -> the name the profile uses
    names = {"_Z9sun_apply7SunArgs": "sun_apply"}
    assert len(seen) == 1 and sorted(seen) == sorted(names)
    profile = (ROOT / "profiles" / "sun.md").read_text()
    for mangled, name in names.items():
        line = re.search(re.escape(f"`{name}`") + r": LDS (\d+) bytes, (\d+) VGPRs, (\d+) SGPRs, scratch (\d+) bytes", profile)
        assert line, f"profiles/sun.md does not record the figures of {name}"
        want = dict(zip(("lds", "vgprs", "sgprs", "scratch"), map(int, line.groups())))
        print(f"{name}: {seen[mangled]}; profiles/sun.md: {want}")
        assert seen[mangled] == want
        # no spills; the two lines of nodes of a strip row and the waves' partial counts, and registers that leave every wave slot open
        assert seen[mangled]["scratch"] == 0 and 2 * 99 * 4 <= seen[mangled]["lds"] <= 2 * 99 * 4 + 64 and seen[mangled]["vgprs"] <= 32
