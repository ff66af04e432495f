"""What the compiler makes of csrc/equalise.hip for gfx950 (CPU suite: hipcc cross-compiles, no GPU needed): six kernels, three
instances each of equalise_tables and equalise_apply, whose LDS, register and scratch figures are the ones profiles/equalise.md
records.  Only the kernels' metadata is read."""
from __future__ import annotations

import re
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_equalise_kernels_compile_to_what_the_profile_records(tmp_path):
    from meteor_demod_amd import build
    out = tmp_path / "equalise.s"
    r = subprocess.run([build._hipcc(), *build.COMMON, "-x", "hip", "--offload-device-only", "-S", str(build.CSRC / "equalise.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)"
                         r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        seen[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sgprs=int(m.group(4)), vgprs=int(m.group(5)))
    print(seen)
    # mangled name -> the name the profile uses
    names = {"_Z15equalise_tablesILi1ELi1EEv6EqArgs": "equalise_tables<1, 1>", "_Z15equalise_tablesILi3ELi1EEv6EqArgs": "equalise_tables<3, 1>",
             "_Z15equalise_tablesILi3ELi3EEv6EqArgs": "equalise_tables<3, 3>", "_Z14equalise_applyILi1ELi1ELb0EEv6EqArgs": "equalise_apply<1, 1, false>",
             "_Z14equalise_applyILi3ELi1ELb1EEv6EqArgs": "equalise_apply<3, 1, true>", "_Z14equalise_applyILi3ELi3ELb0EEv6EqArgs": "equalise_apply<3, 3, false>"}
    assert len(seen) == 6 and sorted(seen) == sorted(names)
    profile = (ROOT / "profiles" / "equalise.md").read_text()
    for mangled, name in names.items():
        line = re.search(re.escape(f"`{name}`") + r": LDS (\d+) bytes, (\d+) VGPRs, (\d+) SGPRs, scratch (\d+) bytes", profile)
        assert line, f"profiles/equalise.md does not record the figures of {name}"
        want = dict(zip(("lds", "vgprs", "sgprs", "scratch"), map(int, line.groups())))
        print(f"{name}: {seen[mangled]}; profiles/equalise.md: {want}")
        assert seen[mangled] == want
        # no spills; per-wave histograms of every channel, or the four tables of every channel
        assert seen[mangled]["scratch"] == 0 and seen[mangled]["lds"] <= (4 * 3 * 256 * 4 + 256 if "tables" in name else 3072) and seen[mangled]["vgprs"] <= 64
