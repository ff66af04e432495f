"""The C host's product lines against transcripts (tests/golden/cli_products, written by tests/golden/make_cli_products.py from the
commit before the writers of --map, --mosaic and --map-proj stereo were put on shared helpers): exact stdout, exact stderr and exit
status, the names of the files written and the text of every .wld and .prj.  One CLI run per case."""
from __future__ import annotations

import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, str(GOLDEN))
import make_cli_products as MCP  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(MCP.CASES))
def test_cli_products_are_the_transcripts(case, tmp_path, gpu_device):
    got = MCP.transcript(ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd", case, tmp_path, gpu_device)
    print(got["stdout"], got["stderr"], sep="")
    for part in MCP.PARTS:
        assert got[part] == (MCP.OUT / f"{case}.{part}").read_text(), f"{case}.{part}"
