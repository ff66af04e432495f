"""What the C host refuses, word for word and in which order, against the transcript tests/golden/cli_refusals.json (written by
tests/golden/make_cli_refusals.py from the commit before the host's options, checks and stages became functions of their own): per
case the exact stderr, the exact stdout and the exit status, and nothing written.  The host is built here against the stub back end
(no layer), against the stub with do-nothing frame, transfer-frame and image layers, and against that with the interleaved mode; the
tree's own program is the fourth binary.  gcc -Wall has nothing to say about either build.  No GPU is touched: every case ends before
the first input file is demodulated."""
from __future__ import annotations

import json
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, str(GOLDEN))
import make_cli_refusals as MCR  # noqa: E402

WANT = json.loads(MCR.OUT.read_text())


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    exes, said = MCR.build(ROOT, tmp_path_factory.mktemp("cli_refusals"))
    exes["lib"] = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    return exes, said


def test_the_transcript_holds_every_case():
    assert sorted(WANT) == sorted(MCR.CASES)
    assert "between the 0.5 % and 99.5 % points of its pixels\n" in WANT["help"]["stderr"] and WANT["help"]["status"] == 0


@pytest.mark.parametrize("case", list(MCR.CASES))
def test_cli_refusals_are_the_transcript(case, binaries, tmp_path):
    exes, said = binaries
    assert said == {name: "" for name in MCR.BINARIES}, said                 # no warning from gcc -std=gnu11 -Wall
    got = MCR.transcript(exes, case, tmp_path)
    print(got["stderr"], got["stdout"], got["status"], sep="")
    for part in ("stderr", "stdout", "status"):
        assert got[part] == WANT[case][part], f"{case}: {part}"
    assert got["new"] == [], f"{case}: the run left {got['new']} behind"
