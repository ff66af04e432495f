"""GPU test of the C host's --int / --int-delay (include/meteor_demod_amd_interleave.h): an OQPSK recording built like
link_util.recording from an interleaved channel stream (M = 8) of Reed-Solomon coded frames, through -m oqpsk --int --int-delay 8
--vcdu, plain and with --diff: the .vcdu holds the VCDUs that were sent, the interleaver's line is on stdout, --skew beside --int is
noted and ignored, and --int is refused with --stdout and without --cadu / --vcdu."""
from __future__ import annotations

import re
import subprocess

import pytest

import frames_util as U
import interleave_util as IU

pytestmark = pytest.mark.gpu


def _cli():
    from conftest import ROOT
    return str(ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd")


@pytest.mark.parametrize("differential", [False, True], ids=["plain", "diff"])
def test_cli_oqpsk_int_vcdu(differential, tmp_path, gpu_device):
    st, iq = IU.recording(differential)
    wav = tmp_path / "pass.wav"
    wav.write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    out = tmp_path / "pass.s"
    flags = ["--diff"] if differential else ["--skew"]                       # (--skew beside --int: accepted, noted, ignored)
    p = subprocess.run([_cli(), "-q", "-B", "-m", "oqpsk", "--device", str(gpu_device), "--int", "--int-delay", str(IU.REC_M), "--vcdu", *flags,
                        "-o", str(out), str(wav)], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    lines = p.stdout.strip().splitlines()
    line = next(ln for ln in lines if "interleaver:" in ln)
    found = re.search(r"interleaver: (\d+) segments, (\d+) periods, mean sync score (-?\d+) / 24576", line)
    # (the .s begins at the demodulator's lock and ends with its last whole read: some periods fewer than were sent)
    assert found and int(found.group(1)) >= 1 and st.periods - 200 <= int(found.group(2)) <= st.periods and int(found.group(3)) > 24576 // 2
    assert ("--skew: ignored with --int" in p.stderr) == (not differential)
    got = (tmp_path / "pass.vcdu").read_bytes()
    assert f"{len(st.vcdus)} frames, 0 uncorrectable" in lines[-1]
    assert got == b"".join(bytes(v) for v in st.vcdus)
    assert not (tmp_path / "pass.cadu").exists()                             # (written only with --cadu)
    # the same file through the Python layer: the same bytes
    from meteor_demod_amd import frames
    cadu, rep = frames.decode_file(out, device=gpu_device, interleaved=True, branch_delay=IU.REC_M, differential=differential)
    assert rep.frames == len(st.vcdus) and cadu == b"".join(st.frames)


def test_cli_int_refusals(tmp_path, gpu_device):
    raw = tmp_path / "x.raw"
    raw.write_bytes(bytes(65536))
    base = [_cli(), "-q", "-B", "-s", "288000", "--device", str(gpu_device)]
    for more in ([], ["--vcdu"]):
        p = subprocess.run([*base, "--int", *more, "--stdout", str(raw)], capture_output=True, cwd=tmp_path, timeout=60)
        assert p.returncode == 1 and b"not with --stdout" in p.stderr and p.stdout == b""
        assert more or b"--int: not with --stdout" in p.stderr
    p = subprocess.run([*base, "--int", "-o", str(tmp_path / "o.s"), str(raw)], capture_output=True, cwd=tmp_path, timeout=60)
    assert p.returncode == 1 and b"--int: only with --cadu or --vcdu" in p.stderr
    p = subprocess.run([*base, "--int", "--int-delay", "0", "--cadu", "-o", str(tmp_path / "o.s"), str(raw)], capture_output=True, cwd=tmp_path, timeout=60)
    assert p.returncode == 1 and b"--int-delay" in p.stderr
    assert not (tmp_path / "o.s").exists()
