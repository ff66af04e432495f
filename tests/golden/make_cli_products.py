#!/usr/bin/env python3
"""Transcripts of what the C host says and writes for its picture, map, mosaic and polar products: tests/golden/cli_products/<case>.*.

    python tests/golden/make_cli_products.py <path of a meteor_demod_amd binary> [device]

runs every case of CASES with that binary on a GPU and writes, per case, the exact stdout (<case>.stdout), the exact stderr with the
exit status in a last line (<case>.stderr), the sorted names of the files the run wrote (<case>.files) and the text of every .wld
and .prj among them (<case>.sidecars).  Picture bytes are not recorded: the CLI tests of the layers hold those against the Python
entries.  tests/test_gpu_cli_products.py calls transcript() on the tree's binary and compares for equality, so the committed files are
recorded from the commit whose output is to be kept."""
from __future__ import annotations

import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

OUT = HERE / "cli_products"
PARTS = ("stdout", "stderr", "files", "sidecars")

_MAP = ("--cadu", "--image", "--map", "tle.txt", "--scan-angle", "108")
_STEREO = (*_MAP, "--map-proj", "stereo", "--map-res", "4000")
# case: (input files; "noise" in a name: a file without a frame, which gives no picture), flags
CASES = {
    "map_321_graticule": (("one.wav",), (*_MAP, "--map-scale", "60", "--composite", "321", "--graticule", "5")),
    "map_per_channel": (("one.wav",), (*_MAP, "--map-scale", "60")),
    "mosaic_auto_best": (("one.wav", "two.wav"), (*_MAP, "--map-scale", "60", "--composite", "auto", "--mosaic", "both", "--mosaic-blend", "best")),
    "stereo_mosaic_321_graticule": (("one.wav", "two.wav"), (*_STEREO, "--composite", "321", "--graticule", "5", "--mosaic", "both")),
    "stereo_per_channel_jpeg": (("one.wav",), (*_STEREO, "--jpeg", "85")),
    "mosaic_one_file_without_picture": (("one.wav", "noise.wav"), (*_MAP, "--map-scale", "60", "--composite", "321", "--mosaic", "both")),
    "stereo_mosaic_one_file_without_picture": (("one.wav", "noise.wav"), (*_STEREO, "--composite", "321", "--mosaic", "both")),
    "rectify_321_equalise": (("one.wav",), ("--image", "--rectify", "--composite", "321", "--equalise", "3", "--equalise-tile", "64")),
    "map_vcdu_sun": (("one.wav",), (*_MAP, "--vcdu", "--map-scale", "60", "--sun", "--sun-ref", "50")),
    "map_overlay_jpeg": (("one.wav",), (*_MAP, "--map-scale", "60", "--overlay", "coast.txt", "--overlay-colour", "00ff00", "--overlay-width", "2", "--jpeg", "85")),
    "mosaic_321_jpeg": (("one.wav", "two.wav"), (*_MAP, "--map-scale", "60", "--composite", "321", "--mosaic", "both", "--jpeg", "85")),
}
# the file of --overlay: two short polylines inside the grid of map_per_channel (lat 12.7 .. 16.5, lon 116.4 .. 140.6)
COAST = "120 13\n128 15\n136 16\n>\n125 16\n130 13.5\n"


def transcript(exe, case: str, workdir: Path, device: int = 0) -> dict:
    """One run of `exe` in the empty directory `workdir`: {part: text} for the parts of PARTS."""
    import frames_util as U
    import map_util as MU
    files, flags = CASES[case]
    _, iq = MU.recording()
    (workdir / "tle.txt").write_text((HERE / "map_tle.txt").read_text())
    (workdir / "coast.txt").write_text(COAST)
    for name in files:
        (workdir / name).write_bytes(U.wav_bytes(U.REC_SAMPLERATE, U.noise(len(iq), 5) if "noise" in name else iq))
    given = {p.name for p in workdir.iterdir()}
    # (one file alone would be named after the time of the run: it gets the name a run of several files gives it)
    named = ("-o", files[0] + ".s") if len(files) == 1 else ()
    p = subprocess.run([str(exe), "-q", "-B", "--device", str(device), *flags, *named, *files], capture_output=True, text=True, cwd=workdir, timeout=300)
    made = sorted(q.name for q in workdir.iterdir() if q.name not in given)
    sidecars = "".join(f"== {name}\n{(workdir / name).read_text()}" for name in made if name.endswith((".wld", ".prj")))
    return {"stdout": p.stdout, "stderr": p.stderr + f"exit status {p.returncode}\n", "files": "".join(n + "\n" for n in made), "sidecars": sidecars}


def main() -> None:
    import tempfile
    exe, device = Path(sys.argv[1]).resolve(), int(sys.argv[2]) if len(sys.argv) > 2 else 0
    OUT.mkdir(exist_ok=True)
    for case in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            got = transcript(exe, case, Path(tmp), device)
        for part in PARTS:
            (OUT / f"{case}.{part}").write_text(got[part])
        print(f"{case}: {len(got['stdout'].splitlines())} lines of stdout, {len(got['stderr'].splitlines()) - 1} of stderr, {len(got['files'].splitlines())} files")


if __name__ == "__main__":
    main()
