#!/usr/bin/env python3
"""Transcript of what the C host refuses, and in which order: tests/golden/cli_refusals.json.

    python tests/golden/make_cli_refusals.py <root of a checkout> [<its built meteor_demod_amd>]

builds the binaries of BINARIES from host/meteor_demod_amd.c of that checkout, runs every case of CASES and writes, per case, the exact
stderr, the exact stdout and the exit status.  tests/test_cli_refusals_host.py builds the same binaries from the tree, calls
transcript() and compares for equality, so the committed file is recorded from the commit whose behaviour is to be kept: the one before
the host's options, checks and stages were put into functions of their own.  No case reaches a GPU: every one ends before the first
input file is demodulated.

One line is not what that commit printed: its usage text held bare percent signs, which fprintf took for conversions.  In the "help"
case, and in the three refusals that print the usage text as well, the line of --rectify is that commit's text with the line put
right by hand (HELP_LINE below); the recorder does it after the run.

The binaries: "stub" is the host plus tests/sanitize/stub_backend.c, with no layer at all; "partial" adds do-nothing entries of the
frame, transfer-frame and image layers, so that --image passes its own check and the refusals behind it are reached; "interleave" adds
the interleaved mode's entries to that, for the two rules that come after its own check; "lib" is the tree's built program."""
from __future__ import annotations

import json
import re
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "cli_refusals.json"

_PARTIAL_C = """
#include "meteor_demod_amd_frames.h"
#include "meteor_demod_amd_rs.h"
#include "meteor_demod_amd_image.h"
void mdemod_frames_default_opts(mdemod_frames_opts *o) { (void)o; }
int mdemod_frames_decode_host(const mdemod_frames_opts *o, const int8_t *s, uint64_t m, uint8_t *c, mdemod_frame_info *f, uint64_t cap, uint64_t *n, int d)
{ (void)o; (void)s; (void)m; (void)c; (void)f; (void)cap; (void)d; *n = 0; return 0; }
void mdemod_rs_default_opts(mdemod_rs_opts *o) { (void)o; }
int mdemod_rs_decode_host(const mdemod_rs_opts *o, const uint8_t *c, uint64_t n, uint8_t *v, mdemod_rs_info *i, int d)
{ (void)o; (void)c; (void)n; (void)v; (void)i; (void)d; return 0; }
void mdemod_rs_vcdu_header(const uint8_t *v, mdemod_rs_header *out) { (void)v; (void)out; }
void mdemod_image_default_opts(mdemod_image_opts *o) { (void)o; }
int mdemod_image_decode_host(const mdemod_image_opts *o, const uint8_t *v, const mdemod_rs_info *i, uint64_t n, mdemod_image_result *out, int d)
{ (void)o; (void)v; (void)i; (void)n; (void)out; (void)d; return 0; }
void mdemod_image_free(mdemod_image_result *out) { (void)out; }
"""
_INTERLEAVE_C = """
#include "meteor_demod_amd_interleave.h"
void mdemod_il_default_opts(mdemod_il_opts *o) { (void)o; }
uint64_t mdemod_il_windows(uint64_t m) { return m; }
uint64_t mdemod_il_max_output_symbols(uint64_t m) { return m; }
int mdemod_il_decode_host(const mdemod_il_opts *o, const int8_t *s, uint64_t m, int8_t *out, uint64_t cap, mdemod_il_segment *g, uint64_t gc, uint64_t *ns,
                          uint64_t *np, int32_t *mean, int d)
{ (void)o; (void)s; (void)m; (void)out; (void)cap; (void)g; (void)gc; (void)ns; (void)np; (void)mean; (void)d; return 0; }
"""
# binary: the generated C files linked beside the host and the stub ("lib" is not built here)
BINARIES = {"stub": (), "partial": (_PARTIAL_C,), "interleave": (_PARTIAL_C, _INTERLEAVE_C)}

HELP_LINE = "                           than 1568) and contrast-stretched between the 0.5 % and 99.5 % points of its pixels\n"

_IMG, _MAP = ("--image",), ("--image", "--map", "tle.txt")


def _one(*flags):
    """The usual run: one input file, quiet, the output named."""
    return ("-q", "-o", "out.s", *flags, "in.wav")


_NINE = tuple("abcdefghi")
# (binary, arguments).  First the values the option loop refuses, then every rule of the checks, then two rules broken at once (the
# first one wins), then what leaves without a refusal.
_LIST = [
    # ---- values
    ("stub", ("--devices", "0,x", "--plan", "a")), ("stub", _one("--jobs", "0")),
    ("stub", _one("--apids", "64,65")), ("stub", _one("--apids", "64,64,65")), ("stub", _one("--apids", "63,65,66")), ("stub", _one("--apids", "64,65,70")),
    ("stub", _one("--apids", "64,65,66,67")),
    ("stub", _one("--composite", "421")), ("stub", _one("--composite", "32")),
    ("stub", _one("--altitude", "-1")), ("stub", _one("--altitude", "x")), ("stub", _one("--scan-angle", "0")), ("stub", _one("--scan-angle", "1x")),
    ("stub", _one("--norad", "0")), ("stub", _one("--norad", "abc")), ("stub", _one("--norad", "1000000000")),
    ("stub", _one("--map-scale", "x")), ("stub", _one("--time-offset", "1s")),
    ("stub", _one("--date", "2024-13-01")), ("stub", _one("--date", "2024-1")), ("stub", _one("--date", "1956-01-01")), ("stub", _one("--date", "2024-01-01x")),
    ("stub", _one("--scan-side", "2")),
    ("stub", _one("--overlay", "a", "--overlay", "b", "--overlay", "c", "--overlay", "d")),
    ("stub", _one("--graticule", "0.001")), ("stub", _one("--graticule", "91")), ("stub", _one("--graticule", "x")),
    ("stub", _one("--overlay-colour", "12345")), ("stub", _one("--overlay-colour", "gggggg")),
    ("stub", _one("--overlay-width", "17")), ("stub", _one("--overlay-width", "-1")), ("stub", _one("--overlay-width", "2px")),
    ("stub", _one("--jpeg", "0")), ("stub", _one("--jpeg", "101")), ("stub", _one("--jpeg", "5x")),
    ("stub", _one("--equalise", "0.5")), ("stub", _one("--equalise", "257")), ("stub", _one("--equalise", "")),
    ("stub", _one("--equalise-tile", "20")), ("stub", _one("--equalise-tile", "8")), ("stub", _one("--equalise-tile", "520")),
    ("stub", _one("--equalise-amount", "101")), ("stub", _one("--equalise-amount", "-1")),
    ("stub", _one("--sun-ref", "81")), ("stub", _one("--sun-ref", "-1")), ("stub", _one("--sun-limit", "59")), ("stub", _one("--sun-limit", "90")),
    ("stub", _one("--map-proj", "mercator")),
    ("stub", _one("--map-res", "x")), ("stub", _one("--map-res", "99")), ("stub", _one("--map-res", "100001")), ("stub", _one("--map-res", "auto")),
    ("stub", _one("--map-lon0", "x")), ("stub", _one("--map-lon0", "361")),
    ("stub", _one("--map-lat-ts", "0")), ("stub", _one("--map-lat-ts", "91")), ("stub", _one("--map-lat-ts", "7o")),
    ("stub", _one("--mosaic-blend", "mean")),
    ("stub", _one("--offset", "x")), ("stub", _one("--offset", "3q")), ("stub", _one("--decimate", "0")), ("stub", _one("--decimate", "2x")),
    ("stub", _one("--tui-selftest")), ("stub", _one("--carrier-seed", "x")), ("stub", _one("--nonsense")), ("stub", ("-q",)),
    # ---- the checks, one rule each
    ("stub", ("-q", "-o", "out.s", "a", "b")), ("stub", ("-q", "--stdout", "a", "b")),
    ("stub", _one("--offset", "1k")), ("stub", _one("--decimate", "2")), ("stub", _one("--scan")),
    ("stub", _one("--cadu", "--stdout")), ("stub", _one("--cadu")), ("stub", _one("--vcdu", "--stdout")), ("stub", _one("--vcdu")),
    ("stub", _one(*_MAP, "--map-proj", "stereo")), ("stub", _one("--map-res", "1000")), ("stub", _one("--map-lon0", "auto")),
    ("lib", _one(*_MAP, "--map-proj", "stereo", "--map-scale", "60")),
    ("stub", _one("--mosaic", "m")), ("stub", _one("--overlay", "coast.txt")), ("stub", _one("--graticule", "auto")), ("stub", _one("--overlay-colour", "ff0000")),
    ("stub", _one("--map", "tle.txt")),
    ("stub", _one("--apids", "64,65,66")), ("stub", _one("--image", "--stdout")), ("stub", _one("--image")),
    ("stub", _one("--rectify")), ("stub", _one("--composite", "321")), ("stub", _one("--composite", "auto")),
    ("lib", _one("--map", "tle.txt")), ("stub", _one("--norad", "5")), ("stub", _one("--map-proj", "latlon")),
    ("partial", _one(*_IMG, "--norad", "5")), ("partial", _one(*_IMG, "--time-offset", "0")), ("partial", _one(*_IMG, "--scan-side", "-1")),
    ("lib", _one(*_IMG, "--mosaic", "m")), ("lib", _one(*_MAP, "--mosaic-blend", "best")),
    ("lib", _one(*_IMG, "--graticule", "5")), ("lib", _one(*_IMG, "--overlay", "coast.txt")), ("lib", _one(*_MAP, "--overlay-width", "2")),
    ("stub", _one("--equalise-tile", "64")), ("stub", _one("--equalise-amount", "50")), ("stub", _one("--equalise", "3")),
    ("partial", _one(*_IMG, "--equalise", "3")),
    ("stub", _one("--sun-ref", "50")), ("stub", _one("--sun-limit", "80")), ("stub", _one("--sun")), ("partial", _one(*_IMG, "--sun")),
    ("partial", _one(*_IMG, "--rectify", "--equalise", "3")),
    ("stub", _one("--jpeg", "50")), ("partial", _one(*_IMG, "--jpeg", "50")),
    ("lib", ("-q", *_MAP, "--mosaic", "m", *_NINE)),
    ("lib", _one("--image", "--map", "/nonexistent")), ("lib", _one("--image", "--map", "coast.txt")), ("lib", _one(*_MAP, "--norad", "12345")),
    ("lib", _one(*_MAP, "--map-scale", "5000")), ("lib", _one(*_MAP, "--map-scale", "0")), ("lib", _one(*_MAP, "--scan-angle", "170")),
    ("lib", _one(*_MAP, "--overlay", "/nonexistent")), ("lib", _one(*_MAP, "--overlay", "coast.txt", "--overlay", "tle.txt")),
    ("partial", _one(*_IMG, "--altitude", "800")), ("partial", _one(*_IMG, "--scan-angle", "100")), ("lib", _one(*_MAP, "--altitude", "800")),
    ("partial", _one(*_IMG, "--rectify")), ("partial", _one(*_IMG, "--composite", "321")),
    ("lib", _one(*_IMG, "--rectify", "--altitude", "100")), ("lib", _one(*_IMG, "--rectify", "--scan-angle", "140")),
    ("stub", _one("--diff")), ("stub", _one("--skew")), ("stub", _one("--int", "--stdout")), ("stub", _one("--int")),
    ("partial", _one("--cadu", "--int")), ("interleave", _one("--cadu", "--int", "--int-delay", "0")), ("interleave", _one("--vcdu", "--int", "--int-delay", "x")),
    ("partial", _one("--cadu", "--diff")), ("partial", _one("--image", "--skew")),
    ("lib", ("-q", "-o", "out.s", "--offset", "auto", "-")), ("lib", ("-q", "-o", "out.s", "--scan", "-")),
    ("stub", _one("--plan")),
    ("stub", ("-q", "-o", "out.s", "nonexistent.wav")), ("stub", ("-q", "-o", "out.s", "coast.txt")),
    # ---- two rules broken at once: the first one wins
    ("stub", ("-q", "-o", "out.s", "--equalise", "3", "--jpeg", "50", "x")),
    ("stub", ("-q", "-o", "out.s", "--image", "--map", "/nonexistent", "--sun", "x")),
    ("stub", ("-q", "-o", "out.s", "--image", "--rectify", "--altitude", "-1", "x")),
    ("stub", ("-q", "-o", "out.s", "--image", "--diff", "x")),
    ("stub", ("-q", "-o", "out.s", "--cadu", "--stdout", "x")),
    ("stub", _one("--offset", "auto", "--scan")), ("stub", _one("--vcdu", "--cadu", "--stdout")), ("stub", _one("--vcdu", "--image")),
    ("stub", _one("--map-res", "500", "--mosaic", "m")), ("stub", _one("--mosaic", "m", "--overlay", "coast.txt", "--map", "tle.txt")),
    ("stub", _one("--overlay", "coast.txt", "--map", "tle.txt")), ("stub", _one("--apids", "64,65,66", "--rectify")),
    ("stub", _one("--rectify", "--norad", "5")), ("stub", _one("--equalise-tile", "64", "--sun-ref", "50")), ("stub", _one("--sun", "--jpeg", "50")),
    ("stub", _one("--diff", "--int")), ("stub", _one("--jobs", "0", "--apids", "1")), ("stub", _one("--apids", "1", "--jobs", "0")),
    ("stub", ("-q", "-o", "out.s", "--offset", "1k", "a", "b")), ("stub", _one("--int", "--stdout", "--plan")),
    ("partial", _one(*_IMG, "--sun", "--equalise", "3")), ("partial", _one(*_IMG, "--jpeg", "50", "--rectify")),
    ("partial", _one(*_IMG, "--rectify", "--int")), ("partial", _one("--cadu", "--int", "--diff")), ("partial", _one(*_IMG, "--altitude", "800", "--composite", "321")),
    ("partial", _one(*_IMG, "--mosaic-blend", "best", "--norad", "5")), ("partial", _one(*_IMG, "--sun", "--sun-ref", "50", "--jpeg", "50")),
    ("interleave", _one("--cadu", "--int", "--int-delay", "0", "--skew")), ("interleave", _one("--cadu", "--int", "--skew", "--diff")),
    ("lib", ("-q", "--image", "--map", "/nonexistent", "--mosaic", "m", *_NINE)),
    ("lib", _one("--image", "--map", "/nonexistent", "--overlay", "/nonexistent")), ("lib", _one(*_MAP, "--overlay", "/nonexistent", "--altitude", "800")),
    ("lib", _one(*_MAP, "--map-scale", "5000", "--rectify", "--altitude", "100")), ("lib", _one(*_MAP, "--sun-ref", "50", "--overlay-width", "2")),
    ("lib", ("-q", "-o", "out.s", "--offset", "auto", "--plan", "-")),
    # ---- no refusal, and no work either
    ("stub", ("-v",)), ("lib", ("-v",)), ("stub", ("--devices", "0,1", "--plan", "a", "b", "c")), ("lib", ("--devices", "0,1", "--plan", "a", "b", "c")),
    ("stub", ("--devices", "3,1,2", "--plan", "a")), ("stub", ("--plan", "a", "b")), ("stub", ("--help",)),
    # (--skew beside --int: a warning, and the run goes on - here to the plan, which writes nothing)
    ("interleave", ("-q", "-o", "out.s", "--cadu", "--int", "--skew", "--devices", "0", "--plan", "in.wav")),
]
CASES = {f"{binary}: {' '.join(args)}": (binary, args) for binary, args in _LIST}
assert len(CASES) == len(_LIST)
CASES["help"] = CASES.pop("stub: --help")


def build(root: Path, workdir: Path) -> tuple[dict, dict]:
    """The binaries of BINARIES from the host source under `root`, into `workdir`: ({name: path}, {name: what gcc said})."""
    exes, said = {}, {}
    for name, parts in BINARIES.items():
        extra = []
        for k, text in enumerate(parts):
            extra.append(workdir / f"{name}_{k}.c")
            extra[-1].write_text(text)
        exes[name] = workdir / f"cli_{name}"
        r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(root / "include"), str(root / "host" / "meteor_demod_amd.c"),
                            str(root / "tests" / "sanitize" / "stub_backend.c"), *map(str, extra), "-pthread", "-lm", "-o", str(exes[name])], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        said[name] = r.stderr
    return exes, said


def transcript(exes: dict, case: str, workdir: Path) -> dict:
    """One run in the empty directory `workdir`: the exact stderr and stdout, the exit status, and the names the run left behind
    ("new": empty for every case)."""
    import struct
    binary, args = CASES[case]
    n = 16384
    head = b"RIFF" + struct.pack("<I", 36 + 4 * n) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 288000, 288000 * 4, 4, 16) + b"data" + struct.pack("<I", 4 * n)
    (workdir / "in.wav").write_bytes(head + bytes(4 * n))
    (workdir / "tle.txt").write_text((HERE / "map_tle.txt").read_text())
    (workdir / "coast.txt").write_text("10 50\n11 51\n12 50\n")
    given = {p.name for p in workdir.iterdir()}
    # (the program's own name stands in the usage text and in getopt's messages: the same one for every binary)
    p = subprocess.run(["meteor_demod_amd", *args], executable=str(exes[binary]), capture_output=True, text=True, cwd=workdir, stdin=subprocess.DEVNULL, timeout=60)
    return {"stderr": p.stderr, "stdout": p.stdout, "status": p.returncode, "new": sorted(q.name for q in workdir.iterdir() if q.name not in given)}


def main() -> None:
    import tempfile
    root = Path(sys.argv[1]).resolve()
    with tempfile.TemporaryDirectory() as tmp:
        exes, _ = build(root, Path(tmp))
        exes["lib"] = Path(sys.argv[2]).resolve() if len(sys.argv) > 2 else root / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
        out = {}
        for case in CASES:
            with tempfile.TemporaryDirectory() as run:
                got = transcript(exes, case, Path(run))
            assert not got.pop("new"), case
            out[case] = got
    mended = 0
    for got in out.values():
        got["stderr"], n = re.subn(r"^ +than 1568\) and contrast-stretched between the .*\n", HELP_LINE, got["stderr"], flags=re.M)
        mended += n
    assert mended == 4 and HELP_LINE in out["help"]["stderr"]
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    print(f"{len(out)} cases, {sum(1 for v in out.values() if v['status'])} of them refusals")


if __name__ == "__main__":
    main()
