#!/usr/bin/env python3
"""Generates tests/golden/live_reference.json from the REAL reference.

Runs only where oracle/_ref was built (oracle/Makefile, from the reference's own
sources).  The tests that meet the reference live - tests/test_oracle_vs_live_reference.py
and test_hip_equals_the_live_reference in tests/test_gpu_parity.py - draw their
settings from seeds; this runs the reference on exactly those inputs and records
the sha256 of what it produced (soft symbols, per-symbol trace, .s files), so the
same tests check the same bytes on a checkout without the reference.

What is committed is data only: digests and symbol / byte counts.
"""
from __future__ import annotations

import hashlib
import json
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE.parent))

import oracle_py as O                                      # noqa: E402
import test_gpu_parity as P                                # noqa: E402
import test_oracle_vs_live_reference as L                  # noqa: E402
from golden_cases import sha                               # noqa: E402


def main() -> None:
    if not O.have_ref() or not O.REF_BINARY.exists():
        raise SystemExit("oracle/_ref is not built: run `make -C oracle` where the reference's sources are")
    out = {"generator": "tests/golden/make_live_digests.py", "restatement": {}, "file_model": {}, "hip": {}}
    for seed in (11, 12, 13, 14):
        rows = []
        for cfg, _s, iq in L.restatement_cases(seed):
            soft, trace = O.ref_demod(cfg, iq, want_trace=True)
            rows.append({"symbols": int(soft.shape[0]), "soft": sha(soft), "trace": sha(trace)})
        out["restatement"][str(seed)] = rows
    with tempfile.TemporaryDirectory() as td:
        for case, _cfg, container, args, _body, data in L.file_cases():
            inp, res = Path(td) / f"in.{container}", Path(td) / "out.s"
            inp.write_bytes(data)
            subprocess.run([str(O.REF_BINARY), "-q", "-B", "-o", str(res), *args, str(inp)], check=True, capture_output=True, timeout=120)
            got = res.read_bytes()
            out["file_model"][str(case)] = {"bytes": len(got), "sha256": hashlib.sha256(got).hexdigest()}
    for seed in (21, 22):
        rows = []
        for cfg, iq in P.live_reference_cases(seed):
            soft = O.ref_demod(cfg, iq)[0]
            rows.append({"symbols": int(soft.shape[0]), "soft": sha(soft)})
        out["hip"][str(seed)] = rows
    (HERE / "live_reference.json").write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", HERE / "live_reference.json", {k: len(v) for k, v in out.items() if isinstance(v, dict)})


if __name__ == "__main__":
    main()
