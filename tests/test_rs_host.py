"""CPU tests of the transfer-frame layer (include/meteor_demod_amd_rs.h): the constants of the specification, the host model
(csrc/rs_host.cpp) against words it must and must not correct, the header fields, the exports and layouts of the new entries, the
C host linked without them, and a sanitizer fuzz of the model.  No GPU is touched."""
from __future__ import annotations

import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import frames_util as U
import rs_util as R
from conftest import ROOT

CSRC = ROOT / "meteor_demod_amd" / "csrc"
HEADER = ROOT / "include" / "meteor_demod_amd_rs.h"
RS_SOURCES = [CSRC / "rs.hip", CSRC / "rs_host.cpp"]


# ------------------------------------------------------------------------------------------------------------- constants
def test_generator_and_parity_check_value():
    from meteor_demod_amd import rs
    g = rs.model_generator()
    assert bytes(g).hex() == "015b7f56101e0deb61a5082a3656ab207120ab56362a08a561eb0d1e10567f5b01"
    assert np.array_equal(g, g[::-1])                                          # self-reciprocal
    assert [int(R.LOG[x]) for x in g[:17]] == [0, 249, 59, 66, 4, 43, 126, 251, 97, 30, 3, 213, 50, 66, 170, 5, 24]
    # its roots are alpha^(11 j), j = 112 .. 143: the generator as a word has 32 zero syndromes
    assert not R.syndromes(np.concatenate([np.zeros(255 - 33, dtype=np.uint8), g[::-1]])).any()
    assert bytes(rs.model_parity(np.arange(223))).hex() == "2fbd4fb4748494b9acd554627212eeb3ebed41191de1d36320ea49290b25abcf"


def test_randomiser_sequence():
    from meteor_demod_amd import rs
    p = rs.pn()
    assert bytes(p[:8]).hex() == "ff480ec09a0d70bc"
    assert np.array_equal(p, R.pn_numpy())
    # the period is 255 bytes (the register runs on into the same bytes) and no less
    assert np.array_equal(R.pn_numpy(1020), np.tile(p, 4))
    assert all(not np.array_equal(p, np.roll(p, s)) for s in range(1, 255))
    v = np.zeros(892, dtype=np.uint8)
    c = rs.model_encode(v, derandomise=1)
    assert bytes(c[:4]) == U.MARKER and np.array_equal(c[4: 4 + 892], np.tile(p, 4)[:892])      # zeros (parity zero too) show the sequence
    assert np.array_equal(c[4:], np.tile(p, 4))
    assert not rs.model_encode(v, derandomise=0)[4:].any()


def test_dual_basis_table():
    from meteor_demod_amd import rs
    t, tinv = rs.model_dual()
    assert bytes(t[:16]).hex() == "007bafd499e2364dfa81552e6318ccb7"
    assert sorted(t) == list(range(256)) and np.array_equal(tinv[t], np.arange(256))
    tal = [0x8D, 0xEF, 0xEC, 0x86, 0xFA, 0x99, 0xAF, 0x7B]
    for i in (1, 2, 0x80, 0xA5, 0xFF):
        want = 0
        for j in range(8):
            if i >> j & 1:
                want ^= tal[7 - j]
        assert t[i] == want


# ------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("opts", R.OPTS, ids=str)
def test_encoded_words_have_zero_syndromes_and_round_trip(opts):
    """Every encoded word has 32 zero syndromes (computed in numpy, with tables made here); the VCDU sits in the CADU in its natural
    order; decoding gives it back with nothing corrected."""
    from meteor_demod_amd import rs
    rng = np.random.default_rng(11)
    for _ in range(6):
        v = R.vcdu(rng)
        c = rs.model_encode(v, **opts)
        assert bytes(c[:4]) == U.MARKER
        for w in R.words(c, **opts):
            assert not R.syndromes(w).any()
        assert np.array_equal(R.plain(c, **opts), v)
        out, info = rs.model_decode(c, **opts)
        assert np.array_equal(out[0], v) and not info.any()
    assert rs.model_decode(np.zeros((0, 1024), dtype=np.uint8))[0].shape == (0, 892)


def test_every_single_error_position():
    """One error at each position 0 .. 254 (0 and 254: the ends of the Chien search; 222 and 223: the data / parity border), three
    error values each, in a codeword that changes with the position."""
    from meteor_demod_amd import rs
    rng = np.random.default_rng(12)
    v = R.vcdu(rng)
    clean = rs.model_encode(v)
    batch, where = [], []
    for p in range(255):
        for e in (0x01, 0x80, 0xFF):
            c = clean.copy()
            c[4 + 4 * p + p % 4] ^= e
            batch.append(c)
            where.append(p % 4)
    out, info = rs.model_decode(np.stack(batch))
    assert (out == v).all()
    want = np.zeros((len(batch), 8), dtype=np.uint8)
    want[np.arange(len(batch)), where] = 1
    assert np.array_equal(info, want)
    assert {0, 222, 223, 254} <= set(range(255))


@pytest.mark.parametrize("opts", R.OPTS, ids=str)
def test_mixed_loads_follow_the_decoding_rule(opts):
    """0, 1, 2, 8, 15 and exactly 16 errors: corrected, with the count; 17 and 32 errors and random frames: 255, the output the
    derandomised input; errors in the parity only: counted, the data untouched; the other codewords of a flagged frame corrected."""
    from meteor_demod_amd import rs
    sent, cadu, loads = R.mixed_batch(24, seed=13, **opts)
    flat = [x for row in loads for x in row]
    assert {0, 1, 8, 15, 16, 17, 32, "parity", "random"} <= set(flat)
    out, info = rs.model_decode(cadu, **opts)
    R.check_against_what_was_sent(sent, cadu, loads, out, info, **opts)
    assert any(1 in (info[f, :4] == 255) and (info[f, :4] < 255).any() and info[f, :4].max() == 255 and 0 < info[f, :4].min() < 255
               for f in range(len(loads)))                                    # a flagged frame with corrected codewords beside


def test_beyond_the_code_is_left_alone():
    """17, 18 and 32 errors, and random bytes, many times over (fixed seeds): always 255, never a false correction, the word as
    received."""
    from meteor_demod_amd import rs
    rng = np.random.default_rng(14)
    v = R.vcdu(rng)
    clean = rs.model_encode(v)
    batch = []
    for count in (17, 18, 32) * 20:
        c = clean.copy()
        for k in range(4):
            R.damage(c, k, count, rng)
        batch.append(c)
    for _ in range(20):
        c = clean.copy()
        c[4:] = rng.integers(0, 256, 1020, dtype=np.uint8)
        batch.append(c)
    batch = np.stack(batch)
    out, info = rs.model_decode(batch)
    assert (info[:, :4] == 255).all() and (info[:, 4] == 1).all()
    assert np.array_equal(out, np.stack([R.plain(c) for c in batch]))


def test_bursts():
    """A burst of 64 bytes in the frame is 16 per codeword: corrected.  66 bytes from an offset of 1: codewords 1 and 2 get 17 and are
    flagged, 0 and 3 get 16 and are corrected."""
    from meteor_demod_amd import rs
    rng = np.random.default_rng(15)
    v = R.vcdu(rng)
    clean = rs.model_encode(v)
    for start in (0, 333, 1020 - 64):
        c = clean.copy()
        c[4 + start: 4 + start + 64] ^= rng.integers(1, 256, 64, dtype=np.uint8)
        out, info = rs.model_decode(c)
        assert np.array_equal(out[0], v) and list(info[0]) == [16, 16, 16, 16, 0, 0, 0, 0], (start, info)
    c = clean.copy()
    c[4 + 401: 4 + 401 + 66] ^= rng.integers(1, 256, 66, dtype=np.uint8)             # 401 % 4 = 1: codewords 1 and 2 first
    out, info = rs.model_decode(c)
    assert list(info[0]) == [16, 255, 255, 16, 1, 0, 0, 0]
    for k in (0, 3):
        assert np.array_equal(out[0, k::4], v[k::4])
    for k in (1, 2):
        assert np.array_equal(out[0, k::4], R.plain(c)[k::4])


def test_options_are_checked():
    from meteor_demod_amd import _capi, rs
    c = rs.model_encode(np.zeros(892, dtype=np.uint8))
    for bad, word in ((dict(derandomise=2), "derandomise"), (dict(dual_basis=7), "dual_basis"), (dict(piece_frames=(1 << 20) + 1), "piece_frames")):
        with pytest.raises(_capi.MdemodError) as e:
            rs.model_decode(c, **bad)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    with pytest.raises(TypeError):
        rs.model_decode(c, derandomize=1)
    o = rs.make_opts()
    assert (o.derandomise, o.dual_basis, o.piece_frames) == (1, 0, 0)


def test_header_fields():
    from meteor_demod_amd import rs
    h = rs.header(bytes([0x40 | 0x27, 0x40 | 0x05, 0x12, 0x34, 0x56, 0x00]))
    assert (h.version, h.spacecraft, h.vcid, h.counter) == (1, (0x27 << 2) | 1, 5, 0x123456)
    h = rs.header(bytes([0xFF] * 6))
    assert (h.version, h.spacecraft, h.vcid, h.counter) == (3, 255, 63, 0xFFFFFF)
    rng = np.random.default_rng(16)
    h = rs.header(R.vcdu(rng, vcid=33, counter=70000, spacecraft=0x9D))
    assert (h.version, h.spacecraft, h.vcid, h.counter) == (1, 0x9D, 33, 70000)
    vc = np.stack([R.vcdu(rng, vcid=v, counter=k) for v, k in ((5, 1), (5, 2), (9, 7), (5, 4), (9, 8), (5, 5))])
    info = np.zeros((6, 8), dtype=np.uint8)
    info[4, 0], info[4, 4], info[0, 1] = 255, 1, 3
    rep = rs.report(vc, info)
    assert (rep.frames, rep.uncorrectable_frames, rep.bytes_corrected) == (6, 1, 3)
    assert rep.frames_per_vcid == {5: 4, 9: 1} and rep.counter_gaps_per_vcid == {5: 1, 9: 0}


def test_noisy_stream_through_the_models():
    """The issue's CPU figures, through the two host models: the five RS-encoded frames at 2 dB, decoded at the sent positions, one
    hypothesis here (the GPU test runs all eight): byte errors in every frame, all within the code, every VCDU as sent."""
    from meteor_demod_amd import frames, rs
    st = R.stream()
    soft = st.received(3, 2.0, seed=203)
    cadu, _ = frames.model_viterbi(soft, [frames.Frame(p, 3, 0, 0, 0, 0) for p in st.positions])
    assert sum(bytes(c) != f for c, f in zip(cadu, st.frames)) == 5
    out, info = rs.model_decode(cadu)
    print(f"2 dB, h 3: corrected per codeword {info[:, :4].tolist()}")
    assert [bytes(v) for v in out] == [bytes(v) for v in st.vcdus]
    assert not info[:, 4].any() and (info[:, :4].astype(int).sum(axis=1) > 0).all() and info[:, :4].max() <= 16


# ---------------------------------------------------------------------------------------------------- exports and layout
def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", HEADER.read_text(), re.M)


def test_rs_entries_exported_and_bound():
    """Every entry of the new header is exported by the library and typed in rs.py's own table; the older binding tables and headers
    are untouched; the model is exported beside them."""
    from meteor_demod_amd import _capi, frames, frontend, rs, survey
    names = _header_entries()
    assert sorted(names) == sorted(["mdemod_rs_default_opts", "mdemod_rs_decode_device", "mdemod_rs_decode_host", "mdemod_rs_vcdu_header"])
    lib = rs.lib()
    for n in names + list(rs.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(rs.SIGNATURES) == sorted(names)
    assert all(n.startswith("mdemod_rs_model_") for n in rs.MODEL_SIGNATURES)
    for n in ("mdemod_rs_model_encode", "mdemod_rs_model_decode", "mdemod_rs_model_pn"):
        assert n in rs.MODEL_SIGNATURES
    others = list(_capi.SIGNATURES) + list(frontend.SIGNATURES) + list(survey.SIGNATURES) + list(frames.SIGNATURES) + list(frames.MODEL_SIGNATURES)
    assert not any("_rs_" in n for n in others)
    assert not any(w in n for n in list(rs.SIGNATURES) + list(rs.MODEL_SIGNATURES) for w in ("frames", "survey", "spectrum", "mdemod_fe_"))
    for h in ("meteor_demod_amd.h", "meteor_demod_amd_frontend.h", "meteor_demod_amd_survey.h", "meteor_demod_amd_frames.h"):
        assert "mdemod_rs_" not in (ROOT / "include" / h).read_text()
    assert _capi.lib().mdemod_abi_version() == 5
    import meteor_demod_amd
    for n in ("rs", "RsInfo"):
        assert n in meteor_demod_amd.__all__ and hasattr(meteor_demod_amd, n)
    for f in ("decode", "model_encode", "model_decode", "pn", "header", "decode_file", "soft_to_vcdu"):
        assert callable(getattr(rs, f))


def test_rs_int_entries_are_function_try_blocks():
    from meteor_demod_amd import rs
    found = 0
    entries = set(_header_entries()) | set(rs.MODEL_SIGNATURES)
    for src in RS_SOURCES:
        text = src.read_text()
        for m in re.finditer(r"^(?:extern \"C\" )?int\n(mdemod_\w+)\(", text, re.M):
            assert m.group(1) in entries, m.group(1)
            found += 1
            body = text[m.end():]
            head = body[: body.index("{")]
            assert head.rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            end = body.index("\n}")
            assert body[end:].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 2 + 2, found


def test_rs_struct_layouts(tmp_path):
    from meteor_demod_amd.rs import MdemodRsHeader, MdemodRsInfo, MdemodRsOpts
    assert C.sizeof(MdemodRsOpts) == 16 and C.sizeof(MdemodRsInfo) == 8 and C.sizeof(MdemodRsHeader) == 16
    assert MdemodRsOpts.dual_basis.offset == 4 and MdemodRsOpts.piece_frames.offset == 8 and MdemodRsInfo.flags.offset == 4
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_rs.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(mdemod_rs_opts), sizeof(mdemod_rs_info), sizeof(mdemod_rs_header), offsetof(mdemod_rs_info, flags), '
           'offsetof(mdemod_rs_opts, piece_frames), offsetof(mdemod_rs_header, counter)); return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 8, 16, 4, 8, 12]


def test_rs_host_code_is_hip_free_and_the_kernel_uses_no_atomics():
    for name in ("rs_host.cpp", "rs_host.h"):
        host = (CSRC / name).read_text()
        assert not re.search(r"\bhip[A-Z_]|__global__|__device__|hip_runtime|hip_host", host), name
    kernels = (CSRC / "rs.hip").read_text()
    code = re.sub(r"/\*.*?\*/", "", kernels, flags=re.S)
    assert "atomic" not in code.lower()
    device_code = code[: code.index("namespace {")]
    assert "__global__" in device_code and "while (" not in device_code          # the kernel's loops are counted
    assert "__ballot" in device_code and "__shfl" in device_code
    build_py = (ROOT / "meteor_demod_amd" / "build.py").read_text()
    assert '"rs.hip"' in build_py and '"rs_host.cpp"' in build_py


# ---------------------------------------------------------------------------------------------- the C host, no such layer
def test_cli_without_rs_layer_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has neither the frame layer nor this one): it links, --help lists
    --vcdu, and --vcdu exits non-zero naming what the library lacks - not "unrecognized option" - and writes nothing.  With --stdout
    it is refused whatever the library."""
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--vcdu" in h.stderr and "--cadu" in h.stderr
    wav = tmp_path / "in.wav"
    wav.write_bytes(U.wav_bytes(288000, np.zeros((16384, 2), dtype=np.int16)))
    r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), "--vcdu", str(wav)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0
    assert "--vcdu" in r.stderr and "this library has no" in r.stderr and "unrecognized" not in r.stderr, r.stderr
    assert r.stdout == "" and sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    for exe_ in (exe, cli_exe):
        r = subprocess.run([str(exe_), "--vcdu", "--stdout", str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "--vcdu" in r.stderr and "--stdout" in r.stderr and r.stdout == "", r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
    assert "mdemod_rs_" not in (ROOT / "tests" / "sanitize" / "stub_backend.c").read_text()


# ------------------------------------------------------------------------------------------------------- sanitizer fuzz
@pytest.mark.timeout(300)
def test_rs_fuzz_under_asan_ubsan(tmp_path):
    """tests/sanitize/fuzz_rs.cpp, a program of its own over rs_host.cpp: random options, 0 .. 40 errors per codeword, 0 .. 9
    frames; the decoding rule holds for every word; no sanitizer report."""
    exe = tmp_path / "fuzz_rs"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                        str(ROOT / "tests" / "sanitize" / "fuzz_rs.cpp"), str(CSRC / "rs_host.cpp"), str(CSRC / "demod_host.cpp"), "-pthread",
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), "400", "7"], capture_output=True, text=True, timeout=240)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["cases"] == 400 and rep["refused"] > 10 and rep["words"] > 4000, rep
    assert rep["clean"] > 50 and rep["corrected"] > 1000 and rep["failed"] > 1000 and rep["false_corrections"] == 0, rep
