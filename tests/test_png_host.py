"""CPU tests of the host model of the PNG encoder (csrc/png_host.cpp through meteor_demod_amd.png.model_*), the specification of the
kernels: its files read back through the independent reader of png_ref.py (zlib's inflate and crc32) and through PIL where it
imports, to the exact picture and mask; the filter of every row is the header's rule restated in numpy; crafted byte arrays inflate
back; the files are as small as one Z_RLE stream of zlib over the same bytes, up to the measured bar.  Every test prints the figures
it asserts on."""
from __future__ import annotations

import io
import re
import struct
import zlib

import numpy as np
import pytest

import png_cases as K
import png_ref as R
from conftest import ROOT

FILTERS = (0, 1, 2, 3, 4, 5)
SEGMENTS = (1, 32)
# The size yardstick (profiles/png.md): over the six pictures of png_cases.yardstick_pictures() at 32 KiB the model's file exceeded
# zlib's Z_RLE stream in PNG framing by 0.089 .. 0.286 % (the whole file, its 17 bytes a segment included).  The bar is twice the
# largest excess measured, 0.006, plus the derived 17 bytes a segment.
SIZE_BAR, SIZE_MEASURED = 0.006, 0.00286


def _segments(n_bytes: int, segment: int) -> int:
    return -(-n_bytes // ((segment or 32) * 1024))


# ---------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("width,height", K.SIZES)
def test_round_trip(width, height):
    """Planes 1 and 3, with and without a mask, filters 0 .. 5, segments of 1 and 32 KiB: the file parses, every CRC and the Adler-32
    hold, the header says what was asked, the chunks are the zlib header, one IDAT per segment and the Adler-32, the pixels and the mask
    come back exactly, the filter bytes are those of the numpy restatement, the file is within its bound and the same on a second call;
    PIL, where present, opens the file and agrees."""
    from meteor_demod_amd import png as P
    try:
        from PIL import Image
    except ImportError:
        Image = None
    files = 0
    for planes in (1, 3):
        pic = K.picture(width, height, planes)
        for valid in (None, K.mask(width, height)):
            ch = planes + (valid is not None)
            for filt in FILTERS:
                want = K.filtered_reference(pic, valid, filt)
                assert np.array_equal(P.model_filter(pic, valid, filt), want), (planes, valid is not None, filt)
                for segment in SEGMENTS:
                    data = P.model_encode(pic, valid, filt, segment)
                    r = R.read(data)
                    assert r["colour_type"] == {1: 0, 3: 2, 2: 4, 4: 6}[ch] and len(data) <= P.bound(width, height, planes, valid is not None, segment)
                    assert np.array_equal(r["pixels"].reshape(pic.shape), pic) and np.array_equal(r["filtered"], want)
                    assert (r["alpha"] is None) if valid is None else np.array_equal(r["alpha"], np.where(valid != 0, 255, 0))
                    assert np.array_equal(r["filters"], want[:, 0]) and (filt == 5 or (r["filters"] == filt).all())
                    idat = r["idat"]
                    assert idat[0] == b"\x78\x01" and len(idat) == 2 + _segments(want.size, segment) and len(idat[-1]) == 4
                    assert idat[-1] == struct.pack(">I", zlib.adler32(want.tobytes()))
                    assert data[:P.HEAD].endswith(idat[0] + struct.pack(">I", zlib.crc32(b"IDAT" + idat[0]))) and len(data) - data.rindex(b"IDAT", 0, -20) + 4 == P.TAIL
                    assert P.model_encode(pic, valid, filt, segment) == data
                    if Image is not None:
                        im = Image.open(io.BytesIO(data))
                        im.load()
                        assert im.size == (width, height) and im.mode == {1: "L", 3: "RGB", 2: "LA", 4: "RGBA"}[ch]
                        assert np.array_equal(np.asarray(im).reshape(height, width, ch)[:, :, :planes].reshape(pic.shape), pic)
                    files += 1
    used = sorted(set(int(f) for f in K.filtered_reference(K.picture(width, height, 3), None, 5)[:, 0]))
    print(f"{width} x {height}: {files} files; filter 5 chose {used} on the colour picture")
    assert files == 2 * 2 * 6 * 2


def test_pil_reads_every_file():
    """PIL (libpng, zlib's inflate) on the files of the round trip's corner sizes: the same pixels and alpha."""
    Image = pytest.importorskip("PIL.Image")
    from meteor_demod_amd import png as P
    for (w, h) in ((1, 1), (17, 23), (8192, 2)):
        for planes in (1, 3):
            pic, valid = K.picture(w, h, planes, 1), K.mask(w, h, 1)
            im = Image.open(io.BytesIO(P.model_encode(pic, valid, 5, 1)))
            a = np.asarray(im).reshape(h, w, planes + 1)
            assert np.array_equal(a[:, :, :planes].reshape(pic.shape), pic) and np.array_equal(a[:, :, planes], np.where(valid != 0, 255, 0))


def test_every_filter_is_chosen_somewhere():
    """The pictures of the round trip make filter 5 choose each of the five filters on some row, and ties go to the lower number."""
    from meteor_demod_amd import png as P
    seen = set()
    for (w, h) in K.SIZES:
        for planes in (1, 3):
            seen |= set(int(f) for f in P.model_filter(K.picture(w, h, planes), None, 5)[:, 0])
    print(f"filters chosen: {sorted(seen)}")
    assert seen == {0, 1, 2, 3, 4}
    flat = np.zeros((4, 9), np.uint8)                                              # all five sums are 0: filter 0
    assert (P.model_filter(flat, None, 5)[:, 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------- deflate stage
def _payloads(chunks: bytes) -> list:
    return [b for k, b in R.chunks(chunks, 0) if k == b"IDAT"]


@pytest.mark.parametrize("name", sorted(K.crafted()))
def test_crafted_bytes_inflate_back(name):
    """The crafted arrays through model_deflate: chunks with good CRCs, one per segment, whose payloads together are a raw deflate
    stream that ends in its last block and gives the bytes back; every segment alone is a whole number of bytes; within the bound."""
    from meteor_demod_amd import png as P
    data, segment = K.crafted()[name]
    out, stored = P.model_deflate(data, segment, with_stored=True)
    parts = _payloads(out)
    n_seg = _segments(data.size, segment)
    assert len(parts) == n_seg and len(out) <= P.deflate_bound(data.size, segment) == data.size + 17 * n_seg
    assert R.inflate_raw(b"".join(parts)) == data.tobytes()
    sb = segment * 1024
    for s, part in enumerate(parts[:-1]):                                          # a segment alone: bytes, then the sync block ends it
        d = zlib.decompressobj(-15)
        assert d.decompress(part) == data[s * sb:(s + 1) * sb].tobytes() and not d.eof
    print(f"{name}: {data.size} bytes in {n_seg} segments of {segment} KiB, {len(out)} bytes out, {stored} stored")
    assert P.model_deflate(data, segment) == out
    if name.startswith("noise"):
        assert stored >= (3 if name == "noise" else 1) and all(len(p) == min(sb, data.size - s * sb) + 5 for s, p in enumerate(parts[:stored]))
    if name.startswith("equal"):
        assert stored == 0 and len(out) <= 40 * n_seg + data.size // 258                   # (a match of 258 in a byte at most)
    if name == "one_byte":
        assert stored == 1 and parts[0] == b"\x01\x01\x00\xfe\xff\xc8"


def test_run_rule():
    """inflate hides the tokens of a stream, so the parse rule is restated here as a token count per run length, and the dynamic block
    of "runs" must lie between those tokens at 1 bit each and at 15 + 5 + 1 bits each with the longest header."""
    from meteor_demod_amd import png as P

    def tokens(L):
        m = L - 1
        if m < 3:
            return L
        full, rem = divmod(m, 258)
        return 1 + full + (1 if rem >= 3 else rem)
    want = {1: 1, 2: 2, 3: 3, 4: 2, 5: 2, 258: 2, 259: 2, 260: 3, 261: 4, 262: 3, 517: 3, 4097: 17}
    assert {L: tokens(L) for L in K.RUN_LENGTHS} == want
    data, segment = K.crafted()["runs"]
    n_tok = sum(want.values()) + 1
    part = _payloads(P.model_deflate(data, segment))[0]
    print(f"runs: {data.size} bytes, {n_tok} tokens with the end-of-block, {len(part)} bytes")
    assert n_tok / 8 < len(part) < (n_tok * 21 + 14 + 19 * 3 + 287 * 14) / 8 + 6


def test_length_limit_is_forced():
    """An unlimited Huffman code of the literal counts of "skewed" is 18 bits deep.  The array decodes, so the limited code is complete
    and at most 15 bits long: zlib's inflate refuses an over-subscribed or incomplete literal/length code.  ("skewed_short" does the
    same to the code-length code, limit 7, in test_crafted_bytes_inflate_back.)"""
    from meteor_demod_amd import png as P
    depth = K.huffman_depth(K.skewed_counts())
    data, segment = K.crafted()["skewed"]
    out, stored = P.model_deflate(data, segment, with_stored=True)
    print(f"skewed: unlimited depth {depth}; {data.size} bytes into {len(out)}, {stored} stored")
    assert depth > 15 and stored == 0 and (data[1:] != data[:-1]).all()
    assert R.inflate_raw(b"".join(_payloads(out))) == data.tobytes()
    # the entropy of these counts is 2.6 bits a byte; a limited code stays near it
    assert len(out) < data.size * 3 // 8


# ------------------------------------------------------------------------------------------------------ bound, noise, rooms
def test_noise_takes_the_stored_path_within_the_bound():
    from meteor_demod_amd import png as P
    rng = np.random.default_rng(8)
    for planes in (1, 3):
        shape = (64, 100, 3) if planes == 3 else (64, 100)
        pic = rng.integers(0, 256, shape, dtype=np.uint8)
        for filt in (0, 5):
            for segment in SEGMENTS:
                data = P.model_encode(pic, None, filt, segment)
                f = P.model_filter(pic, None, filt)
                _, stored = P.model_deflate(f, segment, with_stored=True)
                n_seg = _segments(f.size, segment)
                print(f"noise x {planes}, filter {filt}, {segment} KiB: {len(data)} bytes of a bound of {P.bound(100, 64, planes, False, segment)}, {stored} of {n_seg} segments stored")
                assert len(data) <= P.bound(100, 64, planes, False, segment) == P.HEAD + P.TAIL + f.size + 17 * n_seg
                assert stored >= n_seg - 1 and np.array_equal(R.read(data)["pixels"].reshape(shape), pic)
                if filt == 0:
                    assert stored == n_seg and len(data) == P.bound(100, 64, planes, False, segment)


def test_refusals_and_rooms():
    """Every refusal with its code and text, and nothing written; too small a room answers with the bytes needed."""
    from meteor_demod_amd import _capi, png as P
    import ctypes as C
    pic = K.picture(16, 16, 3)
    for word, call in (("filter", lambda: P.model_encode(pic, None, 6)), ("segment", lambda: P.model_encode(pic, None, 5, 33)),
                       ("segment", lambda: P.model_deflate(np.zeros(4, np.uint8), 33)), ("bytes", lambda: P.model_deflate(np.zeros(0, np.uint8), 1)),
                       ("filter", lambda: P.model_filter(pic, None, 9))):
        with pytest.raises(_capi.MdemodError) as e:
            call()
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail
    lib = P.lib()
    out, n = np.full(4096, 0xAB, np.uint8), C.c_uint64(77)
    flat = np.ascontiguousarray(pic)
    for word, (w, h, planes) in (("planes", (16, 16, 2)), ("width", (0, 16, 3)), ("width", (8193, 1, 3)), ("height", (16, 0, 3)), ("height", (1, 16385, 3))):
        rc = lib.mdemod_png_model_encode(flat.ctypes.data, None, w, h, planes, 5, 0, out.ctypes.data, out.size, C.byref(n))
        assert rc == _capi.MDEMOD_ERR_PARAM and word in _capi.last_error() and (out == 0xAB).all() and n.value == 77
    assert lib.mdemod_png_model_encode(None, None, 16, 16, 3, 5, 0, out.ctypes.data, out.size, C.byref(n)) == _capi.MDEMOD_ERR_PARAM and "needed" in _capi.last_error()
    for valid in (None, K.mask(16, 16)):
        need = len(P.model_encode(pic, valid))
        for room in (0, 1, need - 1):
            with pytest.raises(_capi.MdemodError) as e:
                P.model_encode(pic, valid, out_room=room)
            assert e.value.code == _capi.MDEMOD_ERR_OVERFLOW and str(need) in e.value.detail
        rc = lib.mdemod_png_model_encode(flat.ctypes.data, None, 16, 16, 3, 5, 0, out.ctypes.data, 10, C.byref(n))
        assert rc == _capi.MDEMOD_ERR_OVERFLOW and (out == 0xAB).all() and n.value == len(P.model_encode(pic))
        assert len(P.model_encode(pic, valid, out_room=need)) == need
    data = np.arange(5000, dtype=np.uint8)
    need = len(P.model_deflate(data, 1))
    with pytest.raises(_capi.MdemodError) as e:
        P.model_deflate(data, 1, out_room=need - 1)
    assert e.value.code == _capi.MDEMOD_ERR_OVERFLOW and str(need) in e.value.detail
    assert P.bound(8193, 8, 1) == 0 and P.bound(8, 16385, 1) == 0 and P.bound(8, 8, 2) == 0 and P.bound(8, 8, 1, False, 33) == 0 and P.bound(0, 8, 1) == 0
    assert P.bound(10, 3, 3, True, 1) == 47 + 28 + 3 * 41 + 17 and P.workspace(8, 8, 2) == 0 and P.workspace(8, 8, 1) > 72 + 17
    with pytest.raises(ValueError):
        P.model_encode(pic, np.zeros((3, 3), np.uint8))


# ------------------------------------------------------------------------------------------------------------- entries
def _header_entries() -> list:
    text = (ROOT / "include" / "meteor_demod_amd_png.h").read_text()
    return re.findall(r"^\w[\w \*]*?\b(mdemod_png_\w+)\(", text, re.M)


def test_png_entries_exported_and_bound():
    """Every entry of the header is exported and typed, the model's entries are those of csrc/png_host.h, the older binding tables do not
    know them, no other header names them, and every entry that returns a status stands inside the boundary's try / catch."""
    from meteor_demod_amd import _capi, jpeg as J, map as MP, mosaic as M, overlay as O, png as P
    names = _header_entries()
    assert sorted(names) == sorted(P.SIGNATURES) and len(names) == 9
    lib = P.lib()
    for n in names + list(P.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(P.MODEL_SIGNATURES) == ["mdemod_png_model_deflate", "mdemod_png_model_encode", "mdemod_png_model_filter"]
    listed = (ROOT / "meteor_demod_amd" / "csrc" / "png_host.h").read_text()
    assert all(n in listed for n in P.MODEL_SIGNATURES)
    others = list(_capi.SIGNATURES)
    for mod in (J, MP, M, O):
        others += list(mod.SIGNATURES) + list(mod.MODEL_SIGNATURES)
    assert not any("png" in n for n in others) and len(J.SIGNATURES) == 9 and len(J.MODEL_SIGNATURES) == 5
    for h in (ROOT / "include").glob("*.h"):
        if h.name != "meteor_demod_amd_png.h":
            assert "mdemod_png_" not in h.read_text(), h.name
    assert _capi.lib().mdemod_abi_version() == 5
    for f in ("encode", "write", "deflate", "model_filter", "model_deflate", "model_encode", "main", "read_pnm"):
        assert callable(getattr(P, f))
    found = 0
    for src in ("png.hip", "png_host.cpp"):
        text = (ROOT / "meteor_demod_amd" / "csrc" / src).read_text()
        for m in re.finditer(r"^int\n(mdemod_\w+)\(", text, re.M):
            body = text[m.end():]
            assert body[: body.index("{")].rstrip().endswith("try") and body[body.index("\n}"):].startswith("\n} MDEMOD_API_CATCH"), m.group(1)
            found += 1
    assert found == 4 + 3
    assert (P.HEAD, P.TAIL, P.SEGMENT_OVERHEAD, P.MAX_WIDTH, P.MAX_HEIGHT, P.MAX_SEGMENT) == tuple(
        int(re.search(rf"#define MDEMOD_PNG_{k}\s+(\d+)", (ROOT / "include" / "meteor_demod_amd_png.h").read_text()).group(1))
        for k in ("HEAD", "TAIL", "SEGMENT_OVERHEAD", "MAX_WIDTH", "MAX_HEIGHT", "MAX_SEGMENT"))


def test_read_pnm(tmp_path):
    from meteor_demod_amd import png as P
    pic = K.picture(17, 23, 3)
    (tmp_path / "a.ppm").write_bytes(b"P6\n# made here\n17 23\n255\n" + pic.tobytes())
    (tmp_path / "b.pgm").write_bytes(b"P5 17 23 255\n" + pic[:, :, 0].tobytes())
    (tmp_path / "c.pgm").write_bytes(b"P5 17 23 65535\n" + bytes(17 * 23 * 2))
    (tmp_path / "d.pgm").write_bytes(b"P2 1 1 255\n0\n")
    assert np.array_equal(P.read_pnm(tmp_path / "a.ppm"), pic) and np.array_equal(P.read_pnm(tmp_path / "b.pgm"), pic[:, :, 0])
    for bad in ("c.pgm", "d.pgm"):
        with pytest.raises(ValueError):
            P.read_pnm(tmp_path / bad)


# --------------------------------------------------------------------------------------------------------- size yardstick
def test_size_against_zlib_rle():
    """The model's file against one zlib stream (level 6, window 15, memLevel 9, Z_RLE) over the same filtered bytes in PNG framing,
    at 32 KiB: the excess of every picture within the bar above.  zlib level 6 and PIL's writer are printed beside them; no bar."""
    from meteor_demod_amd import png as P
    try:
        from PIL import Image
    except ImportError:
        Image = None
    worst = -1.0
    for name, pic in K.yardstick_pictures().items():
        h, w = pic.shape[:2]
        ctype = 0 if pic.ndim == 2 else 2
        f = P.model_filter(pic, None, 5).tobytes()
        mine = P.model_encode(pic, None, 5, 32)

        def z(strategy):
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, strategy)
            return R.frame(c.compress(f) + c.flush(), w, h, ctype)
        rle, six = z(zlib.Z_RLE), z(zlib.Z_DEFAULT_STRATEGY)
        pil = 0
        if Image is not None:
            b = io.BytesIO()
            Image.fromarray(pic).save(b, "PNG")
            pil = len(b.getvalue())
        n_seg = _segments(len(f), 32)
        excess = (len(mine) - len(rle)) / len(rle)
        worst = max(worst, excess)
        print(f"{name}: {len(mine)} bytes in {n_seg} segments; Z_RLE {len(rle)} ({100 * excess:+.3f} %); level 6 {len(six)}; PIL {pil}; raw {pic.size}")
        assert n_seg >= 16 and len(mine) <= len(rle) * (1 + SIZE_BAR) + 17 * n_seg
    print(f"largest excess {worst:.5f} (measured {SIZE_MEASURED}, bar {SIZE_BAR} and 17 bytes a segment)")
