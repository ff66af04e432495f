"""CPU tests of the host model of the JPEG encoder (csrc/jpeg_host.cpp through meteor_demod_amd.jpeg.model_*), the specification of
the kernels: its files decode with the independent decoder of jpeg_ref.py and with libjpeg (through PIL, where it imports), its
coefficients are those of a float64 DCT up to ties, its pictures are as good and as small as libjpeg's own, and its entropy coder
reads back exactly on crafted coefficients.  Every test prints the figures it asserts on."""
from __future__ import annotations

import io

import numpy as np
import pytest

import jpeg_cases as K
import jpeg_ref as R


def _pil():
    return pytest.importorskip("PIL.Image")


def _save(Image, pic, quality, **more) -> bytes:
    b = io.BytesIO()
    Image.fromarray(pic).save(b, "JPEG", quality=quality, subsampling=0, optimize=False, **more)
    return b.getvalue()


# --------------------------------------------------------------------------------------------------- the test decoder itself
@pytest.mark.parametrize("quality", K.QUALITIES)
def test_the_test_decoder_reads_what_libjpeg_wrote(quality):
    """Files saved by PIL (4:4:4, standard tables, restart every 5 MCUs and none) through jpeg_ref against PIL's own pixels.  libjpeg's
    inverse transform is the integer one whose samples lie within 1 of the exact ones (IEEE 1180's peak error), and it rounds Y, Cb and
    Cr before its colour conversion: a grey pixel may differ by 1; a colour one by 1 + 1.402 x 1 and a rounding, so by 3 at most, and
    by less than 0.5 on average.  Measured: at most 1 (grey) and 2 (colour), means up to 0.02 and 0.41."""
    Image = _pil()
    for name, pic in K.psnr_pictures().items():
        for grey in (False, True):
            p = np.ascontiguousarray(pic[..., 1]) if grey else pic
            for blocks in (5, 0):
                data = _save(Image, p, quality, restart_marker_blocks=blocks)
                ref = R.decode(data)
                pil = np.asarray(Image.open(io.BytesIO(data)))
                d = np.abs(ref.pixels.astype(int) - pil.astype(int))
                mcus = ((p.shape[0] + 7) // 8) * ((p.shape[1] + 7) // 8)
                assert ref.pixels.shape == pil.shape and ref.segments == (-(-mcus // blocks) if blocks else 1)
                assert d.max() <= (1 if grey else 3) and d.mean() < 0.5, (name, grey, quality, blocks, d.max(), d.mean())
    print(f"quality {quality}: last picture differs by at most {d.max()}, {d.mean():.3f} on average")


# ---------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("width,height", K.SIZES)
def test_pixel_round_trip(width, height):
    """Grey and colour, qualities 1, 50, 90 and 100, Ri of 1, 32 and 64: the model's file parses, its size, mode, tables, interval and
    markers are those asked for, the coefficients in the stream are mdemod_jpeg_model_coefficients exactly, jpeg_ref's pixels are
    near the picture, and PIL opens and loads the file to the pixels jpeg_ref gives (the tolerance of the decoder test)."""
    from meteor_demod_amd import jpeg as J
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for planes in (1, 3):
        pic = K.picture(width, height, planes)
        mcus = ((width + 7) // 8) * ((height + 7) // 8)
        for quality in K.QUALITIES:
            q, bits, vals, _, _ = J.model_tables(quality)
            coef = J.model_coefficients(pic, quality)
            for ri in K.INTERVALS:
                data = J.model_encode(pic, quality, ri)
                j = R.decode(data)
                assert (j.width, j.height, j.planes, j.restart_interval) == (width, height, planes, ri) and j.jfif == (1, 1, 0, 1, 1)
                assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9" and len(data) <= J.bound(width, height, planes, ri)
                segs = -(-mcus // ri)
                assert j.segments == segs and j.markers[:7] == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA]
                assert j.markers[7:] == [0xD0 + (s % 8) for s in range(segs - 1)] + [0xD9]
                assert np.array_equal(j.qt[0], q[0]) and (planes == 1 or np.array_equal(j.qt[1], q[1])) and len(j.qt) == (1 if planes == 1 else 2)
                for k in range(2 if planes == 1 else 4):
                    b, v = j.dht[(k & 1, k >> 1)]
                    assert np.array_equal(b, bits[k]) and np.array_equal(v, vals[k][: len(v)])
                assert [c[1:] for c in j.components] == [(1, 1, 0 if c == 0 else 1) for c in range(planes)]
                assert np.array_equal(j.coef, coef), (planes, quality, ri)
                if Image is not None:
                    im = Image.open(io.BytesIO(data))
                    im.load()
                    assert im.size == (width, height) and im.mode == ("L" if planes == 1 else "RGB")
                    d = np.abs(np.asarray(im).astype(int) - j.pixels.astype(int))
                    assert d.max() <= (1 if planes == 1 else 3)
            near = K.psnr(j.pixels, pic)
            print(f"{width} x {height} x {planes}, quality {quality}: {len(data)} bytes, {K.psnr(j.pixels, pic):.2f} dB")
            # (a 1 x 1 picture is its DC alone; everything else must look like the picture at the better qualities)
            assert near > (30.0 if quality >= 90 else 8.0)


def test_header_sizes_and_bound():
    from meteor_demod_amd import jpeg as J
    for planes in (1, 3):
        data = J.model_encode(K.picture(8, 8, planes), 50, 1)
        sos = data.index(b"\xff\xda")
        assert sos + 2 + int.from_bytes(data[sos + 2: sos + 4], "big") == J.HEAD[planes]
    assert J.bound(8193, 8, 1) == 0 and J.bound(8, 16385, 1) == 0 and J.bound(8, 8, 2) == 0 and J.bound(8, 8, 1, 65) == 0 and J.bound(0, 8, 1) == 0
    assert J.bound(17, 9, 3, 4) == 613 + 2 * 208 * 6 * 3 + 2 * 2 and J.bound(8, 8, 1) == 330 + 416 + 2


# ---------------------------------------------------------------------------------------------------------- coefficients
def test_forward_transform_against_float():
    """One block: R / 2^18 against the float64 DCT.  A line's t carries half a unit of 2^7 x 2 sqrt 2 = 362 per sample, a column
    adds up eight of them with weights that sum to 2.83 at most: 0.0039, and the last shifts add 2^-17."""
    from meteor_demod_amd import jpeg as J
    rng = np.random.default_rng(2)
    c = R.dct_matrix()
    worst = 0.0
    for k in range(200):
        s = rng.integers(0, 256, (8, 8), dtype=np.uint8) if k % 4 else np.full((8, 8), (0, 255, 128, 1)[k // 4 % 4], np.uint8)
        if k % 4 == 1:
            s = ((np.indices((8, 8)).sum(0) % 2) * 255).astype(np.uint8)
        got = J.model_fdct(s) / 2.0 ** 18
        want = c @ (s.astype(float) - 128.0) @ c.T
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"largest error of a coefficient: {worst:.5f}")
    assert worst <= 0.004
    assert J.model_fdct(np.zeros((8, 8), np.uint8))[0, 0] == -1024 << 18


@pytest.mark.parametrize("quality", K.QUALITIES)
def test_coefficients_against_float(quality):
    """The model's levels against round(float64 DCT / Q): never more than 1 apart, and apart only where the quotient stands within
    0.004 of a tie (the transform's error above, Q >= 1) - or on it, where float64 itself decides by its last bit.  The share of
    such coefficients was measured first (profiles/jpeg.md): 0 .. 0.0025 at qualities 1, 50 and 90, up to 0.0066 at 100 (0.0072 on
    another draw of the pictures), where Q is 1 and every coefficient of a noisy picture is spread over the ties.  The bar is
    twice the largest share measured, 0.015."""
    from meteor_demod_amd import jpeg as J
    q = J.model_tables(quality)[0]
    worst = 0.0
    for name, pic in K.psnr_pictures().items():
        for grey in (False, True):
            p = np.ascontiguousarray(pic[..., 1]) if grey else pic
            mine = J.model_coefficients(p, quality).astype(np.int64)
            want, x = K.float_levels(p, q)
            d = np.abs(mine - want)
            off = np.abs(np.abs(x) - np.floor(np.abs(x)) - 0.5)[d != 0]
            share = float((d != 0).mean())
            worst = max(worst, share)
            assert d.max() <= 1 and (off.size == 0 or off.max() <= 0.004) and share <= 0.015, (name, grey, int(d.max()), share)
    print(f"quality {quality}: largest share of coefficients off the float64 rounding {worst:.5f}")


# ----------------------------------------------------------------------------------------------------- against libjpeg
@pytest.mark.parametrize("quality", K.QUALITIES)
def test_psnr_and_size_against_libjpeg(quality):
    """The reference is PIL's file of the same picture at the same quality, 4:4:4, standard tables, no restarts; both files are decoded
    by PIL.  The two encoders share tables and differ in the rounding of the transform, so the PSNR against the source moves by
    hundredths of a dB: measured over these 12 pictures and 4 qualities -0.044 .. +1.0 dB (the gains at quality 100).  The bar is
    0.1 dB below libjpeg.  The size may exceed libjpeg's by the restart overhead - per segment a marker, up to a byte of padding
    and up to two bytes per component for a DC value coded again from 0 - plus the 6 bytes of DRI, plus 1 %."""
    Image = _pil()
    from meteor_demod_amd import jpeg as J
    for name, pic in K.psnr_pictures().items():
        for grey in (False, True):
            p = np.ascontiguousarray(pic[..., 1]) if grey else pic
            planes = 1 if grey else 3
            mine, ref = J.model_encode(p, quality, 32), _save(Image, p, quality)
            a, b = K.psnr(np.asarray(Image.open(io.BytesIO(mine))), p), K.psnr(np.asarray(Image.open(io.BytesIO(ref))), p)
            segs = -(-(((p.shape[0] + 7) // 8) * ((p.shape[1] + 7) // 8)) // 32)
            room = len(ref) + segs * (3 + 2 * planes) + 6 + len(ref) // 100
            print(f"{name} x {planes}, quality {quality}: {a:.3f} dB against {b:.3f} dB, {len(mine)} bytes against {len(ref)} (+ {room - len(ref)} allowed)")
            assert a >= b - 0.1 and len(mine) <= room


# ------------------------------------------------------------------------------------------------------ entropy coder
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("ri", [1, 2, 32, 64])
def test_entropy_coder_on_crafted_coefficients(planes, ri):
    """Runs of 15, 16, 17, 32 and 62, a block without EOB, all-zero blocks, every DC category edge and +-2047, the largest magnitudes,
    values outside the range (clamped), read back exactly by jpeg_ref."""
    from meteor_demod_amd import jpeg as J
    coef = K.crafted_for(planes)
    n_mcus = len(coef) // planes
    data = J.model_entropy(coef, planes, ri)
    assert len(data) <= int(J.lib().mdemod_jpeg_entropy_bound(n_mcus, planes, ri))
    back = R.entropy_only(data, n_mcus, planes, ri, K.dht_of(J))
    assert np.array_equal(back, K.clamped(coef))
    if planes == 1 and ri % 2 == 0:
        got = sorted(set(int(back[k + 1, 0] - back[k, 0]) for k in range(6, 6 + 2 * len(K.DC_DIFFS), 2)))
        assert got == sorted(set(K.DC_DIFFS)) and 2047 in got and -2047 in got
    parts = K.split_segments(data)
    assert len(parts) == -(-n_mcus // ri)
    print(f"{planes} planes, Ri {ri}: {len(data)} bytes in {len(parts)} segments, {data.count(bytes([255, 0]))} stuffed bytes")


def test_fixture_stuffs_and_ends_on_ff():
    """The crafted stream really holds a segment with at least 32 stuffed bytes and one that ends on an FF (and its 00)."""
    from meteor_demod_amd import jpeg as J
    for ri in (1, 32):
        parts = K.split_segments(J.model_entropy(K.crafted_for(1), 1, ri))
        most = max(p.count(b"\xff\x00") for p in parts)
        print(f"Ri {ri}: at most {most} stuffed bytes in a segment; the last segment ends on {parts[-1][-2:].hex()}")
        assert most >= 32 and parts[-1].endswith(b"\xff\x00")
        assert all(p[k + 1] == 0 for p in parts for k in range(len(p) - 1) if p[k] == 0xFF) and all(p[-1] != 0xFF for p in parts)


def test_model_refusals():
    from meteor_demod_amd import _capi, jpeg as J
    pic = K.picture(16, 16, 3)
    for word, call in (("quality", lambda: J.model_encode(pic, 0)), ("quality", lambda: J.model_encode(pic, 101)), ("restart interval", lambda: J.model_encode(pic, 50, 65)),
                       ("planes", lambda: J.model_entropy(np.zeros((2, 64), np.int16), 2)), ("MCUs", lambda: J.model_entropy(np.zeros((0, 64), np.int16), 1))):
        with pytest.raises(_capi.MdemodError) as e:
            call()
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, e.value.detail
    need = len(J.model_encode(pic, 50))
    with pytest.raises(_capi.MdemodError) as e:
        J.model_encode(pic, 50, out_room=need - 1)
    assert e.value.code == _capi.MDEMOD_ERR_OVERFLOW and str(need) in e.value.detail
    assert len(J.model_encode(pic, 50, out_room=need)) == need
