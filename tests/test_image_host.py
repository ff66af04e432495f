"""CPU tests of the image layer (include/meteor_demod_amd_image.h): the tables, the quantiser and the integer transform of the host
model against image_util's independent restatements, condition (C1) on the transform, the synthetic sender through the model and
the independent decoder, the failure rule at every truncation length, the demultiplexing rule on a batch with every kind of damage,
the placement, and the pieces of the host entry's model path.  Every test prints the figures it asserts on."""
from __future__ import annotations

import numpy as np
import pytest

import image_util as I


@pytest.fixture(scope="module")
def image():
    from meteor_demod_amd import image as m
    return m


def _one(image, packet: bytes):
    """One packet through the multiplexer, the model's demux and the model's decoder."""
    vcdu, _, _ = I.mux([packet])
    desc = image.model_find(vcdu)
    strips, sinfo = image.model_decode(vcdu, desc[:1])
    return desc[0], strips[0], sinfo[0]


def _same(si, strip, ref):
    assert (int(si["mcus"]), int(si["flags"]), int(si["q"]), int(si["mcun"]), int(si["bits_used"])) == (ref["mcus"], ref["flags"], ref["q"], ref["mcun"], ref["bits_used"])
    assert (int(si["day"]), int(si["ms"]), int(si["us"])) == (ref["day"], ref["ms"], ref["us"])
    assert np.array_equal(strip, ref["strip"])


# -------------------------------------------------------------------------------------------------------------------- tables
def test_tables(image):
    t = image.model_tables()
    assert list(t["dc_bits"]) == I.DC_BITS and list(t["ac_bits"]) == I.AC_BITS and list(t["dc_val"]) == I.DC_VAL and list(t["ac_val"]) == I.AC_VAL
    assert list(t["zigzag"]) == I.ZIGZAG and np.array_equal(t["std"], I.STD_Q) and np.array_equal(t["m"], I.M)
    for table, count, kraft in ((I.DC_TABLE, 12, sum(b / 2 ** (k + 1) for k, b in enumerate(I.DC_BITS))),
                                (I.AC_TABLE, 162, sum(b / 2 ** (k + 1) for k, b in enumerate(I.AC_BITS)))):
        words = [format(code, f"0{length}b") for length, code in table]
        assert len(words) == count == len(set(table.values()))
        assert not any(a != b and b.startswith(a) for a in words for b in words)                  # prefix-free
        got = sum(2.0 ** -len(w) for w in words)
        print(f"{count} codes, Kraft sum {got}")
        assert got == kraft and got < 1                                                           # Annex K leaves the all-ones word free
    assert sorted(I.ZIGZAG) == list(range(64))


def test_quantiser_every_q(image):
    for q in range(256):
        got = image.model_quant(q)
        assert np.array_equal(got, I.quant(q)) and got.min() >= 1, q
    assert image.model_quant(100).max() == 1 and list(image.model_quant(50)[:8]) == [16, 11, 10, 16, 24, 40, 51, 61]


def test_model_idct_equals_the_numpy_restatement(image):
    rng = np.random.default_rng(11)
    blocks = np.concatenate([rng.integers(-2048, 2048, (300, 8, 8)), rng.integers(-256, 256, (300, 8, 8)), rng.integers(-3000, 3000, (50, 8, 8))])
    for b in blocks:
        assert np.array_equal(image.model_idct(b), I.idct_int(b))


def test_c1_the_transform_is_within_one_grey_level(image):
    """(C1): +-1 of the float64 transform on 10 000 random blocks in -256 .. 255 and 10 000 in -2048 .. 2047 (the peak error IEEE
    1180 allows an integer IDCT), exact on DC-only blocks.  The numpy restatement is the model's (the test above)."""
    rng = np.random.default_rng(12)
    for lim in (256, 2048):
        c = rng.integers(-lim, lim, (10000, 8, 8))
        a, b = I.idct_int(c).astype(int), I.idct_float(c).astype(int)
        print(f"+-{lim}: peak error {np.abs(a - b).max()}, pixels that differ {(a != b).mean():.5f}")
        assert np.abs(a - b).max() <= 1
        for k in range(0, 10000, 97):
            assert np.array_equal(image.model_idct(c[k]), a[k])
    dc = np.zeros((4096, 8, 8), dtype=int)
    dc[:, 0, 0] = np.arange(-2048, 2048)
    assert np.array_equal(I.idct_int(dc), I.idct_float(dc))
    for d in (-2048, -12, -4, 0, 4, 5, 1016, 2047):
        assert np.array_equal(image.model_idct(dc[d + 2048]), I.idct_float(dc[d + 2048]))


# ------------------------------------------------------------------------------------------------------------ sender, decoder
@pytest.mark.parametrize("q", [10, 50, 80, 100])
def test_encode_then_decode(image, q):
    """The sender's packets through the model equal the independent decoder byte for byte; at q = 100 every quantiser step is 1,
    a coefficient is off by at most 1/2, a pixel by at most 1/2 (7.4723 / (2 sqrt 2))^2 = 3.49, + 1/2 for the rounding and 0.2
    for the transform: 4 grey levels."""
    for kind in I.KINDS:
        for seed in (1, 2):
            src = I.strip(kind, 10 * q + seed)
            p = image.model_encode_packet(src, q, 14 * seed, 64 + seed, 500 + seed, 9, 123456, 789)
            d, strip, si = _one(image, p)
            ref = I.decode_packet(p)
            _same(si, strip, ref)
            err = int(np.abs(strip.astype(int) - src).max())
            print(f"q {q} {kind}: {len(p)} bytes, {ref['bits_used']} bits, peak error {err}")
            assert (int(d["apid"]), int(d["seq"]), int(d["length"]), int(d["flags"])) == (64 + seed, 500 + seed, len(p), 3 | 4)
            assert ref["mcus"] == 14 and ref["flags"] == 0 and (ref["day"], ref["ms"], ref["us"], ref["mcun"], ref["q"]) == (9, 123456, 789, 14 * seed, q)
            if q == 100:
                assert err <= 4


def test_every_truncation_length(image):
    """One packet cut to every length from 7 bytes on (its length field says so): blocks, flags and zero tails follow the failure
    rule and agree with the independent decoder."""
    p = image.model_encode_packet(I.strip("gradient", 5), 80, 42, 66, 9)
    full = I.decode_packet(p)
    seen = set()
    for n in range(7, len(p) + 1):
        cut = p[:4] + bytes([(n - 7) >> 8, (n - 7) & 0xFF]) + p[6:n]
        _, strip, si = _one(image, cut)
        ref = I.decode_packet(cut)
        _same(si, strip, ref)
        m = int(si["mcus"])
        seen.add(m)
        if n < 21:
            assert int(si["flags"]) == I.NOT_IMAGE and not strip.any()
        else:
            assert int(si["flags"]) == (I.TRUNCATED if m < 14 else 0)
            assert np.array_equal(strip[:, : 8 * m], full["strip"][:, : 8 * m]) and not strip[:, 8 * m:].any()
    print(f"{len(p)} bytes: blocks decoded over the cuts {sorted(seen)}")
    assert seen == set(range(15))


def _bits_packet(bits: str, mcun: int = 0, apid: int = 64) -> bytes:
    bits += "0" * (-len(bits) % 8)
    body = bytes(int(bits[i: i + 8], 2) for i in range(0, len(bits), 8))
    n = 20 + len(body)
    return bytes([0x08 | apid >> 8, apid & 0xFF, 0xC0, 1, (n - 7) >> 8, (n - 7) & 0xFF]) + bytes(8) + bytes([mcun, 0, 0, 0xFF, 0xF0, 100]) + body


def test_corrupt_streams_are_flagged(image):
    code = {sym: format(c, f"0{length}b") for (length, c), sym in I.AC_TABLE.items()}
    dc0 = next(format(c, f"0{length}b") for (length, c), sym in I.DC_TABLE.items() if sym == 0)
    good = dc0 + code[0]                                                          # one flat block
    cases = {"all ones": "1" * 64, "run past 63": good + dc0 + code[0xF0] * 3 + code[0xF1] + "1" + code[0],
             "four skips": good + dc0 + code[0xF0] * 4 + code[0], "three skips and 14": (dc0 + code[0xF0] * 3 + code[0xE1] + "1") * 14}
    for name, bits in cases.items():
        p = _bits_packet(bits)
        _, strip, si = _one(image, p)
        _same(si, strip, I.decode_packet(p))
        print(f"{name}: mcus {si['mcus']}, flags {si['flags']}, bits used {si['bits_used']}")
        want = {"all ones": 0, "run past 63": 1, "four skips": 1, "three skips and 14": 14}[name]
        assert int(si["mcus"]) == want and int(si["flags"]) == (I.TRUNCATED if want < 14 else 0)
        assert (strip[:, : 8 * want] == 128).all() or name == "three skips and 14"
        assert not strip[:, 8 * want:].any()
    for mcun, apid in ((15, 64), (196, 65), (28, 69)):
        p = _bits_packet(good * 14, mcun=mcun, apid=apid)
        _, strip, si = _one(image, p)
        _same(si, strip, I.decode_packet(p))
        assert int(si["flags"]) == (0 if mcun == 28 else I.BAD_HEADER) and int(si["mcus"]) == 14 and (strip == 128).all()
    bad_segment = bytearray(_bits_packet(good * 14))
    bad_segment[18] = 0xF1
    assert int(_one(image, bytes(bad_segment))[2]["flags"]) == I.BAD_HEADER
    for p in (I.plain_packet(70, 1, 69, sec=1), I.plain_packet(64, 1, 69, sec=0), I.idle_packet(100)):
        _, strip, si = _one(image, p)
        assert int(si["flags"]) == I.NOT_IMAGE and not strip.any() and int(si["mcus"]) == 0
    # a descriptor that points outside the batch is reported, not followed
    vcdu, _, _ = I.mux([_bits_packet(good * 14)])
    desc = image.model_find(vcdu)[:1].copy()
    for start, length in ((len(vcdu) * 882 - 10, 40), (0, 6), (0, 70000), (0xFFFFFFF0, 100)):
        desc["start"], desc["length"] = start, length
        strips, sinfo = image.model_decode(vcdu, desc)
        assert int(sinfo[0]["flags"]) == I.OUTSIDE and not strips.any()


# --------------------------------------------------------------------------------------------------------------------- demux
def _keys(desc):
    return [(int(d["apid"]), int(d["seq"]), int(d["length"])) for d in desc]


def test_demux_clean_layout(image):
    """The undamaged unit: every packet is found where the multiplexer put it, idle packets included."""
    vcdu, info, meta, want = I.demux_batch(I.UNIT_FRAMES)
    desc = image.model_find(vcdu, info)
    print([(int(d["start"]) // 882, int(d["start"]) % 882, int(d["length"])) for d in desc])
    assert [(int(d["start"]), int(d["length"]), int(d["apid"]), int(d["seq"])) for d in desc] == meta[: len(I.UNIT_STARTS)]
    assert _keys(desc) == want and [int(d["flags"]) for d in desc] == [3 | (k & 1) << 2 for k in range(len(desc))]
    fhps = [((int(v[8]) & 7) << 8) | int(v[9]) for v in vcdu]
    assert fhps[0] == 0 and fhps[8] == fhps[9] == I.NO_HEADER and {880, 879, 878, 877, 700, 300, 50} <= set(fhps)


@pytest.mark.parametrize("n", [1, 2, 5, 11, 33, 67, 77])
@pytest.mark.parametrize("with_info", [True, False])
def test_demux_damaged_batch(image, n, with_info):
    """Invalid pointer, missing frame, uncorrectable frame, foreign VCID, corrupted length: the accepted list is exactly the packets
    wholly inside linked runs, in order (without the reports the uncorrectable frame counts as good)."""
    vcdu, info, meta, want = I.demux_batch(n)
    if not with_info:
        info = None
        f = 3 * I.UNIT_FRAMES + 4
        want = [(a, s, l) for st, l, a, s in meta if (a, s, l) in set(want) or (st // 882 <= f <= (st + l - 1) // 882 < n)]
    desc = image.model_find(vcdu, info)
    print(f"n {n}: {len(desc)} of {sum(1 for m in meta if m[0] < 882 * n)} packets accepted")
    assert _keys(desc) == want
    assert all(int(a["start"]) < int(b["start"]) for a, b in zip(desc, desc[1:]))
    if n == 77:
        assert 0 < len(desc) < len(meta) and len(want) == len(meta) - 2 - 1 - (2 if with_info else 0) - 1 - 2


def test_demux_cap_and_refusals(image):
    import ctypes as C
    from meteor_demod_amd import _capi
    vcdu, info, _, want = I.demux_batch(22)
    full = image.model_find(vcdu, info)
    desc = np.zeros(5, dtype=image.DESC_DTYPE)
    total = C.c_uint64(0)
    assert image.lib().mdemod_image_model_find(None, vcdu.ctypes.data, info.ctypes.data, 22, desc.ctypes.data, 4, C.byref(total)) == 0
    assert total.value == len(want) and np.array_equal(desc[:4], full[:4]) and not desc[4]["length"]
    for word, opts in (("vcid", dict(vcid=64)), ("period", dict(period=0)), ("apid", dict(apids=(64, 65, 70))), ("repeated", dict(apids=(64, 65, 64))),
                       ("piece_frames", dict(piece_frames=(1 << 20) + 1))):
        with pytest.raises(_capi.MdemodError) as e:
            image.model_find(vcdu, info, **opts)
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, (word, e.value.detail)


# ----------------------------------------------------------------------------------------------------------------- placement
def _synthetic(image, rows):
    """(desc, sinfo) of clean image packets [(apid, seq, mcun), ...]."""
    desc, sinfo = np.zeros(len(rows), dtype=image.DESC_DTYPE), np.zeros(len(rows), dtype=image.SINFO_DTYPE)
    for i, (apid, seq, mcun) in enumerate(rows):
        desc[i] = (100 * i, 60, apid, seq, 7)
        sinfo[i]["mcus"], sinfo[i]["mcun"], sinfo[i]["q"] = 14, mcun, 50
    return desc, sinfo


def _sender(first_seq, strip_rows, apids=(64, 65, 66)):
    rows, seq = [], first_seq
    for _ in range(strip_rows):
        for a in apids:
            for c in range(14):
                rows.append((a, seq & 0x3FFF, 14 * c))
                seq += 1
        rows.append((70, seq & 0x3FFF, 0))
        seq += 1
    return rows


def test_placement_wrap_and_late_start(image):
    rows = _sender(16383 - 50, 4)                                                  # the counter wraps inside the second strip row
    for skip in (0, 14, 28, 2, 30):                                                # first packet seen: slot 0, 1, 2, mcun 28, slot 2 mcun 28
        desc, sinfo = _synthetic(image, rows[skip:])
        pl, summ = image.place(desc, sinfo)
        print(f"skip {skip}: first {summ['first']}, rows {summ['rows']}, placed {summ['placed']}, gaps {summ['seq_gaps']}")
        assert summ["rows"] == 4 and summ["placed"] == 4 * 42 - skip and summ["dropped"] == 0 and summ["seq_gaps"] == 0 and summ["first"] == 16383 - 50
        for (apid, _, mcun), p, k in zip(rows[skip:], pl, range(skip, len(rows))):
            want = (-1, 0, 0) if apid == 70 else (apid - 64, k // 43, mcun // 14)
            assert (int(p["channel"]), int(p["row"]), int(p["cell"])) == want
    # a flagged packet before the anchor is dropped; bad headers are never placed
    desc, sinfo = _synthetic(image, rows)
    sinfo[0]["flags"], sinfo[5]["flags"] = I.TRUNCATED, I.BAD_HEADER
    pl, summ = image.place(desc, sinfo)
    assert summ["dropped"] == 1 and summ["placed"] == 4 * 42 - 2 and pl[0]["channel"] == -1 and pl[5]["channel"] == -1 and summ["first"] == 16383 - 50


def test_placement_lost_strip_and_other_apids(image):
    apids = (64, 65, 68)
    pic = I.picture(8, 3)
    packets = I.picture_packets(pic, q=40, first_seq=16383 - 60, apids=apids)
    kept = packets[:43] + packets[86:]                                             # the middle strip row is lost
    vcdu, _, _ = I.mux(kept, counter=77)
    res = image.model_host(vcdu, apids=apids)
    want = I.expected_picture(packets, 3, apids)
    print(res.summary)
    assert res.summary["rows"] == 3 and res.summary["placed"] == 84 and res.summary["seq_gaps"] == 1 and res.summary["cells_filled"] == 84
    for k, a in enumerate(apids):
        assert res.images[a].shape == (24, 1568)
        assert np.array_equal(res.images[a][:8], want[k][:8]) and np.array_equal(res.images[a][16:], want[k][16:]) and not res.images[a][8:16].any()
        assert res.filled[a][0].all() and res.filled[a][2].all() and not res.filled[a][1].any()
    default = image.model_host(vcdu)                                               # 68 is not active, 66 never comes
    assert default.summary["placed"] == 56 and not default.images[66].any() and np.array_equal(default.images[65], res.images[65])
    assert default.summary["per_apid"][68] == 28


# --------------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("piece", [1, 2, 3])
def test_pieces_equal_one_batch(image, piece):
    """The host entry's model path in pieces of 1, 2, 3 frames: packets that cross piece boundaries (up to three frames long) come
    out exactly as in one batch, on the damaged batch and on the picture."""
    vcdu, info, _, want = I.demux_batch()
    whole = image.model_host(vcdu, info, piece_frames=8192)
    got = image.model_host(vcdu, info, piece_frames=piece)
    assert _keys(whole.desc) == want and np.array_equal(got.desc, whole.desc) and np.array_equal(got.sinfo, whole.sinfo)
    pic, packets, frames = I.sent()
    whole = image.model_host(frames)
    got = image.model_host(frames, piece_frames=piece)
    for name in ("desc", "sinfo", "strips", "place"):
        assert np.array_equal(getattr(got, name), getattr(whole, name)), name
    assert got.summary == whole.summary and all(np.array_equal(got.images[a], whole.images[a]) for a in (64, 65, 66))
    assert np.array_equal(np.stack([whole.images[a] for a in (64, 65, 66)]), I.expected_picture(packets, I.PIC_ROWS))
    # a packet longer than the overlap's worth of ordinary frames: 40 000 bytes, 46 frames, in pieces of `piece`
    long_one = [I.plain_packet(64, 1, 300), I.plain_packet(65, 2, 40000), I.plain_packet(66, 3, 500)]
    v, _, _ = I.mux(long_one, offset=0)
    assert _keys(image.model_host(v, piece_frames=piece).desc)[:3] == [(64, 1, 300), (65, 2, 40000), (66, 3, 500)]
