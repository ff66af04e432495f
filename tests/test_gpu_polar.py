"""GPU tests of the polar layer (include/meteor_demod_amd_polar.h): the node kernel against the host solver by the header's rule of
agreement, inside canaries and with its inputs unchanged, on frames from 1 x 1 pixel to the pass over the pole, both hemispheres and
1, 3 and 8 passes in one launch; the whole entry against the host path byte for byte, in bands, grey and colour, feather and best;
the device entry's argument checks; polar.draw against the overlay layer's model byte for byte across a band border.  Every GPU step runs once; every test prints the figures it asserts on."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import map_util as MU
import polar_util as PU_

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0x5A5A5A5A, 64                       # words of canary on either side of every node buffer


# ------------------------------------------------------------------------------------------------------- node kernel cases
def _raans(n):
    return [None] + [150.0 + 7.0 * k for k in range(1, n)]


@functools.lru_cache(maxsize=None)
def node_case(name):
    """(passes, numpy passes, frame or None for the passes' own, resolution)."""
    from meteor_demod_amd import polar as P
    short = PU_.polar_pass(PU_.SHORT_U, PU_.SHORT_ROWS)
    if name == "40 lines over the pole, 4000 m":
        return [short[0]], [short[1]], None, 4000.0
    if name == "1 x 1 pixel":
        return [short[0]], [short[1]], P.Frame(1, 1, 4000.0, -2000.0, 50000.0, 1, 70.0, 47.0), 4000.0
    if name == "node (1, 2) on the pole":
        return [short[0]], [short[1]], P.Frame(64, 48, 100.0, -32.5 * 100.0, 16.5 * 100.0, 1, 70.0, 47.0), 100.0
    if name == "360 nodes, more than a block and no multiple of it":
        return [short[0]], [short[1]], P.Frame(300, 270, 4000.0, -700000.0, 600000.0, 1, 60.0, -120.0), 4000.0
    if name == "the southern pass":
        south = PU_.polar_pass(PU_.SOUTH_U, 77)
        return [south[0]], [south[1]], None, 8000.0
    n = {"1 pass of 3 rows": 1, "3 passes of 3, 40 and 77 rows": 3, "8 passes of 3, 40 and 77 rows": 8}[name]
    rows = [(3, 40, 77)[k % 3] for k in range(n)]
    both = [PU_.polar_pass(80.0, rows[k], raan, later=5 * k) for k, raan in enumerate(_raans(n))]
    return [b[0] for b in both], [b[1] for b in both], None, 8000.0


NODE_CASES = ("40 lines over the pole, 4000 m", "1 x 1 pixel", "node (1, 2) on the pole", "360 nodes, more than a block and no multiple of it", "the southern pass",
              "1 pass of 3 rows", "3 passes of 3, 40 and 77 rows", "8 passes of 3, 40 and 77 rows")


@functools.lru_cache(maxsize=None)
def host_nodes(name):
    """The host solver's grid of a case: computed once."""
    from meteor_demod_amd import polar as P
    passes, _, frame, res = node_case(name)
    return P.grid(passes, metres_per_pixel=res) if frame is None else P.model_nodes(passes, frame, metres_per_pixel=res)


@pytest.mark.parametrize("name", NODE_CASES)
def test_node_kernel_agrees_with_the_host_solver(name, gpu_device):
    import torch
    from meteor_demod_amd import polar as P
    passes, refs, _, _ = node_case(name)
    g = host_nodes(name)
    frame, n = g.frame, len(passes)
    words = int(np.prod(frame.nodes_shape))
    dev = f"cuda:{gpu_device}"
    arena = torch.full((n, words + 2 * GUARD), CANARY, dtype=torch.int32, device=dev)
    out = [arena[k, GUARD: GUARD + words].view(frame.nodes_shape) for k in range(n)]
    need = sum(24 * s.table.shape[0] for s in g.solvers)
    work_arena = torch.full((need + 128,), 0xA5, dtype=torch.uint8, device=dev)
    tables = [s.table.copy() for s in g.solvers]
    fields = [dict(s.fields) for s in g.solvers]
    P.nodes_device(frame, g.solvers, device=dev, out=out, work=work_arena[64: 64 + need])
    torch.cuda.synchronize(gpu_device)
    got, work = arena.cpu().numpy(), work_arena.cpu().numpy()
    assert (got[:, :GUARD] == CANARY).all() and (got[:, GUARD + words:] == CANARY).all() and (work[:64] == 0xA5).all() and (work[64 + need:] == 0xA5).all()
    assert all(np.array_equal(t, s.table) for t, s in zip(tables, g.solvers)) and all(f == s.fields for f, s in zip(fields, g.solvers))
    assert np.array_equal(work[64: 64 + need].view(np.float64), np.concatenate([t.reshape(-1) for t in tables]))           # the tables, as the host made them
    broken = differ = total = there = 0
    for k in range(n):
        nodes = got[k, GUARD: GUARD + words].reshape(frame.nodes_shape)
        b, d, t = PU_.agreement(nodes, g.nodes[k], refs[k], passes[k].images[0].shape[0])
        broken, differ, total, there = broken + b, differ + d, total + t, there + int((~PU_.missing(nodes)).sum())
    print(f"{name}: {frame.width} x {frame.height}, {n} x {frame.nodes_shape[0]} x {frame.nodes_shape[1]} nodes, {there} of {total} present; {differ} differ from the host's "
          f"({100.0 * differ / total:.3f} %), {broken} break the rule")
    assert broken == 0 and there > 0
    if name == "node (1, 2) on the pole":
        assert not PU_.missing(got[0, GUARD: GUARD + words].reshape(frame.nodes_shape)).any()


def test_nodes_device_refusals(gpu_device):
    """Each with its text, and nothing written: the node buffer and the work buffer keep their canaries."""
    import torch
    from meteor_demod_amd import _capi, polar as P
    g = host_nodes("40 lines over the pole, 4000 m")
    frame, dev = g.frame, f"cuda:{gpu_device}"
    words = int(np.prod(frame.nodes_shape))
    nodes = torch.full((words + 2,), CANARY, dtype=torch.int32, device=dev)
    need = 24 * g.solvers[0].table.shape[0]
    work = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device=dev)
    lib = P.lib()

    def call(frame=frame, solver=g.solvers[0], n=1, node_ptr=nodes.data_ptr(), work_ptr=work.data_ptr(), work_bytes=need, solvers=True, ptrs=True, **fields):
        f, s = frame.c(), solver.c()
        for k, v in fields.items():
            setattr(s if hasattr(s, k) else f, k, v)
        arr = (P.MdemodPolarSolver * 9)(*([s] * 9))
        p = (C.c_void_p * 9)(*([node_ptr] + [node_ptr] * 8))
        return lib.mdemod_polar_nodes_device(C.byref(f), arr if solvers else None, n, p if ptrs else None, C.c_void_p(work_ptr), work_bytes, gpu_device,
                                             C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream))
    cases = (("more than a polar picture takes", dict(n=9)), ("passes and their node buffers", dict(solvers=False)), ("passes and their node buffers", dict(ptrs=False)),
             ("node buffer of pass 0", dict(node_ptr=None)), ("multiples of 4", dict(node_ptr=nodes.data_ptr() + 2)), ("work buffer is needed", dict(work_ptr=None)),
             ("multiple of 8", dict(work_ptr=work.data_ptr() + 4)), ("the tables take", dict(work_bytes=need - 1)), ("intersect", dict(n=2, work_bytes=2 * need)),
             ("intersect", dict(work_ptr=nodes.data_ptr(), work_bytes=4 * words + 8)), ("table of pass 0", dict(table=None)), ("table of pass 0", dict(table_n=0)),
             ("entries", dict(table_n=(1 << 20) + 1)), ("not a number", dict(u=float("nan"))), ("not a number", dict(sec_hi=float("inf"))), ("must be positive", dict(line_period=0.0)),
             ("scan side", dict(side=0)), ("width is 0", dict(width=0)), ("height is 16385", dict(height=16385)), ("nodes do not go with", dict(node_cols=frame.nodes_shape[1] + 1)),
             ("pole is 0", dict(pole=0)), ("resolution", dict(res=50.0)), ("standard parallel", dict(lat_ts_deg=0.0)), ("projection 3", dict(projection=3)))
    for word, kw in cases:
        rc = call(**kw)
        detail = _capi.last_error()
        print(f"{word}: '{detail}'")
        assert rc == _capi.MDEMOD_ERR_PARAM and word in detail, (word, rc, detail)
    torch.cuda.synchronize(gpu_device)
    assert (nodes.cpu().numpy() == CANARY).all() and (work.cpu().numpy() == 0xA5).all()
    assert call(n=0, solvers=False, ptrs=False, work_ptr=None, work_bytes=0) == 0          # nothing to do
    assert int(lib.mdemod_polar_nodes_work_bytes(None, 0)) == 0 and int(lib.mdemod_polar_nodes_work_bytes((P.MdemodPolarSolver * 1)(g.solvers[0].c()), 1)) == need


# ------------------------------------------------------------------------------------------------------------ whole entry
RES = 4000.0


@functools.lru_cache(maxsize=None)
def picture_passes():
    """Two passes of 40 and 32 strip rows over the pole, random bytes of different brightness, 15 % of the strips lost, the second
    with its node 12 degrees further east and 6 row periods later."""
    from meteor_demod_amd import mosaic as M
    rng = np.random.default_rng(61)
    out = []
    for k, (rows, text, later, top) in enumerate(((40, MU.tle_text(), 0, 256), (32, MU.with_raan(162.0), 6, 140))):
        s0 = MU.mid_latitude_s0(86.0) + later * MU.ROW_PERIOD
        place, info = MU.packets(rows, s0, keep=rng.random((rows, 3, 14)) >= 0.15)
        images = [rng.integers(20 * k, top, (8 * rows, 1568), dtype=np.uint8) for _ in range(3)]
        out.append(M.Pass(text, images, MU.filled_of(place, rows), place, info))
    return out


@functools.lru_cache(maxsize=None)
def composed(select, blend, stretch, nodes_on_host, piece_lines=0):
    from meteor_demod_amd import polar as P
    return P.compose(picture_passes(), select, metres_per_pixel=RES, blend=blend, stretch=stretch, nodes_on_host=nodes_on_host, piece_lines=piece_lines)


@functools.lru_cache(maxsize=None)
def modelled(select, blend, stretch):
    from meteor_demod_amd import polar as P
    return P.model_host(picture_passes(), select, metres_per_pixel=RES, blend=blend, stretch=stretch)


def _same(a, b):
    return np.array_equal(a.pixels, b.pixels) and np.array_equal(a.valid, b.valid) and np.array_equal(a.cover, b.cover)


@pytest.mark.parametrize("select,blend,stretch", [((2, 1, 0), "feather", 1), ((1,), "best", 2), ((0, 0, 2), "best", 0), ((2,), "feather", 0)])
def test_compose_with_host_nodes_is_the_model(select, blend, stretch, gpu_device):
    got, want = composed(select, blend, stretch, 1), modelled(select, blend, stretch)
    print(f"select {select}, {blend}, stretch {stretch}: {got.width} x {got.height}, {100 * got.valid_share:.1f} % valid, {100 * got.overlap_share:.1f} % seen by both, "
          f"limits {[r.limits for r in got.passes]}")
    assert got.nodes_on_host and got.frame == want.frame and _same(got, want) and np.array_equal(got.nodes, want.nodes)
    assert [r.limits for r in got.passes] == [r.limits for r in want.passes] and [r.covered for r in got.passes] == [r.covered for r in want.passes]
    assert (got.valid_pixels, got.overlap_pixels) == (want.valid_pixels, want.overlap_pixels) and got.valid_share > 0.2 and (blend == "best" or got.overlap_share > 0.05)


@pytest.mark.parametrize("select,blend", [((2, 1, 0), "feather"), ((1,), "best")])
def test_compose_with_device_nodes(select, blend, gpu_device):
    """The picture is the mosaic layer's model blend run over the nodes the result returns, byte for byte, and those nodes agree with
    the host solver's by the header's rule."""
    from meteor_demod_amd import mosaic as M, polar as P
    passes = picture_passes()
    got = composed(select, blend, 0, 0)
    assert not got.nodes_on_host and got.nodes.shape == (2, *got.frame.nodes_shape)
    ident = np.arange(256, dtype=np.uint8)[None].repeat(len(select), 0)
    src = [(p.images, p.filled, ident, got.nodes[k]) for k, p in enumerate(passes)]
    out, val, cov = M.model_blend(src, select, got.width, got.height, blend, valid=True, cover=True)
    px = got.pixels if len(select) == 3 else got.pixels[..., None]
    assert np.array_equal(px, out) and np.array_equal(got.valid, val) and np.array_equal(got.cover, cov)
    host = P.model_nodes(passes, got.frame, metres_per_pixel=RES)
    refs = [MU.ref_pass(40, s0=MU.mid_latitude_s0(86.0)), MU.ref_pass(32, s0=MU.mid_latitude_s0(86.0) + 6 * MU.ROW_PERIOD, text=MU.with_raan(162.0))]
    broken = differ = total = 0
    for k, (ref, rows) in enumerate(zip(refs, (40, 32))):
        b, d, t = PU_.agreement(got.nodes[k], host.nodes[k], ref, 8 * rows)
        broken, differ, total = broken + b, differ + d, total + t
    print(f"select {select}, {blend}: {got.width} x {got.height}, {100 * got.valid_share:.1f} % valid; {differ} of {total} nodes differ from the host's, {broken} break the rule")
    assert broken == 0 and got.valid_share > 0.2


def test_cli_map_proj_stereo(tmp_path, gpu_device):
    """The one-row recording with real stamps through --image --composite 321 --map --map-proj stereo --graticule 5: the picture, its
    world file, its .prj, the overlay picture and the lines; the pixels are those of polar.images_to_polar on the same data, the
    overlay those of polar.draw; two files with --mosaic give the picture of both passes; without --map-proj the outputs are those
    of --map-proj latlon and of map.image_to_map, byte for byte."""
    import re
    import subprocess

    import frames_util as U
    from conftest import GOLDEN, ROOT
    from meteor_demod_amd import image, map as MP, polar as P, rs
    from test_gpu_map import _pnm
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    tle = GOLDEN / "map_tle.txt"
    st, iq = MU.recording()
    dirs = {}
    for name in ("stereo", "plain", "latlon"):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
        (dirs[name] / "one.wav").write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))
    (dirs["stereo"] / "two.wav").write_bytes(U.wav_bytes(U.REC_SAMPLERATE, iq))

    def run(cwd, files, *flags):
        return subprocess.run([str(cli_exe), "-q", "-B", "--device", str(gpu_device), *flags, *files], capture_output=True, text=True, cwd=cwd, timeout=300)

    common = ("--cadu", "--image", "--composite", "321", "--map", str(tle), "--scan-angle", "108")
    p = run(dirs["stereo"], ["one.wav", "two.wav"], *common, "--map-proj", "stereo", "--map-res", "4000", "--graticule", "5", "--mosaic", "both")
    assert p.returncode == 0, p.stderr
    print(p.stdout)
    names = sorted(x.name for x in dirs["stereo"].iterdir())
    for stem in ("one.wav_321_polar", "two.wav_321_polar", "both_321_polar"):
        for ext in (".ppm", ".wld", ".prj", "_overlay.ppm", "_overlay.wld", "_overlay.prj"):
            assert stem + ext in names, (stem + ext, names)
    assert not any("_map" in x or "_mosaic" in x for x in names)
    cadu = np.frombuffer((dirs["stereo"] / "one.wav.cadu").read_bytes(), dtype=np.uint8).reshape(-1, 1024)
    vcdu, info = rs.model_decode(cadu)
    res = image.vcdu_to_image(vcdu, info, device=gpu_device)
    want = P.images_to_polar([res], tle.read_text(), composite="321", device=gpu_device, metres_per_pixel=4000, scan_deg=108)
    got = _pnm(dirs["stereo"] / "one.wav_321_polar.ppm", rb"P6", 3)
    print(f"{want.width} x {want.height}, {100 * want.valid_share:.2f} % valid, pole {want.frame.pole}, lon0 {want.frame.lon0_deg}")
    assert np.array_equal(got, want.pixels) and want.valid.any() and want.frame.pole == 1
    assert np.array_equal(got, _pnm(dirs["stereo"] / "two.wav_321_polar.ppm", rb"P6", 3))
    wld = (dirs["stereo"] / "one.wav_321_polar.wld").read_text()
    assert len(wld.split()) == 6 and wld == want.world_file() and [float(v) for v in wld.split()][:4] == [4000.0, 0.0, 0.0, -4000.0]
    prj = (dirs["stereo"] / "one.wav_321_polar.prj").read_text()
    assert prj == want.prj() and 'PROJECTION["Polar_Stereographic"]' in prj and 'PARAMETER["latitude_of_origin",70]' in prj
    assert f'PARAMETER["central_meridian",{want.frame.lon0_deg:g}]' in prj
    both = P.images_to_polar([res, res], tle.read_text(), composite="321", device=gpu_device, metres_per_pixel=4000, scan_deg=108)
    assert np.array_equal(_pnm(dirs["stereo"] / "both_321_polar.ppm", rb"P6", 3), both.pixels) and np.array_equal(both.cover, 3 * (both.valid != 0))
    # the overlay: the graticule through vertices and the overlay layer's kernel, style 1 of the C host (the overlay layer's defaults)
    lon, lat, first, step = P.graticule(want.frame, 5.0)
    pts = P.vertices(want.frame, lon, lat, first)
    over = _pnm(dirs["stereo"] / "one.wav_321_polar_overlay.ppm", rb"P6", 3)
    changed = (over != want.pixels).any(axis=-1)
    x, y = pts[0] / 256.0, pts[1] / 256.0
    inside = (x > 2) & (x < want.width - 3) & (y > 2) & (y < want.height - 3)
    on_line = changed[np.rint(y[inside]).astype(int), np.rint(x[inside]).astype(int)]
    print(f"overlay: {int(changed.sum())} pixels changed; {int(on_line.sum())} of {int(inside.sum())} graticule vertices inside the picture lie on a changed pixel")
    assert step == 5.0 and inside.sum() > 10 and on_line.mean() > 0.9 and changed.mean() < 0.2
    line = [l for l in p.stdout.splitlines() if l.startswith("one.wav: polar 321")]
    m = re.fullmatch(r"one.wav: polar 321 \(feather\): (\d+) x (\d+) at 4000 m; north pole, central meridian ([-\d.]+), true scale at 70; E (-?\d+) \.\. (-?\d+), "
                     r"N (-?\d+) \.\. (-?\d+); 1 pass; first lines (\S+)Z; ([\d.]+) % of pixels valid; ([\d.]+) % seen by two or more passes", line[0])
    assert m, line
    assert [int(m.group(1)), int(m.group(2))] == [want.width, want.height] and float(m.group(3)) == want.frame.lon0_deg
    assert float(m.group(4)) == want.frame.e_left and float(m.group(7)) == want.frame.n_top and abs(float(m.group(9)) - 100 * want.valid_share) < 0.051
    assert sum(l.startswith("both: polar 321") for l in p.stdout.splitlines()) == 1 and sum("_polar_overlay:" in l for l in p.stdout.splitlines()) == 3
    # nothing changes without the option
    plain_flags = (*common, "--map-scale", "60", "-o", "one.wav.s")                 # (the name a run of several files gives it)
    a, b = run(dirs["plain"], ["one.wav"], *plain_flags), run(dirs["latlon"], ["one.wav"], *plain_flags, "--map-proj", "latlon")
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout, (a.stderr, b.stderr)
    files = sorted(x.name for x in dirs["plain"].iterdir())
    assert files == sorted(x.name for x in dirs["latlon"].iterdir()) and "one.wav_321_map.ppm" in files and not any("polar" in x for x in files)
    for name in files:
        assert (dirs["plain"] / name).read_bytes() == (dirs["latlon"] / name).read_bytes(), name
    plain = MP.image_to_map(res, tle.read_text(), composite="321", device=gpu_device, px_per_deg=60, scan_deg=108)
    assert np.array_equal(_pnm(dirs["plain"] / "one.wav_321_map.ppm", rb"P6", 3), plain.pixels)


def test_bands_equal_one_batch(gpu_device):
    whole = composed((2, 1, 0), "feather", 0, 0)
    assert whole.height > 48
    for piece in (16, 48, 1024):
        banded = composed((2, 1, 0), "feather", 0, 0, piece)
        print(f"bands of {piece} lines over {whole.height}: equal to one batch: {_same(banded, whole)}")
        assert _same(banded, whole) and np.array_equal(banded.nodes, whole.nodes)
    assert _same(composed((1,), "best", 2, 1, 16), composed((1,), "best", 2, 1))


# ------------------------------------------------------------------------------------------------------------------ lines
DRAW_W, DRAW_H = 36, 1060                            # a multiple of 4 and none of the 32-pixel tile; the band border at line 1024 inside
DRAW_STYLES = [(128, 256, (255, 0, 0), False), (64, 160, (0, 255, 0), False), (2048, 200, (0, 0, 255), False), (300, 256, (255, 255, 0), True)]


def _line(*points):
    """One polyline through pixel coordinates as (x, y, first) in fixed point."""
    x, y = (np.rint(256.0 * np.array(c, dtype=np.float64)).astype(np.int32) for c in zip(*points))
    return x, y, np.array([0, len(points)], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def draw_layers():
    """((x, y, first), style): a diagonal across lines 1023 / 1024, a vertical line on the tile edge x = 31.5, a wide line whose square
    cap reaches across the band border, an inside_only line, and a layer without a line."""
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.uint32))
    return ((_line((2, 1000), (33, 1050)), 0), (_line((31.5, 10), (31.5, 1055)), 1), (_line((5, 1016), (20, 1021)), 2), (_line((0, 500), (35, 540)), 3), (none, 0))


@pytest.mark.parametrize("planes", [3, 1])
def test_draw_is_the_overlay_layers_model(planes, gpu_device):
    """polar.draw goes through the overlay layer's banded draw: the bytes are those of that layer's model over the pieces of every
    layer in layer order, the report's pieces those counted per style, its tiles and items those of the overlay layer's bins."""
    from meteor_demod_amd import overlay as OV, polar as P
    rng = np.random.default_rng(17 + planes)
    pixels = rng.integers(0, 256, (DRAW_H, DRAW_W, 3) if planes == 3 else (DRAW_H, DRAW_W), dtype=np.uint8)
    valid = (rng.random((DRAW_H, DRAW_W)) >= 0.3).astype(np.uint8)              # holes for the inside_only style
    styles = [OV.Style(*s) for s in DRAW_STYLES]
    pcs = np.concatenate([OV.pieces(OV.Points(*pts), s, DRAW_STYLES[s][0], DRAW_W, DRAW_H) for pts, s in draw_layers()])
    want, mask = OV.model_pieces(pixels, pcs, styles, valid)
    tile_first, items = OV.bins(pcs, styles, DRAW_W, DRAW_H)
    got, rep = P.draw(pixels, list(draw_layers()), DRAW_STYLES, valid=valid, device=gpu_device)
    counts = [int((pcs["style"] == s).sum()) for s in range(4)]
    changed = (got != pixels).reshape(DRAW_H, DRAW_W, -1).any(axis=-1)
    print(f"{planes} planes: {len(pcs)} pieces {counts}, report {rep}; {int(changed.sum())} pixels changed, {int(changed[1024:].sum())} of them below the band border, "
          f"{int((mask != 0).sum())} in the model's mask")
    assert np.array_equal(got, want)
    assert rep["pieces"] == counts and all(counts) and rep["tiles"] == int((np.diff(tile_first.astype(np.int64)) > 0).sum()) and rep["items"] == items.size
    assert changed[:1024].any() and changed[1024:].any() and changed[1023].any() and changed[1024].any()
    assert (mask == 8).any() and (valid == 0).any() and not (mask & 8)[valid == 0].any()       # the inside_only line keeps out of the holes
    # no layer at all: the picture comes back unchanged
    same, none = P.draw(pixels, [], DRAW_STYLES, valid=valid, device=gpu_device)
    assert np.array_equal(same, pixels) and none == dict(pieces=[0, 0, 0, 0], tiles=0, items=0)
