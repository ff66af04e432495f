/*
 * fuzz_polar.cpp — the host side of the polar layer (csrc/polar_host.cpp over csrc/mosaic_host.cpp and csrc/map_host.cpp) under
 * ASan + UBSan (tests/test_polar_sanitize.py): 1 .. 4 passes of 1 .. 6 strip rows anywhere on the orbit (both poles, the equator,
 * where the frame refuses), within seconds of each other so that they overlap, random options (some out of range: refused with
 * MDEMOD_ERR_PARAM and a text), the frame with its host nodes and solver constants, the same nodes through the model's entry on the
 * frame that came back, the projection both ways, the graticule, vertices of it and of random polylines that cross the equator and
 * the date line, the world file and the .prj into buffers exactly as long as they must be, and the whole-picture entry's model path
 * in bands of 16 .. 96 lines against one batch.  Every buffer is exactly as long as the interface says and comes from the heap, so
 * that one byte too far is a report.  What comes back is checked against the rules that hold for any input.  Prints one JSON line.
 * Usage: fuzz_polar <cases> <seed> <tle file>
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/meteor_demod_amd_polar.h"
#include "../../meteor_demod_amd/csrc/polar_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

struct PassData {
	uint32_t rows = 0;
	size_t n_desc = 0;
	std::unique_ptr<mdemod_placement[]> place;
	std::unique_ptr<mdemod_strip_info[]> sinfo;
	std::unique_ptr<uint8_t[]> img[3], fil[3];
	std::unique_ptr<char[]> text;
};

static void
check_points(const mdemod_polar_points &p, const char *what)
{
	if (!p.first || p.first[p.n_lines] != p.n_points) { FAIL("%s: first[] does not end at the points", what); return; }
	for (uint32_t l = 0; l < p.n_lines; l++)
		if (p.first[l + 1] < p.first[l] + 2) FAIL("%s: line %u has fewer than two vertices", what, l);
	long sum = 0;
	for (uint32_t k = 0; k < p.n_points; k++) sum += (p.x[k] & 1) + (p.y[k] & 1);          /* every word is read */
	if (sum < 0) FAIL("%s: impossible", what);
}

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 100;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	std::string text;
	if (FILE *f = argc > 3 ? fopen(argv[3], "rb") : nullptr) {
		char block[512];
		for (size_t n; (n = fread(block, 1, sizeof block, f)) > 0;) text.append(block, n);
		fclose(f);
	}
	mdemod_map_tle tle;
	if (mdemod_map_parse_tle(text.c_str(), 0, &tle) != MDEMOD_OK) { fprintf(stderr, "the element set of %s is not read: %s\n", argc > 3 ? argv[3] : "(none)", mdemod_last_error()); return 2; }
	long refused = 0, frame_refused = 0, frames = 0, north = 0, south = 0, passes_total = 0, nodes_there = 0, bands = 0, lines_cut = 0, vertices = 0, graticules = 0, most = 0;
	for (long i = 0; i < cases; i++) {
		const uint32_t n = 1 + static_cast<uint32_t>(rng() % 4);
		const double start = static_cast<double>(rng() % 86400000) / 1000.0;
		std::vector<PassData> data(n);
		auto passes = exact<mdemod_polar_pass>(n);
		memset(passes.get(), 0, n * sizeof(mdemod_polar_pass));
		for (uint32_t k = 0; k < n; k++) {
			PassData &d = data[k];
			d.rows = 1 + static_cast<uint32_t>(rng() % 6);
			const double s0 = start + static_cast<double>(rng() % 120) / 10.0, period = 1.0 + static_cast<double>(rng() % 500) / 1000.0;
			std::vector<mdemod_placement> pl;
			std::vector<mdemod_strip_info> si;
			for (uint32_t r = 0; r < d.rows; r++)
				for (int ch = 0; ch < 3; ch++)
					for (uint32_t c = 0; c < 14; c++) {
						if (rng() % 5 == 0) continue;
						const double s = fmod(s0 + r * period, 86400.0);
						mdemod_placement p = { rng() % 9 ? ch : -1, r, c, 0 };
						mdemod_strip_info q;
						memset(&q, 0, sizeof q);
						q.ms = static_cast<uint32_t>(s * 1000.0);
						pl.push_back(p);
						si.push_back(q);
					}
			d.n_desc = pl.size();
			d.place = exact<mdemod_placement>(pl.size());
			d.sinfo = exact<mdemod_strip_info>(si.size());
			if (!pl.empty()) { memcpy(d.place.get(), pl.data(), pl.size() * sizeof pl[0]); memcpy(d.sinfo.get(), si.data(), si.size() * sizeof si[0]); }
			d.text = exact<char>(text.size() + 1);
			memcpy(d.text.get(), text.c_str(), text.size() + 1);
			for (int s = 0; s < 3; s++) {
				d.img[s] = exact<uint8_t>(d.rows * PIC_LINE_BYTES);
				d.fil[s] = exact<uint8_t>(static_cast<size_t>(d.rows) * PIC_CELLS);
				for (size_t b = 0; b < d.rows * PIC_LINE_BYTES; b++) d.img[s][b] = static_cast<uint8_t>(rng());
				for (size_t b = 0; b < static_cast<size_t>(d.rows) * PIC_CELLS; b++) d.fil[s][b] = static_cast<uint8_t>(rng() % 4 ? 1 + rng() % 255 : 0);
			}
			mdemod_polar_pass &p = passes[k];
			p.tle_text = d.text.get();
			p.norad = rng() % 4 ? 0 : tle.norad;
			p.date = rng() % 3 ? MDEMOD_POLAR_DATE_AUTO : tle.epoch_day + static_cast<int32_t>(rng() % 5) - 2;
			for (int s = 0; s < 3; s++) { p.image[s] = d.img[s].get(); p.filled[s] = d.fil[s].get(); }
			p.rows = d.rows; p.place = d.place.get(); p.sinfo = d.sinfo.get(); p.n_desc = d.n_desc;
		}
		mdemod_polar_opts o;
		mdemod_polar_default_opts(&o);
		o.metres_per_pixel = 8000.0 + static_cast<double>(rng() % 60000);
		o.scan_deg = rng() & 1 ? 110.0 : 1.0 + static_cast<double>(rng() % 12001) / 100.0;
		o.side = rng() & 1 ? 1 : -1;
		o.pole = static_cast<int32_t>(rng() % 5 ? 0 : rng() % 2 ? 1 : -1);
		o.lat_ts_deg = rng() % 3 ? 70.0 : 0.5 + static_cast<double>(rng() % 896) / 10.0;
		if (rng() % 3 == 0) o.lon0_deg = static_cast<double>(rng() % 7201) / 10.0 - 360.0;
		o.stretch = static_cast<uint32_t>(rng() % 3);
		o.clip_low = static_cast<uint32_t>(rng() % 500);
		o.clip_high = static_cast<uint32_t>(rng() % 500);
		o.piece_lines = 16 * static_cast<uint32_t>(rng() % 7);
		o.blend = static_cast<uint32_t>(rng() & 1);
		const uint32_t planes = rng() & 1 ? 3 : 1;
		const uint32_t select[3] = { static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3), static_cast<uint32_t>(rng() % 3) };
		mdemod_polar_nodes grid, again;
		if (rng() % 8 == 0) {
			uint32_t count = n;
			switch (rng() % 9) {
			case 0: o.metres_per_pixel = rng() & 1 ? 99.0 : 100001.0; break;
			case 1: o.scan_deg = rng() & 1 ? 0.5 : 131.0; break;
			case 2: o.side = static_cast<int32_t>(rng() % 5) * 2; break;
			case 3: o.pole = rng() & 1 ? 2 : -2; break;
			case 4: o.lat_ts_deg = rng() & 1 ? 0.0 : 90.5; break;
			case 5: o.lon0_deg = rng() & 1 ? 360.5 : -1.0e300; break;
			case 6: o.blend = 2; break;
			case 7: o.piece_lines = 8; break;
			default: count = rng() & 1 ? 0 : 9; break;
			}
			const int rc = mdemod_polar_grid(&o, count == 9 ? nullptr : passes.get(), count, &grid);
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: options out of range gave %d '%s'", i, rc, mdemod_last_error());
			mdemod_polar_grid_free(&grid);
			refused++;
			continue;
		}
		const int rc = mdemod_polar_grid(&o, passes.get(), n, &grid);
		if (rc == MDEMOD_ERR_PARAM) {
			if (!*mdemod_last_error()) FAIL("case %ld: a refusal without a text", i);
			if (grid.nodes[0] || grid.solver[0].table) FAIL("case %ld: a refused grid holds memory", i);
			frame_refused++;
			continue;
		}
		if (rc != MDEMOD_OK) { FAIL("case %ld: mdemod_polar_grid gave %d '%s'", i, rc, mdemod_last_error()); continue; }
		frames++;
		passes_total += n;
		most = n > static_cast<uint32_t>(most) ? n : most;
		const mdemod_polar_frame f = grid.frame;
		(f.pole > 0 ? north : south)++;
		const size_t count = static_cast<size_t>(f.node_rows) * f.node_cols;
		if (f.width % 4 || !f.width || f.width > MDEMOD_POLAR_MAX_WIDTH || !f.height || f.height > MDEMOD_POLAR_MAX_HEIGHT || f.node_rows != (f.height + 15) / 16 + 1 ||
		    f.node_cols != (f.width + 15) / 16 + 1 || (f.pole != 1 && f.pole != -1) || f.lat_ts_deg * f.pole <= 0 || !(f.lon0_deg >= -180.0 && f.lon0_deg < 180.0) || grid.n != n)
			FAIL("case %ld: a frame of %u x %u, pole %d, parallel %g, meridian %g", i, f.width, f.height, f.pole, f.lat_ts_deg, f.lon0_deg);
		/* the same frame through the model's entry: the same nodes, into memory of its own */
		if (mdemod_polar_model_nodes(&o, passes.get(), n, &f, &again) != MDEMOD_OK) FAIL("case %ld: the frame that came back is refused: %s", i, mdemod_last_error());
		for (uint32_t k = 0; k < n; k++) {
			const mdemod_polar_solver &s = grid.solver[k];
			if (!s.table || !s.table_n || !(s.sec_hi > s.sec_lo) || !(s.line_period > 0)) FAIL("case %ld: the solver of pass %u", i, k);
			double norm = 0;
			for (uint32_t t = 0; t < 3 * s.table_n; t++) norm += s.table[t] * s.table[t];
			if (fabs(norm - s.table_n) > 1e-6 * s.table_n) FAIL("case %ld: the table of pass %u holds no unit vectors", i, k);
			for (size_t a = 0; a < count; a++) {
				const int32_t X = grid.nodes[k][2 * a], Y = grid.nodes[k][2 * a + 1];
				nodes_there += X != MDEMOD_POLAR_NO_NODE;
				if ((X == MDEMOD_POLAR_NO_NODE) != (Y == MDEMOD_POLAR_NO_NODE)) FAIL("case %ld: half a node", i);
				if (again.nodes[k] && (again.nodes[k][2 * a] != X || again.nodes[k][2 * a + 1] != Y)) { FAIL("case %ld: the two entries differ at node %zu of pass %u", i, a, k); break; }
			}
		}
		mdemod_polar_grid_free(&again);
		/* the projection both ways at the corners of the picture */
		{
			auto e = exact<double>(4), nn = exact<double>(4), lat = exact<double>(4), lon = exact<double>(4), e2 = exact<double>(4), n2 = exact<double>(4);
			for (int c = 0; c < 4; c++) { e[c] = f.e_left + (c & 1 ? f.width * f.res : 0.0); nn[c] = f.n_top - (c & 2 ? f.height * f.res : 0.0); }
			if (mdemod_polar_inverse(f.pole, fabs(f.lat_ts_deg), f.lon0_deg, e.get(), nn.get(), 4, lat.get(), lon.get()) != MDEMOD_OK ||
			    mdemod_polar_forward(f.pole, fabs(f.lat_ts_deg), f.lon0_deg, lat.get(), lon.get(), 4, e2.get(), n2.get()) != MDEMOD_OK)
				FAIL("case %ld: the projection refuses its own frame: %s", i, mdemod_last_error());
			else
				for (int c = 0; c < 4; c++)
					if (!(fabs(e2[c] - e[c]) < 1e-3 && fabs(n2[c] - nn[c]) < 1e-3)) FAIL("case %ld: corner %d comes back %g, %g m off", i, c, e2[c] - e[c], n2[c] - nn[c]);
		}
		/* the texts into buffers that just fit, and one byte less */
		for (int t = 0; t < 2; t++) {
			char big[1024];
			if ((t ? mdemod_polar_prj(&f, big, sizeof big) : mdemod_polar_world_file(&f, big, sizeof big)) != MDEMOD_OK) { FAIL("case %ld: text %d: %s", i, t, mdemod_last_error()); continue; }
			const size_t len = strlen(big) + 1;
			auto tight = exact<char>(len), small = exact<char>(len - 1);
			if ((t ? mdemod_polar_prj(&f, tight.get(), len) : mdemod_polar_world_file(&f, tight.get(), len)) != MDEMOD_OK || strcmp(tight.get(), big)) FAIL("case %ld: text %d does not fit its own length", i, t);
			if ((t ? mdemod_polar_prj(&f, small.get(), len - 1) : mdemod_polar_world_file(&f, small.get(), len - 1)) != MDEMOD_ERR_PARAM) FAIL("case %ld: text %d fits one byte less", i, t);
		}
		/* the graticule and its vertices; random polylines anywhere on the globe */
		{
			mdemod_polar_lines g;
			mdemod_polar_points p;
			const double steps[] = { 0.0, 1.0, 5.0, 10.0, 30.0 };
			if (mdemod_polar_graticule(&f, steps[rng() % 5], &g) != MDEMOD_OK) FAIL("case %ld: the graticule: %s", i, mdemod_last_error());
			else {
				graticules++;
				if (g.first[g.n_lines] != g.n_points) FAIL("case %ld: the graticule's first[]", i);
				if (mdemod_polar_vertices(&f, g.lon, g.lat, g.first, g.n_lines, &p) != MDEMOD_OK) FAIL("case %ld: the graticule's vertices: %s", i, mdemod_last_error());
				else { check_points(p, "graticule"); vertices += p.n_points; }
				mdemod_polar_points_free(&p);
			}
			mdemod_polar_lines_free(&g);
			const uint32_t n_lines = static_cast<uint32_t>(rng() % 6);
			std::vector<uint32_t> first_v(1, 0);
			std::vector<double> lon_v, lat_v;
			for (uint32_t l = 0; l < n_lines; l++) {
				const uint32_t m = static_cast<uint32_t>(rng() % 7);
				for (uint32_t v = 0; v < m; v++) { lon_v.push_back(static_cast<double>(rng() % 7201) / 10.0 - 360.0); lat_v.push_back(static_cast<double>(rng() % 1801) / 10.0 - 90.0); }
				first_v.push_back(static_cast<uint32_t>(lon_v.size()));
			}
			auto lo = exact<double>(lon_v.size()), la = exact<double>(lat_v.size());
			auto fi = exact<uint32_t>(first_v.size());
			if (!lon_v.empty()) { memcpy(lo.get(), lon_v.data(), lon_v.size() * sizeof(double)); memcpy(la.get(), lat_v.data(), lat_v.size() * sizeof(double)); }
			memcpy(fi.get(), first_v.data(), first_v.size() * sizeof(uint32_t));
			if (mdemod_polar_vertices(&f, lo.get(), la.get(), fi.get(), n_lines, &p) != MDEMOD_OK) FAIL("case %ld: random polylines: %s", i, mdemod_last_error());
			else { check_points(p, "polylines"); lines_cut += p.n_lines; vertices += p.n_points; }
			mdemod_polar_points_free(&p);
		}
		mdemod_polar_grid_free(&grid);
		/* the whole picture by the model: bands against one batch */
		mdemod_polar_result res, whole;
		const int rb = mdemod_polar_model_host(&o, passes.get(), n, select, planes, &res);
		mdemod_polar_opts one = o;
		one.piece_lines = 16384;
		const int rw = mdemod_polar_model_host(&one, passes.get(), n, select, planes, &whole);
		if (rb != MDEMOD_OK || rw != MDEMOD_OK) FAIL("case %ld: the picture of an accepted frame gave %d and %d: %s", i, rb, rw, mdemod_last_error());
		else {
			const size_t area = static_cast<size_t>(res.frame.width) * res.frame.height;
			bands++;
			if (res.frame.width != f.width || res.frame.height != f.height || whole.frame.width != f.width || memcmp(res.pixels, whole.pixels, area * planes) ||
			    memcmp(res.valid, whole.valid, area) || memcmp(res.cover, whole.cover, area))
				FAIL("case %ld: bands of %u lines differ from one batch", i, o.piece_lines);
			uint64_t valid = 0;
			for (size_t a = 0; a < area; a++) valid += res.valid[a] != 0;
			if (valid != res.valid_pixels || !res.nodes[n - 1]) FAIL("case %ld: the counts or the nodes of the result", i);
			else nodes_there += res.nodes[n - 1][2 * count - 1] != MDEMOD_POLAR_NO_NODE;                 /* (the last word is there) */
		}
		mdemod_polar_free(&res);
		mdemod_polar_free(&whole);
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"bad\": %ld, \"refused\": %ld, \"frame_refused\": %ld, \"frames\": %ld, \"north\": %ld, \"south\": %ld, \"passes\": %ld, \"most\": %ld, "
	       "\"nodes\": %ld, \"bands\": %ld, \"graticules\": %ld, \"lines\": %ld, \"vertices\": %ld}\n", bad ? "false" : "true", cases, bad, refused, frame_refused, frames, north, south,
	       passes_total, most, nodes_there, bands, graticules, lines_cut, vertices);
	return bad ? 1 : 0;
}
