/*
 * fuzz_overlay.cpp — the host side of the overlay layer (csrc/overlay_host.cpp) under ASan + UBSan (tests/test_overlay_sanitize.py).
 * Per case: a vector file, a shapefile or text, well formed or hostile (truncated, lengths that lie, part indices out of order, NaN
 * and coordinates out of range, stray bytes) through mdemod_overlay_read; polylines of any int32 vertices through the cut, the bins
 * and the model, over every piece and tile by tile; polylines in degrees through the whole-picture entry's model path in bands of
 * 32 .. 96 lines against one batch.  Every buffer is exactly as long as the interface says and comes from the heap, so that one byte
 * too far is a report.  What comes back is checked against the rules that hold for any input.  Prints one JSON line.
 * Usage: fuzz_overlay <cases> <seed> <directory for the vector files>
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/meteor_demod_amd_overlay.h"
#include "../../meteor_demod_amd/csrc/overlay_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

static void put_be32(std::string &s, uint32_t v) { for (int k = 3; k >= 0; k--) s.push_back(static_cast<char>(v >> (8 * k))); }
static void put_le32(std::string &s, uint32_t v) { for (int k = 0; k < 4; k++) s.push_back(static_cast<char>(v >> (8 * k))); }
static void put_double(std::string &s, double d) { char b[8]; memcpy(b, &d, 8); s.append(b, 8); }

static std::string
shapefile(std::mt19937_64 &rng, bool hostile)
{
	std::string body;
	const int records = static_cast<int>(rng() % 5);
	for (int r = 0; r < records; r++) {
		std::string c;
		const uint32_t types[8] = { 3, 5, 13, 15, 23, 25, 0, 1 };
		const uint32_t type = hostile && rng() % 12 == 0 ? static_cast<uint32_t>(rng() % 40) : types[rng() % 8];
		put_le32(c, type);
		if (type == 0) { /* nothing more */ }
		else if (type == 1) { put_double(c, 1.0); put_double(c, 2.0); }
		else {
			for (int k = 0; k < 4; k++) put_double(c, 0.0);
			const uint32_t parts = 1 + static_cast<uint32_t>(rng() % 3), points = parts + static_cast<uint32_t>(rng() % 9);
			put_le32(c, hostile && rng() % 10 == 0 ? static_cast<uint32_t>(rng()) : parts);
			put_le32(c, hostile && rng() % 10 == 0 ? static_cast<uint32_t>(rng()) : points);
			for (uint32_t p = 0; p < parts; p++) put_le32(c, hostile && rng() % 10 == 0 ? static_cast<uint32_t>(rng() % 12) - 2 : p);
			for (uint32_t q = 0; q < points; q++) {
				double lon = static_cast<double>(rng() % 720000) / 1000.0 - 360.0, lat = static_cast<double>(rng() % 180000) / 1000.0 - 90.0;
				if (hostile && rng() % 30 == 0) lon = rng() & 1 ? NAN : 361.0;
				if (hostile && rng() % 30 == 0) lat = rng() & 1 ? INFINITY : -90.5;
				put_double(c, lon); put_double(c, lat);
			}
			if (type > 9) for (uint32_t q = 0; q < 2 + points; q++) put_double(c, 1.5);         /* the Z / M tail is not read */
			if (c.size() % 2) c.push_back(0);
		}
		put_be32(body, static_cast<uint32_t>(r + 1));
		put_be32(body, hostile && rng() % 10 == 0 ? static_cast<uint32_t>(rng() % 4000) : static_cast<uint32_t>(c.size() / 2));
		body += c;
	}
	std::string f;
	put_be32(f, hostile && rng() % 15 == 0 ? 9993 : 9994);
	for (int k = 0; k < 5; k++) put_be32(f, 0);
	put_be32(f, hostile && rng() % 10 == 0 ? static_cast<uint32_t>(rng() % 5000) : static_cast<uint32_t>((100 + body.size()) / 2));
	put_le32(f, hostile && rng() % 15 == 0 ? 1001 : 1000);
	put_le32(f, 3);
	for (int k = 0; k < 8; k++) put_double(f, 0.0);
	f += body;
	if (hostile && rng() % 4 == 0) f.resize(rng() % (f.size() + 1));                         /* truncated */
	if (hostile && rng() % 4 == 0 && f.size() > 100) f[100 + rng() % (f.size() - 100)] = static_cast<char>(rng());
	return f;
}

static std::string
textfile(std::mt19937_64 &rng, bool hostile)
{
	std::string f;
	const int lines = static_cast<int>(rng() % 30);
	for (int l = 0; l < lines; l++) {
		char row[96];
		const char *sep = rng() % 3 == 0 ? "," : rng() & 1 ? "\t" : "  ";
		switch (rng() % 8) {
		case 0: f += "\n"; break;
		case 1: f += "> next\n"; break;
		case 2: f += "# note\n"; break;
		default:
			snprintf(row, sizeof row, "%.4f%s%.4f%s\n", static_cast<double>(rng() % 720000) / 1000.0 - 360.0, sep, static_cast<double>(rng() % 180000) / 1000.0 - 90.0,
			         rng() % 5 == 0 ? " # here" : "");
			f += row;
		}
		if (hostile && rng() % 12 == 0) {
			static const char *junk[6] = { "nan 5\n", "5\n", "1 2 3\n", "12 91\n", "abc def\n", "-400 0\n" };
			f += junk[rng() % 6];
		}
	}
	if (hostile && rng() % 4 == 0 && !f.empty()) f[rng() % f.size()] = static_cast<char>(rng() % 5 == 0 ? 0 : rng());
	if (hostile && rng() % 6 == 0) f.resize(rng() % (f.size() + 1));
	return f;
}

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 100;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	const std::string dir = argc > 3 ? argv[3] : ".";
	long refused = 0, accepted = 0, banded = 0, cut_cases = 0, pieces_total = 0, wild = 0, drawn = 0, shp = 0, txt = 0;
	for (long i = 0; i < cases; i++) {
		/* ---- a vector file ---- */
		const bool hostile = rng() % 3 != 0, binary = rng() & 1;
		const std::string bytes = binary ? shapefile(rng, hostile) : textfile(rng, hostile);
		const std::string path = dir + "/fuzz_overlay_" + std::to_string(i) + (binary ? ".shp" : ".txt");
		FILE *f = fopen(path.c_str(), "wb");
		if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) { fprintf(stderr, "could not write %s\n", path.c_str()); return 2; }
		fclose(f);
		mdemod_overlay_vectors v;
		int rc = mdemod_overlay_read(path.c_str(), &v);
		const int read_rc = rc;
		remove(path.c_str());
		if (rc != MDEMOD_OK) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error() || v.lon || v.lat || v.first || v.n_points) FAIL("case %ld: a refused file gave rc %d, text '%s'", i, rc, mdemod_last_error());
			if (!hostile) FAIL("case %ld: a well-formed file was refused: %s", i, mdemod_last_error());
			refused++;
		} else {
			bool fine = v.first && v.first[0] == 0 && v.first[v.n_lines] == v.n_points;
			for (uint32_t l = 0; fine && l < v.n_lines; l++) fine = v.first[l] < v.first[l + 1];
			for (uint32_t k = 0; fine && k < v.n_points; k++) fine = std::isfinite(v.lon[k]) && std::fabs(v.lon[k]) <= 360.0 && std::fabs(v.lat[k]) <= 90.0;
			if (!fine) FAIL("case %ld: an accepted file breaks the rules (%u lines, %u points)", i, v.n_lines, v.n_points);
			accepted++;
			if (binary) shp++; else txt++;
		}
		/* ---- any int32 vertices through the cut, the bins and the model ---- */
		const uint32_t W = 4 * (1 + static_cast<uint32_t>(rng() % 17)), H = 1 + static_cast<uint32_t>(rng() % 40), planes = rng() & 1 ? 3 : 1;
		const uint32_t n_styles = 1 + static_cast<uint32_t>(rng() % 4);
		auto styles = exact<mdemod_overlay_style>(n_styles);
		bool need_valid = false;
		for (uint32_t s = 0; s < n_styles; s++) {
			styles[s].half_width = rng() % 4 == 0 ? 2048 : static_cast<uint32_t>(rng() % 600);
			styles[s].opacity = static_cast<uint32_t>(rng() % 257);
			for (int p = 0; p < 3; p++) styles[s].colour[p] = static_cast<uint8_t>(rng());
			styles[s].inside_only = rng() % 4 == 0;
			need_valid = need_valid || styles[s].inside_only;
		}
		const bool any_int = rng() % 3 == 0;
		wild += any_int;
		mdemod_overlay_pieces pcs;
		memset(&pcs, 0, sizeof pcs);
		for (uint32_t s = 0; s < n_styles; s++) {
			const uint32_t lines = 1 + static_cast<uint32_t>(rng() % 3);
			std::vector<uint32_t> first{ 0 };
			std::vector<int32_t> xs, ys;
			for (uint32_t l = 0; l < lines; l++) {
				const uint32_t n = static_cast<uint32_t>(rng() % 6);
				for (uint32_t k = 0; k < n; k++) {
					const bool far = any_int && rng() % 3 == 0;
					xs.push_back(far ? static_cast<int32_t>(rng()) : static_cast<int32_t>(rng() % (256 * W + 8000)) - 4000);
					ys.push_back(far ? static_cast<int32_t>(rng()) : static_cast<int32_t>(rng() % (256 * H + 8000)) - 4000);
				}
				first.push_back(static_cast<uint32_t>(xs.size()));
			}
			auto px = exact<int32_t>(xs.size()), py = exact<int32_t>(ys.size());
			auto pf = exact<uint32_t>(first.size());
			if (!xs.empty()) { memcpy(px.get(), xs.data(), xs.size() * 4); memcpy(py.get(), ys.data(), ys.size() * 4); }
			memcpy(pf.get(), first.data(), first.size() * 4);
			const mdemod_overlay_points pts = { px.get(), py.get(), pf.get(), lines, static_cast<uint32_t>(xs.size()) };
			if ((rc = mdemod_overlay_cut(&pts, s, styles[s].half_width, W, H, &pcs)) != MDEMOD_OK) FAIL("case %ld: the cut refused: %s", i, mdemod_last_error());
		}
		cut_cases++;
		pieces_total += static_cast<long>(pcs.n);
		auto held = exact<mdemod_overlay_piece>(pcs.n);
		if (pcs.n) memcpy(held.get(), pcs.piece, pcs.n * sizeof(mdemod_overlay_piece));
		for (uint64_t k = 0; k < pcs.n; k++)
			if (held[k].L < 1 || held[k].L > 23171 || std::abs(held[k].ax) > MDEMOD_OVERLAY_VERTEX_TOP || std::abs(held[k].ay) > MDEMOD_OVERLAY_VERTEX_TOP)
				{ FAIL("case %ld: piece %llu has length %d at %d %d", i, static_cast<unsigned long long>(k), held[k].L, held[k].ax, held[k].ay); break; }
		const uint64_t n_pieces = pcs.n;
		mdemod_overlay_pieces_free(&pcs);
		mdemod_overlay_bins bins;
		if ((rc = mdemod_overlay_bin(held.get(), n_pieces, styles.get(), n_styles, W, H, &bins)) != MDEMOD_OK) { FAIL("case %ld: the bins refused: %s", i, mdemod_last_error()); continue; }
		const size_t tiles = static_cast<size_t>(bins.tiles_x) * bins.tiles_y, area = static_cast<size_t>(W) * H;
		auto tf = exact<uint32_t>(tiles + 1);
		auto it = exact<uint32_t>(bins.n_items);
		memcpy(tf.get(), bins.tile_first, (tiles + 1) * 4);
		if (bins.n_items) memcpy(it.get(), bins.items, bins.n_items * 4);
		const uint64_t n_items = bins.n_items;
		if (bins.tiles_x != overlay_tiles(W) || bins.tiles_y != overlay_tiles(H) || tf[0] != 0 || tf[tiles] != n_items) FAIL("case %ld: the bins are %u x %u with %llu items", i, bins.tiles_x, bins.tiles_y, static_cast<unsigned long long>(n_items));
		for (uint64_t k = 0; k < n_items; k++) if (it[k] >= n_pieces) { FAIL("case %ld: item %llu is no piece", i, static_cast<unsigned long long>(k)); break; }
		mdemod_overlay_bins_free(&bins);
		auto start = exact<uint8_t>(area * planes), one = exact<uint8_t>(area * planes), two = exact<uint8_t>(area * planes);
		auto valid = exact<uint8_t>(area), m1 = exact<uint8_t>(area), m2 = exact<uint8_t>(area);
		for (size_t b = 0; b < area * planes; b++) start[b] = static_cast<uint8_t>(rng());
		for (size_t b = 0; b < area; b++) valid[b] = static_cast<uint8_t>(rng() % 3 ? rng() | 1 : 0);
		memcpy(one.get(), start.get(), area * planes);
		memcpy(two.get(), start.get(), area * planes);
		const uint8_t *val = need_valid || rng() & 1 ? valid.get() : nullptr;
		const bool with_mask = rng() % 4 != 0;
		if (mdemod_overlay_model_draw(held.get(), n_pieces, styles.get(), n_styles, W, H, planes, one.get(), val, m1.get()) != MDEMOD_OK ||
		    mdemod_overlay_model_tiles(held.get(), n_pieces, tf.get(), it.get(), n_items, styles.get(), n_styles, W, H, planes, two.get(), val, with_mask ? m2.get() : nullptr) != MDEMOD_OK)
			FAIL("case %ld: the model refused: %s", i, mdemod_last_error());
		else {
			if (memcmp(one.get(), two.get(), area * planes) || (with_mask && memcmp(m1.get(), m2.get(), area))) FAIL("case %ld: the bins change the picture (%u x %u, %llu pieces)", i, W, H, static_cast<unsigned long long>(n_pieces));
			for (size_t b = 0; b < area; b++) {
				if (m1[b] >> n_styles) { FAIL("case %ld: mask[%zu] = %u with %u styles", i, b, m1[b], n_styles); break; }
				if (!m1[b] && memcmp(one.get() + b * planes, start.get() + b * planes, planes)) { FAIL("case %ld: pixel %zu changed without a bit of the mask", i, b); break; }
				drawn += m1[b] != 0;
			}
		}
		const mdemod_overlay_style wide = { 2049, 256, { 0, 0, 0 }, 0 }, thick = { 128, 257, { 0, 0, 0 }, 0 };
		if (mdemod_overlay_model_draw(held.get(), n_pieces, styles.get(), 5, W, H, planes, one.get(), val, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_overlay_model_draw(held.get(), n_pieces, &wide, 1, W, H, planes, one.get(), val, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_overlay_model_draw(held.get(), n_pieces, &thick, 1, W, H, planes, one.get(), val, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_overlay_model_draw(held.get(), n_pieces, styles.get(), n_styles, W + 2, H, planes, one.get(), val, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_overlay_model_draw(held.get(), n_pieces, styles.get(), n_styles, W, 16385, planes, one.get(), val, nullptr) != MDEMOD_ERR_PARAM ||
		    mdemod_overlay_model_draw(held.get(), n_pieces, styles.get(), n_styles, W, H, 2, one.get(), val, nullptr) != MDEMOD_ERR_PARAM)
			FAIL("case %ld: an argument out of range was accepted", i);
		/* ---- degrees through the whole-picture entry's model path: the bands equal one batch ---- */
		mdemod_overlay_geo geo;
		memset(&geo, 0, sizeof geo);
		geo.width = 4 * (1 + static_cast<uint32_t>(rng() % 20)); geo.height = 1 + static_cast<uint32_t>(rng() % 150);
		geo.sx = 1 + static_cast<uint32_t>(rng() % 6); geo.sy = 0.5 + static_cast<double>(rng() % 60) / 10.0;
		geo.lat_top = static_cast<double>(rng() % 1600) / 10.0 - 70.0; geo.lon_left = static_cast<double>(rng() % 3600) / 10.0 - 180.0;
		const uint32_t n_pts = 2 + static_cast<uint32_t>(rng() % 12);
		auto lon = exact<double>(n_pts), lat = exact<double>(n_pts);
		auto lf = exact<uint32_t>(3);
		for (uint32_t k = 0; k < n_pts; k++) {
			lon[k] = geo.lon_left + static_cast<double>(rng() % 1000) / 1000.0 * geo.width / geo.sx;
			lon[k] -= 360.0 * std::floor((lon[k] + 180.0) / 360.0);
			lat[k] = geo.lat_top - static_cast<double>(rng() % 1000) / 1000.0 * geo.height / geo.sy;
			lat[k] = lat[k] > 90.0 ? 90.0 : lat[k] < -90.0 ? -90.0 : lat[k];
		}
		lf[0] = 0; lf[1] = static_cast<uint32_t>(rng() % (n_pts + 1)); lf[2] = n_pts;
		mdemod_overlay_vectors coast = { lon.get(), lat.get(), lf.get(), 2, n_pts, 0, 0 }, grat;
		if (mdemod_overlay_graticule(&geo, rng() & 1 ? 0.0 : 1.0 + static_cast<double>(rng() % 30), &grat) != MDEMOD_OK) { FAIL("case %ld: the graticule refused: %s", i, mdemod_last_error()); continue; }
		const mdemod_overlay_layer layers[2] = { { &coast, static_cast<uint32_t>(rng() % n_styles), 0 }, { &grat, static_cast<uint32_t>(rng() % n_styles), 0 } };
		const size_t g_area = static_cast<size_t>(geo.width) * geo.height;
		auto g_start = exact<uint8_t>(g_area * planes), g_one = exact<uint8_t>(g_area * planes), g_two = exact<uint8_t>(g_area * planes);
		auto g_valid = exact<uint8_t>(g_area), g_m1 = exact<uint8_t>(g_area), g_m2 = exact<uint8_t>(g_area);
		for (size_t b = 0; b < g_area * planes; b++) g_start[b] = static_cast<uint8_t>(rng());
		for (size_t b = 0; b < g_area; b++) g_valid[b] = static_cast<uint8_t>(rng() & 1);
		memcpy(g_one.get(), g_start.get(), g_area * planes);
		memcpy(g_two.get(), g_start.get(), g_area * planes);
		const uint32_t piece = 32 * (1 + static_cast<uint32_t>(rng() % 3));
		mdemod_overlay_report r1, r2;
		if (mdemod_overlay_model_host(&geo, layers, 2, styles.get(), n_styles, planes, g_one.get(), g_valid.get(), g_m1.get(), piece, &r1) != MDEMOD_OK ||
		    mdemod_overlay_model_host(&geo, layers, 2, styles.get(), n_styles, planes, g_two.get(), g_valid.get(), rng() & 1 ? g_m2.get() : nullptr, 16384, &r2) != MDEMOD_OK)
			FAIL("case %ld: the host entry refused: %s", i, mdemod_last_error());
		else if (memcmp(g_one.get(), g_two.get(), g_area * planes) || memcmp(&r1, &r2, sizeof r1)) FAIL("case %ld: bands of %u lines change the picture", i, piece);
		else banded++;
		if (mdemod_overlay_model_host(&geo, layers, 2, styles.get(), n_styles, planes, g_one.get(), g_valid.get(), nullptr, 40, nullptr) != MDEMOD_ERR_PARAM || !*mdemod_last_error())
			FAIL("case %ld: bands of 40 lines were accepted", i);
		mdemod_overlay_vectors_free(&grat);
		if (read_rc == MDEMOD_OK) mdemod_overlay_vectors_free(&v);
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"refused\": %ld, \"accepted\": %ld, \"shp\": %ld, \"txt\": %ld, \"banded\": %ld, \"cut\": %ld, \"pieces\": %ld, \"wild\": %ld, "
	       "\"drawn\": %ld, \"bad\": %ld}\n", bad ? "false" : "true", cases, refused, accepted, shp, txt, banded, cut_cases, pieces_total, wild, drawn, bad);
	return bad ? 1 : 0;
}
