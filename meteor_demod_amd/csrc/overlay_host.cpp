/*
 * overlay_host.cpp — host side of the overlay layer (include/meteor_demod_amd_overlay.h): the readers of vector files, the
 * graticule, the projection to fixed point, the pieces with their culling, the bins, the bands of the whole-picture entry, and the
 * host model of the kernel of csrc/overlay.hip (mdemod_overlay_model_*: the rule as plain loops in 64-bit integers).  Free of the
 * GPU runtime.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "overlay_host.h"
#include "mdemod_internal_api.h"

namespace {

constexpr int64_t VERTEX_TOP = MDEMOD_OVERLAY_VERTEX_TOP;
constexpr size_t  FILE_TOP = static_cast<size_t>(1) << 30;                     /* no vector file is read beyond 1 GiB */
constexpr uint64_t COUNT_TOP = 1ull << 31;                                     /* vertices, pieces, items */

int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }
int64_t abs64(int64_t v) { return v < 0 ? -v : v; }

uint64_t
isqrt64(uint64_t v)
{
	uint64_t r = static_cast<uint64_t>(std::sqrt(static_cast<double>(v)));
	while (r * r > v) r--;
	while ((r + 1) * (r + 1) <= v) r++;
	return r;
}

/* ---------------------------------------------------------------------------------------------------------------- vectors */
struct Lines {
	std::vector<double> lon, lat;
	std::vector<uint32_t> first{ 0 };
	uint32_t skipped = 0;
	void end_line() { if (first.back() != lon.size()) first.push_back(static_cast<uint32_t>(lon.size())); }
};

int
give_out(Lines &l, mdemod_overlay_vectors *v)
{
	l.end_line();
	const size_t n = l.lon.size(), lines = l.first.size() - 1;
	v->lon = static_cast<double *>(malloc((n ? n : 1) * sizeof(double)));
	v->lat = static_cast<double *>(malloc((n ? n : 1) * sizeof(double)));
	v->first = static_cast<uint32_t *>(malloc((lines + 1) * sizeof(uint32_t)));
	if (!v->lon || !v->lat || !v->first) { mdemod_overlay_vectors_free(v); return MDEMOD_ERR_NOMEM; }
	if (n) { memcpy(v->lon, l.lon.data(), n * sizeof(double)); memcpy(v->lat, l.lat.data(), n * sizeof(double)); }
	memcpy(v->first, l.first.data(), (lines + 1) * sizeof(uint32_t));
	v->n_lines = static_cast<uint32_t>(lines); v->n_points = static_cast<uint32_t>(n); v->skipped = l.skipped;
	return MDEMOD_OK;
}

int
check_coordinate(const char *where, uint64_t at, double lon, double lat)
{
	if (!std::isfinite(lon) || !std::isfinite(lat)) REFUSE("overlay: %s %llu: a coordinate is not finite", where, static_cast<unsigned long long>(at));
	if (std::fabs(lat) > 90.0) REFUSE("overlay: %s %llu: latitude %g is beyond 90 degrees", where, static_cast<unsigned long long>(at), lat);
	if (std::fabs(lon) > 360.0) REFUSE("overlay: %s %llu: longitude %g is beyond 360 degrees", where, static_cast<unsigned long long>(at), lon);
	return MDEMOD_OK;
}

uint32_t be32(const uint8_t *p) { return static_cast<uint32_t>(p[0]) << 24 | static_cast<uint32_t>(p[1]) << 16 | static_cast<uint32_t>(p[2]) << 8 | p[3]; }
uint32_t le32(const uint8_t *p) { return static_cast<uint32_t>(p[3]) << 24 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[1]) << 8 | p[0]; }
double
le_double(const uint8_t *p)
{
	uint64_t w = 0;
	for (int k = 7; k >= 0; k--) w = w << 8 | p[k];
	double d;
	memcpy(&d, &w, sizeof d);
	return d;
}

int
read_shapefile(const uint8_t *b, size_t size, Lines &out)
{
	if (size < 100) REFUSE("overlay: a shapefile of %zu bytes has no header (100 bytes)", size);
	if (be32(b) != 9994) REFUSE("overlay: the file code is %u: neither text nor a shapefile (9994)", be32(b));
	if (le32(b + 28) != 1000) REFUSE("overlay: shapefile version %u (1000 is read)", le32(b + 28));
	const uint64_t said = 2ull * be32(b + 24);
	if (said < 100 || said > size) REFUSE("overlay: the header says %llu bytes, the file has %zu: a record runs past the file", static_cast<unsigned long long>(said), size);
	size_t at = 100;
	uint64_t rec = 0;
	while (at < said) {
		rec++;
		if (said - at < 8) REFUSE("overlay: record %llu: its header runs past the file", static_cast<unsigned long long>(rec));
		const uint64_t len = 2ull * be32(b + at + 4);
		at += 8;
		if (len > said - at) REFUSE("overlay: record %llu: %llu bytes of content run past the file", static_cast<unsigned long long>(rec), static_cast<unsigned long long>(len));
		const uint8_t *c = b + at;
		at += len;
		if (len < 4) REFUSE("overlay: record %llu: no shape type within its content length", static_cast<unsigned long long>(rec));
		const uint32_t type = le32(c);
		if (type == 0 || type == 1 || type == 8 || type == 11 || type == 18 || type == 21 || type == 28 || type == 31) { out.skipped++; continue; }
		if (!(type == 3 || type == 5 || type == 13 || type == 15 || type == 23 || type == 25))
			REFUSE("overlay: record %llu: shape type %u is not known", static_cast<unsigned long long>(rec), type);
		if (len < 44) REFUSE("overlay: record %llu: the counts run past its own content length", static_cast<unsigned long long>(rec));
		const uint64_t parts = le32(c + 36), points = le32(c + 40);
		if (parts > len || points > len || 44 + 4 * parts + 16 * points > len)
			REFUSE("overlay: record %llu: %llu parts and %llu points run past its own content length of %llu bytes", static_cast<unsigned long long>(rec),
			       static_cast<unsigned long long>(parts), static_cast<unsigned long long>(points), static_cast<unsigned long long>(len));
		if (out.lon.size() + points >= COUNT_TOP) REFUSE("overlay: more than 2^31 vertices");
		const uint8_t *pi = c + 44, *pt = pi + 4 * parts;
		for (uint64_t p = 0; p < parts; p++) {
			const uint64_t from = le32(pi + 4 * p), to = p + 1 < parts ? le32(pi + 4 * (p + 1)) : points;
			if (from >= points || (p + 1 < parts && to <= from))
				REFUSE("overlay: record %llu: part %llu begins at point %llu: the parts must ascend inside the %llu points", static_cast<unsigned long long>(rec),
				       static_cast<unsigned long long>(p), static_cast<unsigned long long>(from), static_cast<unsigned long long>(points));
			if (to > points) REFUSE("overlay: record %llu: part %llu begins at point %llu: the parts must ascend inside the %llu points", static_cast<unsigned long long>(rec),
			                        static_cast<unsigned long long>(p + 1), static_cast<unsigned long long>(to), static_cast<unsigned long long>(points));
			for (uint64_t q = from; q < to; q++) {
				const double lon = le_double(pt + 16 * q), lat = le_double(pt + 16 * q + 8);
				const int rc = check_coordinate("record", rec, lon, lat);
				if (rc) return rc;
				out.lon.push_back(lon);
				out.lat.push_back(lat);
			}
			out.end_line();
		}
	}
	return MDEMOD_OK;
}

int
read_text(const uint8_t *b, size_t size, Lines &out)
{
	size_t at = 0;
	uint64_t line = 0;
	while (at < size) {
		size_t end = at;
		while (end < size && b[end] != '\n') end++;
		line++;
		std::string s(reinterpret_cast<const char *>(b) + at, end - at);
		at = end + 1;
		const size_t hash = s.find('#');
		const bool had_comment = hash != std::string::npos;
		if (had_comment) s.erase(hash);
		for (char &ch : s) if (ch == ',' || ch == '\t' || ch == '\r') ch = ' ';
		const size_t a = s.find_first_not_of(' ');
		if (a == std::string::npos) { if (!had_comment) out.end_line(); continue; }          /* (a comment alone ends nothing) */
		if (s[a] == '>') { out.end_line(); continue; }
		if (s.find('\0') != std::string::npos) REFUSE("overlay: line %llu: not two numbers", static_cast<unsigned long long>(line));
		const char *p = s.c_str() + a;
		char *e1 = nullptr, *e2 = nullptr;
		const double lon = strtod(p, &e1);
		if (e1 == p || *e1 != ' ') REFUSE("overlay: line %llu: not two numbers", static_cast<unsigned long long>(line));
		const double lat = strtod(e1, &e2);
		if (e2 == e1) REFUSE("overlay: line %llu: not two numbers", static_cast<unsigned long long>(line));
		while (*e2 == ' ') e2++;
		if (*e2) REFUSE("overlay: line %llu: not two numbers", static_cast<unsigned long long>(line));
		const int rc = check_coordinate("line", line, lon, lat);
		if (rc) return rc;
		if (out.lon.size() + 1 >= COUNT_TOP) REFUSE("overlay: more than 2^31 vertices");
		out.lon.push_back(lon);
		out.lat.push_back(lat);
	}
	return MDEMOD_OK;
}

bool
is_text_byte(uint8_t c)
{
	return c == '\t' || c == '\n' || c == '\r' || (c >= 32 && c < 127);
}

/* ------------------------------------------------------------------------------------------------------------- projection */
int
check_geo(const char *who, const mdemod_overlay_geo *g)
{
	if (!g) REFUSE("%s: the grid is needed", who);
	if (!g->width || g->width > MDEMOD_OVERLAY_MAX_WIDTH || !g->height || g->height > MDEMOD_OVERLAY_MAX_HEIGHT)
		REFUSE("%s: a picture of %u x %u (1 .. 8192 x 1 .. 16384)", who, g->width, g->height);
	if (!g->sx || g->sx > 100000 || !(g->sy > 0.0) || !(g->sy <= 100000.0)) REFUSE("%s: a scale of %u x %g pixels per degree", who, g->sx, g->sy);
	if (!std::isfinite(g->lat_top) || !std::isfinite(g->lon_left) || std::fabs(g->lat_top) > 1000.0 || std::fabs(g->lon_left) > 1000.0)
		REFUSE("%s: the picture's corner stands at latitude %g, longitude %g", who, g->lat_top, g->lon_left);
	return MDEMOD_OK;
}

double wrap180(double a) { return a - 360.0 * std::floor((a + 180.0) / 360.0); }

int64_t
to_fixed(double v)
{
	const double f = std::floor(v + 0.5);
	return f >= 2147483647.0 ? 2147483647 : f <= -2147483647.0 ? -2147483647 : static_cast<int64_t>(f);
}

int32_t saturate(int64_t v) { return v > 2147483647 ? 2147483647 : v < -2147483647 ? -2147483647 : static_cast<int32_t>(v); }

/* ----------------------------------------------------------------------------------------------------------------- pieces */
/* the part t0 .. t1 of A + t D, 0 <= t <= 1, inside the rectangle; false: none */
bool
clip(double ax, double ay, double dx, double dy, double x0, double x1, double y0, double y1, double &t0, double &t1)
{
	t0 = 0.0; t1 = 1.0;
	const double p[4] = { -dx, dx, -dy, dy }, q[4] = { ax - x0, x1 - ax, ay - y0, y1 - ay };
	for (int k = 0; k < 4; k++) {
		if (p[k] == 0.0) { if (q[k] < 0.0) return false; continue; }
		const double r = q[k] / p[k];
		if (p[k] < 0.0) { if (r > t1) return false; if (r > t0) t0 = r; }
		else { if (r < t0) return false; if (r < t1) t1 = r; }
	}
	return t0 <= t1;
}

int
push_piece(mdemod_overlay_pieces *out, const mdemod_overlay_piece &p)
{
	if (out->n == out->room) {
		const uint64_t room = out->room ? 2 * out->room : 1024;
		if (room >= COUNT_TOP) REFUSE("overlay: more than 2^30 pieces");
		void *grown = realloc(out->piece, room * sizeof(mdemod_overlay_piece));
		if (!grown) return MDEMOD_ERR_NOMEM;
		out->piece = static_cast<mdemod_overlay_piece *>(grown);
		out->room = room;
	}
	out->piece[out->n++] = p;
	return MDEMOD_OK;
}

mdemod_overlay_piece
make_piece(int64_t ax, int64_t ay, int64_t dx, int64_t dy, uint32_t style)
{
	const int64_t l16 = static_cast<int64_t>(isqrt64(256ull * static_cast<uint64_t>(dx * dx + dy * dy)));
	mdemod_overlay_piece p;
	memset(&p, 0, sizeof p);
	p.ax = static_cast<int32_t>(ax); p.ay = static_cast<int32_t>(ay);
	p.tx = static_cast<int32_t>(floor_div(524288 * dx + l16, 2 * l16));
	p.ty = static_cast<int32_t>(floor_div(524288 * dy + l16, 2 * l16));
	p.L = static_cast<int32_t>((l16 + 8) >> 4);
	p.style = static_cast<int32_t>(style);
	return p;
}

/* the pieces of A -> B that can reach the rectangle 0 .. x_top x 0 .. y_top of pixel centres within `reach` */
int
cut_segment(int64_t ax, int64_t ay, int64_t bx, int64_t by, uint32_t style, int64_t reach, int64_t x_top, int64_t y_top, mdemod_overlay_pieces *out)
{
	const int64_t dx = bx - ax, dy = by - ay, longest = abs64(dx) > abs64(dy) ? abs64(dx) : abs64(dy);
	if (!longest) return MDEMOD_OK;
	const int64_t k = (longest + OVERLAY_PIECE_TOP - 1) / OVERLAY_PIECE_TOP;
	const int64_t x0 = -reach, x1 = x_top + reach, y0 = -reach, y1 = y_top + reach;
	if ((ax < x0 && bx < x0) || (ax > x1 && bx > x1) || (ay < y0 && by < y0) || (ay > y1 && by > y1)) return MDEMOD_OK;
	double t0, t1;
	if (!clip(static_cast<double>(ax), static_cast<double>(ay), static_cast<double>(dx), static_cast<double>(dy), static_cast<double>(x0 - 2), static_cast<double>(x1 + 2),
	          static_cast<double>(y0 - 2), static_cast<double>(y1 + 2), t0, t1))
		return MDEMOD_OK;
	int64_t m = static_cast<int64_t>(std::floor(t0 * static_cast<double>(k))) - 1, m_end = static_cast<int64_t>(std::ceil(t1 * static_cast<double>(k))) + 1;
	m = m < 0 ? 0 : m;
	m_end = m_end > k ? k : m_end;
	int64_t px = ax + floor_div(2 * m * dx + k, 2 * k), py = ay + floor_div(2 * m * dy + k, 2 * k);
	for (; m < m_end; m++) {
		const int64_t qx = ax + floor_div(2 * (m + 1) * dx + k, 2 * k), qy = ay + floor_div(2 * (m + 1) * dy + k, 2 * k);
		const int64_t ex = qx - px, ey = qy - py, fx = px, fy = py;
		px = qx; py = qy;
		if (!ex && !ey) continue;
		double u0, u1;
		if (!clip(static_cast<double>(fx), static_cast<double>(fy), static_cast<double>(ex), static_cast<double>(ey), static_cast<double>(x0 - 2), static_cast<double>(x1 + 2),
		          static_cast<double>(y0 - 2), static_cast<double>(y1 + 2), u0, u1))
			continue;
		const int rc = push_piece(out, make_piece(fx, fy, ex, ey, style));
		if (rc) return rc;
	}
	return MDEMOD_OK;
}

int
check_styles(const char *who, const mdemod_overlay_style *styles, uint32_t n_styles)
{
	if (!n_styles || n_styles > OVERLAY_MAX_STYLES) REFUSE("%s: %u styles (1 .. 4)", who, n_styles);
	if (!styles) REFUSE("%s: the styles are needed", who);
	for (uint32_t s = 0; s < n_styles; s++) {
		if (styles[s].half_width > MDEMOD_OVERLAY_MAX_HALF) REFUSE("%s: the half width of style %u is %u (0 .. 2048, in 1/256 pixel)", who, s, styles[s].half_width);
		if (styles[s].opacity > 256) REFUSE("%s: the opacity of style %u is %u (0 .. 256)", who, s, styles[s].opacity);
	}
	return MDEMOD_OK;
}

/* what mdemod_overlay_cut makes, which is what the kernel's 32-bit arithmetic counts on: a length of at most 16384 per axis and a
 * tangent of about 16384 */
int
check_pieces(const char *who, const mdemod_overlay_piece *pieces, uint64_t n, uint32_t n_styles)
{
	if (n && !pieces) REFUSE("%s: the pieces are needed", who);
	if (n >= COUNT_TOP) REFUSE("%s: more than 2^31 pieces", who);
	for (uint64_t k = 0; k < n; k++) {
		const mdemod_overlay_piece &p = pieces[k];
		if (p.style < 0 || static_cast<uint32_t>(p.style) >= n_styles) REFUSE("%s: piece %llu has style %d of %u", who, static_cast<unsigned long long>(k), p.style, n_styles);
		if (p.L < 0 || p.L > 23172 || abs64(p.tx) > 17500 || abs64(p.ty) > 17500)
			REFUSE("%s: piece %llu is none that mdemod_overlay_cut makes (length %d, tangent %d %d)", who, static_cast<unsigned long long>(k), p.L, p.tx, p.ty);
	}
	return MDEMOD_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ model */
int64_t
coverage(const mdemod_overlay_piece &p, int64_t px, int64_t py, int64_t w128)
{
	const int64_t dx = px - p.ax, dy = py - p.ay;
	const int64_t along = (static_cast<int64_t>(p.tx) * dx + static_cast<int64_t>(p.ty) * dy) >> 14;
	const int64_t perp = abs64(static_cast<int64_t>(p.tx) * dy - static_cast<int64_t>(p.ty) * dx) >> 14;
	int64_t d = perp > -along ? perp : -along;
	d = along - p.L > d ? along - p.L : d;
	d = d < 0 ? 0 : d;
	const int64_t a = w128 - d;
	return a < 0 ? 0 : a > 256 ? 256 : a;
}

void
blend_pixel(const int64_t *A, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t planes, uint8_t *px, bool inside, uint8_t *mask)
{
	uint8_t bits = 0;
	for (uint32_t s = 0; s < n_styles; s++) {
		const int64_t a = styles[s].inside_only && !inside ? 0 : A[s];
		if (a <= 0) continue;
		bits |= static_cast<uint8_t>(1u << s);
		const int64_t o = (a * styles[s].opacity + 128) >> 8;
		for (uint32_t p = 0; p < planes; p++) px[p] = static_cast<uint8_t>((px[p] * (256 - o) + styles[s].colour[p] * o + 128) >> 8);
	}
	if (mask) *mask = bits;
}

void
model_all(const mdemod_overlay_piece *pieces, uint64_t n, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes,
          uint8_t *pixels, const uint8_t *valid, uint8_t *mask)
{
	for (uint32_t i = 0; i < height; i++)
		for (uint32_t j = 0; j < width; j++) {
			int64_t A[OVERLAY_MAX_STYLES] = { 0, 0, 0, 0 };
			for (uint64_t k = 0; k < n; k++) {
				const uint32_t s = static_cast<uint32_t>(pieces[k].style);
				if (s >= n_styles) continue;
				const int64_t a = coverage(pieces[k], 256ll * j, 256ll * i, styles[s].half_width + 128ll);
				A[s] = a > A[s] ? a : A[s];
			}
			const size_t at = static_cast<size_t>(i) * width + j;
			blend_pixel(A, styles, n_styles, planes, pixels + at * planes, !valid || valid[at], mask ? mask + at : nullptr);
		}
}

/* the kernel's arguments: `height` lines whose first is line 32 tile_row of the picture the bins were made for */
void
model_tiles(const mdemod_overlay_piece *pieces, uint64_t n, const uint32_t *tile_first, const uint32_t *items, uint64_t n_items, const mdemod_overlay_style *styles,
            uint32_t n_styles, uint32_t width, uint32_t tile_row, uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask)
{
	const uint32_t tiles_x = overlay_tiles(width);
	if (mask) memset(mask, 0, static_cast<size_t>(height) * width);
	for (uint32_t ty = 0; ty < overlay_tiles(height); ty++)
		for (uint32_t tx = 0; tx < tiles_x; tx++) {
			const size_t tile = static_cast<size_t>(tile_row + ty) * tiles_x + tx;
			uint64_t from = tile_first[tile], to = tile_first[tile + 1];
			to = to > n_items ? n_items : to;
			if (from >= to) continue;
			for (uint32_t i = OVERLAY_TILE * ty; i < OVERLAY_TILE * (ty + 1) && i < height; i++)
				for (uint32_t j = OVERLAY_TILE * tx; j < OVERLAY_TILE * (tx + 1) && j < width; j++) {
					int64_t A[OVERLAY_MAX_STYLES] = { 0, 0, 0, 0 };
					for (uint64_t k = from; k < to; k++) {
						if (items[k] >= n) continue;
						const mdemod_overlay_piece &p = pieces[items[k]];
						const uint32_t s = static_cast<uint32_t>(p.style);
						if (s >= n_styles) continue;
						const int64_t a = coverage(p, 256ll * j, 256ll * (OVERLAY_TILE * static_cast<int64_t>(tile_row) + i), styles[s].half_width + 128ll);
						A[s] = a > A[s] ? a : A[s];
					}
					const size_t at = static_cast<size_t>(i) * width + j;
					blend_pixel(A, styles, n_styles, planes, pixels + at * planes, !valid || valid[at], mask ? mask + at : nullptr);
				}
		}
}

struct ModelBackend : OverlayBackend {
	const mdemod_overlay_pieces *pieces = nullptr;
	const mdemod_overlay_bins *bins = nullptr;
	const mdemod_overlay_style *styles = nullptr;
	uint32_t n_styles = 0, width = 0, planes = 0;
	int begin(const mdemod_overlay_pieces &p, const mdemod_overlay_bins &b, const mdemod_overlay_style *st, uint32_t ns, uint32_t w, uint32_t pl, uint32_t, bool, bool) override
	{
		pieces = &p; bins = &b; styles = st; n_styles = ns; width = w; planes = pl;
		return MDEMOD_OK;
	}
	int band(uint32_t tile_row, uint32_t height, uint8_t *pixels, const uint8_t *valid, uint8_t *mask) override
	{
		model_tiles(pieces->piece, pieces->n, bins->tile_first, bins->items, bins->n_items, styles, n_styles, width, tile_row, height, planes, pixels, valid, mask);
		return MDEMOD_OK;
	}
};

} /* namespace */

int
overlay_check_draw(const char *who, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes, const void *pixels,
                   const void *valid)
{
	const int rc = check_styles(who, styles, n_styles);
	if (rc) return rc;
	if (planes != 1 && planes != 3) REFUSE("%s: %u planes (1: grey, 3: colour)", who, planes);
	if (width < 4 || width > MDEMOD_OVERLAY_MAX_WIDTH || width % 4) REFUSE("%s: a width of %u (a multiple of 4, 4 .. 8192)", who, width);
	if (height > MDEMOD_OVERLAY_MAX_HEIGHT) REFUSE("%s: a height of %u (at most 16384)", who, height);
	if (height && !pixels) REFUSE("%s: the picture is needed", who);
	for (uint32_t s = 0; s < n_styles; s++)
		if (styles[s].inside_only && height && !valid) REFUSE("%s: style %u is inside_only: valid is needed", who, s);
	return MDEMOD_OK;
}

int
overlay_draw_bands(const char *who, const mdemod_overlay_geo *geo, const mdemod_overlay_layer *layers, uint32_t n_layers, const mdemod_overlay_style *styles,
                   uint32_t n_styles, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines, mdemod_overlay_report *report,
                   OverlayBackend &backend)
{
	if (report) memset(report, 0, sizeof *report);
	int rc = check_geo(who, geo);
	if (rc) return rc;
	if ((rc = overlay_check_draw(who, styles, n_styles, geo->width, geo->height, planes, pixels, valid))) return rc;
	if (piece_lines % OVERLAY_TILE) REFUSE("%s: piece_lines is %u (0, or a multiple of 32)", who, piece_lines);
	if (n_layers > 64) REFUSE("%s: %u layers (at most 64)", who, n_layers);
	if (n_layers && !layers) REFUSE("%s: the layers are needed", who);
	for (uint32_t l = 0; l < n_layers; l++) {
		if (!layers[l].vectors) REFUSE("%s: the vectors of layer %u are needed", who, l);
		if (layers[l].style >= n_styles) REFUSE("%s: layer %u has style %u of %u", who, l, layers[l].style, n_styles);
	}
	struct Points : std::vector<mdemod_overlay_points> { ~Points() { for (mdemod_overlay_points &p : *this) mdemod_overlay_points_free(&p); } } pts;
	pts.resize(n_layers);                                                      /* (zeroed: nothing to free yet) */
	std::vector<const mdemod_overlay_points *> of(n_layers);
	std::vector<uint32_t> style_of(n_layers);
	for (uint32_t l = 0; l < n_layers; l++) {
		if ((rc = mdemod_overlay_project(geo, layers[l].vectors, &pts[l]))) return rc;
		of[l] = &pts[l];
		style_of[l] = layers[l].style;
	}
	/* (the report counts pixels in the mask: one of its own where none was asked for) */
	std::vector<uint8_t> own;
	if (!mask && report) { own.resize(static_cast<size_t>(geo->height) * geo->width); mask = own.data(); }
	return overlay_draw_points(of.data(), style_of.data(), n_layers, styles, n_styles, geo->width, geo->height, planes, pixels, valid, mask, piece_lines, report, backend);
}

int
overlay_draw_points(const mdemod_overlay_points *const *layers, const uint32_t *style_of, uint32_t n_layers, const mdemod_overlay_style *styles, uint32_t n_styles,
                    uint32_t W, uint32_t H, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines, mdemod_overlay_report *report,
                    OverlayBackend &backend)
{
	int rc;
	const uint32_t P = piece_lines ? piece_lines : 1024;
	if (report) memset(report, 0, sizeof *report);
	mdemod_overlay_pieces pieces;
	mdemod_overlay_bins bins;
	memset(&pieces, 0, sizeof pieces);
	memset(&bins, 0, sizeof bins);
	struct Keep { mdemod_overlay_pieces *p; mdemod_overlay_bins *b; ~Keep() { mdemod_overlay_pieces_free(p); mdemod_overlay_bins_free(b); } } keep{ &pieces, &bins };
	for (uint32_t l = 0; l < n_layers; l++)
		if ((rc = mdemod_overlay_cut(layers[l], style_of[l], styles[style_of[l]].half_width, W, H, &pieces))) return rc;
	if ((rc = mdemod_overlay_bin(pieces.piece, pieces.n, styles, n_styles, W, H, &bins))) return rc;
	if ((rc = backend.begin(pieces, bins, styles, n_styles, W, planes, P < H ? P : overlay_tiles(H) * OVERLAY_TILE, valid != nullptr, mask != nullptr))) return rc;
	for (uint32_t at = 0; at < H; at += P)
		if ((rc = backend.band(at / OVERLAY_TILE, P < H - at ? P : H - at, pixels + static_cast<size_t>(at) * W * planes, valid ? valid + static_cast<size_t>(at) * W : nullptr,
		                       mask ? mask + static_cast<size_t>(at) * W : nullptr)))
			return rc;
	if (report) {
		for (uint64_t k = 0; k < pieces.n; k++) report->pieces[pieces.piece[k].style]++;
		for (size_t k = 0; mask && k < static_cast<size_t>(H) * W; k++)
			for (uint32_t s = 0; s < n_styles; s++) report->pixels[s] += (mask[k] >> s) & 1u;
		for (size_t t = 0; t < static_cast<size_t>(bins.tiles_x) * bins.tiles_y; t++) report->tiles += bins.tile_first[t + 1] > bins.tile_first[t];
		report->items = bins.n_items;
	}
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_overlay_vectors_free(mdemod_overlay_vectors *v)
{
	if (!v) return;
	free(v->lon); free(v->lat); free(v->first);
	memset(v, 0, sizeof *v);
}

void
mdemod_overlay_points_free(mdemod_overlay_points *p)
{
	if (!p) return;
	free(p->x); free(p->y); free(p->first);
	memset(p, 0, sizeof *p);
}

void
mdemod_overlay_pieces_free(mdemod_overlay_pieces *p)
{
	if (!p) return;
	free(p->piece);
	memset(p, 0, sizeof *p);
}

void
mdemod_overlay_bins_free(mdemod_overlay_bins *b)
{
	if (!b) return;
	free(b->tile_first); free(b->items);
	memset(b, 0, sizeof *b);
}

int
mdemod_overlay_read(const char *path, mdemod_overlay_vectors *vectors)
try { MDEMOD_API_ENTER
	if (!vectors) REFUSE("mdemod_overlay_read: the vectors are needed");
	memset(vectors, 0, sizeof *vectors);
	if (!path) REFUSE("mdemod_overlay_read: the path is needed");
	FILE *f = fopen(path, "rb");
	if (!f) REFUSE("overlay: could not open %s", path);
	std::vector<uint8_t> bytes;
	uint8_t block[65536];
	size_t got;
	while ((got = fread(block, 1, sizeof block, f)) > 0) {
		if (bytes.size() + got > FILE_TOP) { fclose(f); REFUSE("overlay: %s is larger than 1 GiB", path); }
		bytes.insert(bytes.end(), block, block + got);
	}
	const bool failed = ferror(f) != 0;
	fclose(f);
	if (failed) REFUSE("overlay: reading %s failed", path);
	Lines lines;
	bool text = true;
	for (size_t k = 0; k < 4 && k < bytes.size(); k++) text = text && is_text_byte(bytes[k]);
	const int rc = text ? read_text(bytes.data(), bytes.size(), lines) : read_shapefile(bytes.data(), bytes.size(), lines);
	if (rc) return rc;
	return give_out(lines, vectors);
} MDEMOD_API_CATCH

int
mdemod_overlay_graticule(const mdemod_overlay_geo *geo, double step_deg, mdemod_overlay_vectors *vectors)
try { MDEMOD_API_ENTER
	if (!vectors) REFUSE("mdemod_overlay_graticule: the vectors are needed");
	memset(vectors, 0, sizeof *vectors);
	int rc = check_geo("mdemod_overlay_graticule", geo);
	if (rc) return rc;
	double step = step_deg;
	if (step == 0.0) {
		static const double steps[6] = { 1, 2, 5, 10, 15, 30 };
		step = 30.0;
		for (int k = 5; k >= 0; k--) if (steps[k] * geo->sy >= 128.0) step = steps[k];
	}
	if (!(step >= 0.01 && step <= 90.0)) REFUSE("mdemod_overlay_graticule: a step of %g degrees (0: auto, or 0.01 .. 90)", step_deg);
	const double lon0 = geo->lon_left, lon1 = geo->lon_left + static_cast<double>(geo->width) / geo->sx;
	double lat1 = geo->lat_top, lat0 = geo->lat_top - static_cast<double>(geo->height) / geo->sy;
	lat1 = lat1 > 90.0 ? 90.0 : lat1;
	lat0 = lat0 < -90.0 ? -90.0 : lat0;
	Lines lines;
	if (lat0 <= lat1) {
		const int64_t m0 = static_cast<int64_t>(std::ceil(lon0 / step)), m1 = static_cast<int64_t>(std::floor(lon1 / step));
		const int64_t p0 = static_cast<int64_t>(std::ceil(lat0 / step)), p1 = static_cast<int64_t>(std::floor(lat1 / step));
		if (m1 - m0 > 100000 || p1 - p0 > 100000) REFUSE("mdemod_overlay_graticule: a step of %g degrees makes more than 100000 lines", step);
		for (int64_t m = m0; m <= m1; m++) {
			const double lon = wrap180(static_cast<double>(m) * step);
			lines.lon.push_back(lon); lines.lat.push_back(lat1);
			lines.lon.push_back(lon); lines.lat.push_back(lat0);
			lines.end_line();
		}
		/* a parallel from the meridian at or before the left edge to the one at or after the right edge, a vertex at each */
		for (int64_t p = p0; p <= p1; p++) {
			const double lat = static_cast<double>(p) * step;
			for (int64_t m = static_cast<int64_t>(std::floor(lon0 / step)); m <= static_cast<int64_t>(std::ceil(lon1 / step)); m++) {
				lines.lon.push_back(wrap180(static_cast<double>(m) * step));
				lines.lat.push_back(lat);
			}
			lines.end_line();
		}
	}
	return give_out(lines, vectors);
} MDEMOD_API_CATCH

int
mdemod_overlay_project(const mdemod_overlay_geo *geo, const mdemod_overlay_vectors *vectors, mdemod_overlay_points *points)
try { MDEMOD_API_ENTER
	if (!points) REFUSE("mdemod_overlay_project: the points are needed");
	memset(points, 0, sizeof *points);
	int rc = check_geo("mdemod_overlay_project", geo);
	if (rc) return rc;
	if (!vectors || !vectors->first || (vectors->n_points && (!vectors->lon || !vectors->lat))) REFUSE("mdemod_overlay_project: the vectors are needed");
	if (vectors->first[vectors->n_lines] > vectors->n_points) REFUSE("mdemod_overlay_project: the lines run past the %u vertices", vectors->n_points);
	const double c = static_cast<double>(geo->width) / (2.0 * geo->sx), sx = geo->sx, sy = geo->sy;
	const int64_t turn = 92160ll * geo->sx, reach = overlay_reach(MDEMOD_OVERLAY_MAX_HALF);
	const int64_t x_top = 256ll * (geo->width - 1), y_top = 256ll * (geo->height - 1);
	std::vector<int64_t> X, Y;
	std::vector<int32_t> ox, oy;
	std::vector<uint32_t> first{ 0 };
	for (uint32_t l = 0; l < vectors->n_lines; l++) {
		const uint32_t from = vectors->first[l], to = vectors->first[l + 1];
		if (to < from || to > vectors->n_points) REFUSE("mdemod_overlay_project: line %u runs from vertex %u to %u of %u", l, from, to, vectors->n_points);
		if (to == from) continue;
		X.clear(); Y.clear();
		double dl = 0.0;
		int64_t lo_x = INT64_MAX, hi_x = INT64_MIN, lo_y = INT64_MAX, hi_y = INT64_MIN;
		for (uint32_t v = from; v < to; v++) {
			const double lon = vectors->lon[v], lat = vectors->lat[v];
			if (!std::isfinite(lon) || !std::isfinite(lat) || std::fabs(lon) > 1e6 || std::fabs(lat) > 1e6) REFUSE("mdemod_overlay_project: vertex %u is not a place (%g, %g)", v, lon, lat);
			dl = v == from ? c + wrap180(lon - geo->lon_left - c) : dl + wrap180(lon - vectors->lon[v - 1]);
			const int64_t x = to_fixed(256.0 * (dl * sx - 0.5)), y = to_fixed(256.0 * ((geo->lat_top - lat) * sy - 0.5));
			X.push_back(x); Y.push_back(y);
			lo_x = x < lo_x ? x : lo_x; hi_x = x > hi_x ? x : hi_x; lo_y = y < lo_y ? y : lo_y; hi_y = y > hi_y ? y : hi_y;
		}
		if (hi_y < -reach || lo_y > y_top + reach) continue;
		for (int shift = -1; shift <= 1; shift++) {
			const int64_t off = shift * turn;
			if (hi_x + off < -reach || lo_x + off > x_top + reach) continue;
			if (ox.size() + X.size() >= COUNT_TOP) REFUSE("mdemod_overlay_project: more than 2^31 vertices");
			for (size_t v = 0; v < X.size(); v++) { ox.push_back(saturate(X[v] + off)); oy.push_back(saturate(Y[v])); }
			first.push_back(static_cast<uint32_t>(ox.size()));
		}
	}
	const size_t n = ox.size();
	points->x = static_cast<int32_t *>(malloc((n ? n : 1) * sizeof(int32_t)));
	points->y = static_cast<int32_t *>(malloc((n ? n : 1) * sizeof(int32_t)));
	points->first = static_cast<uint32_t *>(malloc(first.size() * sizeof(uint32_t)));
	if (!points->x || !points->y || !points->first) { mdemod_overlay_points_free(points); return MDEMOD_ERR_NOMEM; }
	if (n) { memcpy(points->x, ox.data(), n * sizeof(int32_t)); memcpy(points->y, oy.data(), n * sizeof(int32_t)); }
	memcpy(points->first, first.data(), first.size() * sizeof(uint32_t));
	points->n_lines = static_cast<uint32_t>(first.size() - 1); points->n_points = static_cast<uint32_t>(n);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_overlay_cut(const mdemod_overlay_points *points, uint32_t style, uint32_t half_width, uint32_t width, uint32_t height, mdemod_overlay_pieces *pieces)
try { MDEMOD_API_ENTER
	if (!pieces) REFUSE("mdemod_overlay_cut: the pieces are needed");
	if (pieces->n > pieces->room || (pieces->room && !pieces->piece)) REFUSE("mdemod_overlay_cut: the pieces are no list of this library (all zero before the first call)");
	if (!points || !points->first || (points->n_points && (!points->x || !points->y))) REFUSE("mdemod_overlay_cut: the points are needed");
	if (style >= OVERLAY_MAX_STYLES) REFUSE("mdemod_overlay_cut: style %u (0 .. 3)", style);
	if (half_width > MDEMOD_OVERLAY_MAX_HALF) REFUSE("mdemod_overlay_cut: a half width of %u (0 .. 2048, in 1/256 pixel)", half_width);
	if (!width || width > MDEMOD_OVERLAY_MAX_WIDTH || !height || height > MDEMOD_OVERLAY_MAX_HEIGHT) REFUSE("mdemod_overlay_cut: a picture of %u x %u (1 .. 8192 x 1 .. 16384)", width, height);
	const int64_t reach = overlay_reach(half_width), x_top = 256ll * (width - 1), y_top = 256ll * (height - 1);
	for (uint32_t l = 0; l < points->n_lines; l++) {
		const uint32_t from = points->first[l], to = points->first[l + 1];
		if (to < from || to > points->n_points) REFUSE("mdemod_overlay_cut: line %u runs from vertex %u to %u of %u", l, from, to, points->n_points);
		for (uint32_t v = from; v + 1 < to; v++) {
			const int64_t ax = points->x[v], ay = points->y[v], bx = points->x[v + 1], by = points->y[v + 1];
			if (abs64(ax) > VERTEX_TOP || abs64(ay) > VERTEX_TOP || abs64(bx) > VERTEX_TOP || abs64(by) > VERTEX_TOP) continue;   /* the polyline breaks */
			const int rc = cut_segment(ax, ay, bx, by, style, reach, x_top, y_top, pieces);
			if (rc) return rc;
		}
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_overlay_bin(const mdemod_overlay_piece *pieces, uint64_t n_pieces, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height,
                   mdemod_overlay_bins *bins)
try { MDEMOD_API_ENTER
	if (!bins) REFUSE("mdemod_overlay_bin: the bins are needed");
	memset(bins, 0, sizeof *bins);
	int rc = check_styles("mdemod_overlay_bin", styles, n_styles);
	if (rc) return rc;
	if (!width || width > MDEMOD_OVERLAY_MAX_WIDTH || !height || height > MDEMOD_OVERLAY_MAX_HEIGHT) REFUSE("mdemod_overlay_bin: a picture of %u x %u (1 .. 8192 x 1 .. 16384)", width, height);
	if (n_pieces && !pieces) REFUSE("mdemod_overlay_bin: the pieces are needed");
	if ((rc = check_pieces("mdemod_overlay_bin", pieces, n_pieces, n_styles))) return rc;
	const uint32_t tiles_x = overlay_tiles(width), tiles_y = overlay_tiles(height);
	const size_t tiles = static_cast<size_t>(tiles_x) * tiles_y;
	int64_t reach[OVERLAY_MAX_STYLES];
	for (uint32_t s = 0; s < n_styles; s++) reach[s] = overlay_reach(styles[s].half_width);
	constexpr int64_t SPAN = 256 * OVERLAY_TILE, LAST = 256 * (OVERLAY_TILE - 1);
	/* the tiles x0 .. x1, y0 .. y1 of a piece; false: none */
	auto range = [&](const mdemod_overlay_piece &p, int64_t &x0, int64_t &x1, int64_t &y0, int64_t &y1) {
		/* the far end from the tangent: B = A + t L / 16384 to within a unit per axis; one more for the rounding of L */
		const int64_t bx = p.ax + floor_div(static_cast<int64_t>(p.tx) * p.L, 16384), by = p.ay + floor_div(static_cast<int64_t>(p.ty) * p.L, 16384);
		const int64_t r = reach[p.style] + 4;
		const int64_t lo_x = (p.ax < bx ? p.ax : bx) - r, hi_x = (p.ax > bx ? p.ax : bx) + r, lo_y = (p.ay < by ? p.ay : by) - r, hi_y = (p.ay > by ? p.ay : by) + r;
		x0 = ceil_div(lo_x - LAST, SPAN); x1 = floor_div(hi_x, SPAN); y0 = ceil_div(lo_y - LAST, SPAN); y1 = floor_div(hi_y, SPAN);
		x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
		x1 = x1 > static_cast<int64_t>(tiles_x) - 1 ? static_cast<int64_t>(tiles_x) - 1 : x1;
		y1 = y1 > static_cast<int64_t>(tiles_y) - 1 ? static_cast<int64_t>(tiles_y) - 1 : y1;
		return x0 <= x1 && y0 <= y1;
	};
	std::vector<uint64_t> count(tiles + 1, 0);
	for (uint64_t k = 0; k < n_pieces; k++) {
		const mdemod_overlay_piece &p = pieces[k];
		int64_t x0, x1, y0, y1;
		if (!range(p, x0, x1, y0, y1)) continue;
		for (int64_t y = y0; y <= y1; y++)
			for (int64_t x = x0; x <= x1; x++) count[static_cast<size_t>(y) * tiles_x + x + 1]++;
	}
	for (size_t t = 0; t < tiles; t++) count[t + 1] += count[t];
	if (count[tiles] >= COUNT_TOP) REFUSE("mdemod_overlay_bin: more than 2^31 items");
	bins->tile_first = static_cast<uint32_t *>(malloc((tiles + 1) * sizeof(uint32_t)));
	bins->items = static_cast<uint32_t *>(malloc((count[tiles] ? count[tiles] : 1) * sizeof(uint32_t)));
	if (!bins->tile_first || !bins->items) { mdemod_overlay_bins_free(bins); return MDEMOD_ERR_NOMEM; }
	for (size_t t = 0; t <= tiles; t++) bins->tile_first[t] = static_cast<uint32_t>(count[t]);
	std::vector<uint64_t> next(count.begin(), count.end() - 1);
	for (uint32_t s = 0; s < n_styles; s++)                                    /* ascending in style, then in index */
		for (uint64_t k = 0; k < n_pieces; k++) {
			if (static_cast<uint32_t>(pieces[k].style) != s) continue;
			int64_t x0, x1, y0, y1;
			if (!range(pieces[k], x0, x1, y0, y1)) continue;
			for (int64_t y = y0; y <= y1; y++)
				for (int64_t x = x0; x <= x1; x++) bins->items[next[static_cast<size_t>(y) * tiles_x + x]++] = static_cast<uint32_t>(k);
		}
	bins->tiles_x = tiles_x; bins->tiles_y = tiles_y; bins->n_items = count[tiles];
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_overlay_model_draw(const mdemod_overlay_piece *pieces, uint64_t n_pieces, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height,
                          uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask)
try { MDEMOD_API_ENTER
	int rc = overlay_check_draw("mdemod_overlay_model_draw", styles, n_styles, width, height, planes, pixels, valid);
	if (rc) return rc;
	if ((rc = check_pieces("mdemod_overlay_model_draw", pieces, n_pieces, n_styles))) return rc;
	model_all(pieces, n_pieces, styles, n_styles, width, height, planes, pixels, valid, mask);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_overlay_model_tiles(const mdemod_overlay_piece *pieces, uint64_t n_pieces, const uint32_t *tile_first, const uint32_t *items, uint64_t n_items,
                           const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid,
                           uint8_t *mask)
try { MDEMOD_API_ENTER
	int rc = overlay_check_draw("mdemod_overlay_model_tiles", styles, n_styles, width, height, planes, pixels, valid);
	if (rc) return rc;
	if (!height) return MDEMOD_OK;
	if ((rc = check_pieces("mdemod_overlay_model_tiles", pieces, n_pieces, n_styles))) return rc;
	if (!tile_first || (n_items && !items)) REFUSE("mdemod_overlay_model_tiles: the bins are needed");
	model_tiles(pieces, n_pieces, tile_first, items, n_items, styles, n_styles, width, 0, height, planes, pixels, valid, mask);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_overlay_model_host(const mdemod_overlay_geo *geo, const mdemod_overlay_layer *layers, uint32_t n_layers, const mdemod_overlay_style *styles, uint32_t n_styles,
                          uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines, mdemod_overlay_report *report)
try { MDEMOD_API_ENTER
	ModelBackend model;
	return overlay_draw_bands("mdemod_overlay_model_host", geo, layers, n_layers, styles, n_styles, planes, pixels, valid, mask, piece_lines, report, model);
} MDEMOD_API_CATCH

} /* extern "C" */
