/*
 * map_host.cpp — host side of the map layer (include/meteor_demod_amd_map.h): the TLE parser, the circular J2 orbit, the time fit,
 * the forward function (pixel to latitude / longitude), the grid with its nodes (the forward function inverted), the bands of the
 * whole-map entry, and the host model of the kernel of csrc/map.hip (mdemod_map_model_*: a plain loop over the warp's model, which
 * csrc/warp_model.h holds once for this layer and the mosaic layer).  Free of the GPU runtime.
 *
 * The inverse.  A ground point G is seen from line time t exactly when it lies in the scan plane of that moment, the plane through
 * the satellite spanned by r and h: G . v(t) = 0 in Earth-fixed coordinates (r . v = 0).  That is one equation in one unknown, and
 * the scan angle follows in closed form: theta = atan2(side (G - a r) . h, -(G - a r) . r).  G . v has one root per half revolution;
 * the one with the satellite over G is found from a table of r(t) every 8 s over the pass and its margin (the entry with the
 * largest G . r), then Newton steps with the derivative -du/dt G . r - w_e G . (z x v) (the drift of the node left out: it is four
 * orders below and only slows the last step).  Four or five steps reach 1e-7 s.
 */
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "map_host.h"
#include "mdemod_internal_api.h"
#include "warp_model.h"

namespace {

constexpr double MAP_MU = 398600.4418, MAP_RE = 6378.137, MAP_F = 1.0 / 298.257223563, MAP_J2 = 1.08262668e-3;
constexpr double MAP_PI = 3.14159265358979323846, MAP_RAD = MAP_PI / 180.0;
constexpr double MAP_B = MAP_RE * (1.0 - MAP_F), MAP_E2 = MAP_F * (2.0 - MAP_F);
constexpr double MAP_EARTH_RATE = 360.98564736629 * MAP_RAD / 86400.0;          /* rad/s */
constexpr double MAP_TABLE_STEP = 8.0;

struct Orbit {
	double a, ci, si, raan0, u0, raan_dot, u_dot, epoch_sec;
	int32_t epoch_day;
};

/* r, v, h in Earth-fixed coordinates */
struct Frame { double r[3], v[3], h[3]; };

Orbit
orbit_of(const mdemod_map_tle &t)
{
	Orbit o;
	const double n = t.mean_motion * 2.0 * MAP_PI / 86400.0, inc = t.inclination_deg * MAP_RAD;
	o.a = cbrt(MAP_MU / (n * n));
	o.ci = cos(inc);
	o.si = sin(inc);
	const double k = 1.5 * MAP_J2 * (MAP_RE / o.a) * (MAP_RE / o.a) * n;
	o.raan0 = t.raan_deg * MAP_RAD;
	o.u0 = (t.argp_deg + t.mean_anomaly_deg) * MAP_RAD;
	o.raan_dot = -k * o.ci;
	o.u_dot = n + 0.5 * k * (5.0 * o.ci * o.ci - 1.0);
	o.epoch_day = t.epoch_day;
	o.epoch_sec = t.epoch_sec;
	return o;
}

/* `sec` UTC seconds of day `date` (any real number) */
void
frame_at(const Orbit &o, int32_t date, double sec, Frame &f)
{
	const double dt = (static_cast<double>(date) - static_cast<double>(o.epoch_day)) * 86400.0 + (sec - o.epoch_sec);
	const double raan = o.raan0 + o.raan_dot * dt, u = o.u0 + o.u_dot * dt;
	const double d = (static_cast<double>(date) - 10957.0) + (sec - 43200.0) / 86400.0;
	const double g = fmod(280.46061837 + 360.98564736629 * d, 360.0) * MAP_RAD;
	const double cO = cos(raan), sO = sin(raan), cu = cos(u), su = sin(u), cg = cos(g), sg = sin(g);
	const double r[3] = { cO * cu - sO * su * o.ci, sO * cu + cO * su * o.ci, su * o.si };
	const double v[3] = { -cO * su - sO * cu * o.ci, -sO * su + cO * cu * o.ci, cu * o.si };
	const double h[3] = { sO * o.si, -cO * o.si, o.ci };
	auto turn = [&](const double *in, double *out) {
		out[0] = in[0] * cg + in[1] * sg;
		out[1] = -in[0] * sg + in[1] * cg;
		out[2] = in[2];
	};
	turn(r, f.r); turn(v, f.v); turn(h, f.h);
}

inline double dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* the ray from a r along -cos theta r + side sin theta h against the ellipsoid; false: not visible */
bool
ground_point(const Orbit &o, const Frame &f, double theta, int side, double &lat, double &lon)
{
	const double c = cos(theta), s = side * sin(theta);
	double S[3], L[3];
	for (int k = 0; k < 3; k++) { S[k] = o.a * f.r[k]; L[k] = -c * f.r[k] + s * f.h[k]; }
	const double ia = 1.0 / (MAP_RE * MAP_RE), ib = 1.0 / (MAP_B * MAP_B);
	const double A = (L[0] * L[0] + L[1] * L[1]) * ia + L[2] * L[2] * ib;
	const double B = (S[0] * L[0] + S[1] * L[1]) * ia + S[2] * L[2] * ib;
	const double C = (S[0] * S[0] + S[1] * S[1]) * ia + S[2] * S[2] * ib - 1.0;
	const double disc = B * B - A * C;
	if (!(disc >= 0.0)) return false;
	const double t = (-B - sqrt(disc)) / A;
	if (!(t > 0.0)) return false;
	const double x = S[0] + t * L[0], y = S[1] + t * L[1], z = S[2] + t * L[2];
	lat = atan2(z, (1.0 - MAP_E2) * hypot(x, y)) / MAP_RAD;
	lon = atan2(y, x) / MAP_RAD;
	return true;
}

struct Pass {
	Orbit orbit;
	int32_t date;
	int side;
	double s0, line_period, offset, step;         /* step: D, radians per column */
	double sec_of(double y) const { return s0 + y * line_period - offset; }
};

bool
forward(const Pass &p, double y, double x, double &lat, double &lon)
{
	Frame f;
	frame_at(p.orbit, p.date, p.sec_of(y), f);
	return ground_point(p.orbit, f, (x - 783.5) * p.step, p.side, lat, lon);
}

inline double wrap180(double d) { d = fmod(d, 360.0); return d >= 180.0 ? d - 360.0 : d < -180.0 ? d + 360.0 : d; }

int64_t
days_from_civil(int64_t y, unsigned m, unsigned d)
{
	y -= m <= 2;
	const int64_t era = (y >= 0 ? y : y - 399) / 400;
	const unsigned yoe = static_cast<unsigned>(y - era * 400), doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1, doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
	return era * 146097 + static_cast<int64_t>(doe) - 719468;
}

double
median(std::vector<double> &v)
{
	std::sort(v.begin(), v.end());
	const size_t n = v.size();
	return 0.5 * (v[(n - 1) / 2] + v[n / 2]);
}

/* columns first .. last (from 1) of a TLE line as a number; false when it is none */
bool
field(const std::string &line, int first, int last, const char *prefix, double &out)
{
	std::string s = line.substr(first - 1, last - first + 1);
	const size_t a = s.find_first_not_of(' '), b = s.find_last_not_of(' ');
	if (a == std::string::npos) return false;
	s = s.substr(a, b - a + 1);
	for (char c : s)
		if (!((c >= '0' && c <= '9') || c == '.' || c == '+' || c == '-')) return false;
	s = prefix + s;
	char *end = nullptr;
	out = strtod(s.c_str(), &end);
	return end && !*end && std::isfinite(out);
}

int
checksum(const std::string &line)
{
	int sum = 0;
	for (int k = 0; k < 68; k++) sum += line[k] >= '0' && line[k] <= '9' ? line[k] - '0' : line[k] == '-' ? 1 : 0;
	return sum % 10;
}

int
resolve_date(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, uint32_t lines, int32_t &date)
{
	if (tm.date != MDEMOD_MAP_DATE_AUTO) { date = tm.date; return MDEMOD_OK; }
	const double mid = tm.s0 + static_cast<double>(lines / 2) * tm.row_period / 8.0 - o.time_offset;
	const double days = floor((static_cast<double>(tle.epoch_day) * 86400.0 + tle.epoch_sec - mid) / 86400.0 + 0.5);
	if (!(fabs(days) < 1.0e6)) REFUSE("map: no date can be found from the epoch and the line times");
	date = static_cast<int32_t>(days);
	return MDEMOD_OK;
}

int
check_tle(const char *who, const mdemod_map_tle *t)
{
	if (!t) REFUSE("%s: the element set is needed", who);
	if (!(t->mean_motion >= 0.5 && t->mean_motion <= 20.0)) REFUSE("%s: the mean motion is %g revolutions per day (0.5 .. 20)", who, t->mean_motion);
	if (!(t->inclination_deg >= 0.0 && t->inclination_deg <= 180.0)) REFUSE("%s: the inclination is %g degrees (0 .. 180)", who, t->inclination_deg);
	if (!std::isfinite(t->raan_deg) || !std::isfinite(t->argp_deg) || !std::isfinite(t->mean_anomaly_deg) || !(t->epoch_sec >= 0.0 && t->epoch_sec <= 86400.0))
		REFUSE("%s: the element set holds a field that is not a number", who);
	return MDEMOD_OK;
}

int
check_timing(const char *who, const mdemod_map_timing *tm)
{
	if (!tm) REFUSE("%s: the line times are needed", who);
	if (!(tm->row_period >= 0.1 && tm->row_period <= 10.0)) REFUSE("%s: the row period is %g s (0.1 .. 10)", who, tm->row_period);
	if (!(fabs(tm->s0) <= 1.0e6)) REFUSE("%s: the time of line 0 is %g s", who, tm->s0);
	return MDEMOD_OK;
}

Pass
pass_of(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date)
{
	Pass p;
	p.orbit = orbit_of(tle);
	p.date = date;
	p.side = o.side;
	p.s0 = tm.s0;
	p.line_period = tm.row_period / 8.0;
	p.offset = o.time_offset;
	p.step = o.scan_deg / PIC_SRC_W * MAP_RAD;
	return p;
}

/* the source pixel that sees (lat, lon) in degrees; false: no node */
struct Inverse {
	const Pass &p;
	double sec_lo, sec_hi, table_t0, theta_max;
	std::vector<double> table;                      /* r every MAP_TABLE_STEP seconds */

	Inverse(const Pass &pass, uint32_t lines, double scan_deg) : p(pass)
	{
		sec_lo = p.sec_of(0.0) - MDEMOD_MAP_TIME_MARGIN;
		sec_hi = p.sec_of(static_cast<double>(lines - 1)) + MDEMOD_MAP_TIME_MARGIN;
		theta_max = (scan_deg / 2.0 + MDEMOD_MAP_SCAN_MARGIN) * MAP_RAD;
		table_t0 = sec_lo - 4.0 * MAP_TABLE_STEP;
		const size_t n = static_cast<size_t>((sec_hi - sec_lo) / MAP_TABLE_STEP) + 10;
		table.resize(3 * n);
		for (size_t k = 0; k < n; k++) {
			Frame f;
			frame_at(p.orbit, p.date, table_t0 + MAP_TABLE_STEP * static_cast<double>(k), f);
			memcpy(&table[3 * k], f.r, sizeof f.r);
		}
	}

	bool solve(double lat, double lon, double &y, double &x) const
	{
		const double phi = lat * MAP_RAD, lam = lon * MAP_RAD, N = MAP_RE / sqrt(1.0 - MAP_E2 * sin(phi) * sin(phi));
		const double G[3] = { N * cos(phi) * cos(lam), N * cos(phi) * sin(lam), N * (1.0 - MAP_E2) * sin(phi) };
		size_t best = 0;
		double most = -1.0e30;
		for (size_t k = 0; 3 * k < table.size(); k++) {
			const double d = dot(G, &table[3 * k]);
			if (d > most) { most = d; best = k; }
		}
		double t = table_t0 + MAP_TABLE_STEP * static_cast<double>(best);
		Frame f;
		bool done = false;
		for (int it = 0; it < 12 && !done; it++) {
			frame_at(p.orbit, p.date, t, f);
			const double zxv[3] = { -f.v[1], f.v[0], 0.0 };
			const double slope = -p.orbit.u_dot * dot(G, f.r) - MAP_EARTH_RATE * dot(G, zxv);
			if (!(fabs(slope) > 1.0e-9)) return false;
			double dt = -dot(G, f.v) / slope;
			if (!std::isfinite(dt)) return false;
			dt = dt > 60.0 ? 60.0 : dt < -60.0 ? -60.0 : dt;
			t += dt;
			done = fabs(dt) < 1.0e-7;
			if (t < sec_lo - 600.0 || t > sec_hi + 600.0) return false;
		}
		if (!done || t < sec_lo || t > sec_hi) return false;
		frame_at(p.orbit, p.date, t, f);
		double D[3];
		for (int k = 0; k < 3; k++) D[k] = G[k] - p.orbit.a * f.r[k];
		/* the nearer root: the ray meets the surface from outside */
		const double normal[3] = { G[0] / (MAP_RE * MAP_RE), G[1] / (MAP_RE * MAP_RE), G[2] / (MAP_B * MAP_B) };
		if (!(dot(D, normal) < 0.0)) return false;
		const double theta = atan2(p.side * dot(D, f.h), -dot(D, f.r));
		if (!(fabs(theta) <= theta_max)) return false;
		y = (t + p.offset - p.s0) / p.line_period;
		x = theta / p.step + 783.5;
		return true;
	}
};

void
model_warp(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes, const uint8_t *lut,
           const int32_t *nodes, uint32_t width, uint32_t height, uint8_t *out, uint8_t *valid)
{
	const uint32_t nc = map_node_count(width);
	for (uint32_t i = 0; i < height; i++)
		for (uint32_t j = 0; j < width; j++) {
			uint8_t *px = out + (static_cast<size_t>(i) * width + j) * planes;
			uint8_t seen = 0;
			int64_t X, Y;
			memset(px, 0, planes);
			if (warp_model_point(nodes, nc, rows, i, j, X, Y))
				for (uint32_t pl = 0; pl < planes; pl++) {
					uint32_t v;
					if (!warp_model_value(image[select[pl]], filled[select[pl]], rows, X, Y, v)) continue;
					px[pl] = lut[256 * pl + v];
					seen |= static_cast<uint8_t>(1u << pl);
				}
			if (valid) valid[static_cast<size_t>(i) * width + j] = seen;
		}
}

struct ModelBackend : MapBackend {
	const uint8_t *img[3], *fil[3];
	const int32_t *nodes = nullptr;
	const uint8_t *lut = nullptr;
	uint32_t rows = 0, width = 0, nc = 0;
	int begin(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t r, const mdemod_map_nodes &grid, uint32_t, uint32_t) override
	{
		for (int s = 0; s < 3; s++) { img[s] = image[s]; fil[s] = filled[s]; }
		rows = r; nodes = grid.nodes; width = grid.width; nc = grid.node_cols;
		return MDEMOD_OK;
	}
	int histogram(uint32_t *hist) override { return mdemod_picture_model_histogram(img, fil, rows, hist); }
	int tables(const uint8_t *t, uint32_t) override { lut = t; return MDEMOD_OK; }
	int band(const uint32_t *select, uint32_t planes, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid) override
	{
		model_warp(img, fil, rows, select, planes, lut, nodes + 2 * static_cast<size_t>(node_row) * nc, width, height, out, valid);
		return MDEMOD_OK;
	}
};

} /* namespace */

/* ---------------------------------------------------------------- what mdemod_map_grid and the mosaic layer's grid are made of */
int
map_check_pass(const char *who, const mdemod_map_tle *tle, const mdemod_map_timing *timing)
{
	const int rc = check_tle(who, tle);
	return rc ? rc : check_timing(who, timing);
}

int
map_check_lines(uint32_t lines)
{
	if (!lines || lines % 8) REFUSE("map: the picture has %u lines (a multiple of 8, at least 8)", lines);
	if (lines / 8 > MDEMOD_MAP_MAX_ROWS) REFUSE("map: %u strip rows are more than a map takes (8192)", lines / 8);
	return MDEMOD_OK;
}

int
map_resolve_date(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, uint32_t lines, int32_t &date)
{
	return resolve_date(tle, tm, o, lines, date);
}

int
map_swath_centre(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, double &lon_c)
{
	const Pass p = pass_of(tle, tm, o, date);
	double lat_c;
	if (!forward(p, (lines - 1) / 2.0, 783.5, lat_c, lon_c)) REFUSE("map: the middle of the picture does not see the Earth");
	return MDEMOD_OK;
}

int
map_swath_border(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, double lon_c, MapRange &range)
{
	const Pass p = pass_of(tle, tm, o, date);
	int rc;
	auto sample = [&](double y, double x) -> int {
		double lat, lon;
		if (!forward(p, y, x, lat, lon)) REFUSE("map: line %.0f, column %.0f on the border of the swath does not see the Earth (scan angle %g)", y, x, o.scan_deg);
		if (fabs(lat) > MDEMOD_MAP_MAX_LAT)
			REFUSE("map: line %.0f, column %.0f lies at %.2f degrees of latitude, beyond 85: a polar pass wants another projection", y, x, lat);
		const double dl = wrap180(lon - lon_c);
		range.lat_lo = std::min(range.lat_lo, lat); range.lat_hi = std::max(range.lat_hi, lat);
		range.lon_lo = std::min(range.lon_lo, dl); range.lon_hi = std::max(range.lon_hi, dl);
		return MDEMOD_OK;
	};
	for (uint32_t y = 0;; y = std::min(y + 8, lines - 1)) {
		if ((rc = sample(y, 0.0)) || (rc = sample(y, PIC_LAST))) return rc;
		if (y == lines - 1) break;
	}
	for (uint32_t x = 0;; x = std::min<uint32_t>(x + 16, PIC_LAST)) {
		if ((rc = sample(0.0, x)) || (rc = sample(lines - 1, x))) return rc;
		if (x == PIC_LAST) break;
	}
	return MDEMOD_OK;
}

int
map_frame(const mdemod_map_opts &o, const MapRange &range, double lon_c, MapFrame &f)
{
	const double sy = o.px_per_deg, lat_mid = 0.5 * (range.lat_lo + range.lat_hi);
	const double sx = std::max(1.0, floor(sy * cos(lat_mid * MAP_RAD) + 0.5));
	const double lat_top = ceil(range.lat_hi * sy) / sy, left = floor((lon_c + range.lon_lo) * sx) / sx;
	const double h = std::max(1.0, ceil((lat_top - range.lat_lo) * sy)), w = std::max(4.0, ceil(ceil((lon_c + range.lon_hi - left) * sx) / 4.0) * 4.0);
	if (w > MDEMOD_MAP_MAX_WIDTH || h > MDEMOD_MAP_MAX_HEIGHT) {
		const double fit = floor(sy * std::min(MDEMOD_MAP_MAX_WIDTH / (w + 8.0), MDEMOD_MAP_MAX_HEIGHT / (h + 2.0)));
		REFUSE("map: %.0f x %.0f pixels at %g pixels per degree are more than a map takes (8192 x 16384): a scale of %.0f fits", w, h, sy, std::max(1.0, fit));
	}
	f.sy = sy; f.sx = sx; f.lat_top = lat_top; f.left = left;
	f.width = static_cast<uint32_t>(w); f.height = static_cast<uint32_t>(h);
	return MDEMOD_OK;
}

double
map_frame_lon_left(const MapFrame &f)
{
	return f.left >= 180.0 ? f.left - 360.0 : f.left < -180.0 ? f.left + 360.0 : f.left;
}

namespace {

/* one node: the source pixel that sees (lat, lon), rounded to 1 / 256 pixel */
inline void
put_node(const Inverse &inv, double lat, double lon, int32_t *node)
{
	double y, x;
	node[0] = node[1] = MDEMOD_MAP_NO_NODE;
	if (!inv.solve(lat, lon, y, x)) return;
	const double X = floor(256.0 * x + 0.5), Y = floor(256.0 * y + 0.5);
	if (!(fabs(X) < 2.0e9 && fabs(Y) < 2.0e9)) return;
	node[0] = static_cast<int32_t>(X);
	node[1] = static_cast<int32_t>(Y);
}

} /* namespace */

void
map_nodes_on(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, const MapFrame &f, int32_t *nodes)
{
	const Pass p = pass_of(tle, tm, o, date);
	const Inverse inv(p, lines, o.scan_deg);
	const uint32_t node_rows = map_node_count(f.height), node_cols = map_node_count(f.width);
	for (uint32_t a = 0; a < node_rows; a++)
		for (uint32_t b = 0; b < node_cols; b++)
			put_node(inv, f.lat_top - (MAP_STEP * a + 0.5) / f.sy, f.left + (MAP_STEP * b + 0.5) / f.sx, nodes + 2 * (static_cast<size_t>(a) * node_cols + b));
}

void
map_nodes_at(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, const double *lat, const double *lon,
             size_t n, int32_t *nodes)
{
	const Pass p = pass_of(tle, tm, o, date);
	const Inverse inv(p, lines, o.scan_deg);
	for (size_t k = 0; k < n; k++) {
		if (std::isfinite(lat[k]) && std::isfinite(lon[k])) put_node(inv, lat[k], lon[k], nodes + 2 * k);
		else nodes[2 * k] = nodes[2 * k + 1] = MDEMOD_MAP_NO_NODE;
	}
}

bool
map_forward(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, double y, double x, double &lat, double &lon)
{
	return forward(pass_of(tle, tm, o, date), y, x, lat, lon);
}

void
map_solver_of(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, MapSolver &s)
{
	const Pass p = pass_of(tle, tm, o, date);
	Inverse inv(p, lines, o.scan_deg);
	const double two_pi = 2.0 * MAP_PI;
	const double dt = (static_cast<double>(date) - static_cast<double>(p.orbit.epoch_day)) * 86400.0 + (inv.table_t0 - p.orbit.epoch_sec);
	const double d = (static_cast<double>(date) - 10957.0) + (inv.table_t0 - 43200.0) / 86400.0;
	s.a = p.orbit.a; s.ci = p.orbit.ci; s.si = p.orbit.si;
	s.raan_dot = p.orbit.raan_dot; s.u_dot = p.orbit.u_dot; s.g_dot = MAP_EARTH_RATE;
	s.raan_t0 = fmod(p.orbit.raan0 + p.orbit.raan_dot * dt, two_pi);
	s.u_t0 = fmod(p.orbit.u0 + p.orbit.u_dot * dt, two_pi);
	s.g_t0 = fmod(280.46061837 + 360.98564736629 * d, 360.0) * MAP_RAD;
	s.table_t0 = inv.table_t0; s.table_step = MAP_TABLE_STEP;
	s.sec_lo = inv.sec_lo; s.sec_hi = inv.sec_hi; s.theta_max = inv.theta_max;
	s.s0 = p.s0; s.line_period = p.line_period; s.offset = p.offset; s.step = p.step;
	s.side = p.side;
	s.table.swap(inv.table);
}

int
map_settings(const mdemod_map_opts *opts, mdemod_map_opts &out)
{
	mdemod_map_default_opts(&out);
	if (opts) out = *opts;
	if (!(out.scan_deg >= 1.0 && out.scan_deg <= 130.0)) REFUSE("map: scan angle is %g degrees (the full angle: 1 .. 130)", out.scan_deg);
	if (!(out.px_per_deg >= 1.0 && out.px_per_deg <= 1000.0)) REFUSE("map: the scale is %g pixels per degree (1 .. 1000)", out.px_per_deg);
	if (!(out.time_offset >= -86400.0 && out.time_offset <= 86400.0)) REFUSE("map: the time offset is %g s (-86400 .. 86400)", out.time_offset);
	if (!(out.row_period >= 0.1 && out.row_period <= 10.0)) REFUSE("map: the row period is %g s (0.1 .. 10)", out.row_period);
	if (out.side != 1 && out.side != -1) REFUSE("map: the scan side is %d (1 or -1)", out.side);
	if (out.date != MDEMOD_MAP_DATE_AUTO && (out.date < -1000000 || out.date > 1000000)) REFUSE("map: the date is day %d since 1970 (or auto)", out.date);
	if (out.clip_low > MDEMOD_PICTURE_MAX_CLIP || out.clip_high > MDEMOD_PICTURE_MAX_CLIP)
		REFUSE("map: the clips are %u and %u permille (each 0 .. 499)", out.clip_low, out.clip_high);
	if (out.piece_lines > MDEMOD_MAP_MAX_HEIGHT || out.piece_lines % MAP_STEP)
		REFUSE("map: piece_lines is %u (0 for the default, or a multiple of 16 up to 16384)", out.piece_lines);
	if (!out.piece_lines) out.piece_lines = MDEMOD_MAP_DEFAULT_PIECE;
	return MDEMOD_OK;
}

int
map_check_warp(const char *who, uint32_t rows, const uint32_t *select, uint32_t planes, uint32_t width, uint32_t height)
{
	const int rc = pic_check_select(who, rows, select, planes);
	if (rc) return rc;
	if (width < 4 || width > MDEMOD_MAP_MAX_WIDTH || width % 4) REFUSE("%s: the width is %u (a multiple of 4, 4 .. 8192)", who, width);
	if (height > MDEMOD_MAP_MAX_HEIGHT) REFUSE("%s: the height is %u (at most 16384)", who, height);
	return MDEMOD_OK;
}

int
map_check_compose(const char *who, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                  const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select, uint32_t planes,
                  mdemod_map_result *out)
{
	int rc;
	if (!out) REFUSE("%s: the result is needed", who);
	if ((rc = check_tle(who, tle))) return rc;
	if ((rc = pic_check_select(who, rows, select, planes))) return rc;
	if (!rows) REFUSE("%s: a picture without strip rows cannot be put on a map", who);
	if (rows > MDEMOD_MAP_MAX_ROWS) REFUSE("%s: %u strip rows are more than a map takes (8192)", who, rows);
	if ((rc = pic_check_slots(who, image, filled, select, planes))) return rc;
	if (n_desc && (!place || !sinfo)) REFUSE("%s: the placements and the reports of the packets are needed", who);
	return MDEMOD_OK;
}

int
map_compose_bands(const mdemod_map_opts &o, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                  const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select, uint32_t planes,
                  mdemod_map_result *out, MapBackend &backend)
{
	memset(out, 0, sizeof *out);
	mdemod_map_timing tm;
	int rc = mdemod_map_fit_time(place, sinfo, n_desc, &o, &tm);
	if (rc) return rc;
	mdemod_map_nodes grid;
	if ((rc = mdemod_map_grid(tle, &tm, &o, 8 * rows, &grid))) return rc;
	struct Keep { mdemod_map_nodes *g; ~Keep() { mdemod_map_grid_free(g); } } keep{ &grid };
	tm.date = grid.date;
	out->width = grid.width; out->height = grid.height; out->planes = planes; out->sx = grid.sx;
	out->sy = grid.sy; out->lat_top = grid.lat_top; out->lon_left = grid.lon_left;
	out->timing = tm;
	out->utc0 = tm.s0 - o.time_offset;
	/* only the selected slots are looked at */
	const uint8_t *img[3] = { nullptr, nullptr, nullptr }, *fil[3] = { nullptr, nullptr, nullptr };
	for (uint32_t p = 0; p < planes; p++) { img[select[p]] = image[select[p]]; fil[select[p]] = filled[select[p]]; }
	const uint32_t P = o.piece_lines < grid.height ? o.piece_lines : (grid.height + MAP_STEP - 1) / MAP_STEP * MAP_STEP;
	if ((rc = backend.begin(img, fil, rows, grid, planes, P))) return rc;
	std::vector<uint32_t> hist(3 * 256, 0);
	if (o.stretch && (rc = backend.histogram(hist.data()))) return rc;
	uint8_t lut[3 * 256];
	for (uint32_t p = 0; p < planes; p++) {
		uint32_t lim[2] = { 0, 255 };
		if (o.stretch) {
			if ((rc = mdemod_picture_lut(hist.data() + 256 * select[p], o.clip_low, o.clip_high, lut + 256 * p, lim))) return rc;
		} else {
			for (int v = 0; v < 256; v++) lut[256 * p + v] = static_cast<uint8_t>(v);
		}
		out->lo[p] = lim[0];
		out->hi[p] = lim[1];
	}
	if ((rc = backend.tables(lut, planes))) return rc;
	const size_t W = grid.width, H = grid.height;
	out->pixels = static_cast<uint8_t *>(malloc(H * W * planes));
	out->valid = static_cast<uint8_t *>(malloc(H * W));
	if (!out->pixels || !out->valid) { mdemod_map_free(out); return MDEMOD_ERR_NOMEM; }
	for (uint32_t at = 0; at < H; at += P) {
		rc = backend.band(select, planes, at / MAP_STEP, P < H - at ? P : static_cast<uint32_t>(H - at), out->pixels + at * W * planes, out->valid + at * W);
		if (rc) { mdemod_map_free(out); return rc; }
	}
	for (size_t i = 0; i < H * W; i++) out->valid_pixels += out->valid[i] != 0;
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_map_default_opts(mdemod_map_opts *opts)
{
	if (!opts) return;
	opts->scan_deg = 110.0;
	opts->px_per_deg = 100.0;
	opts->time_offset = 10800.0;
	opts->row_period = 8.0 / 6.5;
	opts->side = 1;
	opts->date = MDEMOD_MAP_DATE_AUTO;
	opts->stretch = 1;
	opts->clip_low = 5;
	opts->clip_high = 5;
	opts->piece_lines = 0;
}

void
mdemod_map_grid_free(mdemod_map_nodes *grid)
{
	if (!grid) return;
	free(grid->nodes);
	memset(grid, 0, sizeof *grid);
}

void
mdemod_map_free(mdemod_map_result *out)
{
	if (!out) return;
	free(out->pixels); free(out->valid);
	memset(out, 0, sizeof *out);
}

int
mdemod_map_parse_tle(const char *text, uint32_t norad, mdemod_map_tle *tle)
try { MDEMOD_API_ENTER
	if (!text || !tle) REFUSE("mdemod_map_parse_tle: the text and the element set are needed");
	std::vector<std::string> lines;
	for (const char *p = text; *p;) {
		const char *e = strchr(p, '\n');
		std::string l(p, e ? static_cast<size_t>(e - p) : strlen(p));
		while (!l.empty() && (l.back() == '\r' || l.back() == ' ' || l.back() == '\t')) l.pop_back();
		if (!l.empty()) lines.push_back(l);
		if (!e) break;
		p = e + 1;
	}
	auto numbered = [](const std::string &l, char c) { return l[0] == c && (l.size() == 1 || l[1] == ' '); };
	bool any = false;
	for (size_t i = 0; i < lines.size(); i++) {
		const std::string &l1 = lines[i];
		if (numbered(l1, '2')) REFUSE("TLE: line %zu is a line 2 without its line 1", i + 1);
		if (!numbered(l1, '1')) continue;                                          /* a name line */
		if (l1.size() < 69) REFUSE("TLE: line %zu is short: %zu characters of 69", i + 1, l1.size());
		if (i + 1 >= lines.size() || !numbered(lines[i + 1], '2')) REFUSE("TLE: line %zu is a line 1, and no line 2 follows it", i + 1);
		const std::string &l2 = lines[++i];
		if (l2.size() < 69) REFUSE("TLE: line %zu is short: %zu characters of 69", i + 1, l2.size());
		double cat1, cat2;
		if (!field(l1, 3, 7, "", cat1) || !field(l2, 3, 7, "", cat2) || cat1 < 0 || cat2 < 0 || cat1 != floor(cat1) || cat2 != floor(cat2))
			REFUSE("TLE: the catalogue number of lines %zu and %zu is missing or not a number", i, i + 1);
		if (cat1 != cat2) REFUSE("TLE: lines %zu and %zu carry the catalogue numbers %.0f and %.0f", i, i + 1, cat1, cat2);
		any = true;
		if (norad && static_cast<uint32_t>(cat1) != norad) continue;
		if (l1[68] < '0' || l1[68] > '9' || checksum(l1) != l1[68] - '0') REFUSE("TLE: the checksum of line 1 (line %zu) is '%c', its digits give %d", i, l1[68], checksum(l1));
		if (l2[68] < '0' || l2[68] > '9' || checksum(l2) != l2[68] - '0') REFUSE("TLE: the checksum of line 2 (line %zu) is '%c', its digits give %d", i + 1, l2[68], checksum(l2));
		double yy, doy, inc, raan, ecc, argp, ma, mm;
		if (!field(l1, 19, 20, "", yy) || !field(l1, 21, 32, "", doy) || !field(l2, 9, 16, "", inc) || !field(l2, 18, 25, "", raan) || !field(l2, 27, 33, "0.", ecc) ||
		    !field(l2, 35, 42, "", argp) || !field(l2, 44, 51, "", ma) || !field(l2, 53, 63, "", mm))
			REFUSE("TLE: a field of the set %.0f is not a number", cat1);
		if (!(doy >= 1.0 && doy < 367.0) || yy < 0) REFUSE("TLE: the epoch of the set %.0f is day %g of year %g", cat1, doy, yy);
		if (!(inc >= 0.0 && inc <= 180.0)) REFUSE("TLE: the inclination is %g degrees (0 .. 180)", inc);
		if (!(ecc >= 0.0 && ecc < 1.0)) REFUSE("TLE: the eccentricity is %g (below 1)", ecc);
		if (!(mm >= 0.5 && mm <= 20.0)) REFUSE("TLE: the mean motion is %g revolutions per day (0.5 .. 20)", mm);
		const int64_t year = static_cast<int64_t>(yy) + (yy < 57 ? 2000 : 1900);
		const double whole = floor(doy);
		memset(tle, 0, sizeof *tle);
		tle->norad = static_cast<uint32_t>(cat1);
		tle->epoch_day = static_cast<int32_t>(days_from_civil(year, 1, 1) + static_cast<int64_t>(whole) - 1);
		tle->epoch_sec = (doy - whole) * 86400.0;
		tle->inclination_deg = inc; tle->raan_deg = raan; tle->eccentricity = ecc; tle->argp_deg = argp; tle->mean_anomaly_deg = ma; tle->mean_motion = mm;
		return MDEMOD_OK;
	}
	if (any) REFUSE("TLE: no element set with the catalogue number %u", norad);
	REFUSE("TLE: no element set (a line 1 and a line 2 of 69 characters each)");
} MDEMOD_API_CATCH

int
mdemod_map_fit_time(const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const mdemod_map_opts *opts, mdemod_map_timing *timing)
try { MDEMOD_API_ENTER
	mdemod_map_opts o;
	const int rc = map_settings(opts, o);
	if (rc) return rc;
	if (!timing) REFUSE("mdemod_map_fit_time: the line times are needed");
	if (n_desc && (!place || !sinfo)) REFUSE("mdemod_map_fit_time: the placements and the reports of the packets are needed");
	struct Point { uint32_t row; double s; };
	std::vector<Point> pts;
	for (uint64_t i = 0; i < n_desc; i++) {
		if (place[i].channel < 0) continue;
		double s = static_cast<double>(sinfo[i].ms) / 1000.0 + static_cast<double>(sinfo[i].us) / 1.0e6;
		if (!pts.empty()) {
			if (s - pts[0].s > 43200.0) s -= 86400.0;
			else if (s - pts[0].s < -43200.0) s += 86400.0;
		}
		pts.push_back({ place[i].row, s });
	}
	if (pts.empty()) REFUSE("map: no placed packet, so no time stamp to fit the line times to");
	/* each row's first placed packet, the rows ascending */
	std::vector<Point> first(pts);
	std::stable_sort(first.begin(), first.end(), [](const Point &a, const Point &b) { return a.row < b.row; });
	first.erase(std::unique(first.begin(), first.end(), [](const Point &a, const Point &b) { return a.row == b.row; }), first.end());
	double period = o.row_period;
	if (first.size() >= 2) {
		std::vector<double> ratio;
		for (size_t k = 1; k < first.size(); k++) ratio.push_back((first[k].s - first[k - 1].s) / static_cast<double>(first[k].row - first[k - 1].row));
		period = median(ratio);
		if (!(period >= 0.1 && period <= 10.0)) REFUSE("map: the stamps give a row period of %g s (0.1 .. 10): they are no onboard times", period);
	}
	std::vector<double> rest;
	for (const Point &p : pts) rest.push_back(p.s - static_cast<double>(p.row) * period);
	timing->row_period = period;
	const double s0 = median(rest);
	timing->s0 = s0 - 86400.0 * floor(s0 / 86400.0);
	timing->date = o.date;
	timing->rows_fit = static_cast<uint32_t>(first.size());
	timing->placed = static_cast<uint32_t>(pts.size() > 0xffffffffu ? 0xffffffffu : pts.size());
	timing->lines = 8 * (first.back().row + 1);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_map_date(const mdemod_map_tle *orbit, const mdemod_map_timing *timing, const mdemod_map_opts *opts, int32_t *date)
try { MDEMOD_API_ENTER
	mdemod_map_opts o;
	int rc = map_settings(opts, o);
	if (rc || (rc = check_tle("mdemod_map_date", orbit)) || (rc = check_timing("mdemod_map_date", timing))) return rc;
	if (!date) REFUSE("mdemod_map_date: the date is needed");
	return resolve_date(*orbit, *timing, o, timing->lines, *date);
} MDEMOD_API_CATCH

int
mdemod_map_geolocate(const mdemod_map_tle *orbit, const mdemod_map_timing *timing, const mdemod_map_opts *opts, const double *y, const double *x, uint64_t n,
                     double *lat, double *lon)
try { MDEMOD_API_ENTER
	mdemod_map_opts o;
	int rc = map_settings(opts, o);
	if (rc || (rc = check_tle("mdemod_map_geolocate", orbit)) || (rc = check_timing("mdemod_map_geolocate", timing))) return rc;
	if (n && (!y || !x || !lat || !lon)) REFUSE("mdemod_map_geolocate: the pixels and the coordinates are needed");
	int32_t date;
	if ((rc = resolve_date(*orbit, *timing, o, timing->lines, date))) return rc;
	const Pass p = pass_of(*orbit, *timing, o, date);
	for (uint64_t k = 0; k < n; k++)
		if (!std::isfinite(y[k]) || !std::isfinite(x[k]) || fabs(y[k]) > 1.0e7 || !forward(p, y[k], x[k], lat[k], lon[k])) lat[k] = lon[k] = NAN;
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_map_grid(const mdemod_map_tle *orbit, const mdemod_map_timing *timing, const mdemod_map_opts *opts, uint32_t lines, mdemod_map_nodes *grid)
try { MDEMOD_API_ENTER
	mdemod_map_opts o;
	int rc = map_settings(opts, o);
	if (rc || (rc = map_check_pass("mdemod_map_grid", orbit, timing))) return rc;
	if (!grid) REFUSE("mdemod_map_grid: the grid is needed");
	memset(grid, 0, sizeof *grid);
	if ((rc = map_check_lines(lines))) return rc;
	int32_t date;
	if ((rc = map_resolve_date(*orbit, *timing, o, lines, date))) return rc;
	double lon_c;
	MapRange range;
	MapFrame f;
	if ((rc = map_swath_centre(*orbit, *timing, o, date, lines, lon_c)) || (rc = map_swath_border(*orbit, *timing, o, date, lines, lon_c, range)) ||
	    (rc = map_frame(o, range, lon_c, f)))
		return rc;
	grid->width = f.width; grid->height = f.height;
	grid->sx = static_cast<uint32_t>(f.sx); grid->sy = f.sy;
	grid->lat_top = f.lat_top;
	grid->lon_left = map_frame_lon_left(f);
	grid->date = date;
	grid->node_rows = map_node_count(grid->height); grid->node_cols = map_node_count(grid->width);
	const size_t count = static_cast<size_t>(grid->node_rows) * grid->node_cols;
	grid->nodes = static_cast<int32_t *>(malloc(count * 2 * sizeof(int32_t)));
	if (!grid->nodes) { memset(grid, 0, sizeof *grid); return MDEMOD_ERR_NOMEM; }
	map_nodes_on(*orbit, *timing, o, date, lines, f, grid->nodes);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_map_model_warp(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes, const uint8_t *lut,
                      const int32_t *nodes, uint32_t width, uint32_t height, uint8_t *out, uint8_t *valid)
try { MDEMOD_API_ENTER
	int rc = map_check_warp("mdemod_map_model_warp", rows, select, planes, width, height);
	if (rc) return rc;
	if (!rows || !height) return MDEMOD_OK;
	if ((rc = pic_check_slots("mdemod_map_model_warp", image, filled, select, planes))) return rc;
	if (!lut || !nodes || !out) REFUSE("mdemod_map_model_warp: the tables, the nodes and the picture are needed");
	model_warp(image, filled, rows, select, planes, lut, nodes, width, height, out, valid);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_map_model_host(const mdemod_map_opts *opts, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                      const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select, uint32_t planes,
                      mdemod_map_result *out)
try { MDEMOD_API_ENTER
	mdemod_map_opts o;
	int rc = map_settings(opts, o);
	if (rc) return rc;
	if ((rc = map_check_compose("mdemod_map_model_host", tle, image, filled, rows, place, sinfo, n_desc, select, planes, out))) return rc;
	ModelBackend model;
	return map_compose_bands(o, tle, image, filled, rows, place, sinfo, n_desc, select, planes, out, model);
} MDEMOD_API_CATCH

} /* extern "C" */
