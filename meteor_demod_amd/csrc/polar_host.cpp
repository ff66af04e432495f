/*
 * polar_host.cpp — host side of the polar layer (include/meteor_demod_amd_polar.h): the projection (csrc/polar_proj.h, shared with
 * the device), the frame from the border samples of the passes, the solver constants of each pass and its nodes through the map
 * layer's solver (csrc/map_host.h: map_nodes_at, one copy of the Newton), the graticule, the vertices, the world file and the .prj
 * text, and the whole picture out of the mosaic layer's tables and bands (csrc/mosaic_host.h: mosaic_bands_on) with the mosaic
 * layer's model blend in the kernel's place (mdemod_polar_model_host).  Free of the GPU runtime.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "polar_host.h"
#include "mdemod_internal_api.h"

namespace {

inline double wrap180(double d) { d = fmod(d, 360.0); return d >= 180.0 ? d - 360.0 : d < -180.0 ? d + 360.0 : d; }

mdemod_map_opts
map_opts_of(const mdemod_polar_opts &o, int32_t date)
{
	mdemod_map_opts m;
	mdemod_map_default_opts(&m);
	m.scan_deg = o.scan_deg; m.time_offset = o.time_offset; m.row_period = o.row_period;
	m.side = o.side; m.date = date; m.stretch = o.stretch ? 1 : 0; m.clip_low = o.clip_low; m.clip_high = o.clip_high; m.piece_lines = o.piece_lines;
	return m;
}

mdemod_mosaic_opts
mosaic_opts_of(const mdemod_polar_opts &o)
{
	mdemod_mosaic_opts m;
	mdemod_mosaic_default_opts(&m);
	m.scan_deg = o.scan_deg; m.time_offset = o.time_offset; m.row_period = o.row_period; m.side = o.side; m.stretch = o.stretch;
	m.clip_low = o.clip_low; m.clip_high = o.clip_high; m.piece_lines = o.piece_lines; m.blend = o.blend;
	return m;
}

/* fixed point of the overlay layer: pixel centres at multiples of 256 */
inline double fixed_of(double pixels) { return 256.0 * (pixels - 0.5); }

inline int32_t
saturated(double v)
{
	const double r = floor(v + 0.5);
	return !(r > -2147483648.0) ? INT32_MIN : r > 2147483647.0 ? INT32_MAX : static_cast<int32_t>(r);
}

int
check_proj(const char *who, int32_t pole, double lat_ts_deg, double lon0_deg)
{
	if (pole != 1 && pole != -1) REFUSE("%s: the pole is %d (1: north, -1: south)", who, pole);
	if (!(fabs(lat_ts_deg) > 0.0 && fabs(lat_ts_deg) <= 90.0)) REFUSE("%s: the standard parallel is %g degrees (0 < .. <= 90)", who, lat_ts_deg);
	if (!(fabs(lon0_deg) <= 360.0)) REFUSE("%s: the central meridian is %g degrees (-360 .. 360)", who, lon0_deg);
	return MDEMOD_OK;
}

PolarProj
proj_of(int32_t pole, double lat_ts_deg, double lon0_deg)
{
	PolarProj p;
	p.pole = pole; p.lon0 = lon0_deg * POLAR_RAD; p.scale = polar_scale(fabs(lat_ts_deg) * POLAR_RAD);
	return p;
}

/* one polyline being written */
struct Points {
	std::vector<int32_t> x, y;
	std::vector<uint32_t> first;
	size_t open = 0;
	void close() { if (x.size() - open >= 2) first.push_back(static_cast<uint32_t>(open)); else { x.resize(open); y.resize(open); } open = x.size(); }
};

struct Projector {
	const mdemod_polar_frame &f;
	PolarProj p;
	explicit Projector(const mdemod_polar_frame &frame) : f(frame), p(polar_proj_of(frame)) {}
	/* degrees to fixed point, unrounded */
	void at(double lon, double lat, double &X, double &Y) const
	{
		double E, N;
		polar_forward(p, lat * POLAR_RAD, lon * POLAR_RAD, E, N);
		X = fixed_of((E - f.e_left) / f.res);
		Y = fixed_of((f.n_top - N) / f.res);
	}
	/* the vertices strictly between A and B */
	void between(double lonA, double latA, double XA, double YA, double lonB, double latB, double XB, double YB, int level, Points &out) const
	{
		if (level >= MDEMOD_POLAR_MAX_LEVELS) return;
		const double lonM = 0.5 * (lonA + lonB), latM = 0.5 * (latA + latB);
		double XM, YM;
		at(lonM, latM, XM, YM);
		if (hypot(XM - 0.5 * (XA + XB), YM - 0.5 * (YA + YB)) <= MDEMOD_POLAR_CHORD_TOP) return;
		between(lonA, latA, XA, YA, lonM, latM, XM, YM, level + 1, out);
		out.x.push_back(saturated(XM)); out.y.push_back(saturated(YM));
		between(lonM, latM, XM, YM, lonB, latB, XB, YB, level + 1, out);
	}
};

template <typename T>
T *
given_out(const std::vector<T> &v)
{
	T *p = static_cast<T *>(malloc((v.size() ? v.size() : 1) * sizeof(T)));
	if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
	return p;
}

int
put_text(const char *who, const std::string &s, char *text, uint64_t size)
{
	if (!text) REFUSE("%s: the text is needed", who);
	if (s.size() + 1 > size) REFUSE("%s: the text takes %zu bytes, %llu are there", who, s.size() + 1, static_cast<unsigned long long>(size));
	memcpy(text, s.c_str(), s.size() + 1);
	return MDEMOD_OK;
}

} /* namespace */

int
polar_settings(const mdemod_polar_opts *opts, mdemod_polar_opts &out)
{
	mdemod_polar_default_opts(&out);
	if (opts) out = *opts;
	/* the fields shared with the mosaic and map layers are checked there, with their texts */
	const mdemod_mosaic_opts m = mosaic_opts_of(out);
	mdemod_mosaic_opts done;
	const int rc = mosaic_settings(&m, done);
	if (rc) return rc;
	if (!(out.metres_per_pixel >= MDEMOD_POLAR_MIN_RES && out.metres_per_pixel <= MDEMOD_POLAR_MAX_RES))
		REFUSE("polar: the resolution is %g metres per pixel (100 .. 100000)", out.metres_per_pixel);
	if (out.pole != 0 && out.pole != 1 && out.pole != -1) REFUSE("polar: the pole is %d (0: from the pass, 1: north, -1: south)", out.pole);
	if (!(out.lat_ts_deg > 0.0 && out.lat_ts_deg <= 90.0)) REFUSE("polar: the standard parallel is %g degrees (a magnitude: 0 < .. <= 90)", out.lat_ts_deg);
	if (!std::isnan(out.lon0_deg) && !(fabs(out.lon0_deg) <= 360.0)) REFUSE("polar: the central meridian is %g degrees (-360 .. 360, or NaN for the pass's own)", out.lon0_deg);
	if (out.nodes_on_host > 1) REFUSE("polar: nodes_on_host is %u (0 or 1)", out.nodes_on_host);
	if (out.projection != MDEMOD_POLAR_STEREOGRAPHIC) REFUSE("polar: projection %u is not there (0: polar stereographic)", out.projection);
	out.piece_lines = done.piece_lines;
	return MDEMOD_OK;
}

int
polar_check_frame(const char *who, const mdemod_polar_frame *f)
{
	if (!f) REFUSE("%s: the frame is needed", who);
	if (f->projection != MDEMOD_POLAR_STEREOGRAPHIC) REFUSE("%s: projection %u is not there (0: polar stereographic)", who, f->projection);
	if (!f->width || f->width > MDEMOD_POLAR_MAX_WIDTH) REFUSE("%s: the width is %u (1 .. 8192)", who, f->width);
	if (!f->height || f->height > MDEMOD_POLAR_MAX_HEIGHT) REFUSE("%s: the height is %u (1 .. 16384)", who, f->height);
	if (f->node_rows != map_node_count(f->height) || f->node_cols != map_node_count(f->width))
		REFUSE("%s: %u x %u nodes do not go with %u x %u pixels (%u x %u)", who, f->node_cols, f->node_rows, f->width, f->height, map_node_count(f->width), map_node_count(f->height));
	if (!(f->res >= MDEMOD_POLAR_MIN_RES && f->res <= MDEMOD_POLAR_MAX_RES)) REFUSE("%s: the resolution is %g metres per pixel (100 .. 100000)", who, f->res);
	if (!(fabs(f->e_left) <= 1.0e9 && fabs(f->n_top) <= 1.0e9)) REFUSE("%s: the corner stands at %g, %g metres", who, f->e_left, f->n_top);
	return check_proj(who, f->pole, f->lat_ts_deg, f->lon0_deg);
}

PolarProj
polar_proj_of(const mdemod_polar_frame &f)
{
	return proj_of(f.pole, f.lat_ts_deg, f.lon0_deg);
}

int
polar_check_compose(const char *who, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes, mdemod_polar_result *out)
{
	int rc;
	if (!out) REFUSE("%s: the result is needed", who);
	if (!n) REFUSE("%s: no pass: a polar picture takes 1 .. 8", who);
	if (n > POLAR_MAX) REFUSE("%s: %u passes are more than a polar picture takes (1 .. 8)", who, n);
	if (!passes) REFUSE("%s: the passes are needed", who);
	if ((rc = pic_check_select(who, 0, select, planes))) return rc;
	for (uint32_t k = 0; k < n; k++) {
		const mdemod_polar_pass &p = passes[k];
		if (!p.tle_text) REFUSE("%s: the element set of pass %u is needed", who, k);
		if (!p.rows) REFUSE("%s: pass %u has no strip rows: it cannot be put on a map", who, k);
		if (p.rows > MDEMOD_MAP_MAX_ROWS) REFUSE("%s: the %u strip rows of pass %u are more than a map takes (8192)", who, p.rows, k);
		if ((rc = pic_check_slots(who, p.image, p.filled, select, planes))) return rc;
		if (p.n_desc && (!p.place || !p.sinfo)) REFUSE("%s: the placements and the reports of the packets of pass %u are needed", who, k);
	}
	return MDEMOD_OK;
}

int
polar_grid_make(const char *who, const mdemod_polar_opts &o, const mdemod_polar_pass *passes, uint32_t n, const mdemod_polar_frame *given, bool host_nodes,
                mdemod_polar_nodes *grid)
{
	int rc;
	memset(grid, 0, sizeof *grid);
	if (!n) REFUSE("%s: no pass: a polar picture takes 1 .. 8", who);
	if (n > POLAR_MAX) REFUSE("%s: %u passes are more than a polar picture takes (1 .. 8)", who, n);
	if (!passes) REFUSE("%s: the passes are needed", who);
	if (given && (rc = polar_check_frame(who, given))) return rc;
	mdemod_map_tle tle[POLAR_MAX];
	mdemod_map_timing tm[POLAR_MAX];
	mdemod_map_opts mo[POLAR_MAX];
	int32_t date[POLAR_MAX];
	for (uint32_t k = 0; k < n; k++) {
		const mdemod_polar_pass &p = passes[k];
		if (!p.tle_text) REFUSE("%s: the element set of pass %u is needed", who, k);
		if (p.n_desc && (!p.place || !p.sinfo)) REFUSE("%s: the placements and the reports of the packets of pass %u are needed", who, k);
		if (p.date != MDEMOD_POLAR_DATE_AUTO && (p.date < -1000000 || p.date > 1000000)) REFUSE("polar: the date of pass %u is day %d since 1970 (or auto)", k, p.date);
		mo[k] = map_opts_of(o, p.date);
		if ((rc = mdemod_map_parse_tle(p.tle_text, p.norad, &tle[k])) || (rc = mdemod_map_fit_time(p.place, p.sinfo, p.n_desc, &mo[k], &tm[k])) ||
		    (rc = map_check_pass(who, &tle[k], &tm[k])) || (rc = map_check_lines(8 * p.rows)) || (rc = map_resolve_date(tle[k], tm[k], mo[k], 8 * p.rows, date[k])))
			return rc;
	}
	mdemod_polar_frame &f = grid->frame;
	if (given) {
		f = *given;
		f.lon0_deg = wrap180(f.lon0_deg);
	} else {
		double lat_c, lon_c;
		if (!map_forward(tle[0], tm[0], mo[0], date[0], (8 * passes[0].rows - 1) / 2.0, 783.5, lat_c, lon_c)) REFUSE("polar: the middle of the picture does not see the Earth");
		f.projection = MDEMOD_POLAR_STEREOGRAPHIC;
		f.pole = o.pole ? o.pole : lat_c < 0.0 ? -1 : 1;
		f.lat_ts_deg = f.pole * o.lat_ts_deg;
		f.lon0_deg = wrap180(std::isnan(o.lon0_deg) ? floor(lon_c + 0.5) : o.lon0_deg);
		f.res = o.metres_per_pixel;
		const PolarProj proj = polar_proj_of(f);
		double e_lo = 1.0e30, e_hi = -1.0e30, n_lo = 1.0e30, n_hi = -1.0e30;
		for (uint32_t k = 0; k < n; k++) {
			const uint32_t lines = 8 * passes[k].rows;
			auto sample = [&](double y, double x) -> int {
				double lat, lon, E, N;
				if (!map_forward(tle[k], tm[k], mo[k], date[k], y, x, lat, lon))
					REFUSE("polar: line %.0f, column %.0f on the border of the swath does not see the Earth (scan angle %g)", y, x, o.scan_deg);
				if (!(lat * f.pole > 0.0))
					REFUSE("polar: line %.0f, column %.0f of pass %u lies at %.2f degrees of latitude, in the other hemisphere than the %s pole: such a pass wants the "
					       "latitude / longitude grid", y, x, k, lat, f.pole > 0 ? "north" : "south");
				polar_forward(proj, lat * POLAR_RAD, lon * POLAR_RAD, E, N);
				e_lo = std::min(e_lo, E); e_hi = std::max(e_hi, E); n_lo = std::min(n_lo, N); n_hi = std::max(n_hi, N);
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
		}
		const double res = f.res;
		f.e_left = floor(e_lo / res) * res;
		f.n_top = ceil(n_hi / res) * res;
		const double w = std::max(4.0, ceil(ceil((e_hi - f.e_left) / res) / 4.0) * 4.0), h = std::max(1.0, ceil((f.n_top - n_lo) / res));
		if (w > MDEMOD_POLAR_MAX_WIDTH || h > MDEMOD_POLAR_MAX_HEIGHT) {
			const double fit = ceil(res * std::max((w + 8.0) / MDEMOD_POLAR_MAX_WIDTH, (h + 2.0) / MDEMOD_POLAR_MAX_HEIGHT));
			REFUSE("polar: %.0f x %.0f pixels at %g metres per pixel are more than a picture takes (8192 x 16384): a resolution of %.0f fits", w, h, res,
			       std::min(fit, MDEMOD_POLAR_MAX_RES));
		}
		f.width = static_cast<uint32_t>(w); f.height = static_cast<uint32_t>(h);
		f.node_rows = map_node_count(f.height); f.node_cols = map_node_count(f.width);
	}
	grid->n = n;
	const size_t count = static_cast<size_t>(f.node_rows) * f.node_cols;
	std::vector<double> lat, lon;
	if (host_nodes) {
		const PolarProj proj = polar_proj_of(f);
		lat.resize(count); lon.resize(count);
		for (uint32_t a = 0; a < f.node_rows; a++)
			for (uint32_t b = 0; b < f.node_cols; b++) {
				double phi, lam;
				polar_inverse(proj, f.e_left + (MAP_STEP * b + 0.5) * f.res, f.n_top - (MAP_STEP * a + 0.5) * f.res, phi, lam);
				lat[static_cast<size_t>(a) * f.node_cols + b] = phi / POLAR_RAD;
				lon[static_cast<size_t>(a) * f.node_cols + b] = lam / POLAR_RAD;
			}
	}
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t lines = 8 * passes[k].rows;
		MapSolver s;
		map_solver_of(tle[k], tm[k], mo[k], date[k], lines, s);
		mdemod_polar_solver &d = grid->solver[k];
		d.a = s.a; d.cos_i = s.ci; d.sin_i = s.si; d.raan = s.raan_t0; d.u = s.u_t0; d.g = s.g_t0; d.raan_rate = s.raan_dot; d.u_rate = s.u_dot; d.g_rate = s.g_dot;
		d.table_t0 = s.table_t0; d.sec_lo = s.sec_lo; d.sec_hi = s.sec_hi; d.theta_max = s.theta_max; d.s0 = s.s0; d.line_period = s.line_period;
		d.time_offset = s.offset; d.step = s.step; d.side = s.side;
		d.table_n = static_cast<uint32_t>(s.table.size() / 3);
		d.table = given_out(s.table);
		grid->nodes[k] = static_cast<int32_t *>(malloc(count * 2 * sizeof(int32_t)));
		if (!d.table || !grid->nodes[k]) { mdemod_polar_grid_free(grid); return MDEMOD_ERR_NOMEM; }
		if (host_nodes) map_nodes_at(tle[k], tm[k], mo[k], date[k], lines, lat.data(), lon.data(), count, grid->nodes[k]);
		else for (size_t i = 0; i < 2 * count; i++) grid->nodes[k][i] = MDEMOD_POLAR_NO_NODE;
		mdemod_polar_timing &t = grid->timing[k];
		t.row_period = tm[k].row_period; t.s0 = tm[k].s0; t.date = date[k]; t.rows_fit = tm[k].rows_fit; t.placed = tm[k].placed; t.lines = lines;
	}
	return MDEMOD_OK;
}

int
polar_compose(const mdemod_polar_opts &o, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes, mdemod_polar_nodes &grid,
              mdemod_polar_result *out, MosaicBackend &backend)
{
	const mdemod_polar_frame &f = grid.frame;
	if (f.width % 4) REFUSE("polar: the width is %u (a picture's is a multiple of 4)", f.width);
	mdemod_mosaic_nodes mg;
	memset(&mg, 0, sizeof mg);
	mg.width = f.width; mg.height = f.height; mg.node_rows = f.node_rows; mg.node_cols = f.node_cols; mg.n = n;
	std::vector<mdemod_mosaic_pass> mp(n);
	for (uint32_t k = 0; k < n; k++) {
		const mdemod_polar_timing &t = grid.timing[k];
		mg.timing[k].row_period = t.row_period; mg.timing[k].s0 = t.s0; mg.timing[k].date = t.date; mg.timing[k].rows_fit = t.rows_fit;
		mg.timing[k].placed = t.placed; mg.timing[k].lines = t.lines;
		mg.nodes[k] = grid.nodes[k];
		const mdemod_polar_pass &p = passes[k];
		mdemod_mosaic_pass &q = mp[k];
		q.tle_text = p.tle_text; q.norad = p.norad; q.date = p.date; q.rows = p.rows; q.reserved = 0; q.place = p.place; q.sinfo = p.sinfo; q.n_desc = p.n_desc;
		for (int s = 0; s < 3; s++) { q.image[s] = p.image[s]; q.filled[s] = p.filled[s]; }
	}
	mdemod_mosaic_result mr;
	const int rc = mosaic_bands_on(mosaic_opts_of(o), mp.data(), n, select, planes, mg, &mr, backend);
	if (rc) return rc;
	out->frame = f; out->planes = planes; out->n = n; out->blend = o.blend; out->nodes_on_host = o.nodes_on_host;
	for (uint32_t k = 0; k < n; k++) {
		out->timing[k] = grid.timing[k];
		out->utc0[k] = mr.utc0[k];
		out->covered[k] = mr.covered[k];
		for (int p = 0; p < 3; p++) { out->lo[k][p] = mr.lo[k][p]; out->hi[k][p] = mr.hi[k][p]; }
		out->nodes[k] = grid.nodes[k];
		grid.nodes[k] = nullptr;
	}
	out->valid_pixels = mr.valid_pixels; out->overlap_pixels = mr.overlap_pixels;
	out->pixels = mr.pixels; out->valid = mr.valid; out->cover = mr.cover;
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_polar_default_opts(mdemod_polar_opts *opts)
{
	if (!opts) return;
	memset(opts, 0, sizeof *opts);
	opts->scan_deg = 110.0;
	opts->time_offset = 10800.0;
	opts->row_period = 8.0 / 6.5;
	opts->metres_per_pixel = 1000.0;
	opts->lat_ts_deg = 70.0;
	opts->lon0_deg = NAN;
	opts->side = 1;
	opts->pole = 0;
	opts->stretch = 1;
	opts->clip_low = 5;
	opts->clip_high = 5;
	opts->piece_lines = 0;
	opts->blend = MDEMOD_POLAR_FEATHER;
	opts->nodes_on_host = 0;
	opts->projection = MDEMOD_POLAR_STEREOGRAPHIC;
}

void
mdemod_polar_grid_free(mdemod_polar_nodes *grid)
{
	if (!grid) return;
	for (int k = 0; k < POLAR_MAX; k++) { free(grid->nodes[k]); free(grid->solver[k].table); }
	memset(grid, 0, sizeof *grid);
}

void
mdemod_polar_free(mdemod_polar_result *out)
{
	if (!out) return;
	free(out->pixels); free(out->valid); free(out->cover);
	for (int k = 0; k < POLAR_MAX; k++) free(out->nodes[k]);
	memset(out, 0, sizeof *out);
}

void
mdemod_polar_lines_free(mdemod_polar_lines *lines)
{
	if (!lines) return;
	free(lines->lon); free(lines->lat); free(lines->first);
	memset(lines, 0, sizeof *lines);
}

void
mdemod_polar_points_free(mdemod_polar_points *points)
{
	if (!points) return;
	free(points->x); free(points->y); free(points->first);
	memset(points, 0, sizeof *points);
}

int
mdemod_polar_forward(int32_t pole, double lat_ts_deg, double lon0_deg, const double *lat, const double *lon, uint64_t n, double *e, double *north)
try { MDEMOD_API_ENTER
	const int rc = check_proj("mdemod_polar_forward", pole, lat_ts_deg, lon0_deg);
	if (rc) return rc;
	if (n && (!lat || !lon || !e || !north)) REFUSE("mdemod_polar_forward: the points and the coordinates are needed");
	const PolarProj p = proj_of(pole, lat_ts_deg, lon0_deg);
	for (uint64_t k = 0; k < n; k++) {
		if (!(fabs(lat[k]) <= 90.0) || !std::isfinite(lon[k])) { e[k] = north[k] = NAN; continue; }
		polar_forward(p, lat[k] * POLAR_RAD, lon[k] * POLAR_RAD, e[k], north[k]);
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_polar_inverse(int32_t pole, double lat_ts_deg, double lon0_deg, const double *e, const double *north, uint64_t n, double *lat, double *lon)
try { MDEMOD_API_ENTER
	const int rc = check_proj("mdemod_polar_inverse", pole, lat_ts_deg, lon0_deg);
	if (rc) return rc;
	if (n && (!lat || !lon || !e || !north)) REFUSE("mdemod_polar_inverse: the points and the coordinates are needed");
	const PolarProj p = proj_of(pole, lat_ts_deg, lon0_deg);
	for (uint64_t k = 0; k < n; k++) {
		if (!std::isfinite(e[k]) || !std::isfinite(north[k])) { lat[k] = lon[k] = NAN; continue; }
		double phi, lam;
		polar_inverse(p, e[k], north[k], phi, lam);
		lat[k] = phi / POLAR_RAD;
		lon[k] = wrap180(lam / POLAR_RAD);
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_polar_grid(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, mdemod_polar_nodes *grid)
try { MDEMOD_API_ENTER
	if (!grid) REFUSE("mdemod_polar_grid: the grid is needed");
	memset(grid, 0, sizeof *grid);
	mdemod_polar_opts o;
	const int rc = polar_settings(opts, o);
	if (rc) return rc;
	return polar_grid_make("mdemod_polar_grid", o, passes, n, nullptr, true, grid);
} MDEMOD_API_CATCH

int
mdemod_polar_model_nodes(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, const mdemod_polar_frame *frame, mdemod_polar_nodes *grid)
try { MDEMOD_API_ENTER
	if (!grid) REFUSE("mdemod_polar_model_nodes: the grid is needed");
	memset(grid, 0, sizeof *grid);
	mdemod_polar_opts o;
	const int rc = polar_settings(opts, o);
	if (rc) return rc;
	if (!frame) REFUSE("mdemod_polar_model_nodes: the frame is needed");
	return polar_grid_make("mdemod_polar_model_nodes", o, passes, n, frame, true, grid);
} MDEMOD_API_CATCH

int
mdemod_polar_model_host(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                        mdemod_polar_result *out)
try { MDEMOD_API_ENTER
	if (out) memset(out, 0, sizeof *out);                                      /* (a refusal leaves nothing to free) */
	mdemod_polar_opts o;
	int rc = polar_settings(opts, o);
	if (rc) return rc;
	if ((rc = polar_check_compose("mdemod_polar_model_host", passes, n, select, planes, out))) return rc;
	mdemod_polar_nodes grid;
	if ((rc = polar_grid_make("mdemod_polar_model_host", o, passes, n, nullptr, true, &grid))) return rc;
	struct Keep { mdemod_polar_nodes *g; ~Keep() { mdemod_polar_grid_free(g); } } keep{ &grid };
	o.nodes_on_host = 1;
	return polar_compose(o, passes, n, select, planes, grid, out, *mosaic_model_backend());
} MDEMOD_API_CATCH

int
mdemod_polar_graticule(const mdemod_polar_frame *frame, double step_deg, mdemod_polar_lines *lines)
try { MDEMOD_API_ENTER
	if (!lines) REFUSE("mdemod_polar_graticule: the lines are needed");
	memset(lines, 0, sizeof *lines);
	const int rc = polar_check_frame("mdemod_polar_graticule", frame);
	if (rc) return rc;
	if (!(step_deg == 0.0 || (step_deg >= 0.1 && step_deg <= 90.0))) REFUSE("mdemod_polar_graticule: the step is %g degrees (0: automatic, or 0.1 .. 90)", step_deg);
	const mdemod_polar_frame &f = *frame;
	const PolarProj p = polar_proj_of(f);
	const double right = f.e_left + f.width * f.res, bottom = f.n_top - f.height * f.res;
	const bool pole_inside = f.e_left <= 0.0 && right >= 0.0 && bottom <= 0.0 && f.n_top >= 0.0;
	/* the extent: the edge pixels every 16 pixels, inverted; |lat| as `a`, longitudes relative to that of the picture's middle */
	double phi, lam, lon_mid;
	polar_inverse(p, 0.5 * (f.e_left + right), 0.5 * (f.n_top + bottom), phi, lam);
	lon_mid = lam / POLAR_RAD;
	double a_lo = 90.0, a_hi = 0.0, d_lo = 0.0, d_hi = 0.0;
	auto edge = [&](uint32_t i, uint32_t j) {
		polar_inverse(p, f.e_left + (j + 0.5) * f.res, f.n_top - (i + 0.5) * f.res, phi, lam);
		const double a = fabs(phi) / POLAR_RAD, d = wrap180(lam / POLAR_RAD - lon_mid);
		a_lo = std::min(a_lo, a); a_hi = std::max(a_hi, a); d_lo = std::min(d_lo, d); d_hi = std::max(d_hi, d);
	};
	for (uint32_t j = 0;; j = std::min(j + MAP_STEP, f.width - 1)) { edge(0, j); edge(f.height - 1, j); if (j == f.width - 1) break; }
	for (uint32_t i = 0;; i = std::min(i + MAP_STEP, f.height - 1)) { edge(i, 0); edge(i, f.width - 1); if (i == f.height - 1) break; }
	if (pole_inside) { a_hi = 90.0; d_lo = -180.0; d_hi = 180.0; lon_mid = f.lon0_deg; }
	double step = step_deg;
	if (step == 0.0) {
		const double mid = 0.5 * (a_lo + a_hi);
		step = 30.0;
		for (double s : { 1.0, 2.0, 5.0, 10.0, 15.0, 30.0 }) {
			const double hi = std::min(90.0, mid + s / 2.0), lo = hi - s;
			if (p.scale * (polar_t(lo * POLAR_RAD) - polar_t(hi * POLAR_RAD)) / f.res >= 128.0) { step = s; break; }
		}
	}
	std::vector<double> lon, lat;
	std::vector<uint32_t> first;
	/* (kept within +-360 degrees, where the vertices take them: the span is a turn at most) */
	const double span = d_hi - d_lo, from = wrap180(lon_mid + d_lo), lon_lo = from + span > 360.0 ? from - 360.0 : from, lon_hi = lon_lo + span;
	const double every = std::min(step, 5.0);
	/* parallels: vertices at lon_lo, the multiples of `every` between, lon_hi */
	for (double k = ceil(a_lo / step); k * step <= a_hi && k * step < 90.0; k += 1.0) {
		if (k * step <= 0.0) continue;
		first.push_back(static_cast<uint32_t>(lon.size()));
		lon.push_back(lon_lo); lat.push_back(f.pole * k * step);
		for (double m = floor(lon_lo / every) + 1.0; m * every < lon_hi; m += 1.0) { lon.push_back(m * every); lat.push_back(f.pole * k * step); }
		lon.push_back(lon_hi); lat.push_back(f.pole * k * step);
	}
	/* meridians: from the lowest latitude of the extent to the highest (the pole itself where it lies inside) */
	if (a_hi > a_lo)
		for (double m = ceil(lon_lo / step); m * step <= lon_hi && (!pole_inside || m * step < lon_hi); m += 1.0) {
			first.push_back(static_cast<uint32_t>(lon.size()));
			lon.push_back(wrap180(m * step)); lat.push_back(f.pole * std::max(a_lo, 1.0e-6));
			lon.push_back(wrap180(m * step)); lat.push_back(f.pole * a_hi);
		}
	first.push_back(static_cast<uint32_t>(lon.size()));
	lines->lon = given_out(lon); lines->lat = given_out(lat); lines->first = given_out(first);
	if (!lines->lon || !lines->lat || !lines->first) { mdemod_polar_lines_free(lines); return MDEMOD_ERR_NOMEM; }
	lines->n_lines = static_cast<uint32_t>(first.size() - 1); lines->n_points = static_cast<uint32_t>(lon.size());
	lines->step_deg = step;
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_polar_vertices(const mdemod_polar_frame *frame, const double *lon, const double *lat, const uint32_t *first, uint32_t n_lines, mdemod_polar_points *points)
try { MDEMOD_API_ENTER
	if (!points) REFUSE("mdemod_polar_vertices: the points are needed");
	memset(points, 0, sizeof *points);
	const int rc = polar_check_frame("mdemod_polar_vertices", frame);
	if (rc) return rc;
	if (n_lines && (!first || !lon || !lat)) REFUSE("mdemod_polar_vertices: the polylines are needed");
	for (uint32_t l = 0; l < n_lines; l++)
		if (first[l + 1] < first[l]) REFUSE("mdemod_polar_vertices: line %u ends before it begins", l);
	for (uint32_t k = n_lines ? first[0] : 0; n_lines && k < first[n_lines]; k++)
		if (!(fabs(lat[k]) <= 90.0) || !(fabs(lon[k]) <= 360.0)) REFUSE("mdemod_polar_vertices: vertex %u stands at %g, %g degrees", k, lon[k], lat[k]);
	const Projector pr(*frame);
	Points out;
	for (uint32_t l = 0; l < n_lines; l++) {
		bool have = false;
		double lonA = 0, latA = 0, XA = 0, YA = 0;
		for (uint32_t k = first[l]; k < first[l + 1]; k++) {
			if (!(lat[k] * frame->pole > 0.0)) { out.close(); have = false; continue; }        /* the other hemisphere: the line ends here */
			const double lonB = have ? lonA + wrap180(lon[k] - lonA) : lon[k], latB = lat[k];
			double XB, YB;
			pr.at(lonB, latB, XB, YB);
			if (have) pr.between(lonA, latA, XA, YA, lonB, latB, XB, YB, 0, out);
			out.x.push_back(saturated(XB)); out.y.push_back(saturated(YB));
			lonA = lonB; latA = latB; XA = XB; YA = YB; have = true;
		}
		out.close();
	}
	out.first.push_back(static_cast<uint32_t>(out.x.size()));
	points->x = given_out(out.x); points->y = given_out(out.y); points->first = given_out(out.first);
	if (!points->x || !points->y || !points->first) { mdemod_polar_points_free(points); return MDEMOD_ERR_NOMEM; }
	points->n_lines = static_cast<uint32_t>(out.first.size() - 1); points->n_points = static_cast<uint32_t>(out.x.size());
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_polar_world_file(const mdemod_polar_frame *frame, char *text, uint64_t size)
try { MDEMOD_API_ENTER
	const int rc = polar_check_frame("mdemod_polar_world_file", frame);
	if (rc) return rc;
	char buf[256];
	snprintf(buf, sizeof buf, "%.10g\n0\n0\n%.10g\n%.12g\n%.12g\n", frame->res, -frame->res, frame->e_left + frame->res / 2.0, frame->n_top - frame->res / 2.0);
	return put_text("mdemod_polar_world_file", buf, text, size);
} MDEMOD_API_CATCH

int
mdemod_polar_prj(const mdemod_polar_frame *frame, char *text, uint64_t size)
try { MDEMOD_API_ENTER
	const int rc = polar_check_frame("mdemod_polar_prj", frame);
	if (rc) return rc;
	char buf[768];
	snprintf(buf, sizeof buf, "PROJCS[\"WGS 84 / Polar Stereographic\",GEOGCS[\"WGS 84\",DATUM[\"WGS_1984\",SPHEROID[\"WGS 84\",6378137,298.257223563]],"
	         "PRIMEM[\"Greenwich\",0],UNIT[\"degree\",0.0174532925199433]],PROJECTION[\"Polar_Stereographic\"],PARAMETER[\"latitude_of_origin\",%.10g],"
	         "PARAMETER[\"central_meridian\",%.10g],PARAMETER[\"false_easting\",0],PARAMETER[\"false_northing\",0],UNIT[\"metre\",1]]\n",
	         frame->pole * fabs(frame->lat_ts_deg), frame->lon0_deg);
	return put_text("mdemod_polar_prj", buf, text, size);
} MDEMOD_API_CATCH

} /* extern "C" */
