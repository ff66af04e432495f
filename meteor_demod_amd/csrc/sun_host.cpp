/*
 * sun_host.cpp — host side of the sun layer (include/meteor_demod_amd_sun.h): the sun's position, the cosine of its zenith angle,
 * the gain nodes of a pass over the map layer's geolocation, the argument checks, and the host model of the kernel of csrc/sun.hip
 * (mdemod_sun_model_apply: the rule of the header as plain loops, one pixel after the other).  Free of the GPU runtime.
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "buffers.h"
#include "mdemod_internal_api.h"
#include "sun_host.h"

namespace {

constexpr double SUN_PI = 3.14159265358979323846, SUN_RAD = SUN_PI / 180.0;

/* the Earth-fixed unit vector to the sun */
void
sun_vector(int32_t date, double utc, double out[3])
{
	const double n = (static_cast<double>(date) - 10957.0) + (utc - 43200.0) / 86400.0;
	const double L = 280.460 + 0.9856474 * n, g = fmod(357.528 + 0.9856003 * n, 360.0) * SUN_RAD;
	const double lambda = fmod(L + 1.915 * sin(g) + 0.020 * sin(2.0 * g), 360.0) * SUN_RAD, eps = (23.439 - 0.0000004 * n) * SUN_RAD;
	const double x = cos(lambda), y = cos(eps) * sin(lambda), z = sin(eps) * sin(lambda);
	const double G = fmod(280.46061837 + 360.98564736629 * n, 360.0) * SUN_RAD, cg = cos(G), sg = sin(G);
	out[0] = x * cg + y * sg;
	out[1] = -x * sg + y * cg;
	out[2] = z;
}

double
cos_zenith(const double s[3], double lat, double lon)
{
	const double cl = cos(lat * SUN_RAD);
	return s[0] * cl * cos(lon * SUN_RAD) + s[1] * cl * sin(lon * SUN_RAD) + s[2] * sin(lat * SUN_RAD);
}

int
sun_settings(const char *who, const mdemod_sun_opts *opts, mdemod_sun_opts &o)
{
	if (opts) o = *opts;
	else mdemod_sun_default_opts(&o);
	if (!(o.limit_deg >= MDEMOD_SUN_MIN_LIMIT && o.limit_deg <= MDEMOD_SUN_MAX_LIMIT))
		REFUSE("%s: limit_deg %g is outside %g .. %g", who, o.limit_deg, MDEMOD_SUN_MIN_LIMIT, MDEMOD_SUN_MAX_LIMIT);
	if (!(o.ref_deg >= 0.0 && o.ref_deg <= MDEMOD_SUN_MAX_REF)) REFUSE("%s: ref_deg %g is outside 0 .. %g", who, o.ref_deg, MDEMOD_SUN_MAX_REF);
	return MDEMOD_OK;
}

bool rows_fine(uint32_t rows) { return rows >= 1 && rows <= MDEMOD_SUN_MAX_ROWS; }

uint32_t
mask_of(const uint32_t apids[3])
{
	uint32_t mask = 0;
	for (int k = 0; k < 3; k++) mask |= (apids[k] >= 64 && apids[k] <= 66 ? 1u : 0u) << k;
	return mask;
}

} /* namespace */

int
sun_check_apply(const char *who, const uint8_t *const image[3], uint8_t *const out[3], uint32_t slot_mask, uint32_t rows, const uint32_t *gain, const void *work,
                uint64_t work_bytes, bool has_work)
{
	if (!rows_fine(rows)) REFUSE("%s: %u strip rows are outside 1 .. %d", who, rows, MDEMOD_SUN_MAX_ROWS);
	if (slot_mask < 1 || slot_mask > 7) REFUSE("%s: the slot mask %u is outside 1 .. 7", who, slot_mask);
	if (!image || !out) REFUSE("%s: the pictures and the outputs are needed", who);
	if (!gain) REFUSE("%s: the gain table is needed", who);
	const uint64_t area = static_cast<uint64_t>(rows) * SUN_ROW_BYTES, table = (static_cast<uint64_t>(rows) + 1) * MDEMOD_SUN_NODE_COLS * 4, need = mdemod_sun_workspace(rows);
	if (has_work) {
		if (!work) REFUSE("%s: the workspace is needed", who);
		if (work_bytes < need) REFUSE("%s: the workspace needs %llu bytes, not %llu", who, static_cast<unsigned long long>(need), static_cast<unsigned long long>(work_bytes));
	}
	uintptr_t low = reinterpret_cast<uintptr_t>(gain) | reinterpret_cast<uintptr_t>(work);
	for (int k = 0; k < 3; k++) {
		if (!(slot_mask >> k & 1u)) continue;
		if (!image[k] || !out[k]) REFUSE("%s: the picture and the output of slot %d are needed", who, k);
		low |= reinterpret_cast<uintptr_t>(image[k]) | reinterpret_cast<uintptr_t>(out[k]);
	}
	if (low & 3u) REFUSE("%s: the pictures, the outputs, the gain table and the workspace must stand at multiples of 4 bytes", who);
	bool hit = has_work && mdm_ranges_intersect(gain, table, work, need);
	for (int k = 0; k < 3; k++) {
		if (!(slot_mask >> k & 1u)) continue;
		hit = hit || mdm_ranges_intersect(out[k], area, gain, table) || (has_work && (mdm_ranges_intersect(out[k], area, work, need) || mdm_ranges_intersect(image[k], area, work, need)));
		for (int j = 0; j < 3; j++) {
			if (!(slot_mask >> j & 1u)) continue;
			if (j != k) hit = hit || mdm_ranges_intersect(out[k], area, out[j], area);
			if (j != k || out[k] != image[j]) hit = hit || mdm_ranges_intersect(out[k], area, image[j], area);
		}
	}
	if (hit) REFUSE("%s: the pictures, the outputs, the gain table and the workspace intersect (only the output of a slot may be its picture itself)", who);
	return MDEMOD_OK;
}

int
sun_prepare(const char *who, const mdemod_sun_opts *sun_opts, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_orbit *orbit, uint8_t *const image[3],
            const uint32_t apids[3], uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, uint32_t *gain,
            mdemod_sun_summary *summary)
{
	mdemod_sun_opts so;
	int rc = sun_settings(who, sun_opts, so);
	if (rc) return rc;
	if (!rows_fine(rows)) REFUSE("%s: %u strip rows are outside 1 .. %d", who, rows, MDEMOD_SUN_MAX_ROWS);
	if (!image || !apids) REFUSE("%s: the pictures and their APIDs are needed", who);
	const uint32_t mask = mask_of(apids);
	for (int k = 0; k < 3; k++)
		if ((mask >> k & 1u) && !image[k]) REFUSE("%s: the picture of slot %d (APID %u) is needed", who, k, apids[k]);
	mdemod_map_opts mo;
	mdemod_map_timing timing;
	mdemod_sun_timing twin;
	if ((rc = mdemod_map_fit_time(place, sinfo, n_desc, sun_twin(pass_opts, mo), &timing))) return rc;
	if ((rc = mdemod_sun_nodes(orbit, sun_twin(&timing, twin), pass_opts, &so, rows, gain, summary))) return rc;
	summary->slot_mask = mask;
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_sun_default_opts(mdemod_sun_opts *opts)
{
	if (!opts) return;
	memset(opts, 0, sizeof *opts);
	opts->limit_deg = 85.0; opts->ref_deg = 45.0;
}

int
mdemod_sun_position(int32_t date, double utc, double out[3])
try { MDEMOD_API_ENTER
	if (!out) REFUSE("mdemod_sun_position: the vector is needed");
	if (!std::isfinite(utc) || fabs(utc) > 1.0e9) REFUSE("mdemod_sun_position: utc %g is no time of day", utc);
	sun_vector(date, utc, out);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_sun_cos_zenith(int32_t date, const double *utc, const double *lat, const double *lon, uint64_t n, double *out)
try { MDEMOD_API_ENTER
	if (n && (!utc || !lat || !lon || !out)) REFUSE("mdemod_sun_cos_zenith: the times, the coordinates and the output are needed");
	for (uint64_t k = 0; k < n; k++) {
		if (!std::isfinite(utc[k]) || fabs(utc[k]) > 1.0e9 || !std::isfinite(lat[k]) || !std::isfinite(lon[k])) { out[k] = NAN; continue; }
		double s[3];
		sun_vector(date, utc[k], s);
		out[k] = cos_zenith(s, lat[k], lon[k]);
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_sun_nodes(const mdemod_sun_orbit *sun_orbit, const mdemod_sun_timing *sun_timing, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_opts *sun_opts, uint32_t rows,
                 uint32_t *gain, mdemod_sun_summary *summary)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_sun_nodes";
	mdemod_sun_opts so;
	mdemod_map_opts mo;
	int rc = sun_settings(who, sun_opts, so);
	if (rc) return rc;
	if (!rows_fine(rows)) REFUSE("%s: %u strip rows are outside 1 .. %d", who, rows, MDEMOD_SUN_MAX_ROWS);
	if (!gain) REFUSE("%s: the gain table is needed", who);
	if (!sun_twin(pass_opts, mo)) mdemod_map_default_opts(&mo);
	mdemod_map_tle tle;
	mdemod_map_timing tm;
	const mdemod_map_tle *orbit = sun_twin(sun_orbit, tle);
	const mdemod_map_timing *timing = sun_twin(sun_timing, tm);
	const size_t count = (static_cast<size_t>(rows) + 1) * MDEMOD_SUN_NODE_COLS;
	std::vector<double> y(count), x(count), lat(count), lon(count);
	for (size_t k = 0; k < count; k++) { y[k] = 8.0 * static_cast<double>(k / MDEMOD_SUN_NODE_COLS); x[k] = 16.0 * static_cast<double>(k % MDEMOD_SUN_NODE_COLS); }
	int32_t date;
	/* (the map layer checks the orbit, the line times and its options, and notes the text) */
	if ((rc = mdemod_map_date(orbit, timing, &mo, &date))) return rc;
	if ((rc = mdemod_map_geolocate(orbit, timing, &mo, y.data(), x.data(), count, lat.data(), lon.data()))) return rc;
	const double cl = cos(so.limit_deg * SUN_RAD), cr = cos(so.ref_deg * SUN_RAD);
	mdemod_sun_summary s;
	memset(&s, 0, sizeof s);
	s.nodes = static_cast<uint32_t>(count); s.date = date;
	double c_min = 2.0, c_max = -2.0, sun[3] = { 0.0, 0.0, 0.0 };
	for (size_t k = 0; k < count; k++) {
		if (k % MDEMOD_SUN_NODE_COLS == 0) sun_vector(date, timing->s0 + y[k] * timing->row_period / 8.0 - mo.time_offset, sun);
		if (!std::isfinite(lat[k]) || !std::isfinite(lon[k])) { gain[k] = MDEMOD_SUN_NO_NODE; s.missing++; continue; }
		const double c = cos_zenith(sun, lat[k], lon[k]);
		c_min = c < c_min ? c : c_min; c_max = c > c_max ? c : c_max;
		s.at_limit += c < cl;
		gain[k] = static_cast<uint32_t>(floor(65536.0 * cr / (c > cl ? c : cl) + 0.5));
	}
	if (s.missing < s.nodes) {
		s.zenith_min = acos(c_max > 1.0 ? 1.0 : c_max) / SUN_RAD;
		s.zenith_max = acos(c_min < -1.0 ? -1.0 : c_min) / SUN_RAD;
	}
	if (summary) *summary = s;
	return MDEMOD_OK;
} MDEMOD_API_CATCH

uint64_t
mdemod_sun_workspace(uint32_t rows)
{
	return rows_fine(rows) ? static_cast<uint64_t>(rows) * 12u : 0u;
}

int
mdemod_sun_model_apply(const uint8_t *const image[3], uint8_t *const out[3], uint32_t slot_mask, uint32_t rows, const uint32_t *gain, uint64_t saturated[3])
try { MDEMOD_API_ENTER
	const int rc = sun_check_apply("mdemod_sun_model_apply", image, out, slot_mask, rows, gain, nullptr, 0, false);
	if (rc) return rc;
	uint64_t sat[3] = { 0, 0, 0 };
	for (uint32_t y = 0; y < 8 * rows; y++) {
		const uint32_t *g0 = gain + static_cast<size_t>(y >> 3) * MDEMOD_SUN_NODE_COLS, *g1 = g0 + MDEMOD_SUN_NODE_COLS, p = y & 7u;
		for (uint32_t x = 0; x < SUN_WIDTH; x++) {
			const uint32_t b = x >> 4, q = x & 15u;
			const bool missing = sun_missing(g0[b], g1[b], g0[b + 1], g1[b + 1]);
			const uint32_t g = sun_across(sun_down(g0[b], g1[b], p), sun_down(g0[b + 1], g1[b + 1], p), q);
			const size_t at = static_cast<size_t>(y) * SUN_WIDTH + x;
			for (int k = 0; k < 3; k++) {
				if (!(slot_mask >> k & 1u)) continue;
				const uint32_t v = image[k][at], t = sun_scaled(v, g);
				if (missing) { out[k][at] = static_cast<uint8_t>(v); continue; }
				sat[k] += t > 255u;
				out[k][at] = static_cast<uint8_t>(t > 255u ? 255u : t);
			}
		}
	}
	if (saturated) for (int k = 0; k < 3; k++) saturated[k] = sat[k];
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_sun_model_host(const mdemod_sun_opts *sun_opts, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_orbit *orbit, uint8_t *const image[3], const uint32_t apids[3],
                      uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, mdemod_sun_summary *summary)
try { MDEMOD_API_ENTER
	mdemod_sun_summary s;
	memset(&s, 0, sizeof s);
	if (summary) *summary = s;
	if (!rows) return MDEMOD_OK;
	std::vector<uint32_t> gain((static_cast<size_t>(rows <= MDEMOD_SUN_MAX_ROWS ? rows : 0) + 1) * MDEMOD_SUN_NODE_COLS);
	int rc = sun_prepare("mdemod_sun_model_host", sun_opts, pass_opts, orbit, image, apids, rows, place, sinfo, n_desc, gain.data(), &s);
	if (rc) return rc;
	if (s.slot_mask) {
		const uint8_t *in[3] = { image[0], image[1], image[2] };
		if ((rc = mdemod_sun_model_apply(in, image, s.slot_mask, rows, gain.data(), s.saturated))) return rc;
	}
	if (summary) *summary = s;
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
