/*
 * picture_host.cpp — host side of the picture layer (include/meteor_demod_amd_picture.h): the option check, the column map, the
 * look-up table, the pieces of the whole-picture entry, and the host model of the kernels of csrc/picture.hip
 * (mdemod_picture_model_*: plain loops over the header's text).  Free of the GPU runtime.
 */
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "picture_host.h"
#include "mdemod_internal_api.h"

namespace {

constexpr double PIC_R = 6371.0, PIC_PI = 3.14159265358979323846;

/* the source coordinate of output column j of w */
double
pic_x(double h, double step, double res, uint32_t w, uint32_t j)
{
	const double g = (static_cast<double>(j) - (static_cast<double>(w) - 1.0) / 2.0) * res, a = g / PIC_R;
	return atan2(PIC_R * sin(a), PIC_R + h - PIC_R * cos(a)) / step + 783.5;
}

void
model_histogram(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, uint32_t *hist)
{
	memset(hist, 0, 3 * 256 * sizeof(uint32_t));
	for (int s = 0; s < 3; s++) {
		if (!image[s]) continue;
		for (uint64_t y = 0; y < 8ull * rows; y++)
			for (uint32_t x = 0; x < PIC_SRC_W; x++)
				if (filled[s][(y / 8) * PIC_CELLS + x / PIC_CELL_W]) hist[256 * s + image[s][y * PIC_SRC_W + x]]++;
	}
}

void
model_render(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes, const uint8_t *lut,
             const uint32_t *map, uint32_t width, uint8_t *out, uint8_t *valid)
{
	for (uint64_t y = 0; y < 8ull * rows; y++)
		for (uint32_t j = 0; j < width; j++) {
			const uint32_t i = map[j] >> 8 < PIC_LAST ? map[j] >> 8 : PIC_LAST, f = map[j] & 255u, i2 = i + 1 < PIC_LAST ? i + 1 : PIC_LAST;
			uint8_t seen = 0;
			for (uint32_t p = 0; p < planes; p++) {
				const uint8_t *src = image[select[p]] + y * PIC_SRC_W, *cells = filled[select[p]] + (y / 8) * PIC_CELLS;
				const uint32_t a = src[i], b = src[i2];
				const bool fa = cells[i / PIC_CELL_W] != 0, fb = cells[i2 / PIC_CELL_W] != 0;
				uint8_t byte = 0;
				if (fa || fb) {
					const uint32_t v = fa && fb ? (a * (256u - f) + b * f + 128u) >> 8 : fa ? a : b;
					byte = lut[256 * p + v];
					seen |= static_cast<uint8_t>(1u << p);
				}
				out[(y * width + j) * planes + p] = byte;
			}
			if (valid && y % 8 == 0) valid[(y / 8) * width + j] = seen;
		}
}

struct ModelBackend : PicBackend {
	int histogram(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, uint32_t *hist) override
	{
		model_histogram(image, filled, rows, hist);
		return MDEMOD_OK;
	}
	int render(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes, const uint8_t *lut,
	           const uint32_t *map, uint32_t width, uint8_t *out, uint8_t *valid) override
	{
		model_render(image, filled, rows, select, planes, lut, map, width, out, valid);
		return MDEMOD_OK;
	}
};

} /* namespace */

int
pic_check_slots(const char *who, const uint8_t *const image[3], const uint8_t *const filled[3], const uint32_t *select, uint32_t planes)
{
	if (!image || !filled) REFUSE("%s: the pictures and the masks are needed", who);
	for (uint32_t p = 0; p < planes; p++)
		if (!image[select[p]] || !filled[select[p]]) REFUSE("%s: the picture and the mask of slot %u are needed", who, select[p]);
	return MDEMOD_OK;
}

int
pic_settings(const mdemod_picture_opts *opts, mdemod_picture_opts &out)
{
	mdemod_picture_default_opts(&out);
	if (opts) out = *opts;
	if (!(out.altitude_km >= 300.0 && out.altitude_km <= 2000.0)) REFUSE("picture: altitude is %g km (300 .. 2000)", out.altitude_km);
	if (!(out.scan_deg >= 1.0 && out.scan_deg <= 130.0)) REFUSE("picture: scan angle is %g degrees (the full angle: 1 .. 130)", out.scan_deg);
	if (sin(out.scan_deg / 2.0 * PIC_PI / 180.0) * (PIC_R + out.altitude_km) / PIC_R >= 1.0)
		REFUSE("picture: the edge of a scan of %g degrees from %g km misses the Earth", out.scan_deg, out.altitude_km);
	if (out.clip_low > MDEMOD_PICTURE_MAX_CLIP || out.clip_high > MDEMOD_PICTURE_MAX_CLIP)
		REFUSE("picture: the clips are %u and %u permille (each 0 .. 499)", out.clip_low, out.clip_high);
	if (out.piece_rows > MDEMOD_IMAGE_MAX_ROWS) REFUSE("picture: piece_rows is %u (0 for the default, or at most 65536)", out.piece_rows);
	if (!out.piece_rows) out.piece_rows = MDEMOD_PICTURE_DEFAULT_PIECE;
	return MDEMOD_OK;
}

int
pic_check_select(const char *who, uint32_t rows, const uint32_t *select, uint32_t planes)
{
	if (rows > MDEMOD_IMAGE_MAX_ROWS) REFUSE("%s: %u strip rows are more than a picture has (65536)", who, rows);
	if (planes != 1 && planes != 3) REFUSE("%s: %u planes (1 for grey, 3 for colour)", who, planes);
	if (!select) REFUSE("%s: the selection of slots is needed", who);
	for (uint32_t p = 0; p < planes; p++)
		if (select[p] > 2) REFUSE("%s: select[%u] is %u (a slot: 0 .. 2)", who, p, select[p]);
	return MDEMOD_OK;
}

int
pic_compose_pieces(const mdemod_picture_opts &o, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select,
                   uint32_t planes, mdemod_picture_result *out, PicBackend &backend)
{
	memset(out, 0, sizeof *out);
	uint32_t width = 0;
	int rc = mdemod_picture_column_map(&o, nullptr, 0, &width);
	if (rc) return rc;
	std::vector<uint32_t> map(width);
	if ((rc = mdemod_picture_column_map(&o, map.data(), width, &width))) return rc;
	out->width = width;
	out->lines = 8 * rows;
	out->planes = planes;
	/* only the selected slots are looked at */
	const uint8_t *img[3] = { nullptr, nullptr, nullptr }, *fil[3] = { nullptr, nullptr, nullptr };
	for (uint32_t p = 0; rows && p < planes; p++) { img[select[p]] = image[select[p]]; fil[select[p]] = filled[select[p]]; }
	const uint32_t P = o.piece_rows;
	auto piece = [&](uint32_t at, const uint8_t *pi[3], const uint8_t *pf[3]) {
		for (int s = 0; s < 3; s++) {
			pi[s] = img[s] ? img[s] + at * PIC_LINE_BYTES : nullptr;
			pf[s] = fil[s] ? fil[s] + static_cast<uint64_t>(at) * PIC_CELLS : nullptr;
		}
	};
	/* the histograms over all pieces */
	std::vector<uint32_t> hist(3 * 256, 0), part(3 * 256);
	for (uint32_t at = 0; at < rows && o.stretch; at += P) {
		const uint8_t *pi[3], *pf[3];
		piece(at, pi, pf);
		if ((rc = backend.histogram(pi, pf, P < rows - at ? P : rows - at, part.data()))) return rc;
		for (int i = 0; i < 3 * 256; i++) hist[i] += part[i];
	}
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
	if (!rows) return MDEMOD_OK;
	out->pixels = static_cast<uint8_t *>(malloc(static_cast<size_t>(8) * rows * width * planes));
	out->valid = static_cast<uint8_t *>(malloc(static_cast<size_t>(rows) * width));
	if (!out->pixels || !out->valid) { mdemod_picture_free(out); return MDEMOD_ERR_NOMEM; }
	for (uint32_t at = 0; at < rows; at += P) {
		const uint8_t *pi[3], *pf[3];
		piece(at, pi, pf);
		rc = backend.render(pi, pf, P < rows - at ? P : rows - at, select, planes, lut, map.data(), width,
		                    out->pixels + static_cast<uint64_t>(8) * at * width * planes, out->valid + static_cast<uint64_t>(at) * width);
		if (rc) { mdemod_picture_free(out); return rc; }
	}
	for (uint64_t i = 0; i < static_cast<uint64_t>(rows) * width; i++) out->valid_cells += out->valid[i] != 0;
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_picture_default_opts(mdemod_picture_opts *opts)
{
	if (!opts) return;
	opts->altitude_km = 820.0;
	opts->scan_deg = 110.0;
	opts->rectify = 1;
	opts->stretch = 1;
	opts->clip_low = 5;
	opts->clip_high = 5;
	opts->piece_rows = 0;
	opts->reserved = 0;
}

void
mdemod_picture_free(mdemod_picture_result *out)
{
	if (!out) return;
	free(out->pixels); free(out->valid);
	memset(out, 0, sizeof *out);
}

int
mdemod_picture_column_map(const mdemod_picture_opts *opts, uint32_t *map, uint32_t cap, uint32_t *width)
try { MDEMOD_API_ENTER
	mdemod_picture_opts o;
	const int rc = pic_settings(opts, o);
	if (rc) return rc;
	if (!width) REFUSE("mdemod_picture_column_map: the width is needed");
	if (!o.rectify) {
		*width = PIC_SRC_W;
		if (map && cap < PIC_SRC_W) REFUSE("mdemod_picture_column_map: room for %u entries, the map has %u", cap, PIC_SRC_W);
		if (map)
			for (uint32_t j = 0; j < PIC_SRC_W; j++) map[j] = 256u * j;
		return MDEMOD_OK;
	}
	const double step = 2.0 * (o.scan_deg / 2.0 * PIC_PI / 180.0) / PIC_SRC_W, res = o.altitude_km * step;
	uint32_t w = 4;
	while (w + 4 <= MDEMOD_PICTURE_MAX_WIDTH && pic_x(o.altitude_km, step, res, w + 4, 0) >= 0.0) w += 4;
	*width = w;
	if (map && cap < w) REFUSE("mdemod_picture_column_map: room for %u entries, the map has %u", cap, w);
	if (map) {
		const int64_t top = static_cast<int64_t>(PIC_LAST) * 256;
		for (uint32_t j = 0; j < w / 2; j++) {
			int64_t m = static_cast<int64_t>(floor(256.0 * pic_x(o.altitude_km, step, res, w, j) + 0.5));
			m = m < 0 ? 0 : m > top ? top : m;
			map[j] = static_cast<uint32_t>(m);
			map[w - 1 - j] = static_cast<uint32_t>(top - m);
		}
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_picture_lut(const uint32_t hist[256], uint32_t clip_low, uint32_t clip_high, uint8_t lut[256], uint32_t limits[2])
try { MDEMOD_API_ENTER
	if (!hist || !lut) REFUSE("mdemod_picture_lut: the histogram and the table are needed");
	if (clip_low > MDEMOD_PICTURE_MAX_CLIP || clip_high > MDEMOD_PICTURE_MAX_CLIP)
		REFUSE("picture: the clips are %u and %u permille (each 0 .. 499)", clip_low, clip_high);
	uint64_t n = 0, cum = 0;
	for (int v = 0; v < 256; v++) n += hist[v];
	int64_t lo = -1, hi = -1;
	for (int v = 0; v < 256; v++) {
		if (1000 * (n - cum) > n * clip_high) hi = v;                             /* (cum is still cum[v - 1]) */
		cum += hist[v];
		if (lo < 0 && 1000 * cum > n * clip_low) lo = v;
	}
	const bool identity = !n || hi <= lo;
	if (identity) { lo = 0; hi = 255; }
	for (int64_t v = 0; v < 256; v++) {
		int64_t num = (v - lo) * 255 + (hi - lo) / 2;
		if (num < 0) num = 0;
		const int64_t q = num / (hi - lo);
		lut[v] = static_cast<uint8_t>(identity ? v : q > 255 ? 255 : q);
	}
	if (limits) { limits[0] = static_cast<uint32_t>(lo); limits[1] = static_cast<uint32_t>(hi); }
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_picture_model_histogram(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, uint32_t *hist)
try { MDEMOD_API_ENTER
	if (!hist) REFUSE("mdemod_picture_model_histogram: the histogram is needed");
	if (rows > MDEMOD_IMAGE_MAX_ROWS) REFUSE("mdemod_picture_model_histogram: %u strip rows are more than a picture has (65536)", rows);
	if (rows && (!image || !filled)) REFUSE("mdemod_picture_model_histogram: the pictures and the masks are needed");
	for (int s = 0; rows && s < 3; s++)
		if (image[s] && !filled[s]) REFUSE("mdemod_picture_model_histogram: the mask of slot %d is needed", s);
	const uint8_t *none[3] = { nullptr, nullptr, nullptr };
	model_histogram(rows ? image : none, rows ? filled : none, rows, hist);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_picture_model_render(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes,
                            const uint8_t *lut, const uint32_t *map, uint32_t width, uint8_t *out, uint8_t *valid)
try { MDEMOD_API_ENTER
	int rc = pic_check_select("mdemod_picture_model_render", rows, select, planes);
	if (rc) return rc;
	if (width < 4 || width > MDEMOD_PICTURE_MAX_WIDTH || width % 4) REFUSE("mdemod_picture_model_render: the width is %u (a multiple of 4, 4 .. 8192)", width);
	if (!rows) return MDEMOD_OK;
	if ((rc = pic_check_slots("mdemod_picture_model_render", image, filled, select, planes))) return rc;
	if (!lut || !map || !out) REFUSE("mdemod_picture_model_render: the tables, the map and the picture are needed");
	model_render(image, filled, rows, select, planes, lut, map, width, out, valid);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_picture_model_host(const mdemod_picture_opts *opts, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                          const uint32_t *select, uint32_t planes, mdemod_picture_result *out)
try { MDEMOD_API_ENTER
	mdemod_picture_opts o;
	int rc = pic_settings(opts, o);
	if (rc) return rc;
	if (!out) REFUSE("mdemod_picture_model_host: the result is needed");
	if ((rc = pic_check_select("mdemod_picture_model_host", rows, select, planes))) return rc;
	if (rows && (rc = pic_check_slots("mdemod_picture_model_host", image, filled, select, planes))) return rc;
	ModelBackend model;
	return pic_compose_pieces(o, image, filled, rows, select, planes, out, model);
} MDEMOD_API_CATCH

} /* extern "C" */
