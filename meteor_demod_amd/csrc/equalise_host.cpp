/*
 * equalise_host.cpp — host side of the equalise layer (include/meteor_demod_amd_equalise.h): the argument checks, the sizes, and the
 * host model of the kernels of csrc/equalise.hip (mdemod_equalise_model_*: the rule of the header as plain loops, one tile and one
 * pixel after the other).  Free of the GPU runtime.
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "buffers.h"
#include "equalise_host.h"
#include "mdemod_internal_api.h"

#define REFUSE_IF_NAMED(...) do { if (who) mdm_note_error(__VA_ARGS__); return MDEMOD_ERR_PARAM; } while (0)

namespace {

bool
counted(const EqPlan &p, const uint8_t *valid, uint32_t y, uint32_t x)
{
	return !valid || valid[static_cast<size_t>(y / p.valid_step) * p.width + x] != 0;
}

/* the value of channel c of the pixel at px */
uint32_t
value_of(const EqPlan &p, const uint8_t *px, uint32_t c)
{
	if (p.planes == 1) return px[0];
	return p.luma ? eq_luma(px[0], px[1], px[2]) : px[c];
}

} /* namespace */

int
eq_check(const char *who, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts, EqPlan *plan)
{
	mdemod_equalise_opts o;
	if (opts) o = *opts;
	else mdemod_equalise_default_opts(&o);
	if (planes != 1 && planes != 3) REFUSE_IF_NAMED("%s: planes must be 1 or 3, not %u", who, planes);
	if (width < 1 || width > MDEMOD_EQUALISE_MAX_WIDTH) REFUSE_IF_NAMED("%s: width %u is outside 1 .. %d", who, width, MDEMOD_EQUALISE_MAX_WIDTH);
	if (height < 1 || height > MDEMOD_EQUALISE_MAX_HEIGHT) REFUSE_IF_NAMED("%s: height %u is outside 1 .. %d", who, height, MDEMOD_EQUALISE_MAX_HEIGHT);
	if (o.tile < MDEMOD_EQUALISE_MIN_TILE || o.tile > MDEMOD_EQUALISE_MAX_TILE || o.tile % 8)
		REFUSE_IF_NAMED("%s: tile %u is no multiple of 8 in %d .. %d", who, o.tile, MDEMOD_EQUALISE_MIN_TILE, MDEMOD_EQUALISE_MAX_TILE);
	if (o.clip_percent < MDEMOD_EQUALISE_MIN_CLIP || o.clip_percent > MDEMOD_EQUALISE_MAX_CLIP)
		REFUSE_IF_NAMED("%s: clip_percent %u is outside %d .. %d", who, o.clip_percent, MDEMOD_EQUALISE_MIN_CLIP, MDEMOD_EQUALISE_MAX_CLIP);
	if (o.amount > MDEMOD_EQUALISE_MAX_AMOUNT) REFUSE_IF_NAMED("%s: amount %u is outside 0 .. %d", who, o.amount, MDEMOD_EQUALISE_MAX_AMOUNT);
	if (planes == 3 && o.mode > 1) REFUSE_IF_NAMED("%s: mode %u is neither 0 (planes) nor 1 (luminance)", who, o.mode);
	if (o.valid_step != 1 && o.valid_step != 8) REFUSE_IF_NAMED("%s: valid_step must be 1 or 8, not %u", who, o.valid_step);
	plan->width = width; plan->height = height; plan->planes = planes;
	plan->luma = planes == 3 && o.mode == MDEMOD_EQUALISE_LUMA;
	plan->channels = planes == 3 && !plan->luma ? 3 : 1;
	plan->tile = o.tile; plan->clip = o.clip_percent; plan->amount = o.amount; plan->valid_step = o.valid_step;
	plan->nx = eq_tiles(width, o.tile); plan->ny = eq_tiles(height, o.tile);
	return MDEMOD_OK;
}

int
eq_check_buffers(const char *who, const EqPlan &p, const void *picture, const void *valid, const void *work, uint64_t work_bytes, const void *out, bool has_out)
{
	const uint64_t area = static_cast<uint64_t>(p.width) * p.height * p.planes, need = eq_public_bytes(p);
	const uint64_t mask = static_cast<uint64_t>((p.height + p.valid_step - 1) / p.valid_step) * p.width;
	if (!picture) REFUSE_IF_NAMED("%s: the picture is needed", who);
	if (!work) REFUSE_IF_NAMED("%s: the workspace is needed", who);
	if (has_out && !out) REFUSE_IF_NAMED("%s: the output is needed", who);
	if (work_bytes < need) REFUSE_IF_NAMED("%s: the workspace needs %llu bytes, not %llu", who, static_cast<unsigned long long>(need), static_cast<unsigned long long>(work_bytes));
	if ((reinterpret_cast<uintptr_t>(picture) & 3u) || (reinterpret_cast<uintptr_t>(work) & 3u) || (has_out && (reinterpret_cast<uintptr_t>(out) & 3u)))
		REFUSE_IF_NAMED("%s: the picture, the workspace and the output must stand at multiples of 4 bytes", who);
	bool hit = mdm_ranges_intersect(picture, area, work, work_bytes) || mdm_ranges_intersect(valid, mask, work, work_bytes) || mdm_ranges_intersect(picture, area, valid, mask);
	if (has_out) hit = hit || mdm_ranges_intersect(out, area, work, work_bytes) || mdm_ranges_intersect(out, area, valid, mask) || (out != picture && mdm_ranges_intersect(out, area, picture, area));
	if (hit) REFUSE_IF_NAMED("%s: the picture, the mask, the workspace and the output intersect (only the output may be the picture itself)", who);
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_equalise_default_opts(mdemod_equalise_opts *opts)
{
	if (!opts) return;
	memset(opts, 0, sizeof *opts);
	opts->tile = 128; opts->clip_percent = 300; opts->amount = 256; opts->mode = MDEMOD_EQUALISE_LUMA; opts->valid_step = 1;
}

uint64_t
mdemod_equalise_workspace(uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts)
{
	EqPlan p;
	if (eq_check(nullptr, width, height, planes, opts, &p) != MDEMOD_OK) return 0;
	return eq_public_bytes(p);                                                   /* the kernels need nothing of their own */
}

uint32_t
mdemod_equalise_model_table(const uint32_t hist[256], uint32_t clip_percent, uint32_t *h2, uint8_t *tab)
{
	const uint32_t clip = clip_percent < MDEMOD_EQUALISE_MIN_CLIP ? MDEMOD_EQUALISE_MIN_CLIP : clip_percent > MDEMOD_EQUALISE_MAX_CLIP ? MDEMOD_EQUALISE_MAX_CLIP : clip_percent;
	uint32_t n = 0, excess = 0, cum = 0;
	for (uint32_t v = 0; v < 256; v++) n += hist[v];
	const uint32_t limit = eq_clip_limit(clip, n);
	for (uint32_t v = 0; v < 256; v++) excess += hist[v] > limit ? hist[v] - limit : 0u;
	for (uint32_t v = 0; v < 256; v++) {
		const uint32_t h = (hist[v] < limit ? hist[v] : limit) + eq_share(v, excess);
		cum += h;
		if (h2) h2[v] = h;
		if (tab) tab[v] = n ? static_cast<uint8_t>(eq_table_entry(cum, n)) : 0;
	}
	return n;
}

int
mdemod_equalise_model_tables(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts, void *work,
                             uint64_t work_bytes)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_equalise_model_tables";
	EqPlan p;
	int rc = eq_check(who, width, height, planes, opts, &p);
	if (rc) return rc;
	if ((rc = eq_check_buffers(who, p, picture, valid, work, work_bytes, nullptr, false))) return rc;
	uint8_t *tab = static_cast<uint8_t *>(work);
	uint8_t *count = tab + eq_tab_bytes(p);                                      /* (written through memcpy: the workspace is only 4-aligned) */
	std::vector<uint32_t> hist(256);
	for (uint32_t c = 0; c < p.channels; c++)
		for (uint32_t ty = 0; ty < p.ny; ty++)
			for (uint32_t tx = 0; tx < p.nx; tx++) {
				std::fill(hist.begin(), hist.end(), 0u);
				for (uint32_t y = eq_tile_begin(ty, p.tile); y < eq_tile_end(ty, p.ny, height, p.tile); y++)
					for (uint32_t x = eq_tile_begin(tx, p.tile); x < eq_tile_end(tx, p.nx, width, p.tile); x++)
						if (counted(p, valid, y, x)) hist[value_of(p, picture + (static_cast<size_t>(y) * width + x) * planes, c)]++;
				const size_t t = (static_cast<size_t>(c) * p.ny + ty) * p.nx + tx;
				const uint32_t n = mdemod_equalise_model_table(hist.data(), p.clip, nullptr, tab + t * 256);
				memcpy(count + t * 4, &n, 4);
			}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_equalise_model_apply(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts,
                            const void *work, uint8_t *out)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_equalise_model_apply";
	EqPlan p;
	int rc = eq_check(who, width, height, planes, opts, &p);
	if (rc) return rc;
	if ((rc = eq_check_buffers(who, p, picture, valid, work, eq_public_bytes(p), out, true))) return rc;
	const uint8_t *tab = static_cast<const uint8_t *>(work);
	const uint8_t *count = tab + eq_tab_bytes(p);
	for (uint32_t y = 0; y < height; y++) {
		uint32_t ya, yb, fy;
		eq_axis(y, p.tile, p.ny, &ya, &yb, &fy);
		for (uint32_t x = 0; x < width; x++) {
			const size_t at = (static_cast<size_t>(y) * width + x) * planes;
			uint8_t px[3] = { picture[at], planes == 3 ? picture[at + 1] : uint8_t(0), planes == 3 ? picture[at + 2] : uint8_t(0) };
			if (!counted(p, valid, y, x)) { for (uint32_t k = 0; k < planes; k++) out[at + k] = px[k]; continue; }
			uint32_t xa, xb, fx, v2[3] = { 0, 0, 0 };
			eq_axis(x, p.tile, p.nx, &xa, &xb, &fx);
			const uint32_t tile_y[4] = { ya, ya, yb, yb }, tile_x[4] = { xa, xb, xa, xb };
			const uint32_t wy[2] = { 2 * p.tile - fy, fy }, wx[2] = { 2 * p.tile - fx, fx };
			for (uint32_t c = 0; c < p.channels; c++) {
				const uint32_t v = value_of(p, px, c);
				uint32_t e[4], w[4];
				for (uint32_t k = 0; k < 4; k++) {
					const size_t t = (static_cast<size_t>(c) * p.ny + tile_y[k]) * p.nx + tile_x[k];
					uint32_t n;
					memcpy(&n, count + t * 4, 4);
					w[k] = n ? wy[k >> 1] * wx[k & 1] : 0u;
					e[k] = tab[t * 256 + v];
				}
				/* (a workspace that is not this picture's could leave no tile: the pixel stays) */
				v2[c] = w[0] + w[1] + w[2] + w[3] ? eq_amount(v, eq_blend(e, w), p.amount) : v;
			}
			if (p.luma) {
				const uint32_t Y = eq_luma(px[0], px[1], px[2]);
				for (uint32_t k = 0; k < 3; k++) out[at + k] = static_cast<uint8_t>(eq_scale(px[k], v2[0], Y));
			} else {
				for (uint32_t k = 0; k < planes; k++) out[at + k] = static_cast<uint8_t>(v2[k]);
			}
		}
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
