/*
 * equalise_host.h — what the host model (csrc/equalise_host.cpp, g++) and the kernels (csrc/equalise.hip) of the equalise layer
 * (include/meteor_demod_amd_equalise.h) share, written once: the tile geometry, the luminance, the clip limit, the share of a bin in
 * the redistribution, the four (tile, weight) pairs of a pixel, the blend and the output rule.  The check that is independent of
 * this file is tests/equalise_ref.py.  Free of the GPU runtime.
 */
#ifndef MDEMOD_EQUALISE_HOST_H
#define MDEMOD_EQUALISE_HOST_H

#include "../../include/meteor_demod_amd_equalise.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EQ_HD __host__ __device__ __forceinline__
#else
#define EQ_HD inline
#endif

/* what the entries work with once the options are checked */
struct EqPlan {
	uint32_t width, height, planes, channels;      /* channels: the sets of tables, 1 or 3 */
	uint32_t tile, clip, amount, luma, valid_step;
	uint32_t nx, ny;
};

EQ_HD uint32_t eq_tiles(uint32_t size, uint32_t tile) { const uint32_t n = (size + tile / 2) / tile; return n ? n : 1u; }
/* the first line (column) of tile t and the one behind its last */
EQ_HD uint32_t eq_tile_begin(uint32_t t, uint32_t tile) { return t * tile; }
EQ_HD uint32_t eq_tile_end(uint32_t t, uint32_t n, uint32_t size, uint32_t tile) { return t + 1 == n ? size : (t + 1) * tile; }

EQ_HD uint32_t eq_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

EQ_HD uint32_t
eq_clip_limit(uint32_t clip, uint32_t n)
{
	const uint64_t l = (static_cast<uint64_t>(clip) * n + 25599u) / 25600u;
	return l ? static_cast<uint32_t>(l) : 1u;
}

/* what bin v receives of an excess E: q and its share of the r odd counts */
EQ_HD uint32_t eq_share(uint32_t v, uint32_t excess) { const uint32_t r = excess & 255u; return (excess >> 8) + (((v + 1u) * r) >> 8) - ((v * r) >> 8); }

EQ_HD uint32_t eq_table_entry(uint32_t cum, uint32_t n) { return (255u * cum + n / 2u) / n; }

/* the two tiles of pixel coordinate x along an axis of n tiles, and the weight of the second (the first has 2 T - f) */
EQ_HD void
eq_axis(uint32_t x, uint32_t tile, uint32_t n, uint32_t *a, uint32_t *b, uint32_t *f)
{
	const int32_t u = static_cast<int32_t>(2u * x + 1u) - static_cast<int32_t>(tile);
	const int32_t t0 = u < 0 ? -1 : u / static_cast<int32_t>(2u * tile);
	*f = static_cast<uint32_t>(u - 2 * static_cast<int32_t>(tile) * t0);
	*a = t0 < 0 ? 0u : static_cast<uint32_t>(t0);
	*b = static_cast<uint32_t>(t0 + 1) < n ? static_cast<uint32_t>(t0 + 1) : n - 1u;
}

/* v' of the four table entries e[k] with weights w[k]; a weight of an empty tile has been set to 0 */
EQ_HD uint32_t
eq_blend(const uint32_t *e, const uint32_t *w)
{
	const uint32_t S = w[0] + w[1] + w[2] + w[3];
	const uint32_t A = w[0] * e[0] + w[1] * e[1] + w[2] * e[2] + w[3] * e[3];
	return (A + S / 2u) / S;
}

EQ_HD uint32_t eq_amount(uint32_t v, uint32_t v1, uint32_t amount) { return (v * (256u - amount) + v1 * amount + 128u) >> 8; }

/* luminance mode: the byte c of a pixel of luminance Y whose luminance becomes v2 */
EQ_HD uint32_t
eq_scale(uint32_t c, uint32_t v2, uint32_t Y)
{
	if (!Y) return v2;
	const uint32_t o = (c * v2 + Y / 2u) / Y;
	return o > 255u ? 255u : o;
}

/* the bytes of the public part of the workspace: tab, then count */
inline uint64_t eq_tab_bytes(const EqPlan &p) { return static_cast<uint64_t>(p.channels) * p.ny * p.nx * 256u; }
inline uint64_t eq_public_bytes(const EqPlan &p) { return static_cast<uint64_t>(p.channels) * p.ny * p.nx * 260u; }

/* The sizes and options of an entry into *plan (opts NULL: the defaults): MDEMOD_OK, or MDEMOD_ERR_PARAM with the text noted
 * (who NULL: no text, for mdemod_equalise_workspace). */
int  eq_check(const char *who, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts, EqPlan *plan);
/* The pointers of an entry: there, at multiples of 4 bytes (picture, workspace), the workspace large enough, nothing intersecting but
 * out == picture.  work_bytes: what the caller says the workspace holds.  out may be NULL for an entry that has none. */
int  eq_check_buffers(const char *who, const EqPlan &plan, const void *picture, const void *valid, const void *work, uint64_t work_bytes, const void *out, bool has_out);

extern "C" {

/* ---- the host model: what the kernels of csrc/equalise.hip must compute, byte for byte (exported for the tests) ---- */

/* One histogram through clip, redistribution and table: h2[256] := h'' (may be NULL), tab[256] := the table (may be NULL; zeroes
 * for n = 0).  Returns n.  clip_percent is not checked beyond being clamped to 100 .. 25 600. */
uint32_t mdemod_equalise_model_table(const uint32_t hist[256], uint32_t clip_percent, uint32_t *h2, uint8_t *tab);
/* The public part of the workspace (tab, count) of a picture in host memory into work[work_bytes]. */
int  mdemod_equalise_model_tables(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts,
                                  void *work, uint64_t work_bytes);
/* The tables of work applied to picture into out (which may be picture). */
int  mdemod_equalise_model_apply(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts,
                                 const void *work, uint8_t *out);

}

#endif
