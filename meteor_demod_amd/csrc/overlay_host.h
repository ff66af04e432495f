/*
 * overlay_host.h — what csrc/overlay_host.cpp (host: the readers, the graticule, the projection, the pieces, the bins, the model, the
 * bands of the whole-picture entry) and csrc/overlay.hip (the kernel and the device entries) share: the argument checks, the bands
 * with a backend in the kernel's place, and the model's entries, exported for the tests.  Free of the GPU runtime.
 */
#ifndef MDEMOD_OVERLAY_HOST_H
#define MDEMOD_OVERLAY_HOST_H

#include <cmath>

#include "../../include/meteor_demod_amd_overlay.h"

#define OVERLAY_TILE       MDEMOD_OVERLAY_TILE
#define OVERLAY_MAX_STYLES MDEMOD_OVERLAY_MAX_STYLES
#define OVERLAY_PIECE_TOP  16384                   /* a piece is no longer than this per axis: 64 pixels */

static_assert(sizeof(mdemod_overlay_piece) == 32, "the kernel stages records of 32 bytes");

/* how far from its bounding box a piece of half width w can colour a pixel: the corner of the square cap, with room for the floors
 * of the rule and the rounding of the tangent */
inline int64_t
overlay_reach(uint32_t half_width)
{
	const uint64_t q = 2ull * (half_width + 130ull) * (half_width + 130ull);
	uint64_t r = static_cast<uint64_t>(std::sqrt(static_cast<double>(q)));
	while (r * r > q) r--;
	while ((r + 1) * (r + 1) <= q) r++;                                        /* isqrt(q) */
	return static_cast<int64_t>(r) + 2;
}

inline uint32_t overlay_tiles(uint32_t pixels) { return (pixels + OVERLAY_TILE - 1) / OVERLAY_TILE; }

/* styles, sizes, planes of a draw call, and valid where a style needs it; MDEMOD_ERR_PARAM with a text */
int  overlay_check_draw(const char *who, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes,
                        const void *pixels, const void *valid);

/* what stands in the kernel's place in the whole-picture entry.  begin: the pieces and the bins of the whole picture, and whether the
 * bands come with valid and want a mask; band: the lines from tile row `tile_row` on, `height` of them, in host memory, drawn in
 * place.  Synchronous. */
struct OverlayBackend {
	virtual int begin(const mdemod_overlay_pieces &pieces, const mdemod_overlay_bins &bins, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width,
	                  uint32_t planes, uint32_t piece_lines, bool with_valid, bool with_mask) = 0;
	virtual int band(uint32_t tile_row, uint32_t height, uint8_t *pixels, const uint8_t *valid, uint8_t *mask) = 0;
	virtual ~OverlayBackend() {}
};

/* the whole-picture entries up to where the projection ends: the argument checks and every layer's vectors to fixed point; then
 * overlay_draw_points */
int  overlay_draw_bands(const char *who, const mdemod_overlay_geo *geo, const mdemod_overlay_layer *layers, uint32_t n_layers, const mdemod_overlay_style *styles,
                        uint32_t n_styles, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines,
                        mdemod_overlay_report *report, OverlayBackend &backend);

/* and from there on, for points in fixed point whatever projection made them (csrc/polar.hip): layer l is cut with style style_of[l],
 * the pieces are binned, the picture goes through the backend in bands of piece_lines lines (0: 1024), the report is filled.  The
 * arguments were checked (overlay_check_draw, style_of below n_styles, piece_lines a multiple of 32); mask and report may be NULL, and
 * without a mask the report's pixels stay 0. */
int  overlay_draw_points(const mdemod_overlay_points *const *layers, const uint32_t *style_of, uint32_t n_layers, const mdemod_overlay_style *styles, uint32_t n_styles,
                         uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines,
                         mdemod_overlay_report *report, OverlayBackend &backend);
/* overlay_draw_points with the kernel of csrc/overlay.hip as the backend; the device is taken when the bands begin */
int  overlay_draw_points_device(const mdemod_overlay_points *const *layers, const uint32_t *style_of, uint32_t n_layers, const mdemod_overlay_style *styles,
                                uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid, mdemod_overlay_report *report,
                                int device);

extern "C" {

/* the rule over every piece, pixel by pixel: no bins */
int  mdemod_overlay_model_draw(const mdemod_overlay_piece *pieces, uint64_t n_pieces, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width,
                               uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask);
/* the model of overlay_draw: host memory, the kernel's arguments, tile by tile through the bins */
int  mdemod_overlay_model_tiles(const mdemod_overlay_piece *pieces, uint64_t n_pieces, const uint32_t *tile_first, const uint32_t *items, uint64_t n_items,
                                const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels,
                                const uint8_t *valid, uint8_t *mask);
/* mdemod_overlay_draw_host with the model in the kernel's place (no device) */
int  mdemod_overlay_model_host(const mdemod_overlay_geo *geo, const mdemod_overlay_layer *layers, uint32_t n_layers, const mdemod_overlay_style *styles,
                               uint32_t n_styles, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines,
                               mdemod_overlay_report *report);

}

#endif
