/*
 * meteor_demod_amd_mosaic.h — several passes blended onto one north-up latitude / longitude grid.  Every pass is what the map layer
 * (include/meteor_demod_amd_map.h) takes for one map: swath pictures and masks of three slots, the placements and reports of its
 * packets, and a two-line element set, here as text with a catalogue number.  The time fit, the date, the orbit and the look of a
 * pass are exactly the map layer's; so are the node rule, the warp rule and the tap rule that this text refers to.  The grid is
 * common to all passes, and the blend runs on the GPU in one launch.  The specification of the kernel is a host model in integer
 * arithmetic (csrc/mosaic_host.cpp, exported as mdemod_mosaic_model_*): GPU bytes equal model bytes.
 *
 *   passes      n passes, 1 <= n <= MDEMOD_MOSAIC_MAX_PASSES (8), in the caller's order.  A pass carries its TLE text and catalogue
 *               number (0: the text's first set), a date (days since 1970-01-01, or MDEMOD_MOSAIC_DATE_AUTO: the date that puts
 *               its middle line nearest the epoch of its set, resolved per pass), three slots of pictures and masks, its strip
 *               rows (passes may differ), placements and reports.  At most 8192 strip rows per pass.
 *   common grid the border samples of every pass as in the map header (lines 0, 8, .. and the last, columns 0, 16, .. and 1567),
 *               with the same refusals: a sample that is not visible, or beyond 85 degrees of latitude.  The reference longitude
 *               is that of pass 0's pixel ((lines_0 - 1) / 2, 783.5); every border longitude of every pass is taken relative to
 *               it and wrapped to +-180; the ranges of latitude and longitude are the union over all passes.  Then the map header's
 *               formulas unchanged: sy = px_per_deg, sx = max(1, round(sy cos lat_mid)), lat_top = ceil(max lat sy) / sy,
 *               lon_left = floor(min lon sx) / sx, H = ceil((lat_top - min lat) sy), W = ceil((max lon - lon_left) sx) rounded
 *               up to a multiple of 4.  Refused: W > 8192 or H > 16 384 (the text names a scale that fits).  For n = 1 this is
 *               the map layer's grid.
 *   nodes       per pass int32 [ceil(H / 16) + 1][ceil(W / 16) + 1][2] on the common grid, by the map header's node rule with that
 *               pass's line times and lines; both words MDEMOD_MOSAIC_NO_NODE where there is none.
 *   blend       integers; >> is a floor; as if in 64 bits.  Output pixel (i, j): for every pass k the map header's warp rule with
 *               pass k's nodes and rows gives (X, Y), or the pass is empty there (a missing corner, or X, Y outside the picture).
 *                 e = min(X, 1567 * 256 - X, Y, (8 rows_k - 1) * 256 - Y),  w_k = 1 + (e >> 8):
 *               1 at the edge of the swath, 784 at nadir.  Per plane p the map header's tap rule on slot select[p] of pass k gives
 *               a value v, or the pass does not count for p; b = lut_k[p][v].
 *                 MDEMOD_MOSAIC_FEATHER (0)  S = sum of w_k over the passes that count for p; the byte is
 *                                            (sum of w_k b + (S >> 1)) / S in integer division.
 *                 MDEMOD_MOSAIC_BEST (1)     the byte is b of the counting pass with the largest w_k; ties go to the lower k.
 *               No pass counts: the byte is 0 and valid bit p is clear.  With n = 1 both modes give the map layer's warp bytes.
 *   outputs     out uint8 [H][W][planes], planes 1 or 3; valid uint8 [H][W], bit p: plane p had a counting pass; cover uint8
 *               [H][W], bit k: pass k went into the byte of at least one plane: with FEATHER every pass that counts for the
 *               plane, with BEST the one whose byte is taken.  valid and cover are optional.
 *   stretch     0: identity tables.  1 (joint): the picture layer's histogram of every pass, summed per plane (slot select[p]) over
 *               the passes, gives one table per plane by the picture layer's rule, used for every pass.  2: per pass, each from its
 *               own histogram, as the map layer does for one.  For n = 1 the settings 1 and 2 coincide with the map layer.
 *   world file  as in the map header: 1 / sx, 0, 0, -1 / sy, lon_left + 0.5 / sx, lat_top - 0.5 / sy.
 */
#ifndef METEOR_DEMOD_AMD_MOSAIC_H
#define METEOR_DEMOD_AMD_MOSAIC_H

#include "meteor_demod_amd_picture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_MOSAIC_MAX_PASSES 8
#define MDEMOD_MOSAIC_FEATHER    0
#define MDEMOD_MOSAIC_BEST       1
#define MDEMOD_MOSAIC_DATE_AUTO  INT32_MIN
#define MDEMOD_MOSAIC_NO_NODE    INT32_MIN
#define MDEMOD_MOSAIC_MAX_WIDTH  8192
#define MDEMOD_MOSAIC_MAX_HEIGHT 16384

typedef struct {
	double   scan_deg;            /* 110.0: the full scan angle, 1 .. 130                                                             */
	double   px_per_deg;          /* 100.0: 1 .. 1000                                                                                 */
	double   time_offset;         /* 10 800.0: onboard clock minus UTC in seconds, -86 400 .. 86 400                                  */
	double   row_period;          /* 8 / 6.5: seconds per strip row where the stamps cannot say (0.1 .. 10)                           */
	int32_t  side;                /* +1 or -1                                                                                         */
	uint32_t stretch;             /* 1: joint; 0: identity tables; 2: per pass                                                        */
	uint32_t clip_low, clip_high; /* 5 and 5 permille, as in the picture layer                                                        */
	uint32_t piece_lines;         /* mdemod_mosaic_compose_host makes bands of this many output lines: 0 = 1024, a multiple of 16     */
	uint32_t blend;               /* MDEMOD_MOSAIC_FEATHER or MDEMOD_MOSAIC_BEST                                                      */
} mdemod_mosaic_opts;

/* One pass, host memory.  mdemod_mosaic_grid looks at the text, the date, rows and the packets only. */
typedef struct {
	const char    *tle_text;      /* NUL-terminated                                                                                   */
	uint32_t       norad;         /* 0: the text's first set                                                                          */
	int32_t        date;          /* days since 1970-01-01, or MDEMOD_MOSAIC_DATE_AUTO                                                */
	const uint8_t *image[3];      /* [8 rows][1568] each; only the selected slots are looked at                                       */
	const uint8_t *filled[3];     /* [rows][14] each                                                                                  */
	uint32_t       rows;
	uint32_t       reserved;
	const mdemod_placement  *place;
	const mdemod_strip_info *sinfo;
	uint64_t       n_desc;
} mdemod_mosaic_pass;

typedef struct {
	double   row_period;          /* seconds per strip row                                                                            */
	double   s0;                  /* onboard seconds of the day of line 0                                                             */
	int32_t  date;                /* the date that was used                                                                           */
	uint32_t rows_fit;            /* rows the period rests on (below 2: the fallback)                                                 */
	uint32_t placed;              /* placed packets s0 rests on                                                                       */
	uint32_t lines;               /* 8 rows                                                                                           */
} mdemod_mosaic_timing;

typedef struct {
	uint32_t width, height;       /* W, H                                                                                             */
	uint32_t sx;                  /* pixels per degree of longitude                                                                   */
	uint32_t node_rows, node_cols;
	uint32_t n;                   /* passes                                                                                           */
	double   sy;                  /* pixels per degree of latitude                                                                    */
	double   lat_top, lon_left;   /* the outer edges of pixel (0, 0), degrees; lon_left in -180 .. 180                                */
	mdemod_mosaic_timing timing[MDEMOD_MOSAIC_MAX_PASSES];
	int32_t *nodes[MDEMOD_MOSAIC_MAX_PASSES];   /* each [node_rows][node_cols][2]: X, Y                                                */
} mdemod_mosaic_nodes;

/* One pass of mdemod_mosaic_blend_device: device pointers.  lut [planes][256], nodes on the common grid; rows = 0: the pass is
 * empty and none of its pointers is looked at. */
typedef struct {
	const uint8_t *image[3];
	const uint8_t *filled[3];
	const uint8_t *lut;
	const int32_t *nodes;
	uint32_t       rows;
	uint32_t       reserved;
} mdemod_mosaic_source;

/* What mdemod_mosaic_compose_host returns: pixels, valid, cover are malloc'ed, and mdemod_mosaic_free gives them back. */
typedef struct {
	uint32_t width, height, planes, sx;
	uint32_t n, blend;
	double   sy, lat_top, lon_left;
	mdemod_mosaic_timing timing[MDEMOD_MOSAIC_MAX_PASSES];
	double   utc0[MDEMOD_MOSAIC_MAX_PASSES];          /* UTC seconds of day timing[k].date of pass k's line 0                          */
	uint32_t lo[MDEMOD_MOSAIC_MAX_PASSES][3], hi[MDEMOD_MOSAIC_MAX_PASSES][3];   /* the stretch limits of each pass and plane          */
	uint64_t covered[MDEMOD_MOSAIC_MAX_PASSES];       /* pixels with cover bit k                                                       */
	uint64_t valid_pixels;        /* non-zero bytes of valid                                                                          */
	uint64_t overlap_pixels;      /* bytes of cover with two or more bits                                                             */
	uint8_t *pixels;              /* [height][width][planes]                                                                          */
	uint8_t *valid;               /* [height][width]                                                                                  */
	uint8_t *cover;               /* [height][width]                                                                                  */
} mdemod_mosaic_result;

/* scan 110, 100 px/deg, offset 10 800, row_period 8 / 6.5, side +1, stretch 1, clips 5 and 5, piece_lines 0, blend 0. */
void mdemod_mosaic_default_opts(mdemod_mosaic_opts *opts);

/* Host only: the common grid, every pass's nodes on it and every pass's line times with the date resolved.  *grid is overwritten;
 * mdemod_mosaic_grid_free. */
int  mdemod_mosaic_grid(const mdemod_mosaic_opts *opts, const mdemod_mosaic_pass *passes, uint32_t n, mdemod_mosaic_nodes *grid);
void mdemod_mosaic_grid_free(mdemod_mosaic_nodes *grid);

/* sources[n] (host memory, holding device pointers), the slots select[0 .. planes - 1] (host memory, each 0 .. 2, planes 1 or 3) of
 * every pass into out_dev[height][width][planes] and, unless NULL, valid_dev[height][width] and cover_dev[height][width].  n at most
 * 8, width a multiple of 4, 4 .. 8192, height at most 16 384, rows at most 65 536.  Device memory; everything but the masks at
 * multiples of 4 bytes; only the selected slots' pointers are looked at.  Queued on hip_stream of `device`; asynchronous.  n = 0 or
 * height = 0 is nothing to do.  Nothing outside the inputs is read and nothing outside the outputs is written.  MDEMOD_ERR_PARAM
 * (text in mdemod_last_error) for a missing or misaligned pointer, a size out of range, or outputs that intersect each other or an
 * input of any pass; nothing is written then. */
int  mdemod_mosaic_blend_device(const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width,
                                uint32_t height, uint8_t *out_dev, uint8_t *valid_dev, uint8_t *cover_dev, int device, void *hip_stream);

/* Passes in host memory to the finished mosaic.  Synchronous.  The time fits, the grid, the stretch tables (the picture layer's
 * histogram on the device), the selected slots of every pass copied whole, the output in bands of opts->piece_lines lines: the
 * result is byte for byte that of one batch.  *out is overwritten; mdemod_mosaic_free(out) afterwards. */
int  mdemod_mosaic_compose_host(const mdemod_mosaic_opts *opts, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                                mdemod_mosaic_result *out, int device);
void mdemod_mosaic_free(mdemod_mosaic_result *out);

#ifdef __cplusplus
}
#endif
#endif
