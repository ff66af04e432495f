/*
 * meteor_demod_amd_picture.h — from channel pictures (include/meteor_demod_amd_image.h) to what a user looks at: the scan lines
 * resampled to equal ground distance (the Earth's curvature and the scanner's constant angular step taken out), the contrast
 * stretched between two percentiles of the filled pixels, and one to three channels interleaved into a grey or colour picture.
 * The histograms and the render run on the GPU; the column map and the look-up tables are small and computed on the host.  The
 * specification of the two kernels is a host model in integer arithmetic (csrc/picture_host.cpp, exported as
 * mdemod_picture_model_*): GPU bytes equal model bytes.
 *
 *   input       per slot k = 0 .. 2 (the image layer's slots) a picture uint8 [8 rows][1568] and a mask filled uint8 [rows][14]
 *               (non-zero: the cell of 8 lines x 112 columns received a strip).  rows <= 65 536.
 *   geometry    R = 6371.0 km, h = altitude_km, thetamax = scan_deg / 2 in radians, D = 2 thetamax / 1568 the scanner's angular
 *               step, res = h D the ground size of a pixel at nadir.  Output column j of W has its centre at ground distance
 *               g = (j - (W - 1) / 2) res from the sub-satellite track, which the scanner sees under the angle
 *               atan2(R sin(g / R), R + h - R cos(g / R)): the source coordinate is x(j) = that angle / D + 783.5.
 *   width       W is the largest multiple of 4 with x(0) >= 0, found by going up from 4 in steps of 4 while x(0) stays >= 0 (an
 *               output line of W or 3 W bytes then starts on a dword).  At most 8192.
 *   map         uint32 [W]: map[j] = floor(256 x(j) + 0.5) for the left half j < W / 2, and the right half is the mirror
 *               map[W - 1 - j] = 1567 * 256 - map[j]: the table is symmetric whatever the library's atan2 does in its last bit.
 *               From an entry: i = min(map >> 8, 1567), f = map & 255, the second tap is min(i + 1, 1567).
 *               rectify = 0 gives the identity: W = 1568, map[j] = 256 j.
 *   refused     altitude_km outside 300 .. 2000, scan_deg outside 1 .. 130, sin(thetamax) (R + h) / R >= 1 (the edge of the scan
 *               misses the Earth), a clip above 499, piece_rows above 65 536: MDEMOD_ERR_PARAM, text in mdemod_last_error.
 *   histogram   uint32 [3][256]: hist[k][v] counts the pixels of value v of slot k that lie in filled cells.  A slot whose picture
 *               pointer is NULL is not counted (its row stays zero).  Exact integers: 65 536 x 8 x 1568 stays below 2^32.
 *   table       from one histogram and two clips in permille (0 .. 499 each): N = sum of hist, cum[v] the running sum,
 *               cum[-1] = 0.  lo is the smallest v with 1000 cum[v] > N clip_low, hi the largest v with
 *               1000 (N - cum[v - 1]) > N clip_high.  N = 0 or hi <= lo: the identity table (limits 0 and 255).  Otherwise
 *               lut[v] = min(max((v - lo) 255 + (hi - lo) / 2, 0) / (hi - lo), 255), the divisions truncating, all in 64 bits.
 *               stretch = 0 (whole-picture entry): the identity table.
 *   render      out uint8 [8 rows][W][planes], planes 1 or 3, interleaved; select[p] is the slot of output plane p.  For output
 *               pixel (y, j), plane p, s = select[p], r = y / 8, i, f and i2 = min(i + 1, 1567) from map[j]:
 *               a = picture_s[y][i], b = picture_s[y][i2], fa = filled_s[r][i / 112] != 0, fb = filled_s[r][i2 / 112] != 0.
 *               fa and fb: v = (a (256 - f) + b f + 128) >> 8.  Only one of them: that tap's value (the border of a missing
 *               strip is not blended with its zeros).  Neither: the byte is 0 and the table is not applied.  Otherwise the byte
 *               is lut[p][v].
 *   valid       uint8 [rows][W], optional: bit p says that plane p had at least one filled tap in that strip row and column.
 *
 *   to be confirmed off air   altitude 820 km and a full scan angle of 110 degrees are nominal figures (a swath of about 2800 km
 *               from about 820 km); no recording and no orbit stands behind them.  The first geolocated pass confirms or
 *               replaces both, and says whether column 783.5 is the nadir.
 */
#ifndef METEOR_DEMOD_AMD_PICTURE_H
#define METEOR_DEMOD_AMD_PICTURE_H

#include "meteor_demod_amd_image.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_PICTURE_MAX_WIDTH     8192
#define MDEMOD_PICTURE_DEFAULT_PIECE 1024
#define MDEMOD_PICTURE_MAX_CLIP      499

typedef struct {
	double   altitude_km;         /* 820.0                                                                                            */
	double   scan_deg;            /* 110.0: the full scan angle                                                                       */
	uint32_t rectify;             /* 1; 0: the identity map, 1568 columns                                                             */
	uint32_t stretch;             /* 1; 0: identity tables (whole-picture entry)                                                      */
	uint32_t clip_low, clip_high; /* 5 and 5: permille of the filled pixels left below lo and above hi, each 0 .. 499                 */
	uint32_t piece_rows;          /* mdemod_picture_compose_host copies pieces of this many strip rows: 0 = 1024, <= 65 536           */
	uint32_t reserved;            /* 0                                                                                                */
} mdemod_picture_opts;

/* What mdemod_picture_compose_host returns: pixels and valid are malloc'ed, and mdemod_picture_free gives them back. */
typedef struct {
	uint32_t width, lines, planes, reserved;
	uint32_t lo[3], hi[3];        /* the stretch limits of each output plane (0 and 255 for an identity table)                        */
	uint64_t valid_cells;         /* non-zero bytes of valid: (strip row, column) pairs where some plane had a filled tap             */
	uint8_t *pixels;              /* [lines][width][planes] (NULL when lines = 0)                                                     */
	uint8_t *valid;               /* [lines / 8][width]                                                                               */
} mdemod_picture_result;

/* altitude 820, scan 110, rectify 1, stretch 1, clips 5 and 5, piece_rows 0. */
void mdemod_picture_default_opts(mdemod_picture_opts *opts);

/* Host only: *width := W; when map is given and cap >= W, map[0 .. W - 1] is written (cap < W with a map: MDEMOD_ERR_PARAM, *width
 * still says how many are needed). */
int  mdemod_picture_column_map(const mdemod_picture_opts *opts, uint32_t *map, uint32_t cap, uint32_t *width);

/* image_dev[k] ([8 rows][1568]) under filled_dev[k] ([rows][14]) into hist_dev[3][256], which the entry zeroes itself.  Device
 * memory; the pictures and the histogram at multiples of 4 bytes.  A NULL picture is a slot not counted.  Queued on hip_stream of
 * `device`; asynchronous.  rows = 0: the zeroes.  Nothing outside the inputs is read and nothing outside the output is written.
 * MDEMOD_ERR_PARAM (text in mdemod_last_error) for a missing or misaligned pointer, more than 65 536 rows, or ranges that intersect. */
int  mdemod_picture_histogram_device(const uint8_t *const image_dev[3], const uint8_t *const filled_dev[3], uint32_t rows, uint32_t *hist_dev,
                                     int device, void *hip_stream);

/* Host only: the table of one histogram (limits, when given, receives lo and hi). */
int  mdemod_picture_lut(const uint32_t hist[256], uint32_t clip_low, uint32_t clip_high, uint8_t lut[256], uint32_t limits[2]);

/* The slots select[0 .. planes - 1] (host memory, each 0 .. 2, planes 1 or 3) through map_dev[width] and lut_dev[planes][256] into
 * out_dev[8 rows][width][planes] and, unless NULL, valid_dev[rows][width].  width is a multiple of 4, 4 .. 8192.  Device memory;
 * everything but the masks at multiples of 4 bytes; only the selected slots' pointers are looked at.  Asynchronous, as above.
 * rows = 0 is nothing to do.  An entry of the map beyond column 1567 reads column 1567. */
int  mdemod_picture_render_device(const uint8_t *const image_dev[3], const uint8_t *const filled_dev[3], uint32_t rows, const uint32_t *select,
                                  uint32_t planes, const uint8_t *lut_dev, const uint32_t *map_dev, uint32_t width, uint8_t *out_dev,
                                  uint8_t *valid_dev, int device, void *hip_stream);

/* Pictures and masks in host memory (what mdemod_image_result holds) to the finished picture.  Synchronous.  The strip rows are
 * copied in pieces of opts->piece_rows: first the histograms of the selected slots over all pieces, then the tables, then each
 * piece is rendered: the result is byte for byte that of one batch.  *out is overwritten; mdemod_picture_free(out) afterwards. */
int  mdemod_picture_compose_host(const mdemod_picture_opts *opts, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                                 const uint32_t *select, uint32_t planes, mdemod_picture_result *out, int device);
void mdemod_picture_free(mdemod_picture_result *out);

#ifdef __cplusplus
}
#endif
#endif
