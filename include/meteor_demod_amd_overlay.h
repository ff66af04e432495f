/*
 * meteor_demod_amd_overlay.h — lines drawn onto a north-up latitude / longitude picture: a graticule and the polylines of a vector
 * file (coastlines, borders).  The picture is any picture on the grid of the map and mosaic layers: W x H pixels, sx and sy pixels
 * per degree, the outer edges of pixel (0, 0) at lat_top and lon_left, so that longitude / latitude to pixel is affine.  Vectors are
 * read and projected on the host in double; from fixed point on everything is integer arithmetic, and the specification of the kernel
 * is a host model (csrc/overlay_host.cpp, exported as mdemod_overlay_model_*): GPU bytes equal model bytes.
 *
 *   vectors     polylines: lon[], lat[] in degrees and first[n_lines + 1], line l being the vertices first[l] .. first[l + 1] - 1.
 *               mdemod_overlay_read takes two formats, told apart by the first four bytes (four bytes of text: the text format;
 *               anything else must be a shapefile).
 *                 shapefile   the main file (.shp) alone.  Header of 100 bytes: file code 9994 big-endian at byte 0, the file's length
 *                             in 16-bit words big-endian at byte 24, version 1000 little-endian at byte 28.  Records: 8 bytes
 *                             big-endian (number, content length in words), then the content, little-endian.  Shape types 3 and 5
 *                             and their Z / M variants 13, 15, 23, 25, of which the common prefix is read: type, box (4 doubles),
 *                             numParts, numPoints, parts[], points[] as x = longitude, y = latitude.  Every part is one polyline; a
 *                             polygon's ring is drawn as stored.  Type 0 and the point types (1, 8, 11, 18, 21, 28) and 31 are
 *                             skipped and counted.
 *                 text        one vertex per line, "lon lat", separated by blanks, tabs or a comma; '#' begins a comment; an empty
 *                             line, or a line beginning with '>', ends the polyline.
 *               Refused (MDEMOD_ERR_PARAM, text in mdemod_last_error): a file that cannot be read, a wrong file code or version, a
 *               record that runs past the file or past its own content length, a part index that does not ascend or lies outside
 *               numPoints, a shape type that is none of the above, a line of text that is not two numbers, a coordinate that is not
 *               finite, |lat| > 90 or |lon| > 360.
 *   graticule   the meridians and parallels at multiples of step degrees that cross the picture, parallels with a vertex at every
 *               multiple of the step (no segment is longer than half the globe).  step 0: the smallest of 1, 2, 5, 10, 15, 30 with
 *               step sy >= 128 pixels, 30 if none.  No labels.
 *   projection  host, double.  Pixel centres stand at multiples of 256.  wrap180(a) = a - 360 floor((a + 180) / 360).  For a
 *               polyline let c = W / (2 sx); the first vertex has dl = c + wrap180(lon - lon_left - c), every later one
 *               dl_n = dl_(n-1) + wrap180(lon_n - lon_(n-1)): the short way round, so a line is continuous across +-180 degrees.
 *                 X = floor(256 (dl sx - 0.5) + 0.5),  Y = floor(256 ((lat_top - lat) sy - 0.5) + 0.5),
 *               saturated to int32.  The polyline is given out at each of the shifts -360, 0, +360 degrees (X -+ 92 160 sx) whose
 *               bounding box, grown by the largest reach (below), meets the picture.  Checked against numpy to +-1 unit; everything
 *               after it is exact.
 *   pieces      integers, as if in 64 bits; >> is a floor.  A segment with an end point of |X| or |Y| above 2^30 is left out (the
 *               polyline breaks there).  A segment A -> B, d = B - A, is cut into k = max(1, ceil(max(|dx|, |dy|) / 16384)) pieces:
 *               vertex m is A + floor((2 m d + k) / (2 k)) per component, so that no piece is longer than 64 pixels per axis.  A
 *               piece with dx = dy = 0 is dropped.  Per piece L16 = isqrt(256 (dx^2 + dy^2)), tx = floor((524288 dx + L16) / (2 L16))
 *               and ty likewise (a unit tangent scaled by 16384), L = (L16 + 8) >> 4.  A record is { ax, ay, tx, ty, L, style } and
 *               two words of zero: 32 bytes.  Pieces that cannot reach the picture are never made (a world coastline is not 10^7
 *               pieces for a regional map); the result is defined as if all were there.
 *   coverage    styles s = 0 .. n_styles - 1, n_styles <= 4: half_width w in 1/256 pixel (0 .. 2048), opacity 0 .. 256, colour[3],
 *               inside_only.  For output pixel (i, j), P = (256 j, 256 i), and a piece of style s:
 *                 dx = Px - ax, dy = Py - ay, along = (tx dx + ty dy) >> 14, perp = |tx dy - ty dx| >> 14,
 *                 d = max(perp, -along, along - L, 0), a = clamp(w_s + 128 - d, 0, 256).
 *               A_s is the maximum of a over the pieces of style s (no order, no atomics); A_s = 0 where inside_only is set and
 *               valid[i][j] == 0; A'_s = (A_s opacity_s + 128) >> 8; in ascending s, for every plane p,
 *               byte = (byte (256 - A'_s) + colour_s[p] A'_s + 128) >> 8.  A grey picture uses colour[0].  mask[i][j] has bit s set
 *               where A_s > 0.  A pixel no piece reaches keeps its byte.
 *   bins        tiles of 32 x 32 pixels, row-major, in CSR form: tile_first[tiles + 1] and items[] (piece indices), the items of a
 *               tile ascending in style, then in index.  A piece is listed in every tile that its bounding box, grown by the reach,
 *               meets.  The reach is not w + 128 along the axes: the square cap's corner stands (w + 128) sqrt 2 from the end point
 *               (the bins take isqrt(2 (w + 130)^2) + 2).
 */
#ifndef METEOR_DEMOD_AMD_OVERLAY_H
#define METEOR_DEMOD_AMD_OVERLAY_H

#include "meteor_demod_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_OVERLAY_MAX_STYLES 4
#define MDEMOD_OVERLAY_MAX_WIDTH  8192
#define MDEMOD_OVERLAY_MAX_HEIGHT 16384
#define MDEMOD_OVERLAY_MAX_HALF   2048
#define MDEMOD_OVERLAY_TILE       32
#define MDEMOD_OVERLAY_VERTEX_TOP (1 << 30)

/* the grid of a picture: what the results of the map and mosaic layers carry */
typedef struct {
	uint32_t width, height;       /* W, H                                                                                             */
	uint32_t sx;                  /* pixels per degree of longitude                                                                   */
	uint32_t reserved;
	double   sy;                  /* pixels per degree of latitude                                                                    */
	double   lat_top, lon_left;   /* the outer edges of pixel (0, 0), degrees                                                         */
} mdemod_overlay_geo;

/* polylines in degrees; lon, lat, first are malloc'ed, and mdemod_overlay_vectors_free gives them back */
typedef struct {
	double   *lon, *lat;          /* [n_points]                                                                                       */
	uint32_t *first;              /* [n_lines + 1]                                                                                    */
	uint32_t  n_lines, n_points;
	uint32_t  skipped;            /* records of a shapefile that hold no line (null shapes, points)                                   */
	uint32_t  reserved;
} mdemod_overlay_vectors;

/* polylines in fixed point; mdemod_overlay_points_free */
typedef struct {
	int32_t  *x, *y;              /* [n_points]                                                                                       */
	uint32_t *first;              /* [n_lines + 1]                                                                                    */
	uint32_t  n_lines, n_points;
} mdemod_overlay_points;

typedef struct {
	int32_t ax, ay, tx, ty, L, style;
	int32_t zero[2];
} mdemod_overlay_piece;

/* pieces, malloc'ed; mdemod_overlay_pieces_free.  mdemod_overlay_cut appends. */
typedef struct {
	mdemod_overlay_piece *piece;
	uint64_t n, room;
} mdemod_overlay_pieces;

typedef struct {
	uint32_t half_width;          /* in 1/256 pixel, 0 .. 2048: 128 is a line of one pixel                                            */
	uint32_t opacity;             /* 0 .. 256                                                                                         */
	uint8_t  colour[3];
	uint8_t  inside_only;         /* draw only where valid is not 0                                                                   */
} mdemod_overlay_style;

/* the bins of a picture; mdemod_overlay_bins_free */
typedef struct {
	uint32_t *tile_first;         /* [tiles_x tiles_y + 1]                                                                            */
	uint32_t *items;              /* [n_items]                                                                                        */
	uint32_t  tiles_x, tiles_y;
	uint64_t  n_items;
} mdemod_overlay_bins;

typedef struct {
	const mdemod_overlay_vectors *vectors;
	uint32_t style;
	uint32_t reserved;
} mdemod_overlay_layer;

/* what mdemod_overlay_draw_host has done */
typedef struct {
	uint64_t pieces[MDEMOD_OVERLAY_MAX_STYLES];   /* pieces kept per style                                                          */
	uint64_t pixels[MDEMOD_OVERLAY_MAX_STYLES];   /* pixels with A_s > 0                                                            */
	uint64_t tiles;                               /* tiles with an item                                                             */
	uint64_t items;
} mdemod_overlay_report;

/* Host only.  *vectors is overwritten. */
int  mdemod_overlay_read(const char *path, mdemod_overlay_vectors *vectors);
int  mdemod_overlay_graticule(const mdemod_overlay_geo *geo, double step_deg, mdemod_overlay_vectors *vectors);
void mdemod_overlay_vectors_free(mdemod_overlay_vectors *vectors);

/* Host only: the projection.  *points is overwritten. */
int  mdemod_overlay_project(const mdemod_overlay_geo *geo, const mdemod_overlay_vectors *vectors, mdemod_overlay_points *points);
void mdemod_overlay_points_free(mdemod_overlay_points *points);

/* Host only: the pieces of style `style` (whose half width is half_width) that can reach a picture of width x height are appended
 * to *pieces, which is all zero before the first call. */
int  mdemod_overlay_cut(const mdemod_overlay_points *points, uint32_t style, uint32_t half_width, uint32_t width, uint32_t height,
                        mdemod_overlay_pieces *pieces);
void mdemod_overlay_pieces_free(mdemod_overlay_pieces *pieces);

/* Host only: the bins.  A piece whose style is not below n_styles is refused.  *bins is overwritten. */
int  mdemod_overlay_bin(const mdemod_overlay_piece *pieces, uint64_t n_pieces, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width,
                        uint32_t height, mdemod_overlay_bins *bins);
void mdemod_overlay_bins_free(mdemod_overlay_bins *bins);

/* pieces_dev[n_pieces], tile_first_dev[tiles + 1] and items_dev[n_items] as mdemod_overlay_bin makes them for this width, height
 * and styles (device memory), styles[n_styles] in host memory, onto pixels_dev[height][width][planes] in place, planes 1 or 3.
 * valid_dev[height][width] is read, and is needed where a style has inside_only; mask_dev[height][width], unless NULL, is written
 * whole.  width a multiple of 4, 4 .. 8192, height at most 16 384; every pointer at a multiple of 4 bytes.  Queued on hip_stream of
 * `device`; asynchronous.  n_pieces = 0 or height = 0: nothing is drawn (the mask is cleared).  An item that is no index into the
 * pieces is passed over, and tile_first is held to n_items: nothing outside the inputs is read and nothing outside the outputs is
 * written.  MDEMOD_ERR_PARAM (text in mdemod_last_error) for a missing or misaligned pointer, a size or a style out of range,
 * inside_only without valid, or outputs that intersect each other or an input; nothing is written then. */
int  mdemod_overlay_draw_device(const mdemod_overlay_piece *pieces_dev, uint64_t n_pieces, const uint32_t *tile_first_dev, const uint32_t *items_dev,
                                uint64_t n_items, const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes,
                                uint8_t *pixels_dev, const uint8_t *valid_dev, uint8_t *mask_dev, int device, void *hip_stream);

/* The whole job for a picture in host memory: pixels[height][width][planes] in place, valid (may be NULL unless a style has
 * inside_only), mask and report (may be NULL).  Projects, cuts and bins the layers, uploads, draws in bands of piece_lines lines
 * (0 = 1024, a multiple of 32) and downloads: the result is byte for byte that of one batch.  Synchronous. */
int  mdemod_overlay_draw_host(const mdemod_overlay_geo *geo, const mdemod_overlay_layer *layers, uint32_t n_layers, const mdemod_overlay_style *styles,
                              uint32_t n_styles, uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines,
                              mdemod_overlay_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
