/*
 * meteor_demod_amd_equalise.h — local contrast for the finished pictures: contrast-limited adaptive histogram equalisation (CLAHE)
 * of a picture, map or mosaic where it lies in GPU memory, between the warp that makes it and the encoder that takes it away.  The
 * whole step is stated in integers; the specification is a host model (csrc/equalise_host.cpp, exported as mdemod_equalise_model_*):
 * GPU bytes equal model bytes.  `/` truncates, and values are 32-bit unless stated otherwise.
 *
 *   picture     uint8 [H][W][planes], planes 1 or 3, W 1 .. 8192, H 1 .. 16 384.  The base address is a multiple of 4 bytes; lines
 *               need not start on a dword.
 *   valid       optional uint8 [ceil(H / valid_step)][W]; valid_step is 1 (maps, mosaics, polar pictures) or 8 (the picture layer's
 *               mask per strip row).  Pixel (y, x) is counted when valid is NULL or valid[y / valid_step][x] != 0.  A pixel that is
 *               not counted enters no histogram, and its bytes are copied to the output unchanged.
 *   channels    planes 1: one channel, the value v is the byte.  planes 3, mode 1 (luminance, the default): one channel,
 *               v = Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, the JPEG layer's Y.  planes 3, mode 0: three channels, each
 *               plane through its own tables.  mode is ignored for planes 1.
 *   tiles       T = tile, a multiple of 8, 16 .. 512, default 128.  nx = max(1, (W + T / 2) / T), ny = max(1, (H + T / 2) / T).
 *               Tile tx covers the columns tx T .. (tx + 1) T - 1, except the last, which runs to W - 1: a last tile is between T / 2
 *               and 3 T / 2 - 1 wide, or W wide when W < T.  Rows alike.  The nominal centre of tile tx is tx T + T / 2, also for the
 *               last tile.
 *   histogram   hist[c][ty][tx][v] counts the counted pixels of the tile whose channel value is v; n is its sum, at most 767^2 (a
 *               last tile is at most 3 T / 2 - 1 = 767 pixels a side at T = 512).
 *   clip        clip_percent 100 .. 25 600, default 300.  In 64 bits: L = max(1, (clip_percent n + 25 599) / 25 600); at 25 600,
 *               L = n and nothing is clipped.  E = sum of max(hist[v] - L, 0), h'[v] = min(hist[v], L).  One pass of redistribution,
 *               no second clip: q = E / 256, r = E % 256, h''[v] = h'[v] + q + (((v + 1) r) / 256 - (v r) / 256).  The sum of h'' is
 *               n again; the r odd counts are spread evenly.
 *   table       cum[v] the running sum of h''.  For n > 0, tab[v] = (255 cum[v] + n / 2) / n.  A tile with n = 0 is empty: its table
 *               is 256 zeroes and is never used.
 *   workspace   first uint8 tab[channels][ny][nx][256], then uint32 count[channels][ny][nx] (n; 0 means empty); what the kernels
 *               need privately comes after these two.  mdemod_equalise_workspace() gives the total.
 *   apply       for a counted pixel (y, x) with channel value v: u = 2 x + 1 - T, tx0 = floor(u / 2T) (-1 for u < 0),
 *               fx = u - 2 T tx0 in 0 .. 2T - 1.  The two tile columns are a = max(tx0, 0) with weight 2T - fx and
 *               b = min(tx0 + 1, nx - 1) with weight fx; rows alike: four (tile, weight) pairs with w = wy wx, a clamped tile simply
 *               appears twice.  S = sum of w over the pairs whose tile is not empty, A = sum of w tab[tile][v] over the same pairs,
 *               v' = (A + S / 2) / S.  The pixel's own tile is always among the four with w >= T^2 > 0 and is not empty, so S > 0;
 *               4 T^2 255 < 2^30: nothing here needs more than 32 bits.
 *   amount      0 .. 256, default 256: v'' = (v (256 - amount) + v' amount + 128) >> 8.
 *   output      one channel per plane: the byte is v''.  Luminance mode: for each plane p with byte c, out = v'' when Y = 0, and
 *               otherwise min(255, (c v'' + Y / 2) / Y).
 *   refused     MDEMOD_ERR_PARAM, text in mdemod_last_error, nothing written: a size, planes, tile, clip, amount, mode or valid_step
 *               out of range, a missing or misaligned pointer, a workspace that is too small, ranges that intersect - with one
 *               exception: the output may be the picture itself (in place), and nothing else.
 */
#ifndef METEOR_DEMOD_AMD_EQUALISE_H
#define METEOR_DEMOD_AMD_EQUALISE_H

#include "meteor_demod_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_EQUALISE_MAX_WIDTH   8192
#define MDEMOD_EQUALISE_MAX_HEIGHT  16384
#define MDEMOD_EQUALISE_MIN_TILE    16
#define MDEMOD_EQUALISE_MAX_TILE    512
#define MDEMOD_EQUALISE_MIN_CLIP    100
#define MDEMOD_EQUALISE_MAX_CLIP    25600
#define MDEMOD_EQUALISE_MAX_AMOUNT  256
#define MDEMOD_EQUALISE_PLANES      0          /* mode: every plane through its own tables */
#define MDEMOD_EQUALISE_LUMA        1          /* mode: the luminance through one set of tables, the planes scaled with it */

typedef struct {
	uint32_t tile;                /* 128: a multiple of 8, 16 .. 512                                                                  */
	uint32_t clip_percent;        /* 300: the clip limit in percent of a flat histogram's count, 100 .. 25 600                        */
	uint32_t amount;              /* 256: 0 (the picture as it is) .. 256 (the equalised one)                                         */
	uint32_t mode;                /* 1: MDEMOD_EQUALISE_LUMA or MDEMOD_EQUALISE_PLANES; ignored for planes 1                          */
	uint32_t valid_step;          /* 1: lines of the picture per line of the mask, 1 or 8                                             */
	uint32_t reserved[3];         /* 0                                                                                                */
} mdemod_equalise_opts;

typedef struct {
	uint32_t nx, ny, channels;    /* the tiles across and down, and the channels (1 or 3) that have tables                            */
	uint32_t empty_tiles;         /* tiles without a counted pixel                                                                    */
} mdemod_equalise_summary;

/* tile 128, clip_percent 300, amount 256, mode 1, valid_step 1. */
void mdemod_equalise_default_opts(mdemod_equalise_opts *opts);

/* Bytes of workspace for such a picture (opts NULL: the defaults); 0 for arguments out of range. */
uint64_t mdemod_equalise_workspace(uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts);

/* The tables of picture_dev[height][width][planes] under valid_dev (may be NULL) into work_dev[work_bytes]: tab and count as the
 * header says.  Device memory; the picture and the workspace at multiples of 4 bytes.  Queued on hip_stream of `device`;
 * asynchronous.  Nothing outside the picture and the mask is read and nothing outside the workspace is written. */
int  mdemod_equalise_tables_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes,
                                   const mdemod_equalise_opts *opts, void *work_dev, uint64_t work_bytes, int device, void *hip_stream);

/* The tables of work_dev (as mdemod_equalise_tables_device left them, of the same picture size and options) applied to picture_dev
 * into out_dev[height][width][planes], which may be picture_dev itself.  Asynchronous, as above. */
int  mdemod_equalise_apply_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes,
                                  const mdemod_equalise_opts *opts, const void *work_dev, uint8_t *out_dev, int device, void *hip_stream);

/* Both, one after the other on hip_stream; asynchronous. */
int  mdemod_equalise_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes,
                            const mdemod_equalise_opts *opts, void *work_dev, uint64_t work_bytes, uint8_t *out_dev, int device, void *hip_stream);

/* pixels[height][width][planes] in host memory, in place, under valid (may be NULL).  Synchronous: uploads, equalises on `device`,
 * downloads.  *out (may be NULL) receives the tile counts. */
int  mdemod_equalise_host(const mdemod_equalise_opts *opts, uint8_t *pixels, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes,
                          mdemod_equalise_summary *out, int device);

#ifdef __cplusplus
}
#endif
#endif
