/*
 * warp_model.h — the host model of the warp, once: the specification of what csrc/warp_device.h does on the GPU, as plain
 * arithmetic over the headers' text (include/meteor_demod_amd_map.h, include/meteor_demod_amd_mosaic.h).  model_warp
 * (csrc/map_host.cpp) and model_blend (csrc/mosaic_host.cpp) are loops over its two functions.  Written on its own: the plain
 * four-weight bilinear form and the tap rule with its branches, and nothing of the device header, so that a GPU test never compares
 * a thing with itself.  Free of the GPU runtime.
 */
#ifndef MDEMOD_WARP_MODEL_H
#define MDEMOD_WARP_MODEL_H

#include <initializer_list>

#include "map_host.h"

/* the tap rule: false when neither counts */
inline bool
model_tap_rule(bool fa, bool fb, uint32_t a, uint32_t b, uint32_t f, uint32_t &v)
{
	if (fa && fb) v = (a * (256u - f) + b * f + 128u) >> 8;
	else if (fa) v = a;
	else if (fb) v = b;
	else return false;
	return true;
}

/* output pixel (i, j) through nodes[][nc][2] into a picture of `rows` strip rows: (X, Y) in 1/256 pixel, or nothing (false: one
 * of the cell's four nodes is missing, or the point lies outside the picture) */
inline bool
warp_model_point(const int32_t *nodes, uint32_t nc, uint32_t rows, uint32_t i, uint32_t j, int64_t &X, int64_t &Y)
{
	const int32_t *n00 = nodes + 2 * (static_cast<size_t>(i >> 4) * nc + (j >> 4)), *n10 = n00 + 2 * nc, *n01 = n00 + 2, *n11 = n10 + 2;
	for (const int32_t *n : { n00, n10, n01, n11 })
		if (n[0] == MDEMOD_MAP_NO_NODE && n[1] == MDEMOD_MAP_NO_NODE) return false;
	const int64_t p = i & 15, q = j & 15;
	const int64_t w00 = (16 - p) * (16 - q), w10 = p * (16 - q), w01 = (16 - p) * q, w11 = p * q;
	X = (w00 * n00[0] + w10 * n10[0] + w01 * n01[0] + w11 * n11[0] + 128) >> 8;
	Y = (w00 * n00[1] + w10 * n10[1] + w01 * n01[1] + w11 * n11[1] + 128) >> 8;
	return X >= 0 && X <= MAP_X_TOP && Y >= 0 && Y <= (8ll * rows - 1) * 256;
}

/* the slot (picture `src`, mask `cells`, `rows` strip rows) at such a point: the tap rule over its four taps, or nothing */
inline bool
warp_model_value(const uint8_t *src, const uint8_t *cells, uint32_t rows, int64_t X, int64_t Y, uint32_t &v)
{
	const uint32_t last = 8 * rows - 1;
	const uint32_t ix = static_cast<uint32_t>(X >> 8), fx = static_cast<uint32_t>(X & 255), ix2 = ix + 1 < PIC_LAST ? ix + 1 : PIC_LAST;
	const uint32_t iy = static_cast<uint32_t>(Y >> 8), fy = static_cast<uint32_t>(Y & 255), iy2 = iy + 1 < last ? iy + 1 : last;
	uint32_t v0 = 0, v1 = 0;
	const bool c0 = model_tap_rule(cells[(iy / 8) * PIC_CELLS + ix / PIC_CELL_W] != 0, cells[(iy / 8) * PIC_CELLS + ix2 / PIC_CELL_W] != 0,
	                               src[static_cast<size_t>(iy) * PIC_SRC_W + ix], src[static_cast<size_t>(iy) * PIC_SRC_W + ix2], fx, v0);
	const bool c1 = model_tap_rule(cells[(iy2 / 8) * PIC_CELLS + ix / PIC_CELL_W] != 0, cells[(iy2 / 8) * PIC_CELLS + ix2 / PIC_CELL_W] != 0,
	                               src[static_cast<size_t>(iy2) * PIC_SRC_W + ix], src[static_cast<size_t>(iy2) * PIC_SRC_W + ix2], fx, v1);
	return model_tap_rule(c0, c1, v0, v1, fy, v);
}

#endif
