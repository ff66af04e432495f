/*
 * warp_device.h — the device side of the warp, once: what a thread of map_warp (csrc/map.hip) and of mosaic_blend
 * (csrc/mosaic.hip) does to bring 4 neighbouring output pixels of one line through a cell of the node grid to source bytes.  The
 * specification is the host model of csrc/warp_model.h, which is written on its own and shares no line with this file.
 *
 * Four pixels at a multiple of 4 lie in one cell, so the cell's four nodes are read once (through the cache) and interpolated down
 * the cell's column first: L = (16 - p) X00 + p X10 and R = (16 - p) X01 + p X11, after which the numerator of pixel q is
 * 16 L + q (R - L) + 128, an addition per pixel; all of it in 64 bits, since a node may hold any int32.  The taps are byte loads
 * straight through the cache.  What does not depend on the plane (WarpTaps) is worked out once per pixel.
 */
#ifndef MDEMOD_WARP_DEVICE_H
#define MDEMOD_WARP_DEVICE_H

#include <hip/hip_runtime.h>

#include "map_host.h"

/* the numerators of the thread's first pixel, and what the next pixel of the line adds: (X, Y) = (nx >> 8, ny >> 8) */
struct WarpQuad { int64_t nx, ny, dx, dy; };

/* the four taps of a point (x, y) inside the picture: columns, fractions, line offsets, the mask cells of the columns and lines */
struct WarpTaps {
	uint32_t ix, ix2, fx, fy, o0, o1, c0, c1, r0, r1;
	bool one_cell;      /* the four taps lie in one cell: all but those at a cell's last column or a strip row's last line */
};

__device__ __forceinline__ bool
warp_no_node(const int32_t *node)
{
	return node[0] == MDEMOD_MAP_NO_NODE && node[1] == MDEMOD_MAP_NO_NODE;
}

__device__ __forceinline__ bool
warp_tap_rule(bool fa, bool fb, uint32_t a, uint32_t b, uint32_t f, uint32_t &v)
{
	v = fa && fb ? (a * (256u - f) + b * f + 128u) >> 8 : fa ? a : b;
	return fa || fb;
}

/* the cell whose first node stands at cell_nodes, for the pixels (i, j0 .. j0 + 3); false: one of its four nodes is missing */
__device__ __forceinline__ bool
warp_quad(const int32_t *cell_nodes, uint32_t node_cols, uint32_t i, uint32_t j0, WarpQuad &c)
{
	int32_t n[4][2];                                        /* 00, 10 (one down), 01 (one to the right), 11 */
	const int32_t *g = cell_nodes;
#pragma unroll
	for (int w = 0; w < 2; w++) { n[0][w] = g[w]; n[1][w] = g[2 * node_cols + w]; n[2][w] = g[2 + w]; n[3][w] = g[2 * node_cols + 2 + w]; }
	bool there = true;
#pragma unroll
	for (int k = 0; k < 4; k++) there = there && !warp_no_node(n[k]);
	const int64_t p = i & 15u, q0 = j0 & 15u;
	const int64_t lx = (16 - p) * n[0][0] + p * n[1][0], rx = (16 - p) * n[2][0] + p * n[3][0];
	const int64_t ly = (16 - p) * n[0][1] + p * n[1][1], ry = (16 - p) * n[2][1] + p * n[3][1];
	c.dx = rx - lx;
	c.dy = ry - ly;
	c.nx = 16 * lx + q0 * c.dx + 128;
	c.ny = 16 * ly + q0 * c.dy + 128;
	return there;
}

/* 0 <= x <= MAP_X_TOP, 0 <= y <= 256 last_line */
__device__ __forceinline__ WarpTaps
warp_taps(uint32_t x, uint32_t y, uint32_t last_line)
{
	WarpTaps t;
	t.ix = x >> 8; t.fx = x & 255u; t.ix2 = min(t.ix + 1, static_cast<uint32_t>(PIC_LAST));
	const uint32_t iy = y >> 8, iy2 = min(iy + 1, last_line);
	t.fy = y & 255u;
	t.c0 = t.ix / PIC_CELL_W; t.c1 = t.ix2 / PIC_CELL_W; t.r0 = (iy >> 3) * PIC_CELLS; t.r1 = (iy2 >> 3) * PIC_CELLS;
	t.o0 = iy * PIC_SRC_W; t.o1 = iy2 * PIC_SRC_W;
	t.one_cell = t.c0 == t.c1 && t.r0 == t.r1;
	return t;
}

/* the mask rule over the four taps of one plane; false: no tap counts */
__device__ __forceinline__ bool
warp_sample(const uint8_t *src, const uint8_t *cells, const WarpTaps &t, uint32_t &v)
{
	uint32_t v0, v1;
	bool f00 = cells[t.r0 + t.c0] != 0, f01 = f00, f10 = f00, f11 = f00;         /* one cell: one mask byte */
	if (!t.one_cell) { f01 = cells[t.r0 + t.c1] != 0; f10 = cells[t.r1 + t.c0] != 0; f11 = cells[t.r1 + t.c1] != 0; }
	const bool l0 = warp_tap_rule(f00, f01, src[t.o0 + t.ix], src[t.o0 + t.ix2], t.fx, v0);
	const bool l1 = warp_tap_rule(f10, f11, src[t.o1 + t.ix], src[t.o1 + t.ix2], t.fx, v1);
	return warp_tap_rule(l0, l1, v0, v1, t.fy, v);
}

/* the 4 x PLANES bytes of pixels at .. at + 3 as PLANES dwords: `at` is a multiple of 4 and the picture dword-aligned */
template <int PLANES>
__device__ __forceinline__ void
warp_store(uint8_t *out, size_t at, const uint32_t (&bytes)[4 * PLANES])
{
	uint32_t *to = reinterpret_cast<uint32_t *>(out + at * PLANES);
#pragma unroll
	for (int d = 0; d < PLANES; d++) to[d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | (bytes[4 * d + 3] << 24);
}

#endif
