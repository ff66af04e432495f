/*
 * mosaic.hip — the mosaic layer on the GPU (include/meteor_demod_amd_mosaic.h): mosaic_blend, and the public entries around it.
 * The specification is the host model of csrc/mosaic_host.cpp over csrc/warp_model.h.
 *
 * mosaic_blend: one launch makes the finished bytes; there is no accumulator image in memory and no atomic.  The geometry is
 *   map_warp's (csrc/map.hip): a block of 256 threads makes a tile of 32 x 32 output pixels, a thread makes 4 neighbouring pixels
 *   of one line, which lie in one cell of the node grid.  The loop over the passes runs inside the thread, and per pass the way from
 *   the cell's nodes to the source bytes is map_warp's own code (csrc/warp_device.h: interpolation, taps, mask rule, packing), not
 *   a copy of it.  Per pixel and plane the thread keeps two words, the weighted sum and the sum of weights (FEATHER) or
 *   the byte with its pass and the weight of the best pass so far (BEST).  The pass descriptors travel by value in the kernel arguments and are
 *   indexed by the loop counter, which is uniform: scalar loads.  All passes' tables sit in LDS (8 x planes x 256 bytes, of which
 *   n x planes x 256 are filled).  A tile of 32 x 32 pixels touches 3 x 3 nodes: every wave looks at the nine nodes of each pass
 *   with nine lanes and one ballot, and a pass none of whose nine nodes exists is skipped by a scalar branch.  The quotient of FEATHER
 *   (numerator below 2^21, divisor at most 6272) is a float reciprocal with one correction step either way: exact.  The result is
 *   4 x planes bytes packed into 3 dwords (colour) or 1 (grey); valid and cover are one dword each: the width is a multiple of 4 and
 *   the outputs dword-aligned.  Nothing but the arguments decides a byte.  The colour instance is asked to fit six waves per SIMD
 *   (76 VGPRs where the compiler takes 88 unasked: measured 5 to 6 % faster, profiles/mosaic.md); eight would spill.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "mosaic_device.h"
#include "warp_device.h"

#define MOSAIC_THREADS 256
#define MOSAIC_TILE_W  32                      /* the tile is MOSAIC_TILE_W x (4 * MOSAIC_THREADS / MOSAIC_TILE_W) pixels */
#define MOSAIC_TILE_H  (4 * MOSAIC_THREADS / MOSAIC_TILE_W)

/* one pass, the slots already resolved through select: plane p reads image[p] */
struct MosaicPass {
	const uint8_t *image[3];
	const uint8_t *filled[3];
	const uint8_t *lut;
	const int32_t *nodes;
	uint32_t rows, reserved;
};

struct MosaicBlend {
	MosaicPass pass[MOSAIC_MAX];
	uint8_t *out;
	uint8_t *valid;
	uint8_t *cover;
	uint32_t width, height, node_rows, node_cols, n, blend;
};

/* n / d for n < 2^21 and 1 <= d <= 6272: the float quotient is off by far less than 1, so one step either way makes it exact */
__device__ __forceinline__ uint32_t
mosaic_quotient(uint32_t n, uint32_t d)
{
	uint32_t q = static_cast<uint32_t>(static_cast<float>(n) * __builtin_amdgcn_rcpf(static_cast<float>(d)));
	const int32_t r = static_cast<int32_t>(n - q * d);
	if (r < 0) q--;
	else if (r >= static_cast<int32_t>(d)) q++;
	return q;
}

template <int PLANES>
__global__ void __launch_bounds__(MOSAIC_THREADS) __attribute__((amdgpu_waves_per_eu(6, 8)))
mosaic_blend(MosaicBlend a)
{
	constexpr int ACROSS = MOSAIC_TILE_W / 4;
	__shared__ uint32_t tab[MOSAIC_MAX * PLANES * 64];
	const uint32_t t = threadIdx.x;
	/* which passes have a node in this tile: lanes 0 .. 8 of every wave look at the tile's 3 x 3 nodes */
	uint32_t alive = 0;
	{
		const uint32_t m = t & 63u, nr = 2 * blockIdx.y + m / 3, nc = 2 * blockIdx.x + m % 3;
		const bool mine = m < 9 && nr < a.node_rows && nc < a.node_cols;
		for (uint32_t k = 0; k < a.n; k++) {
			bool there = false;
			if (a.pass[k].rows) {
				for (uint32_t w = t; w < PLANES * 64; w += MOSAIC_THREADS) tab[k * PLANES * 64 + w] = reinterpret_cast<const uint32_t *>(a.pass[k].lut)[w];
				if (mine) there = !warp_no_node(a.pass[k].nodes + 2 * (static_cast<size_t>(nr) * a.node_cols + nc));
			}
			if (__ballot(there)) alive |= 1u << k;
		}
	}
	const uint32_t i = blockIdx.y * MOSAIC_TILE_H + t / ACROSS, j0 = blockIdx.x * MOSAIC_TILE_W + 4 * (t % ACROSS);
	__syncthreads();
	if (i >= a.height || j0 >= a.width) return;
	const uint8_t *lut = reinterpret_cast<const uint8_t *>(tab);
	const bool feather = a.blend == MDEMOD_MOSAIC_FEATHER;
	const size_t cell = 2 * (static_cast<size_t>(i / MAP_STEP) * a.node_cols + j0 / MAP_STEP);
	uint32_t sum[4 * PLANES], weight[4 * PLANES], from = 0;
#pragma unroll
	for (int c = 0; c < 4 * PLANES; c++) sum[c] = weight[c] = 0;
	for (uint32_t k = 0; k < a.n; k++) {
		if (!((alive >> k) & 1u)) continue;
		const MosaicPass &ps = a.pass[k];
		WarpQuad c;
		if (!warp_quad(ps.nodes + cell, a.node_cols, i, j0, c)) continue;
		const int64_t y_top = (8ll * ps.rows - 1) * 256;
		const uint32_t last_line = 8 * ps.rows - 1;
		const uint8_t *tables = lut + k * PLANES * 256;
#pragma unroll
		for (int px = 0; px < 4; px++) {
			const int64_t X = c.nx >> 8, Y = c.ny >> 8;
			c.nx += c.dx;
			c.ny += c.dy;
			if (!(X >= 0 && X <= MAP_X_TOP && Y >= 0 && Y <= y_top)) continue;
			const uint32_t x = static_cast<uint32_t>(X), y = static_cast<uint32_t>(Y);
			const uint32_t e = min(min(x, static_cast<uint32_t>(MAP_X_TOP) - x), min(y, static_cast<uint32_t>(y_top) - y)), w = 1u + (e >> 8);
			const WarpTaps taps = warp_taps(x, y, last_line);
#pragma unroll
			for (int pl = 0; pl < PLANES; pl++) {
				uint32_t v;
				if (warp_sample(ps.image[pl], ps.filled[pl], taps, v)) {
					const uint32_t b = tables[256 * pl + v];
					uint32_t &s = sum[PLANES * px + pl], &d = weight[PLANES * px + pl];
					if (feather) { s += w * b; d += w; from |= (1u << k) << (8 * px); }
					else if (w > d) { s = b | (k << 8); d = w; }                      /* the byte and whose it is */
				}
			}
		}
	}
	uint32_t bytes[4 * PLANES], seen = 0;
#pragma unroll
	for (int px = 0; px < 4; px++)
#pragma unroll
		for (int pl = 0; pl < PLANES; pl++) {
			const uint32_t s = sum[PLANES * px + pl], d = weight[PLANES * px + pl];
			bytes[PLANES * px + pl] = !d ? 0u : feather ? mosaic_quotient(s + (d >> 1), d) : s & 255u;
			if (d) seen |= (1u << pl) << (8 * px);
			if (d && !feather) from |= (1u << (s >> 8)) << (8 * px);
		}
	const size_t at = static_cast<size_t>(i) * a.width + j0;
	warp_store<PLANES>(a.out, at, bytes);
	if (a.valid) *reinterpret_cast<uint32_t *>(a.valid + at) = seen;
	if (a.cover) *reinterpret_cast<uint32_t *>(a.cover + at) = from;
}

namespace {

/* nodes of every pass: from the band's first node row on */
int
blend_run(const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width, uint32_t height,
          uint8_t *out_dev, uint8_t *valid_dev, uint8_t *cover_dev, hipStream_t st)
{
	if (!n || !height) return MDEMOD_OK;
	MosaicBlend a;
	memset(&a, 0, sizeof a);
	for (uint32_t k = 0; k < n; k++) {
		if (!sources[k].rows) continue;
		for (uint32_t p = 0; p < planes; p++) { a.pass[k].image[p] = sources[k].image[select[p]]; a.pass[k].filled[p] = sources[k].filled[select[p]]; }
		a.pass[k].lut = sources[k].lut; a.pass[k].nodes = sources[k].nodes; a.pass[k].rows = sources[k].rows;
	}
	a.out = out_dev; a.valid = valid_dev; a.cover = cover_dev;
	a.width = width; a.height = height; a.node_rows = map_node_count(height); a.node_cols = map_node_count(width); a.n = n; a.blend = blend;
	const dim3 grid((width + MOSAIC_TILE_W - 1) / MOSAIC_TILE_W, (height + MOSAIC_TILE_H - 1) / MOSAIC_TILE_H);
	if (planes == 3) hipLaunchKernelGGL(mosaic_blend<3>, grid, dim3(MOSAIC_THREADS), 0, st, a);
	else hipLaunchKernelGGL(mosaic_blend<1>, grid, dim3(MOSAIC_THREADS), 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

int
blend_entry(const char *who, const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width,
            uint32_t height, uint8_t *out_dev, uint8_t *valid_dev, uint8_t *cover_dev, int device, void *hip_stream)
{
	int rc = mosaic_check_blend(who, sources, n, select, planes, blend, width, height);
	if (rc) return rc;
	if (!n || !height) return MDEMOD_OK;
	if ((rc = mosaic_check_sources(who, sources, n, select, planes))) return rc;
	if (!out_dev) REFUSE("%s: the picture is needed", who);
	uintptr_t low = reinterpret_cast<uintptr_t>(out_dev) | reinterpret_cast<uintptr_t>(valid_dev) | reinterpret_cast<uintptr_t>(cover_dev);
	for (uint32_t k = 0; k < n; k++) {
		if (!sources[k].rows) continue;
		low |= reinterpret_cast<uintptr_t>(sources[k].lut) | reinterpret_cast<uintptr_t>(sources[k].nodes);
		for (uint32_t p = 0; p < planes; p++) low |= reinterpret_cast<uintptr_t>(sources[k].image[select[p]]);
	}
	if (low & 3u) REFUSE("%s: the pictures, the tables, the nodes and the outputs must stand at multiples of 4 bytes", who);
	const uint64_t area = static_cast<uint64_t>(height) * width;
	const uint64_t node_bytes = 8ull * map_node_count(height) * map_node_count(width);
	MdmBuffers b;
	b.out(out_dev, area * planes).out(valid_dev, area).out(cover_dev, area);
	for (uint32_t k = 0; k < n; k++) {
		const mdemod_mosaic_source &s = sources[k];
		if (!s.rows) continue;
		b.in(s.lut, 256 * planes).in(s.nodes, node_bytes);
		for (uint32_t p = 0; p < planes; p++) b.in(s.image[select[p]], s.rows * PIC_LINE_BYTES).in(s.filled[select[p]], static_cast<uint64_t>(s.rows) * PIC_CELLS);
	}
	if (!b.apart()) REFUSE("%s: the outputs and the inputs intersect (the blocks of one launch would read what others write)", who);
	if ((rc = mdm_select_device(device))) return rc;
	return blend_run(sources, n, select, planes, blend, width, height, out_dev, valid_dev, cover_dev, static_cast<hipStream_t>(hip_stream));
}

} /* namespace */

int
MosaicDeviceBackend::begin(const mdemod_mosaic_pass *passes, const mdemod_mosaic_nodes &grid, uint32_t pl, uint32_t piece_lines)
{
	int rc;
	n = grid.n; width = grid.width; node_cols = grid.node_cols; planes = pl;
	node_words = 2 * static_cast<size_t>(grid.node_rows) * grid.node_cols;
	for (uint32_t k = 0; k < n; k++) {
		rows[k] = passes[k].rows;
		for (int s = 0; s < 3; s++) {
			if (!passes[k].image[s]) continue;
			if ((rc = mem.alloc(&d_image[k][s], rows[k] * PIC_LINE_BYTES)) || (rc = mem.alloc(&d_filled[k][s], static_cast<size_t>(rows[k]) * PIC_CELLS))) return rc;
			HIP_TRY(hipMemcpyAsync(d_image[k][s], passes[k].image[s], rows[k] * PIC_LINE_BYTES, hipMemcpyHostToDevice, nullptr));
			HIP_TRY(hipMemcpyAsync(d_filled[k][s], passes[k].filled[s], static_cast<size_t>(rows[k]) * PIC_CELLS, hipMemcpyHostToDevice, nullptr));
		}
		if ((rc = mem.alloc(&d_nodes[k], node_words))) return rc;
	}
	if ((rc = nodes_in(grid))) return rc;
	if ((rc = mem.alloc(&d_lut, static_cast<size_t>(MOSAIC_MAX) * 3 * 256)) || (rc = mem.alloc(&d_hist, 3 * 256)) ||
	    (rc = mem.alloc(&d_out, static_cast<size_t>(piece_lines) * width * planes)) || (rc = mem.alloc(&d_valid, static_cast<size_t>(piece_lines) * width)) ||
	    (rc = mem.alloc(&d_cover, static_cast<size_t>(piece_lines) * width)))
		return rc;
	HIP_TRY(hipStreamSynchronize(nullptr));
	return MDEMOD_OK;
}

int
MosaicDeviceBackend::nodes_in(const mdemod_mosaic_nodes &grid)
{
	for (uint32_t k = 0; k < n; k++) HIP_TRY(hipMemcpyAsync(d_nodes[k], grid.nodes[k], node_words * sizeof(int32_t), hipMemcpyHostToDevice, nullptr));
	return MDEMOD_OK;
}

int
MosaicDeviceBackend::histogram(uint32_t k, uint32_t *hist)
{
	const int rc = mdemod_picture_histogram_device(d_image[k], d_filled[k], rows[k], d_hist, device, nullptr);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(hist, d_hist, 3 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return MDEMOD_OK;
}

int
MosaicDeviceBackend::tables(const uint8_t *lut, uint32_t pl)
{
	HIP_TRY(hipMemcpyAsync(d_lut, lut, static_cast<size_t>(n) * pl * 256, hipMemcpyHostToDevice, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return MDEMOD_OK;
}

/* (the buffers are the backend's own: the public entry's overlap checks have nothing to find) */
int
MosaicDeviceBackend::band(const uint32_t *select, uint32_t pl, uint32_t blend, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid, uint8_t *cover)
{
	mdemod_mosaic_source src[MOSAIC_MAX];
	memset(src, 0, sizeof src);
	for (uint32_t k = 0; k < n; k++) {
		for (int s = 0; s < 3; s++) { src[k].image[s] = d_image[k][s]; src[k].filled[s] = d_filled[k][s]; }
		src[k].lut = d_lut + static_cast<size_t>(k) * pl * 256;
		src[k].nodes = d_nodes[k] + 2 * static_cast<size_t>(node_row) * node_cols;
		src[k].rows = rows[k];
	}
	const int rc = blend_run(src, n, select, pl, blend, width, height, d_out, d_valid, d_cover, nullptr);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(out, d_out, static_cast<size_t>(height) * width * pl, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipMemcpyAsync(valid, d_valid, static_cast<size_t>(height) * width, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipMemcpyAsync(cover, d_cover, static_cast<size_t>(height) * width, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return MDEMOD_OK;
}

extern "C" {

int
mdemod_mosaic_blend_device(const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width,
                           uint32_t height, uint8_t *out_dev, uint8_t *valid_dev, uint8_t *cover_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	return blend_entry("mdemod_mosaic_blend_device", sources, n, select, planes, blend, width, height, out_dev, valid_dev, cover_dev, device, hip_stream);
} MDEMOD_API_CATCH

int
mdemod_mosaic_compose_host(const mdemod_mosaic_opts *opts, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                           mdemod_mosaic_result *out, int device)
try { MDEMOD_API_ENTER
	if (out) memset(out, 0, sizeof *out);                                      /* (a refusal leaves nothing to free) */
	mdemod_mosaic_opts o;
	int rc = mosaic_settings(opts, o);
	if (rc) return rc;
	if ((rc = mosaic_check_compose("mdemod_mosaic_compose_host", passes, n, select, planes, out))) return rc;
	if ((rc = mdm_select_device(device))) return rc;
	MosaicDeviceBackend dev(device);
	return mosaic_compose_bands(o, passes, n, select, planes, out, dev);
} MDEMOD_API_CATCH

} /* extern "C" */
