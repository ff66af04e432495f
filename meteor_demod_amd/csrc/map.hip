/*
 * map.hip — the map layer on the GPU (include/meteor_demod_amd_map.h): map_warp, and the public entries around it.  The
 * specification is the host model of csrc/map_host.cpp over csrc/warp_model.h.
 *
 * map_warp: a block of 256 threads makes a tile of 32 x 32 output pixels (64 x 16 and 128 x 8 were measured beside it and were
 *   slower); a thread makes 4 neighbouring pixels of one line.  Four pixels at a multiple of 4 lie in one cell of the node grid, so
 *   the thread reads the cell's four nodes once (through the cache: a copy of the tile's nodes in LDS gained nothing).  From the
 *   nodes to the source bytes the thread's work is csrc/warp_device.h, shared with mosaic_blend: the interpolation, the taps, the
 *   mask rule and the packing.  The taps are byte loads straight through the cache:
 *   the source of a tile is a slanted quadrilateral whose bounding box depends on the nodes, neighbouring threads read neighbouring
 *   bytes, and every source byte is used by the one or two tiles it falls into (profiles/map.md has what was tried, with times).
 *   The tables (planes x 256 bytes) sit in LDS.  The result is 4 x planes bytes packed into 3 dwords (colour) or 1 (grey), and
 *   the four valid bytes are one dword: the width is a multiple of 4 and the outputs dword-aligned.  No atomics, and nothing but
 *   the arguments decides a byte.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "map_host.h"
#include "hip_host.h"
#include "warp_device.h"

#define MAP_THREADS 256
#define MAP_TILE_W  32                      /* the tile is MAP_TILE_W x (4 * MAP_THREADS / MAP_TILE_W) pixels */
#define MAP_TILE_H  (4 * MAP_THREADS / MAP_TILE_W)

/* the slots already resolved through select: plane p reads image[p] */
struct MapWarp {
	const uint8_t *image[3];
	const uint8_t *filled[3];
	const uint8_t *lut;
	const int32_t *nodes;
	uint8_t *out;
	uint8_t *valid;
	uint32_t width, height, rows, node_cols;
};

template <int PLANES>
__global__ void __launch_bounds__(MAP_THREADS)
map_warp(MapWarp a)
{
	constexpr int ACROSS = MAP_TILE_W / 4;
	__shared__ uint32_t tab[PLANES * 64];
	const uint32_t t = threadIdx.x;
	for (uint32_t k = t; k < PLANES * 64; k += MAP_THREADS) tab[k] = reinterpret_cast<const uint32_t *>(a.lut)[k];
	const uint32_t i = blockIdx.y * MAP_TILE_H + t / ACROSS, j0 = blockIdx.x * MAP_TILE_W + 4 * (t % ACROSS);
	__syncthreads();
	if (i >= a.height || j0 >= a.width) return;
	const uint8_t *lut = reinterpret_cast<const uint8_t *>(tab);
	WarpQuad c;
	const bool there = warp_quad(a.nodes + 2 * (static_cast<size_t>(i / MAP_STEP) * a.node_cols + j0 / MAP_STEP), a.node_cols, i, j0, c);
	const int64_t y_top = (8ll * a.rows - 1) * 256;
	const uint32_t last_line = 8 * a.rows - 1;
	uint32_t bytes[4 * PLANES], seen = 0;
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const int64_t X = c.nx >> 8, Y = c.ny >> 8;
		c.nx += c.dx;
		c.ny += c.dy;
#pragma unroll
		for (int pl = 0; pl < PLANES; pl++) bytes[PLANES * k + pl] = 0;
		if (!(there && X >= 0 && X <= MAP_X_TOP && Y >= 0 && Y <= y_top)) continue;
		const WarpTaps taps = warp_taps(static_cast<uint32_t>(X), static_cast<uint32_t>(Y), last_line);
#pragma unroll
		for (int pl = 0; pl < PLANES; pl++) {
			uint32_t v;
			if (warp_sample(a.image[pl], a.filled[pl], taps, v)) {
				bytes[PLANES * k + pl] = lut[256 * pl + v];
				seen |= (1u << pl) << (8 * k);
			}
		}
	}
	const size_t at = static_cast<size_t>(i) * a.width + j0;
	warp_store<PLANES>(a.out, at, bytes);
	if (a.valid) *reinterpret_cast<uint32_t *>(a.valid + at) = seen;
}

namespace {

int
warp_run(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes, const uint8_t *lut_dev,
         const int32_t *nodes_dev, uint32_t width, uint32_t height, uint8_t *out_dev, uint8_t *valid_dev, hipStream_t st)
{
	if (!rows || !height) return MDEMOD_OK;
	MapWarp a;
	memset(&a, 0, sizeof a);
	for (uint32_t p = 0; p < planes; p++) { a.image[p] = image[select[p]]; a.filled[p] = filled[select[p]]; }
	a.lut = lut_dev; a.nodes = nodes_dev; a.out = out_dev; a.valid = valid_dev;
	a.width = width; a.height = height; a.rows = rows; a.node_cols = map_node_count(width);
	const dim3 grid((width + MAP_TILE_W - 1) / MAP_TILE_W, (height + MAP_TILE_H - 1) / MAP_TILE_H);
	if (planes == 3) hipLaunchKernelGGL(map_warp<3>, grid, dim3(MAP_THREADS), 0, st, a);
	else hipLaunchKernelGGL(map_warp<1>, grid, dim3(MAP_THREADS), 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

int
warp_entry(const char *who, const uint8_t *const image_dev[3], const uint8_t *const filled_dev[3], uint32_t rows, const uint32_t *select, uint32_t planes,
           const uint8_t *lut_dev, const int32_t *nodes_dev, uint32_t width, uint32_t height, uint8_t *out_dev, uint8_t *valid_dev, int device,
           void *hip_stream)
{
	int rc = map_check_warp(who, rows, select, planes, width, height);
	if (rc) return rc;
	if (!rows || !height) return MDEMOD_OK;
	if ((rc = pic_check_slots(who, image_dev, filled_dev, select, planes))) return rc;
	if (!lut_dev || !nodes_dev || !out_dev) REFUSE("%s: the tables, the nodes and the picture are needed", who);
	uintptr_t low = reinterpret_cast<uintptr_t>(lut_dev) | reinterpret_cast<uintptr_t>(nodes_dev) | reinterpret_cast<uintptr_t>(out_dev) | reinterpret_cast<uintptr_t>(valid_dev);
	for (uint32_t p = 0; p < planes; p++) low |= reinterpret_cast<uintptr_t>(image_dev[select[p]]);
	if (low & 3u) REFUSE("%s: the pictures, the tables, the nodes and the outputs must stand at multiples of 4 bytes", who);
	const uint64_t area = static_cast<uint64_t>(height) * width;
	MdmBuffers b;
	b.in(lut_dev, 256 * planes).in(nodes_dev, 8ull * map_node_count(height) * map_node_count(width)).out(out_dev, area * planes).out(valid_dev, area);
	for (uint32_t p = 0; p < planes; p++) b.in(image_dev[select[p]], rows * PIC_LINE_BYTES).in(filled_dev[select[p]], static_cast<uint64_t>(rows) * PIC_CELLS);
	if (!b.apart()) REFUSE("%s: the outputs and the inputs intersect (the blocks of one launch would read what others write)", who);
	if ((rc = mdm_select_device(device))) return rc;
	return warp_run(image_dev, filled_dev, rows, select, planes, lut_dev, nodes_dev, width, height, out_dev, valid_dev, static_cast<hipStream_t>(hip_stream));
}

/* the kernel in the whole-map entry: the slots and the nodes up once, one band down at a time, on the null stream */
struct DeviceBackend : MapBackend {
	MdmDevMem mem;
	uint8_t *d_image[3] = { nullptr, nullptr, nullptr }, *d_filled[3] = { nullptr, nullptr, nullptr }, *d_lut = nullptr, *d_out = nullptr, *d_valid = nullptr;
	int32_t *d_nodes = nullptr;
	uint32_t *d_hist = nullptr;
	uint32_t rows = 0, width = 0, node_cols = 0;
	int device;
	explicit DeviceBackend(int dev) : device(dev) {}

	int begin(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t r, const mdemod_map_nodes &grid, uint32_t planes, uint32_t piece_lines) override
	{
		int rc;
		rows = r; width = grid.width; node_cols = grid.node_cols;
		for (int s = 0; s < 3; s++) {
			if (!image[s]) continue;
			if ((rc = mem.alloc(&d_image[s], rows * PIC_LINE_BYTES)) || (rc = mem.alloc(&d_filled[s], static_cast<size_t>(rows) * PIC_CELLS))) return rc;
			HIP_TRY(hipMemcpyAsync(d_image[s], image[s], rows * PIC_LINE_BYTES, hipMemcpyHostToDevice, nullptr));
			HIP_TRY(hipMemcpyAsync(d_filled[s], filled[s], static_cast<size_t>(rows) * PIC_CELLS, hipMemcpyHostToDevice, nullptr));
		}
		const size_t node_words = 2 * static_cast<size_t>(grid.node_rows) * grid.node_cols;
		if ((rc = mem.alloc(&d_nodes, node_words)) || (rc = mem.alloc(&d_lut, 3 * 256)) || (rc = mem.alloc(&d_hist, 3 * 256)) ||
		    (rc = mem.alloc(&d_out, static_cast<size_t>(piece_lines) * width * planes)) || (rc = mem.alloc(&d_valid, static_cast<size_t>(piece_lines) * width)))
			return rc;
		HIP_TRY(hipMemcpyAsync(d_nodes, grid.nodes, node_words * sizeof(int32_t), hipMemcpyHostToDevice, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int histogram(uint32_t *hist) override
	{
		const int rc = mdemod_picture_histogram_device(d_image, d_filled, rows, d_hist, device, nullptr);
		if (rc) return rc;
		HIP_TRY(hipMemcpyAsync(hist, d_hist, 3 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int tables(const uint8_t *lut, uint32_t planes) override
	{
		HIP_TRY(hipMemcpyAsync(d_lut, lut, 256 * planes, hipMemcpyHostToDevice, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int band(const uint32_t *select, uint32_t planes, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid) override
	{
		const int rc = warp_run(d_image, d_filled, rows, select, planes, d_lut, d_nodes + 2 * static_cast<size_t>(node_row) * node_cols, width, height, d_out,
		                        d_valid, nullptr);
		if (rc) return rc;
		HIP_TRY(hipMemcpyAsync(out, d_out, static_cast<size_t>(height) * width * planes, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipMemcpyAsync(valid, d_valid, static_cast<size_t>(height) * width, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}
};

} /* namespace */

extern "C" {

int
mdemod_map_warp_device(const uint8_t *const image_dev[3], const uint8_t *const filled_dev[3], uint32_t rows, const uint32_t *select, uint32_t planes,
                       const uint8_t *lut_dev, const int32_t *nodes_dev, uint32_t width, uint32_t height, uint8_t *out_dev, uint8_t *valid_dev, int device,
                       void *hip_stream)
try { MDEMOD_API_ENTER
	return warp_entry("mdemod_map_warp_device", image_dev, filled_dev, rows, select, planes, lut_dev, nodes_dev, width, height, out_dev, valid_dev, device,
	                  hip_stream);
} MDEMOD_API_CATCH

int
mdemod_map_compose_host(const mdemod_map_opts *opts, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                        const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select, uint32_t planes,
                        mdemod_map_result *out, int device)
try { MDEMOD_API_ENTER
	mdemod_map_opts o;
	int rc = map_settings(opts, o);
	if (rc) return rc;
	if ((rc = map_check_compose("mdemod_map_compose_host", tle, image, filled, rows, place, sinfo, n_desc, select, planes, out))) return rc;
	if ((rc = mdm_select_device(device))) return rc;
	DeviceBackend dev(device);
	return map_compose_bands(o, tle, image, filled, rows, place, sinfo, n_desc, select, planes, out, dev);
} MDEMOD_API_CATCH

} /* extern "C" */
