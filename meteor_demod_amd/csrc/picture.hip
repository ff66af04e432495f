/*
 * picture.hip — the picture layer on the GPU (include/meteor_demod_amd_picture.h): picture_histogram, picture_render, and the
 * public entries around them.  The specification is the host model of csrc/picture_host.cpp.
 *
 * picture_histogram: a block walks strip rows (blockIdx, then in steps of the grid).  A thread reads a dword of a line, looks at
 *   the mask of the cell it lies in (112 bytes are 28 dwords: a dword never lies across two cells) and counts its four bytes with
 *   LDS atomics into uint32 [3][256]; at the end every non-zero bin goes to the output with one vector atomic add.  Integers: the
 *   order does not matter.
 * picture_render: one block per strip row.  The 8 lines of the selected slots (planes x 8 x 1568 bytes, at most 37 632) are staged
 *   into LDS with dword loads, the tables (planes x 256 bytes) and the 14-bit fill mask of each plane beside them.  A thread then
 *   makes 4 neighbouring output columns per step: it loads their 4 map entries once, turns them into taps, weights and the
 *   per-plane tap rule, and keeps all that in registers over the 8 lines; per line the taps are byte reads from LDS, the result
 *   4 x planes bytes packed into 3 dwords (colour) or 1 (grey): the width is a multiple of 4 and the output dword-aligned, so a
 *   line never starts inside a dword.  The valid byte of the 4 columns is one dword per step.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "picture_host.h"
#include "hip_host.h"

#define PIC_THREADS     256
#define PIC_ROW_DWORDS  (8 * PIC_SRC_W / 4)      /* 3136: one strip row of one slot */
#define PIC_LINE_DWORDS (PIC_SRC_W / 4)          /* 392 */
#define PIC_HIST_BLOCKS 1024

struct PicSlots {
	const uint8_t *image[3];
	const uint8_t *filled[3];
};

__global__ void __launch_bounds__(PIC_THREADS)
picture_histogram(PicSlots in, uint32_t rows, uint32_t *hist)
{
	__shared__ uint32_t bins[3 * 256];
	const uint32_t t = threadIdx.x;
	for (uint32_t i = t; i < 3 * 256; i += PIC_THREADS) bins[i] = 0;
	__syncthreads();
	for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x)
		for (int s = 0; s < 3; s++) {
			if (!in.image[s]) continue;
			const uint32_t *line = reinterpret_cast<const uint32_t *>(in.image[s]) + static_cast<size_t>(r) * PIC_ROW_DWORDS;
			const uint8_t *cells = in.filled[s] + static_cast<size_t>(r) * PIC_CELLS;
			for (uint32_t i = t; i < PIC_ROW_DWORDS; i += PIC_THREADS) {
				if (!cells[(i % PIC_LINE_DWORDS) / (PIC_CELL_W / 4)]) continue;
				const uint32_t w = line[i];
				atomicAdd(&bins[256 * s + (w & 255u)], 1u);
				atomicAdd(&bins[256 * s + ((w >> 8) & 255u)], 1u);
				atomicAdd(&bins[256 * s + ((w >> 16) & 255u)], 1u);
				atomicAdd(&bins[256 * s + (w >> 24)], 1u);
			}
		}
	__syncthreads();
	for (uint32_t i = t; i < 3 * 256; i += PIC_THREADS)
		if (bins[i]) atomicAdd(&hist[i], bins[i]);
}

/* the slots already resolved through select: plane p reads image[p] */
struct PicRender {
	const uint8_t *image[3];
	const uint8_t *filled[3];
	const uint8_t *lut;
	const uint32_t *map;
	uint8_t *out;
	uint8_t *valid;
	uint32_t width;
};

template <int PLANES>
__global__ void __launch_bounds__(PIC_THREADS)
picture_render(PicRender a)
{
	__shared__ uint32_t src[PLANES][PIC_ROW_DWORDS];
	__shared__ uint32_t tab[PLANES * 64];
	__shared__ uint32_t mask[PLANES];
	const uint32_t t = threadIdx.x, r = blockIdx.x;
#pragma unroll
	for (int p = 0; p < PLANES; p++) {
		const uint32_t *g = reinterpret_cast<const uint32_t *>(a.image[p]) + static_cast<size_t>(r) * PIC_ROW_DWORDS;
		for (uint32_t i = t; i < PIC_ROW_DWORDS; i += PIC_THREADS) src[p][i] = g[i];
	}
	for (uint32_t i = t; i < PLANES * 64; i += PIC_THREADS) tab[i] = reinterpret_cast<const uint32_t *>(a.lut)[i];
	if (t < PLANES) {
		const uint8_t *cells = a.filled[t] + static_cast<size_t>(r) * PIC_CELLS;
		uint32_t m = 0;
		for (uint32_t c = 0; c < PIC_CELLS; c++) m |= (cells[c] ? 1u : 0u) << c;
		mask[t] = m;
	}
	__syncthreads();
	const uint8_t *lut = reinterpret_cast<const uint8_t *>(tab);
	const uint32_t quads = a.width / 4;
	for (uint32_t q = t; q < quads; q += PIC_THREADS) {
		uint32_t i0[4], i1[4], f[4], rule = 0, seen = 0;           /* rule: 2 bits per (column, plane): tap a filled, tap b filled */
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint32_t m = a.map[4 * q + k];
			i0[k] = min(m >> 8, static_cast<uint32_t>(PIC_LAST));
			i1[k] = min(i0[k] + 1, static_cast<uint32_t>(PIC_LAST));
			f[k] = m & 255u;
			const uint32_t ca = i0[k] / PIC_CELL_W, cb = i1[k] / PIC_CELL_W;
#pragma unroll
			for (int p = 0; p < PLANES; p++) {
				const uint32_t fa = (mask[p] >> ca) & 1u, fb = (mask[p] >> cb) & 1u;
				rule |= (fa | (fb << 1)) << (2 * (PLANES * k + p));
				seen |= ((fa | fb) << p) << (8 * k);
			}
		}
		if (a.valid) reinterpret_cast<uint32_t *>(a.valid + static_cast<size_t>(r) * a.width)[q] = seen;
		for (uint32_t y = 0; y < 8; y++) {
			uint32_t bytes[4 * PLANES];
#pragma unroll
			for (int k = 0; k < 4; k++)
#pragma unroll
				for (int p = 0; p < PLANES; p++) {
					const uint8_t *line = reinterpret_cast<const uint8_t *>(src[p]) + y * PIC_SRC_W;
					const uint32_t va = line[i0[k]], vb = line[i1[k]], how = (rule >> (2 * (PLANES * k + p))) & 3u;
					const uint32_t v = how == 3u ? (va * (256u - f[k]) + vb * f[k] + 128u) >> 8 : how == 1u ? va : vb;
					bytes[PLANES * k + p] = how ? lut[256 * p + v] : 0u;
				}
			uint32_t *to = reinterpret_cast<uint32_t *>(a.out + ((static_cast<size_t>(r) * 8 + y) * a.width + 4 * static_cast<size_t>(q)) * PLANES);
#pragma unroll
			for (int d = 0; d < PLANES; d++)
				to[d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | (bytes[4 * d + 3] << 24);
		}
	}
}

namespace {

int
histogram_run(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, uint32_t *hist_dev, hipStream_t st)
{
	HIP_TRY(hipMemsetAsync(hist_dev, 0, 3 * 256 * sizeof(uint32_t), st));
	if (!rows) return MDEMOD_OK;
	PicSlots in;
	for (int s = 0; s < 3; s++) { in.image[s] = image[s]; in.filled[s] = filled[s]; }
	hipLaunchKernelGGL(picture_histogram, dim3(rows < PIC_HIST_BLOCKS ? rows : PIC_HIST_BLOCKS), dim3(PIC_THREADS), 0, st, in, rows, hist_dev);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

int
render_run(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes, const uint8_t *lut_dev,
           const uint32_t *map_dev, uint32_t width, uint8_t *out_dev, uint8_t *valid_dev, hipStream_t st)
{
	if (!rows) return MDEMOD_OK;
	PicRender a;
	memset(&a, 0, sizeof a);
	for (uint32_t p = 0; p < planes; p++) { a.image[p] = image[select[p]]; a.filled[p] = filled[select[p]]; }
	a.lut = lut_dev; a.map = map_dev; a.out = out_dev; a.valid = valid_dev; a.width = width;
	if (planes == 3) hipLaunchKernelGGL(picture_render<3>, dim3(rows), dim3(PIC_THREADS), 0, st, a);
	else hipLaunchKernelGGL(picture_render<1>, dim3(rows), dim3(PIC_THREADS), 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* the kernels in the whole-picture entry: one piece up, one result down, on the null stream */
struct DeviceBackend : PicBackend {
	MdmDevMem mem;
	uint8_t *d_image[3] = { nullptr, nullptr, nullptr }, *d_filled[3] = { nullptr, nullptr, nullptr }, *d_lut = nullptr, *d_out = nullptr, *d_valid = nullptr;
	uint32_t *d_hist = nullptr, *d_map = nullptr;
	uint32_t piece_rows;
	explicit DeviceBackend(uint32_t rows) : piece_rows(rows) {}

	int upload(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint8_t *di[3], const uint8_t *df[3])
	{
		int rc;
		for (int s = 0; s < 3; s++) {
			di[s] = df[s] = nullptr;
			if (!image[s]) continue;
			if (!d_image[s] && ((rc = mem.alloc(&d_image[s], piece_rows * PIC_LINE_BYTES)) || (rc = mem.alloc(&d_filled[s], static_cast<size_t>(piece_rows) * PIC_CELLS))))
				return rc;
			HIP_TRY(hipMemcpyAsync(d_image[s], image[s], rows * PIC_LINE_BYTES, hipMemcpyHostToDevice, nullptr));
			HIP_TRY(hipMemcpyAsync(d_filled[s], filled[s], static_cast<size_t>(rows) * PIC_CELLS, hipMemcpyHostToDevice, nullptr));
			di[s] = d_image[s];
			df[s] = d_filled[s];
		}
		return MDEMOD_OK;
	}

	int histogram(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, uint32_t *hist) override
	{
		const uint8_t *di[3], *df[3];
		int rc;
		if (!d_hist && (rc = mem.alloc(&d_hist, 3 * 256))) return rc;
		if ((rc = upload(image, filled, rows, di, df)) || (rc = histogram_run(di, df, rows, d_hist, nullptr))) return rc;
		HIP_TRY(hipMemcpyAsync(hist, d_hist, 3 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int render(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes, const uint8_t *lut,
	           const uint32_t *map, uint32_t width, uint8_t *out, uint8_t *valid) override
	{
		const uint8_t *di[3], *df[3];
		const size_t out_bytes = static_cast<size_t>(8) * rows * width * planes, valid_bytes = static_cast<size_t>(rows) * width;
		int rc;
		if (!d_out) {
			if ((rc = mem.alloc(&d_lut, 3 * 256)) || (rc = mem.alloc(&d_map, width)) || (rc = mem.alloc(&d_out, static_cast<size_t>(8) * piece_rows * width * planes)) ||
			    (rc = mem.alloc(&d_valid, static_cast<size_t>(piece_rows) * width)))
				return rc;
			HIP_TRY(hipMemcpyAsync(d_lut, lut, 256 * planes, hipMemcpyHostToDevice, nullptr));
			HIP_TRY(hipMemcpyAsync(d_map, map, width * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
		}
		if ((rc = upload(image, filled, rows, di, df)) || (rc = render_run(di, df, rows, select, planes, d_lut, d_map, width, d_out, d_valid, nullptr))) return rc;
		HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipMemcpyAsync(valid, d_valid, valid_bytes, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}
};

} /* namespace */

extern "C" {

int
mdemod_picture_histogram_device(const uint8_t *const image_dev[3], const uint8_t *const filled_dev[3], uint32_t rows, uint32_t *hist_dev, int device,
                                void *hip_stream)
try { MDEMOD_API_ENTER
	if (!hist_dev) REFUSE("mdemod_picture_histogram_device: the histogram is needed");
	if (reinterpret_cast<uintptr_t>(hist_dev) & 3u) REFUSE("mdemod_picture_histogram_device: the histogram must stand at a multiple of 4 bytes");
	if (rows > MDEMOD_IMAGE_MAX_ROWS) REFUSE("mdemod_picture_histogram_device: %u strip rows are more than a picture has (65536)", rows);
	const uint8_t *none[3] = { nullptr, nullptr, nullptr };
	if (rows) {
		if (!image_dev || !filled_dev) REFUSE("mdemod_picture_histogram_device: the pictures and the masks are needed");
		for (int s = 0; s < 3; s++) {
			if (image_dev[s] && !filled_dev[s]) REFUSE("mdemod_picture_histogram_device: the mask of slot %d is needed", s);
			if (reinterpret_cast<uintptr_t>(image_dev[s]) & 3u) REFUSE("mdemod_picture_histogram_device: the pictures must stand at multiples of 4 bytes");
		}
		MdmBuffers b;
		for (int s = 0; s < 3; s++) b.in(image_dev[s], rows * PIC_LINE_BYTES).in(filled_dev[s], static_cast<uint64_t>(rows) * PIC_CELLS);
		if (!b.out(hist_dev, 3 * 256 * sizeof(uint32_t)).apart())
			REFUSE("mdemod_picture_histogram_device: the histogram and the inputs intersect");
	}
	const int rc = mdm_select_device(device);
	if (rc) return rc;
	return histogram_run(rows ? image_dev : none, rows ? filled_dev : none, rows, hist_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_picture_render_device(const uint8_t *const image_dev[3], const uint8_t *const filled_dev[3], uint32_t rows, const uint32_t *select, uint32_t planes,
                             const uint8_t *lut_dev, const uint32_t *map_dev, uint32_t width, uint8_t *out_dev, uint8_t *valid_dev, int device,
                             void *hip_stream)
try { MDEMOD_API_ENTER
	int rc = pic_check_select("mdemod_picture_render_device", rows, select, planes);
	if (rc) return rc;
	if (width < 4 || width > MDEMOD_PICTURE_MAX_WIDTH || width % 4) REFUSE("mdemod_picture_render_device: the width is %u (a multiple of 4, 4 .. 8192)", width);
	if (!rows) return MDEMOD_OK;
	if ((rc = pic_check_slots("mdemod_picture_render_device", image_dev, filled_dev, select, planes))) return rc;
	if (!lut_dev || !map_dev || !out_dev) REFUSE("mdemod_picture_render_device: the tables, the map and the picture are needed");
	uintptr_t low = reinterpret_cast<uintptr_t>(lut_dev) | reinterpret_cast<uintptr_t>(map_dev) | reinterpret_cast<uintptr_t>(out_dev) | reinterpret_cast<uintptr_t>(valid_dev);
	for (uint32_t p = 0; p < planes; p++) low |= reinterpret_cast<uintptr_t>(image_dev[select[p]]);
	if (low & 3u) REFUSE("mdemod_picture_render_device: the pictures, the tables, the map and the outputs must stand at multiples of 4 bytes");
	const uint64_t out_bytes = 8ull * rows * width * planes, valid_bytes = valid_dev ? static_cast<uint64_t>(rows) * width : 0;
	MdmBuffers b;
	for (uint32_t p = 0; p < planes; p++) b.in(image_dev[select[p]], rows * PIC_LINE_BYTES).in(filled_dev[select[p]], static_cast<uint64_t>(rows) * PIC_CELLS);
	if (!b.in(lut_dev, 256 * planes).in(map_dev, 4ull * width).out(out_dev, out_bytes).out(valid_dev, valid_bytes).apart())
		REFUSE("mdemod_picture_render_device: the outputs and the inputs intersect (the blocks of one launch would read what others write)");
	if ((rc = mdm_select_device(device))) return rc;
	return render_run(image_dev, filled_dev, rows, select, planes, lut_dev, map_dev, width, out_dev, valid_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_picture_compose_host(const mdemod_picture_opts *opts, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                            const uint32_t *select, uint32_t planes, mdemod_picture_result *out, int device)
try { MDEMOD_API_ENTER
	mdemod_picture_opts o;
	int rc = pic_settings(opts, o);
	if (rc) return rc;
	if (!out) REFUSE("mdemod_picture_compose_host: the result is needed");
	if ((rc = pic_check_select("mdemod_picture_compose_host", rows, select, planes))) return rc;
	if (rows && (rc = pic_check_slots("mdemod_picture_compose_host", image, filled, select, planes))) return rc;
	if (rows && (rc = mdm_select_device(device))) return rc;
	DeviceBackend dev(o.piece_rows < rows ? o.piece_rows : rows);
	return pic_compose_pieces(o, image, filled, rows, select, planes, out, dev);
} MDEMOD_API_CATCH

} /* extern "C" */
