/*
 * equalise.hip — the kernels and device entries of the equalise layer (include/meteor_demod_amd_equalise.h).
 *
 *   equalise_tables<PLANES, CH>   one block of 256 threads per tile.  The tile's lines are read in groups of 4 pixels that begin at
 *        a multiple of 4 pixels of the whole picture (so at a dword, whatever the line's start): PLANES dwords a group, the pixels
 *        of a group that lie outside the tile's columns are dropped, and the one group that would reach past the picture's last byte
 *        is read byte by byte.  Every wave counts into its own histograms in LDS (ds_add_u32), all channels of mode 0 from one read.
 *        Then thread v owns bin v of every channel: the four histograms are added, n and the excess are reduced in the wave and
 *        across the four waves, the running sum is a wave-level scan plus the totals of the waves before, and the table's byte and
 *        the count are stored.  No global atomics, no private workspace.
 *   equalise_apply<PLANES, CH, LUMA>   one block per slice of 32 lines of a cell between tile centres.  The four tables of every
 *        channel (1 or 3 KB) are copied to LDS as dwords; a thread then takes one pixel at a time, consecutive threads consecutive
 *        pixels of a line: it reads the pixel's bytes, looks its value up in the four tables, blends, and writes the pixel's bytes.
 *        A pixel is read before it is written by the same thread and no other pixel's output depends on it: in place works.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "equalise_host.h"
#include "hip_host.h"

#define EQ_THREADS 256
#define EQ_WAVES   (EQ_THREADS / 64)
#define EQ_SLICE   32                              /* lines of a cell that one block of equalise_apply takes */

static_assert(EQ_THREADS == 256, "a thread per bin");
static_assert(255u * 767u * 767u < (1u << 31) && 4u * 512u * 512u * 255u < (1u << 30), "the table's and the blend's sums fit 32 bits");

struct EqArgs {
	const uint8_t *picture;
	const uint8_t *valid;
	uint8_t *tab;
	uint32_t *count;
	uint8_t *out;
	EqPlan p;
};

/* the sum of x over the block's threads; part[EQ_WAVES] is LDS of this call's own */
__device__ __forceinline__ uint32_t
eq_block_sum(uint32_t x, uint32_t *part, uint32_t tid)
{
	for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
	if ((tid & 63u) == 0) part[tid >> 6] = x;
	__syncthreads();
	return part[0] + part[1] + part[2] + part[3];
}

template <int PLANES, int CH>
__global__ void __launch_bounds__(EQ_THREADS)
equalise_tables(EqArgs a)
{
	__shared__ uint32_t hist[EQ_WAVES][CH][256];
	__shared__ uint32_t part_n[CH][EQ_WAVES], part_e[CH][EQ_WAVES], part_s[CH][EQ_WAVES];
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	const uint32_t tx = blockIdx.x, ty = blockIdx.y, W = a.p.width, T = a.p.tile;
	for (uint32_t i = tid; i < EQ_WAVES * CH * 256; i += EQ_THREADS) (&hist[0][0][0])[i] = 0;
	__syncthreads();

	const uint32_t x0 = eq_tile_begin(tx, T), x1 = eq_tile_end(tx, a.p.nx, W, T);
	const uint32_t y0 = eq_tile_begin(ty, T), y1 = eq_tile_end(ty, a.p.ny, a.p.height, T);
	const uint32_t per_row = (x1 - x0 + 3u) / 4u + 1u;                          /* the groups a line of the tile can touch */
	const uint32_t items = (y1 - y0) * per_row, total = W * a.p.height * PLANES;
	for (uint32_t item = tid; item < items; item += EQ_THREADS) {
		const uint32_t r = item / per_row, y = y0 + r;
		const uint32_t l0 = y * W + x0, l1 = y * W + x1, first = (l0 / 4u + (item - r * per_row)) * 4u;
		if (first >= l1) continue;
		const uint32_t off = first * PLANES;
		uint32_t word[PLANES];
		if (off + 4u * PLANES <= total) {
			const uint32_t *src = reinterpret_cast<const uint32_t *>(a.picture + off);
#pragma unroll
			for (int k = 0; k < PLANES; k++) word[k] = src[k];
		} else {
#pragma unroll
			for (int k = 0; k < PLANES; k++) {
				word[k] = 0;
#pragma unroll
				for (int b = 0; b < 4; b++)
					if (off + 4u * k + b < total) word[k] |= static_cast<uint32_t>(a.picture[off + 4u * k + b]) << (8 * b);
			}
		}
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t l = first + j;
			if (l < l0 || l >= l1) continue;
			if (a.valid && !a.valid[(y / a.p.valid_step) * W + (l - y * W)]) continue;
			uint32_t px[PLANES];
#pragma unroll
			for (int k = 0; k < PLANES; k++) px[k] = (word[(j * PLANES + k) >> 2] >> (8 * ((j * PLANES + k) & 3))) & 255u;
			if (PLANES == 3 && CH == 1) atomicAdd(&hist[wave][0][eq_luma(px[0], px[PLANES > 1 ? 1 : 0], px[PLANES > 2 ? 2 : 0])], 1u);
			else {
#pragma unroll
				for (int c = 0; c < CH; c++) atomicAdd(&hist[wave][c][px[c < PLANES ? c : 0]], 1u);
			}
		}
	}
	__syncthreads();

	/* thread v owns bin v of every channel */
	uint32_t h[CH], n[CH], excess[CH], limit[CH], cum[CH];
#pragma unroll
	for (int c = 0; c < CH; c++) {
		h[c] = 0;
#pragma unroll
		for (int w = 0; w < EQ_WAVES; w++) h[c] += hist[w][c][tid];
		n[c] = eq_block_sum(h[c], part_n[c], tid);
		limit[c] = eq_clip_limit(a.p.clip, n[c]);
		excess[c] = eq_block_sum(h[c] > limit[c] ? h[c] - limit[c] : 0u, part_e[c], tid);
		uint32_t s = (h[c] < limit[c] ? h[c] : limit[c]) + eq_share(tid, excess[c]);
		/* the running sum within the wave, then the totals of the waves before */
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t up = __shfl_up(s, d, 64);
			if (lane >= static_cast<uint32_t>(d)) s += up;
		}
		if (lane == 63u) part_s[c][wave] = s;
		__syncthreads();
		cum[c] = s;
		for (uint32_t w = 0; w < wave; w++) cum[c] += part_s[c][w];
		const size_t t = (static_cast<size_t>(c) * a.p.ny + ty) * a.p.nx + tx;
		a.tab[t * 256u + tid] = n[c] ? static_cast<uint8_t>(eq_table_entry(cum[c], n[c])) : uint8_t(0);
		if (tid == 0) a.count[t] = n[c];
	}
}

template <int PLANES, int CH, bool LUMA>
__global__ void __launch_bounds__(EQ_THREADS)
equalise_apply(EqArgs a)
{
	__shared__ uint32_t tabs[CH][4][64];
	const uint32_t tid = threadIdx.x, W = a.p.width, H = a.p.height, T = a.p.tile, nx = a.p.nx, ny = a.p.ny;
	const uint32_t slices = (T + EQ_SLICE - 1) / EQ_SLICE, cy = blockIdx.y / slices, slice = blockIdx.y - cy * slices;
	const int32_t tx0 = static_cast<int32_t>(blockIdx.x) - 1, ty0 = static_cast<int32_t>(cy) - 1;
	/* the cell: the pixels whose first tile column is tx0 and whose first tile row is ty0 */
	const uint32_t xs = tx0 < 0 ? 0u : static_cast<uint32_t>(tx0) * T + T / 2, xe_full = static_cast<uint32_t>(tx0 + 1) * T + T / 2, xe = xe_full < W ? xe_full : W;
	const uint32_t ys_cell = ty0 < 0 ? 0u : static_cast<uint32_t>(ty0) * T + T / 2, ye_full = static_cast<uint32_t>(ty0 + 1) * T + T / 2, ye_cell = ye_full < H ? ye_full : H;
	const uint32_t ys = ys_cell + slice * EQ_SLICE, ye = ys + EQ_SLICE < ye_cell ? ys + EQ_SLICE : ye_cell;
	if (xs >= xe || ys >= ye) return;                                           /* (the whole block: nothing is waited for) */
	const uint32_t xa = tx0 < 0 ? 0u : static_cast<uint32_t>(tx0), xb = static_cast<uint32_t>(tx0 + 1) < nx ? static_cast<uint32_t>(tx0 + 1) : nx - 1u;
	const uint32_t ya = ty0 < 0 ? 0u : static_cast<uint32_t>(ty0), yb = static_cast<uint32_t>(ty0 + 1) < ny ? static_cast<uint32_t>(ty0 + 1) : ny - 1u;

	bool there[CH][4];
#pragma unroll
	for (int c = 0; c < CH; c++)
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const size_t t = (static_cast<size_t>(c) * ny + ((k & 2) ? yb : ya)) * nx + ((k & 1) ? xb : xa);
			there[c][k] = a.count[t] != 0;
		}
	for (uint32_t i = tid; i < CH * 4u * 64u; i += EQ_THREADS) {
		const uint32_t c = i >> 8, k = (i >> 6) & 3u;
		const size_t t = (static_cast<size_t>(c) * ny + ((k & 2u) ? yb : ya)) * nx + ((k & 1u) ? xb : xa);
		(&tabs[0][0][0])[i] = reinterpret_cast<const uint32_t *>(a.tab)[t * 64u + (i & 63u)];
	}
	__syncthreads();
	const uint8_t *lut = reinterpret_cast<const uint8_t *>(&tabs[0][0][0]);

	const uint32_t cw = xe - xs, pixels = cw * (ye - ys);
	const int32_t ux = 1 - static_cast<int32_t>(T) - 2 * static_cast<int32_t>(T) * tx0, uy = 1 - static_cast<int32_t>(T) - 2 * static_cast<int32_t>(T) * ty0;
	for (uint32_t i = tid; i < pixels; i += EQ_THREADS) {
		const uint32_t r = i / cw, x = xs + (i - r * cw), y = ys + r;
		const size_t at = (static_cast<size_t>(y) * W + x) * PLANES;
		uint32_t px[PLANES];
#pragma unroll
		for (int k = 0; k < PLANES; k++) px[k] = a.picture[at + k];
		if (a.valid && !a.valid[(y / a.p.valid_step) * W + x]) {
#pragma unroll
			for (int k = 0; k < PLANES; k++) a.out[at + k] = static_cast<uint8_t>(px[k]);
			continue;
		}
		const uint32_t fx = static_cast<uint32_t>(static_cast<int32_t>(2u * x) + ux), fy = static_cast<uint32_t>(static_cast<int32_t>(2u * y) + uy);
		const uint32_t wx[2] = { 2u * T - fx, fx }, wy[2] = { 2u * T - fy, fy };
		const uint32_t Y = LUMA ? eq_luma(px[0], px[PLANES > 1 ? 1 : 0], px[PLANES > 2 ? 2 : 0]) : 0u;
		uint32_t v2[CH];
#pragma unroll
		for (int c = 0; c < CH; c++) {
			const uint32_t v = LUMA ? Y : px[c < PLANES ? c : 0];
			uint32_t e[4], w[4];
#pragma unroll
			for (int k = 0; k < 4; k++) {
				e[k] = lut[(c * 4 + k) * 256 + v];
				w[k] = there[c][k] ? wy[k >> 1] * wx[k & 1] : 0u;
			}
			/* (a workspace that is not this picture's could leave no tile: the pixel stays) */
			v2[c] = w[0] + w[1] + w[2] + w[3] ? eq_amount(v, eq_blend(e, w), a.p.amount) : v;
		}
#pragma unroll
		for (int k = 0; k < PLANES; k++) a.out[at + k] = static_cast<uint8_t>(LUMA ? eq_scale(px[k], v2[0], Y) : v2[k < CH ? k : 0]);
	}
}

namespace {

EqArgs
args_of(const EqPlan &p, const uint8_t *picture, const uint8_t *valid, const void *work, uint8_t *out)
{
	EqArgs a;
	memset(&a, 0, sizeof a);
	a.picture = picture; a.valid = valid; a.out = out; a.p = p;
	a.tab = static_cast<uint8_t *>(const_cast<void *>(work));
	a.count = reinterpret_cast<uint32_t *>(a.tab + eq_tab_bytes(p));
	return a;
}

int
tables_run(const EqArgs &a, hipStream_t st)
{
	const dim3 grid(a.p.nx, a.p.ny), block(EQ_THREADS);
	if (a.p.planes == 1) hipLaunchKernelGGL((equalise_tables<1, 1>), grid, block, 0, st, a);
	else if (a.p.luma) hipLaunchKernelGGL((equalise_tables<3, 1>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((equalise_tables<3, 3>), grid, block, 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

int
apply_run(const EqArgs &a, hipStream_t st)
{
	const uint32_t slices = (a.p.tile + EQ_SLICE - 1) / EQ_SLICE;
	const dim3 grid(a.p.nx + 1, (a.p.ny + 1) * slices), block(EQ_THREADS);
	if (a.p.planes == 1) hipLaunchKernelGGL((equalise_apply<1, 1, false>), grid, block, 0, st, a);
	else if (a.p.luma) hipLaunchKernelGGL((equalise_apply<3, 1, true>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((equalise_apply<3, 3, false>), grid, block, 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

} /* namespace */

extern "C" {

int
mdemod_equalise_tables_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts,
                              void *work_dev, uint64_t work_bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_equalise_tables_device";
	EqPlan p;
	int rc = eq_check(who, width, height, planes, opts, &p);
	if (rc) return rc;
	if ((rc = eq_check_buffers(who, p, picture_dev, valid_dev, work_dev, work_bytes, nullptr, false))) return rc;
	if ((rc = mdm_select_device(device))) return rc;
	return tables_run(args_of(p, picture_dev, valid_dev, work_dev, nullptr), static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_equalise_apply_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts,
                             const void *work_dev, uint8_t *out_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_equalise_apply_device";
	EqPlan p;
	int rc = eq_check(who, width, height, planes, opts, &p);
	if (rc) return rc;
	if ((rc = eq_check_buffers(who, p, picture_dev, valid_dev, work_dev, eq_public_bytes(p), out_dev, true))) return rc;
	if ((rc = mdm_select_device(device))) return rc;
	return apply_run(args_of(p, picture_dev, valid_dev, work_dev, out_dev), static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_equalise_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes, const mdemod_equalise_opts *opts,
                       void *work_dev, uint64_t work_bytes, uint8_t *out_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_equalise_device";
	EqPlan p;
	int rc = eq_check(who, width, height, planes, opts, &p);
	if (rc) return rc;
	if ((rc = eq_check_buffers(who, p, picture_dev, valid_dev, work_dev, work_bytes, out_dev, true))) return rc;
	if ((rc = mdm_select_device(device))) return rc;
	const EqArgs a = args_of(p, picture_dev, valid_dev, work_dev, out_dev);
	if ((rc = tables_run(a, static_cast<hipStream_t>(hip_stream)))) return rc;
	return apply_run(a, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_equalise_host(const mdemod_equalise_opts *opts, uint8_t *pixels, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes,
                     mdemod_equalise_summary *out, int device)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_equalise_host";
	EqPlan p;
	int rc = eq_check(who, width, height, planes, opts, &p);
	if (rc) return rc;
	if (!pixels) { mdm_note_error("%s: the picture is needed", who); return MDEMOD_ERR_PARAM; }
	if (out) memset(out, 0, sizeof *out);
	if ((rc = mdm_select_device(device))) return rc;
	const uint64_t area = static_cast<uint64_t>(width) * height * planes, mask = static_cast<uint64_t>((height + p.valid_step - 1) / p.valid_step) * width;
	const uint64_t tiles = static_cast<uint64_t>(p.channels) * p.ny * p.nx;
	MdmDevMem mem;
	uint8_t *d_picture = nullptr, *d_valid = nullptr, *d_work = nullptr;
	if ((rc = mem.alloc(&d_picture, area)) || (rc = mem.alloc(&d_work, eq_public_bytes(p))) || (valid && (rc = mem.alloc(&d_valid, mask)))) return rc;
	HIP_TRY(hipMemcpyAsync(d_picture, pixels, area, hipMemcpyHostToDevice, nullptr));
	if (valid) HIP_TRY(hipMemcpyAsync(d_valid, valid, mask, hipMemcpyHostToDevice, nullptr));
	const EqArgs a = args_of(p, d_picture, d_valid, d_work, d_picture);
	if ((rc = tables_run(a, nullptr)) || (rc = apply_run(a, nullptr))) return rc;
	std::vector<uint32_t> count(tiles);
	HIP_TRY(hipMemcpyAsync(count.data(), a.count, tiles * 4, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipMemcpyAsync(pixels, d_picture, area, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	if (out) {
		out->nx = p.nx; out->ny = p.ny; out->channels = p.channels;
		for (uint64_t t = 0; t < static_cast<uint64_t>(p.ny) * p.nx; t++) out->empty_tiles += count[t] == 0;
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
