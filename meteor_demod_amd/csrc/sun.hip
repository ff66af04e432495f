/*
 * sun.hip — the kernel and the device entries of the sun layer (include/meteor_demod_amd_sun.h).
 *
 *   sun_apply   one block of 256 threads per strip row.  The two lines of nodes of the strip row (2 x 99 words, neighbours in the
 *        table) are copied to LDS.  A thread then takes one dword, 4 pixels of a line, at a time, consecutive threads consecutive
 *        dwords: 3136 of them per slot.  The 4 pixels lie in one cell (16 is a multiple of 4): the cell's two columns of nodes are
 *        taken down to the line once, g is computed once per pixel, and the dword of every selected slot is read, corrected and
 *        written under it.  A dword is read before the same thread writes it and no other depends on it: in place works.  The
 *        pixels held at 255 are counted per thread and slot, added in the wave and across the four waves, and stored as the block's
 *        three words of the workspace: no global atomics.
 */
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "hip_host.h"
#include "sun_host.h"

#define SUN_THREADS    256
#define SUN_WAVES      (SUN_THREADS / 64)
#define SUN_LINE_WORDS (SUN_WIDTH / 4u)            /* 392 dwords a line        */
#define SUN_ROW_WORDS  (8u * SUN_LINE_WORDS)       /* 3136 dwords a strip row  */

static_assert(SUN_WIDTH % 16u == 0 && SUN_WIDTH / 16u + 1u == MDEMOD_SUN_NODE_COLS, "a column of nodes every 16 pixels and one past the picture");
static_assert(static_cast<uint64_t>(MDEMOD_SUN_MAX_ROWS) * SUN_ROW_WORDS < (1ull << 31), "dword indices fit 32 bits");

struct SunArgs {
	const uint32_t *image[3];
	uint32_t *out[3];
	const uint32_t *gain;
	uint32_t *count;                               /* [rows][3] */
	uint32_t mask;
};

__global__ void __launch_bounds__(SUN_THREADS)
sun_apply(SunArgs a)
{
	__shared__ uint32_t node[2 * MDEMOD_SUN_NODE_COLS];
	__shared__ uint32_t part[SUN_WAVES][3];
	const uint32_t tid = threadIdx.x, row = blockIdx.x;
	if (tid < 2u * MDEMOD_SUN_NODE_COLS) node[tid] = a.gain[row * MDEMOD_SUN_NODE_COLS + tid];
	__syncthreads();

	uint32_t sat[3] = { 0, 0, 0 };
	for (uint32_t i = tid; i < SUN_ROW_WORDS; i += SUN_THREADS) {
		const uint32_t p = i / SUN_LINE_WORDS, xw = i - p * SUN_LINE_WORDS, b = xw >> 2, q0 = (xw & 3u) << 2;
		const uint32_t at = row * SUN_ROW_WORDS + i;
		/* the loads of all selected slots first: they are in flight while g is computed (the mask is the same for the whole grid) */
		uint32_t word[3] = { 0, 0, 0 };
#pragma unroll
		for (int k = 0; k < 3; k++)
			if (a.mask >> k & 1u) word[k] = a.image[k][at];
		const uint32_t g00 = node[b], g01 = node[b + 1], g10 = node[MDEMOD_SUN_NODE_COLS + b], g11 = node[MDEMOD_SUN_NODE_COLS + b + 1];
		const bool missing = sun_missing(g00, g10, g01, g11);
		const uint32_t left = sun_down(g00, g10, p), right = sun_down(g01, g11, p);
		uint32_t g[4];
#pragma unroll
		for (int j = 0; j < 4; j++) g[j] = sun_across(left, right, q0 + j);
#pragma unroll
		for (int k = 0; k < 3; k++) {
			if (!(a.mask >> k & 1u)) continue;
			const uint32_t w = word[k];
			uint32_t o = w;
			if (!missing) {
				o = 0;
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const uint32_t t = sun_scaled((w >> (8 * j)) & 255u, g[j]);
					sat[k] += t > 255u;
					o |= (t > 255u ? 255u : t) << (8 * j);
				}
			}
			a.out[k][at] = o;
		}
	}

#pragma unroll
	for (int k = 0; k < 3; k++) {
		uint32_t s = sat[k];
		for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
		if ((tid & 63u) == 0) part[tid >> 6][k] = s;
	}
	__syncthreads();
	if (tid < 3u) a.count[row * 3u + tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
}

namespace {

int
apply_run(const uint8_t *const image[3], uint8_t *const out[3], uint32_t mask, uint32_t rows, const uint32_t *gain, void *work, hipStream_t st)
{
	SunArgs a;
	memset(&a, 0, sizeof a);
	for (int k = 0; k < 3; k++) {
		if (!(mask >> k & 1u)) continue;
		a.image[k] = reinterpret_cast<const uint32_t *>(image[k]);
		a.out[k] = reinterpret_cast<uint32_t *>(out[k]);
	}
	a.gain = gain; a.count = static_cast<uint32_t *>(work); a.mask = mask;
	hipLaunchKernelGGL(sun_apply, dim3(rows), dim3(SUN_THREADS), 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

} /* namespace */

extern "C" {

int
mdemod_sun_apply_device(const uint8_t *const image_dev[3], uint8_t *const out_dev[3], uint32_t slot_mask, uint32_t rows, const uint32_t *gain_dev, void *work_dev,
                        uint64_t work_bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	int rc = sun_check_apply("mdemod_sun_apply_device", image_dev, out_dev, slot_mask, rows, gain_dev, work_dev, work_bytes, true);
	if (rc) return rc;
	if ((rc = mdm_select_device(device))) return rc;
	return apply_run(image_dev, out_dev, slot_mask, rows, gain_dev, work_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_sun_correct_host(const mdemod_sun_opts *sun_opts, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_orbit *orbit, uint8_t *const image[3], const uint32_t apids[3],
                        uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, mdemod_sun_summary *summary, int device)
try { MDEMOD_API_ENTER
	mdemod_sun_summary s;
	memset(&s, 0, sizeof s);
	if (summary) *summary = s;
	if (!rows) return MDEMOD_OK;
	std::vector<uint32_t> gain((static_cast<size_t>(rows <= MDEMOD_SUN_MAX_ROWS ? rows : 0) + 1) * MDEMOD_SUN_NODE_COLS);
	int rc = sun_prepare("mdemod_sun_correct_host", sun_opts, pass_opts, orbit, image, apids, rows, place, sinfo, n_desc, gain.data(), &s);
	if (rc) return rc;
	if (s.slot_mask) {
		if ((rc = mdm_select_device(device))) return rc;
		const size_t area = static_cast<size_t>(rows) * SUN_ROW_BYTES;
		MdmDevMem mem;
		uint8_t *d_image[3] = { nullptr, nullptr, nullptr };
		uint32_t *d_gain = nullptr, *d_work = nullptr;
		if ((rc = mem.alloc(&d_gain, gain.size())) || (rc = mem.alloc(&d_work, static_cast<size_t>(rows) * 3))) return rc;
		HIP_TRY(hipMemcpyAsync(d_gain, gain.data(), gain.size() * 4, hipMemcpyHostToDevice, nullptr));
		for (int k = 0; k < 3; k++) {
			if (!(s.slot_mask >> k & 1u)) continue;
			if ((rc = mem.alloc(&d_image[k], area))) return rc;
			HIP_TRY(hipMemcpyAsync(d_image[k], image[k], area, hipMemcpyHostToDevice, nullptr));
		}
		if ((rc = apply_run(d_image, d_image, s.slot_mask, rows, d_gain, d_work, nullptr))) return rc;
		std::vector<uint32_t> count(static_cast<size_t>(rows) * 3);
		HIP_TRY(hipMemcpyAsync(count.data(), d_work, count.size() * 4, hipMemcpyDeviceToHost, nullptr));
		/* (the pictures change only once everything has come back: a failure above leaves them as they were) */
		HIP_TRY(hipStreamSynchronize(nullptr));
		for (int k = 0; k < 3; k++)
			if (s.slot_mask >> k & 1u) HIP_TRY(hipMemcpy(image[k], d_image[k], area, hipMemcpyDeviceToHost));
		for (size_t r = 0; r < rows; r++)
			for (int k = 0; k < 3; k++) s.saturated[k] += count[r * 3 + k];
	}
	if (summary) *summary = s;
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
