/*
 * encoder_device.h — what the device sides of the two encoders (csrc/jpeg.hip, csrc/png.hip) share: the offset scan of the segments'
 * lengths, the check of a device entry's pointers, the result entry, the download at the end of a host entry.  For hipcc only.
 */
#ifndef MDEMOD_ENCODER_DEVICE_H
#define MDEMOD_ENCODER_DEVICE_H

#include <cstdlib>

#include "hip_host.h"

#define ENC_SCAN_THREADS 1024                   /* segments that one pass of the offset scan holds */

/* The whole block of ENC_SCAN_THREADS threads walks the lengths in chunks of that many: seg_off[i] = carry and what stands before
 * segment i, every segment with `extra` bytes behind it, in 64 bits.  Returns the carry behind the last segment. */
__device__ __forceinline__ uint64_t
enc_scan_offsets(const uint32_t *seg_len, uint64_t *seg_off, uint32_t n_seg, uint32_t extra, uint64_t carry)
{
	__shared__ uint32_t sums[ENC_SCAN_THREADS / 64];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	for (uint32_t chunk = 0; chunk < n_seg; chunk += ENC_SCAN_THREADS) {
		const uint32_t i = chunk + tid;
		const uint32_t mine = i < n_seg ? seg_len[i] + extra : 0u;
		uint32_t incl = mine;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t up = __shfl_up(incl, d, 64);
			if (lane >= static_cast<uint32_t>(d)) incl += up;
		}
		__syncthreads();                                                         /* (the sums of the chunk before have been read) */
		if (lane == 63u) sums[wave] = incl;
		__syncthreads();
		uint32_t before = 0, all = 0;
#pragma unroll
		for (uint32_t k = 0; k < ENC_SCAN_THREADS / 64; k++) {
			const uint32_t s = sums[k];
			if (k < wave) before += s;
			all += s;
		}
		if (i < n_seg) seg_off[i] = carry + before + incl - mine;
		carry += all;
	}
	return carry;
}

/* the pointers of a device entry: there, aligned, apart.  in2 may be missing; `noun` names the first input in the alignment text */
inline int
enc_check_buffers(const char *who, const char *noun, const void *in, uint64_t in_bytes, uint64_t in_align, const void *in2, uint64_t in2_bytes, const uint8_t *out,
                  uint64_t out_room, const uint64_t *result, const void *work, uint64_t work_bytes, uint64_t work_need)
{
	if (!in) REFUSE("%s: the input is needed", who);
	if (!out && out_room) REFUSE("%s: the output is needed", who);
	if (!result) REFUSE("%s: the result is needed", who);
	if (!work) REFUSE("%s: the workspace is needed", who);
	if (work_bytes < work_need) REFUSE("%s: the workspace needs %llu bytes, not %llu", who, static_cast<unsigned long long>(work_need), static_cast<unsigned long long>(work_bytes));
	if ((reinterpret_cast<uintptr_t>(work) & 15u) || (reinterpret_cast<uintptr_t>(in) & (in_align - 1))) REFUSE("%s: the workspace and the %s must stand at multiples of 16 bytes", who, noun);
	if (reinterpret_cast<uintptr_t>(result) & 7u) REFUSE("%s: the result must stand at a multiple of 8 bytes", who);
	if (!MdmBuffers().in(in, in_bytes).in(in2, in2_bytes).out(out, out_room).out(work, work_bytes).out(result, 16).apart())
		REFUSE("%s: the output, the workspace, the result and the input intersect", who);
	return MDEMOD_OK;
}

/* What an encoder left in result_dev: { the bytes the output needs, whether they fitted }.  The body of the two *_result entries. */
inline int
enc_result(const char *who, const uint64_t *result_dev, uint64_t *bytes, int device, void *hip_stream)
{
	if (!result_dev) REFUSE("%s: the result is needed", who);
	int rc = mdm_select_device(device);
	if (rc) return rc;
	uint64_t r[2] = { 0, 0 };
	HIP_TRY(hipMemcpyAsync(r, result_dev, sizeof r, hipMemcpyDeviceToHost, static_cast<hipStream_t>(hip_stream)));
	HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));
	if (bytes) *bytes = r[0];
	if (!r[1]) {
		mdm_note_error("%s: the output needs %llu bytes and out_room was less; nothing was written", who, static_cast<unsigned long long>(r[0]));
		return MDEMOD_ERR_OVERFLOW;
	}
	return MDEMOD_OK;
}

/* the end of a host entry: the n bytes at out_dev into memory that the caller frees */
inline int
enc_download(const char *who, const uint8_t *out_dev, uint64_t n, uint8_t **file, uint64_t *bytes)
{
	uint8_t *host = static_cast<uint8_t *>(malloc(n));
	if (!host) { mdm_note_error("%s: no memory for a file of %llu bytes", who, static_cast<unsigned long long>(n)); return MDEMOD_ERR_NOMEM; }
	const hipError_t e = hipMemcpy(host, out_dev, n, hipMemcpyDeviceToHost);
	if (e != hipSuccess) { free(host); HIP_TRY(e); }
	*file = host; *bytes = n;
	return MDEMOD_OK;
}

#endif
