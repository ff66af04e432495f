/*
 * image.hip — the image layer on the GPU (include/meteor_demod_amd_image.h): packets_find in three passes, image_decode, and the
 * public entries around them.  The specification is the host model of csrc/image_host.cpp; the walk of a frame and the decoding of
 * a packet are the same text (csrc/image_host.h), compiled here for the device.
 *
 * packets_count / packets_scan / packets_fill: one lane per frame walks its headers by the demultiplexing rule (usable and linked
 *   are computed from the frames' headers and the report as the walk needs them); the first pass leaves a count per frame, one
 *   block turns the counts into exclusive offsets (each of its 1024 threads sums a run of frames, the runs are scanned in LDS) and
 *   stores the total, the third pass walks again and stores descriptors from the frame's offset on, as far as cap allows.  The
 *   list is in stream order and the same on every run: no atomics.
 * image_decode: one block is one wave, one lane per packet.  The lane's 64 coefficients live in LDS as [coefficient][lane] (int32:
 *   the first pass of the transform leaves 20-bit values there), its quantiser as [coefficient][lane] of uint16, the Huffman tables
 *   (the canonical max-code / offset walk), the zigzag order and the standard quantiser once per block.  The bytes of the stream
 *   are fetched one by one through a pointer that steps over the 10 bytes between two packet zones; nothing is copied together
 *   first.  The lane that decoded a block transforms it: both passes go eight values at a time through registers.  Stores are two
 *   dwords per row of a block and four for the report.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "image_host.h"
#include "hip_host.h"

#define IMG_THREADS 64
#define FIND_THREADS 256
#define SCAN_THREADS 1024

static_assert(sizeof(mdemod_packet) == 16 && sizeof(mdemod_strip_info) == 16 && sizeof(ImgTables) % 4 == 0, "descriptors, reports and tables are runs of dwords");

__constant__ const ImgTables img_tab = img_make_tables();

__global__ void __launch_bounds__(FIND_THREADS)
packets_count(const uint8_t *vcdu, const mdemod_rs_info *info, uint32_t n, uint32_t vcid, uint32_t *counts)
{
	const uint32_t f = blockIdx.x * FIND_THREADS + threadIdx.x;
	if (f < n) counts[f] = img_walk(vcdu, info, n, f, vcid, nullptr, 0);
}

/* counts[n] into exclusive offsets, in place; *total := their sum */
__global__ void __launch_bounds__(SCAN_THREADS)
packets_scan(uint32_t *counts, uint32_t n, unsigned long long *total)
{
	__shared__ uint32_t part[SCAN_THREADS];
	const uint32_t t = threadIdx.x, run = (n + SCAN_THREADS - 1) / SCAN_THREADS;
	const uint32_t from = min(t * run, n), to = min(from + run, n);
	uint32_t sum = 0;
	for (uint32_t i = from; i < to; i++) sum += counts[i];
	part[t] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < SCAN_THREADS; d <<= 1) {
		const uint32_t add = t >= d ? part[t - d] : 0u;
		__syncthreads();
		part[t] += add;
		__syncthreads();
	}
	uint32_t at = part[t] - sum;
	for (uint32_t i = from; i < to; i++) { const uint32_t c = counts[i]; counts[i] = at; at += c; }
	if (t == SCAN_THREADS - 1) *total = part[t];
}

__global__ void __launch_bounds__(FIND_THREADS)
packets_fill(const uint8_t *vcdu, const mdemod_rs_info *info, uint32_t n, uint32_t vcid, const uint32_t *offsets, mdemod_packet *desc, unsigned long long cap)
{
	const uint32_t f = blockIdx.x * FIND_THREADS + threadIdx.x;
	if (f >= n) return;
	const unsigned long long at = offsets[f];
	if (at < cap) img_walk(vcdu, info, n, f, vcid, desc + at, cap - at);
}

struct LdsBlk {
	int32_t *c;                                                                   /* [coefficient][lane], this lane's column */
	__device__ __forceinline__ int32_t get(uint32_t i) const { return c[i * IMG_THREADS]; }
	__device__ __forceinline__ void set(uint32_t i, int32_t v) const { c[i * IMG_THREADS] = v; }
};
struct LdsQt {
	uint16_t *q;
	__device__ __forceinline__ uint32_t get(uint32_t i) const { return q[i * IMG_THREADS]; }
	__device__ __forceinline__ void set(uint32_t i, uint32_t v) const { q[i * IMG_THREADS] = static_cast<uint16_t>(v); }
};
struct StripOut {
	uint32_t *strip;                                                              /* 224 dwords */
	__device__ __forceinline__ void put(uint32_t k, int y, uint32_t lo, uint32_t hi) const
	{
		strip[28 * y + 2 * k] = lo;
		strip[28 * y + 2 * k + 1] = hi;
	}
};

__global__ void __launch_bounds__(IMG_THREADS)
image_decode(const uint8_t *vcdu, uint32_t n, const mdemod_packet *desc, uint32_t n_desc, uint32_t *strips, uint32_t *sinfo)
{
	__shared__ ImgTables T;
	__shared__ int32_t blk[64 * IMG_THREADS];
	__shared__ uint16_t qt[64 * IMG_THREADS];
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < sizeof(ImgTables) / 4; i += IMG_THREADS) reinterpret_cast<uint32_t *>(&T)[i] = reinterpret_cast<const uint32_t *>(&img_tab)[i];
	__syncthreads();
	const uint32_t i = blockIdx.x * IMG_THREADS + lane;
	if (i >= n_desc) return;
	const mdemod_packet d = desc[i];
	const mdemod_strip_info si = img_decode_packet(T, vcdu, n, d, LdsBlk{ blk + lane }, LdsQt{ qt + lane }, StripOut{ strips + 224ull * i });
	uint32_t *r = sinfo + 4ull * i;
	r[0] = si.mcus | (static_cast<uint32_t>(si.q) << 8) | (static_cast<uint32_t>(si.mcun) << 16) | (static_cast<uint32_t>(si.flags) << 24);
	r[1] = si.day | (static_cast<uint32_t>(si.us) << 16);
	r[2] = si.ms;
	r[3] = si.bits_used;
}

namespace {

int
find_run(const mdemod_image_opts &o, const uint8_t *vcdu_dev, const mdemod_rs_info *info_dev, uint64_t n, mdemod_packet *desc_dev, uint64_t cap,
         uint64_t *total_dev, hipStream_t st)
{
	if (!n) {
		if (total_dev) HIP_TRY(hipMemsetAsync(total_dev, 0, sizeof(uint64_t), st));
		return MDEMOD_OK;
	}
	uint32_t *counts = nullptr;
	HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&counts), n * sizeof(uint32_t), st));
	const uint32_t blocks = static_cast<uint32_t>((n + FIND_THREADS - 1) / FIND_THREADS), n32 = static_cast<uint32_t>(n);
	hipLaunchKernelGGL(packets_count, dim3(blocks), dim3(FIND_THREADS), 0, st, vcdu_dev, info_dev, n32, o.vcid, counts);
	hipLaunchKernelGGL(packets_scan, dim3(1), dim3(SCAN_THREADS), 0, st, counts, n32, reinterpret_cast<unsigned long long *>(total_dev));
	if (cap) hipLaunchKernelGGL(packets_fill, dim3(blocks), dim3(FIND_THREADS), 0, st, vcdu_dev, info_dev, n32, o.vcid, counts, desc_dev, static_cast<unsigned long long>(cap));
	const hipError_t launched = hipGetLastError();
	HIP_TRY(hipFreeAsync(counts, st));
	HIP_TRY(launched);
	return MDEMOD_OK;
}

int
decode_run(const uint8_t *vcdu_dev, uint64_t n, const mdemod_packet *desc_dev, uint64_t n_desc, uint8_t *strips_dev, mdemod_strip_info *sinfo_dev, hipStream_t st)
{
	if (!n_desc) return MDEMOD_OK;
	const uint32_t blocks = static_cast<uint32_t>((n_desc + IMG_THREADS - 1) / IMG_THREADS);
	hipLaunchKernelGGL(image_decode, dim3(blocks), dim3(IMG_THREADS), 0, st, vcdu_dev, static_cast<uint32_t>(n), desc_dev, static_cast<uint32_t>(n_desc),
	                   reinterpret_cast<uint32_t *>(strips_dev), reinterpret_cast<uint32_t *>(sinfo_dev));
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* one piece of the host entry on the device */
int
device_piece(void *, const mdemod_image_opts &o, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t k, std::vector<mdemod_packet> &desc,
             std::vector<mdemod_strip_info> &sinfo, std::vector<uint8_t> &strips)
{
	hipStream_t st = nullptr;
	MdmDevMem mem;
	uint8_t *d_vcdu = nullptr, *d_strips = nullptr;
	mdemod_rs_info *d_info = nullptr;
	mdemod_packet *d_desc = nullptr;
	mdemod_strip_info *d_sinfo = nullptr;
	uint64_t *d_total = nullptr;
	int rc;
	if ((rc = mem.alloc(&d_vcdu, k * IMG_VCDU)) || (rc = mem.alloc(&d_total, 1)) || (info && (rc = mem.alloc(&d_info, k)))) return rc;
	HIP_TRY(hipMemcpyAsync(d_vcdu, vcdu, k * IMG_VCDU, hipMemcpyHostToDevice, st));
	if (info) HIP_TRY(hipMemcpyAsync(d_info, info, k * sizeof(mdemod_rs_info), hipMemcpyHostToDevice, st));
	uint64_t cap = 4 * k + 64, total = 0;
	for (int round = 0; round < 2; round++) {
		if ((rc = mem.alloc(&d_desc, cap))) return rc;
		if ((rc = find_run(o, d_vcdu, d_info, k, d_desc, cap, d_total, st))) return rc;
		HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if (total <= cap) break;
		mem.release(d_desc);
		cap = total;
	}
	desc.resize(total); sinfo.resize(total); strips.resize(total * MDEMOD_IMAGE_STRIP_BYTES);
	if (!total) return MDEMOD_OK;
	if ((rc = mem.alloc(&d_strips, total * MDEMOD_IMAGE_STRIP_BYTES)) || (rc = mem.alloc(&d_sinfo, total))) return rc;
	if ((rc = decode_run(d_vcdu, k, d_desc, total, d_strips, d_sinfo, st))) return rc;
	HIP_TRY(hipMemcpyAsync(desc.data(), d_desc, total * sizeof(mdemod_packet), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(sinfo.data(), d_sinfo, total * sizeof(mdemod_strip_info), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(strips.data(), d_strips, total * MDEMOD_IMAGE_STRIP_BYTES, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MDEMOD_OK;
}

} /* namespace */

extern "C" {

int
mdemod_packets_find_device(const mdemod_image_opts *opts, const uint8_t *vcdu_dev, const mdemod_rs_info *info_dev, uint64_t n, mdemod_packet *desc_dev,
                           uint64_t cap, uint64_t *total_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	mdemod_image_opts o;
	int rc = img_settings(opts, o);
	if (rc) return rc;
	if (n || total_dev) {
		if ((n && !vcdu_dev) || !total_dev || (n && cap && !desc_dev)) REFUSE("mdemod_packets_find_device: the VCDUs, the descriptors and the total are needed");
		if (((reinterpret_cast<uintptr_t>(vcdu_dev) | reinterpret_cast<uintptr_t>(info_dev) | reinterpret_cast<uintptr_t>(desc_dev)) & 3u) ||
		    (reinterpret_cast<uintptr_t>(total_dev) & 7u))
			REFUSE("mdemod_packets_find_device: the VCDUs, the report and the descriptors must stand at multiples of 4 bytes, the total at a multiple of 8");
		if (n > IMG_MAX_FRAMES) REFUSE("image: %llu frames are more than one batch takes (2^20)", (unsigned long long)n);
		const uint64_t in_bytes = n * IMG_VCDU, info_bytes = n * sizeof(mdemod_rs_info), out_bytes = (n ? cap : 0) * sizeof(mdemod_packet);
		if (!MdmBuffers().in(vcdu_dev, in_bytes).in(info_dev, info_bytes).out(desc_dev, out_bytes).out(total_dev, 8).apart())
			REFUSE("mdemod_packets_find_device: the VCDUs, the report, the descriptors and the total intersect");
	}
	rc = mdm_select_device(device);
	if (rc) return rc;
	return find_run(o, vcdu_dev, info_dev, n, desc_dev, cap, total_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_image_decode_device(const mdemod_image_opts *opts, const uint8_t *vcdu_dev, uint64_t n, const mdemod_packet *desc_dev, uint64_t n_desc,
                           uint8_t *strips_dev, mdemod_strip_info *sinfo_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	mdemod_image_opts o;
	int rc = img_settings(opts, o);
	if (rc) return rc;
	if (!n_desc) return MDEMOD_OK;
	if ((n && !vcdu_dev) || !desc_dev || !strips_dev || !sinfo_dev) REFUSE("mdemod_image_decode_device: the VCDUs, the descriptors, the strips and the reports are needed");
	if ((reinterpret_cast<uintptr_t>(vcdu_dev) | reinterpret_cast<uintptr_t>(desc_dev) | reinterpret_cast<uintptr_t>(strips_dev) | reinterpret_cast<uintptr_t>(sinfo_dev)) & 3u)
		REFUSE("mdemod_image_decode_device: the VCDUs, the descriptors, the strips and the reports must stand at multiples of 4 bytes");
	if (n > IMG_MAX_FRAMES) REFUSE("image: %llu frames are more than one batch takes (2^20)", (unsigned long long)n);
	if (n_desc > 0x7FFFFFFFull) REFUSE("image: %llu descriptors are more than one launch takes", (unsigned long long)n_desc);
	const uint64_t in_bytes = n * IMG_VCDU, desc_bytes = n_desc * sizeof(mdemod_packet), strip_bytes = n_desc * MDEMOD_IMAGE_STRIP_BYTES,
	               sinfo_bytes = n_desc * sizeof(mdemod_strip_info);
	if (!MdmBuffers().in(vcdu_dev, in_bytes).in(desc_dev, desc_bytes).out(strips_dev, strip_bytes).out(sinfo_dev, sinfo_bytes).apart())
		REFUSE("mdemod_image_decode_device: the VCDUs, the descriptors, the strips and the reports intersect (the lanes of one launch would read what others write)");
	rc = mdm_select_device(device);
	if (rc) return rc;
	return decode_run(vcdu_dev, n, desc_dev, n_desc, strips_dev, sinfo_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_image_decode_host(const mdemod_image_opts *opts, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, mdemod_image_result *out, int device)
try { MDEMOD_API_ENTER
	mdemod_image_opts o;
	int rc = img_settings(opts, o);
	if (rc) return rc;
	if (!out || (n && !vcdu)) REFUSE("mdemod_image_decode_host: the VCDUs and the result are needed");
	if (n > 4 * static_cast<uint64_t>(IMG_MAX_FRAMES)) REFUSE("image: %llu frames are more than a stream position counts (2^22)", (unsigned long long)n);
	if (n) {
		rc = mdm_select_device(device);
		if (rc) return rc;
	}
	return img_decode_pieces(o, vcdu, info, n, out, device_piece, nullptr);
} MDEMOD_API_CATCH

} /* extern "C" */
