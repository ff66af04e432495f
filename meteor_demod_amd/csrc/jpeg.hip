/*
 * jpeg.hip — the JPEG encoder on the GPU (include/meteor_demod_amd_jpeg.h): jpeg_transform, jpeg_entropy, jpeg_offsets, and the public
 * entries around them.  The specification is the host model of csrc/jpeg_host.cpp; the arithmetic of a block and the coding of a
 * block are the model's own functions (csrc/jpeg_host.h).
 *
 * jpeg_transform: one block of 256 threads per strip of 8 lines x 32 MCUs.  The strip's bytes come in line by line, neighbouring
 *   lanes taking neighbouring bytes (the last column and line repeated by clamping the index), into LDS; a colour strip is turned
 *   into three planes of level-shifted samples there.  Then a thread owns one line of one block (32 lanes: 32 blocks of one line,
 *   8 bytes apart: a ds_read_b64 without a conflict) and, after a barrier, one column of one block.  The intermediate t lies in LDS
 *   with 65 words per block, so that the lanes of a wave, which hold different blocks, hold different banks (65 and 3 x 65 are odd).
 *   The levels go to LDS at their zig-zag place and leave as one run of dwords: the blocks of a strip are adjacent in coef.
 * jpeg_entropy: one wave per restart segment, a lane per MCU.  A lane counts the bits of its MCU, a shuffle scan gives its bit
 *   offset, and it codes the MCU again into the LDS image of the segment: bits gather in a 64-bit register and leave as whole
 *   words by ds_or (the first and last word of a lane are shared with its neighbours).  Lane 0 pads.  Then 64 bytes at a time: a
 *   ballot of the FF bytes and a popcount below the lane give every byte its place behind the 00s before it.  The length pass
 *   keeps the count; the write pass, the same code, stores the bytes and the marker behind them at the segment's final offset.
 *   LDS: 208 bytes per block (the header derives it), 39 936 bytes for 64 colour MCUs, and 2176 bytes of codes.
 * jpeg_offsets: one block runs the encoders' offset scan (csrc/encoder_device.h) over the lengths, each with its marker: the total,
 *   whether it fits; it also stores the file's head and EOI, which the host made.  No global atomics anywhere.
 * The check of the entries' pointers, mdemod_jpeg_result and the host entry's download are the PNG encoder's too (csrc/encoder_device.h).
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "jpeg_host.h"
#include "encoder_device.h"

#define JT_THREADS 256
#define JT_MCUS    32                             /* MCUs of a strip */
#define JT_PITCH   65                             /* words of t per block */
#define JE_THREADS 64

static_assert(MDEMOD_JPEG_MAX_RESTART <= JE_THREADS, "a lane per MCU of a segment");
static_assert(MDEMOD_JPEG_BLOCK_BYTES * 8 >= 22 + 63 * 26 && MDEMOD_JPEG_BLOCK_BYTES % 4 == 0, "the bits of a block fit, in whole words");

__device__ const JpegCodes JPEG_CODES_DEV = jpeg_make_codes();
__device__ const JpegUnzig JPEG_UNZIG_DEV = jpeg_make_unzig();

struct JpegTransform {
	const uint8_t *picture;
	int16_t *coef;
	uint32_t width, height, mcus_x;
	uint8_t q[128];                               /* [0] luminance, [1] chrominance; natural order */
};

template <int PLANES>
__global__ void __launch_bounds__(JT_THREADS)
jpeg_transform(JpegTransform a)
{
	__shared__ __attribute__((aligned(16))) uint8_t raw[8 * 8 * JT_MCUS * PLANES];
	__shared__ __attribute__((aligned(16))) int8_t pix[PLANES][8][8 * JT_MCUS];
	__shared__ int32_t t[JT_MCUS * PLANES * JT_PITCH];
	__shared__ __attribute__((aligned(16))) int16_t zz[JT_MCUS * PLANES * 64];
	__shared__ uint32_t q[128];
	__shared__ uint8_t unzig[64];
	const uint32_t tid = threadIdx.x;
	const uint32_t mcu0 = blockIdx.x * JT_MCUS, n_mcu = min(static_cast<uint32_t>(JT_MCUS), a.mcus_x - mcu0);
	const uint32_t x0 = 8 * mcu0, cols = 8 * n_mcu, last = a.width - 1 - x0;          /* (x0 < width) */
	if (tid < 128) q[tid] = a.q[tid];
	if (tid < 64) unzig[tid] = JPEG_UNZIG_DEV.at[tid];
	for (uint32_t y = 0; y < 8; y++) {
		const uint32_t i = min(blockIdx.y * 8 + y, a.height - 1);
		const uint8_t *line = a.picture + (static_cast<size_t>(i) * a.width + x0) * PLANES;
		for (uint32_t o = tid; o < cols * PLANES; o += JT_THREADS) {
			const uint32_t x = o / PLANES, c = o - x * PLANES;
			raw[y * 8 * JT_MCUS * PLANES + o] = line[min(x, last) * PLANES + c];
		}
	}
	__syncthreads();
	for (uint32_t p = tid; p < 8 * 8 * JT_MCUS; p += JT_THREADS) {
		const uint32_t y = p / (8 * JT_MCUS), x = p % (8 * JT_MCUS);
		if (x >= cols) continue;
		if (PLANES == 1) pix[0][y][x] = static_cast<int8_t>(static_cast<int32_t>(raw[p]) - 128);
		else {
			const int32_t r = raw[3 * p], g = raw[3 * p + 1], b = raw[3 * p + 2];
#pragma unroll
			for (int c = 0; c < PLANES; c++) pix[c][y][x] = static_cast<int8_t>(jpeg_ycc(c, r, g, b) - 128);
		}
	}
	__syncthreads();
	const uint32_t b = tid % JT_MCUS, k = tid / JT_MCUS;                             /* the thread's MCU, and its line or column */
	if (b < n_mcu) {
#pragma unroll
		for (int c = 0; c < PLANES; c++) {
			const uint2 w = *reinterpret_cast<const uint2 *>(&pix[c][k][8 * b]);
			int32_t f[8], s[8];
#pragma unroll
			for (int x = 0; x < 4; x++) {
				f[x] = static_cast<int8_t>(w.x >> (8 * x));
				f[4 + x] = static_cast<int8_t>(w.y >> (8 * x));
			}
			jpeg_line(f, s);
			int32_t *to = t + (b * PLANES + c) * JT_PITCH + 8 * k;
#pragma unroll
			for (int u = 0; u < 8; u++) to[u] = s[u];
		}
	}
	__syncthreads();
	if (b < n_mcu) {
#pragma unroll
		for (int c = 0; c < PLANES; c++) {
			const int32_t *from = t + (b * PLANES + c) * JT_PITCH + k;
			int32_t col[8], R[8];
#pragma unroll
			for (int y = 0; y < 8; y++) col[y] = from[8 * y];
			jpeg_column(col, R);
			int16_t *to = zz + (b * PLANES + c) * 64;
#pragma unroll
			for (int v = 0; v < 8; v++) {
				const uint32_t n = 8 * v + k;
				to[unzig[n]] = static_cast<int16_t>(jpeg_level(R[v], q[(c ? 64 : 0) + n], n == 0));
			}
		}
	}
	__syncthreads();
	uint32_t *out = reinterpret_cast<uint32_t *>(a.coef + (static_cast<size_t>(blockIdx.y) * a.mcus_x + mcu0) * PLANES * 64);
	const uint32_t *in = reinterpret_cast<const uint32_t *>(zz);
	for (uint32_t o = tid; o < n_mcu * PLANES * 32; o += JT_THREADS) out[o] = in[o];
}

/* ---- entropy ---- */
struct JpegEntropy {
	const int16_t *coef;
	uint32_t *seg_len;                            /* [n_seg]: the length pass writes, the write pass does not read */
	const uint64_t *seg_off;                      /* [n_seg + 1]: the write pass; [n_seg] is the total */
	uint8_t *out;
	uint64_t out_room;
	uint32_t n_mcus, n_seg, ri;
};

struct JpegDevSrc {
	const int16_t *p;
	__device__ __forceinline__ void load8(int g, int16_t *w) const
	{
		const int4 v = *reinterpret_cast<const int4 *>(p + 8 * g);
		const int32_t d[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
		for (int j = 0; j < 4; j++) { w[2 * j] = static_cast<int16_t>(d[j] & 0xFFFF); w[2 * j + 1] = static_cast<int16_t>(d[j] >> 16); }
	}
};

struct JpegCount {
	uint32_t n;
	__device__ __forceinline__ void put(uint32_t, uint32_t count) { n += count; }
};

/* bits from bit `pos` of the image on; a word of the image holds its first bit at the top */
struct JpegPack {
	uint32_t *img;
	uint64_t acc;
	uint32_t fill, w;
	__device__ __forceinline__ void open(uint32_t *image, uint32_t pos) { img = image; acc = 0; fill = pos & 31u; w = pos >> 5; }
	__device__ __forceinline__ void put(uint32_t bits, uint32_t count)
	{
		acc = (acc << count) | bits;
		fill += count;
		if (fill >= 32u) {
			fill -= 32u;
			atomicOr(img + w, static_cast<uint32_t>(acc >> fill));
			w++;
			acc &= (1ull << fill) - 1ull;
		}
	}
	__device__ __forceinline__ void close() { if (fill) atomicOr(img + w, static_cast<uint32_t>(acc << (32u - fill))); }
};

template <int PLANES, class Sink>
__device__ __forceinline__ void
jpeg_code_mcu(const uint32_t *codes, const int16_t *coef, uint32_t m, bool first, Sink &sink)
{
#pragma unroll
	for (int c = 0; c < PLANES; c++) {
		const int16_t *p = coef + (static_cast<size_t>(m) * PLANES + c) * 64;
		int32_t pred = 0;
		if (!first) { pred = p[-64 * PLANES]; pred = pred < -1024 ? -1024 : pred > 1023 ? 1023 : pred; }
		const uint32_t *dc = codes + (c ? 16 : 0), *ac = codes + 32 + (c ? 256 : 0);
		jpeg_code_block(dc, ac, JpegDevSrc{ p }, pred, sink);
	}
}

template <int PLANES, bool WRITE>
__global__ void __launch_bounds__(JE_THREADS)
jpeg_entropy(JpegEntropy a)
{
	extern __shared__ uint32_t image[];           /* ri PLANES 208 bytes and two words */
	__shared__ uint32_t codes[2 * 16 + 2 * 256];
	const uint32_t seg = blockIdx.x, lane = threadIdx.x;
	uint64_t at = 0;
	if (WRITE) {
		if (a.seg_off[a.n_seg] > a.out_room) return;                             /* (uniform) it does not fit: nothing is written */
		at = a.seg_off[seg];
	}
	const uint32_t first = seg * a.ri, n = min(a.ri, a.n_mcus - first);
	const uint32_t words = n * PLANES * (MDEMOD_JPEG_BLOCK_BYTES / 4) + 2;
	static_assert(sizeof(JpegCodes) == sizeof codes, "the codes as one array of words");
	for (uint32_t i = lane; i < sizeof codes / 4; i += JE_THREADS) codes[i] = reinterpret_cast<const uint32_t *>(&JPEG_CODES_DEV)[i];
	for (uint32_t i = lane; i < words; i += JE_THREADS) image[i] = 0;
	__syncthreads();
	const bool live = lane < n;
	uint32_t bits = 0;
	if (live) {
		JpegCount count{ 0 };
		jpeg_code_mcu<PLANES>(codes, a.coef, first + lane, lane == 0, count);
		bits = count.n;
	}
	uint32_t incl = bits;
#pragma unroll
	for (int d = 1; d < JE_THREADS; d <<= 1) {
		const uint32_t up = __shfl_up(incl, d, JE_THREADS);
		if (lane >= static_cast<uint32_t>(d)) incl += up;
	}
	const uint32_t total = __shfl(incl, JE_THREADS - 1, JE_THREADS);
	if (live) {
		JpegPack pack;
		pack.open(image, incl - bits);
		jpeg_code_mcu<PLANES>(codes, a.coef, first + lane, lane == 0, pack);
		pack.close();
	}
	const uint32_t n_bytes = (total + 7u) >> 3, pad = 8u * n_bytes - total;
	if (lane == 0 && pad) atomicOr(image + (total >> 5), ((1u << pad) - 1u) << (32u - (total & 31u) - pad));
	__syncthreads();
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_bytes; base += JE_THREADS) {
		const uint32_t b = base + lane;
		const uint32_t v = b < n_bytes ? (image[b >> 2] >> (24u - 8u * (b & 3u))) & 255u : 0u;
		const unsigned long long ff = __ballot(v == 255u);
		if (WRITE && b < n_bytes) {
			uint8_t *to = a.out + at + b + carry + __popcll(ff & ((1ull << lane) - 1ull));
			to[0] = static_cast<uint8_t>(v);
			if (v == 255u) to[1] = 0;
		}
		carry += __popcll(ff);
	}
	if (lane) return;
	if (!WRITE) a.seg_len[seg] = n_bytes + carry;
	else if (seg + 1 < a.n_seg) {
		a.out[at + n_bytes + carry] = 0xFF;
		a.out[at + n_bytes + carry + 1] = static_cast<uint8_t>(0xD0 + (seg & 7u));
	}
}

/* ---- offsets ---- */
struct JpegHead {
	uint32_t n;                                   /* bytes before the first segment; with them the file ends in EOI */
	uint8_t b[JPEG_HEAD_ROOM];
};

__global__ void __launch_bounds__(ENC_SCAN_THREADS)
jpeg_offsets(const uint32_t *seg_len, uint64_t *seg_off, uint32_t n_seg, uint8_t *out, uint64_t out_room, uint64_t *result, JpegHead head)
{
	const uint32_t tid = threadIdx.x;
	const uint64_t carry = enc_scan_offsets(seg_len, seg_off, n_seg, 2u, head.n);  /* a segment and the marker behind it */
	const uint64_t total = carry - 2u + (head.n ? 2u : 0u);                       /* no marker behind the last segment; EOI */
	const bool fits = total <= out_room;
	if (tid == 0) { seg_off[n_seg] = total; result[0] = total; result[1] = fits; }
	if (!fits || !head.n) return;
	for (uint32_t i = tid; i < head.n; i += ENC_SCAN_THREADS) out[i] = head.b[i];
	if (tid == 0) { out[total - 2] = 0xFF; out[total - 1] = 0xD9; }
}

namespace {

struct JpegWork {
	int16_t *coef;
	uint64_t *seg_off;
	uint32_t *seg_len;
};

/* the workspace's parts: the coefficients (when it holds them), the offsets, the lengths */
JpegWork
carve(void *work, uint64_t coef_bytes, uint64_t n_seg)
{
	uint8_t *p = static_cast<uint8_t *>(work);
	JpegWork w;
	w.coef = reinterpret_cast<int16_t *>(p);
	w.seg_off = reinterpret_cast<uint64_t *>(p + coef_bytes);
	w.seg_len = reinterpret_cast<uint32_t *>(p + coef_bytes + (n_seg + 1) * 8);
	return w;
}

int
transform_run(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, int16_t *coef, hipStream_t st)
{
	JpegTransform a;
	memset(&a, 0, sizeof a);
	a.picture = picture; a.coef = coef; a.width = width; a.height = height; a.mcus_x = (width + 7) / 8;
	jpeg_quant_tables(quality, a.q);
	const dim3 grid((a.mcus_x + JT_MCUS - 1) / JT_MCUS, (height + 7) / 8);
	if (planes == 3) hipLaunchKernelGGL(jpeg_transform<3>, grid, dim3(JT_THREADS), 0, st, a);
	else hipLaunchKernelGGL(jpeg_transform<1>, grid, dim3(JT_THREADS), 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* the length pass and the offsets (with `lengths`), the write pass (with `write`); head: the file's, or NULL for the segments alone */
int
entropy_run(const int16_t *coef, uint64_t n_mcus, uint32_t planes, uint32_t ri, uint8_t *out, uint64_t out_room, uint64_t *result, const JpegWork &w,
            const JpegHead *head, bool lengths, bool write, hipStream_t st)
{
	JpegEntropy a;
	memset(&a, 0, sizeof a);
	a.coef = coef; a.seg_len = w.seg_len; a.seg_off = w.seg_off; a.out = out; a.out_room = out_room;
	a.n_mcus = static_cast<uint32_t>(n_mcus); a.ri = ri; a.n_seg = static_cast<uint32_t>((n_mcus + ri - 1) / ri);
	const size_t lds = static_cast<size_t>(ri) * planes * MDEMOD_JPEG_BLOCK_BYTES + 8;
	const dim3 grid(a.n_seg), block(JE_THREADS);
	if (lengths) {
		if (planes == 3) hipLaunchKernelGGL((jpeg_entropy<3, false>), grid, block, lds, st, a);
		else hipLaunchKernelGGL((jpeg_entropy<1, false>), grid, block, lds, st, a);
		HIP_TRY(hipGetLastError());
	}
	JpegHead none;
	memset(&none, 0, sizeof none);
	hipLaunchKernelGGL(jpeg_offsets, dim3(1), dim3(ENC_SCAN_THREADS), 0, st, w.seg_len, w.seg_off, a.n_seg, out, out_room, result, head ? *head : none);
	HIP_TRY(hipGetLastError());
	if (write) {
		if (planes == 3) hipLaunchKernelGGL((jpeg_entropy<3, true>), grid, block, lds, st, a);
		else hipLaunchKernelGGL((jpeg_entropy<1, true>), grid, block, lds, st, a);
		HIP_TRY(hipGetLastError());
	}
	return MDEMOD_OK;
}

} /* namespace */

extern "C" {

int
mdemod_jpeg_encode_device(const uint8_t *picture_dev, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval, uint8_t *out_dev,
                          uint64_t out_room, uint64_t *result_dev, void *work_dev, uint64_t work_bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_jpeg_encode_device";
	int rc = jpeg_check_picture(who, width, height, planes, quality, restart_interval);
	if (rc) return rc;
	const uint64_t n_mcus = jpeg_mcus(width, height), coef_bytes = n_mcus * planes * 128;
	if ((rc = enc_check_buffers(who, "coefficients", picture_dev, static_cast<uint64_t>(width) * height * planes, 1, nullptr, 0, out_dev, out_room, result_dev, work_dev,
	                            work_bytes, mdemod_jpeg_workspace(width, height, planes, restart_interval))))
		return rc;
	if ((rc = mdm_select_device(device))) return rc;
	const uint32_t ri = jpeg_interval(restart_interval);
	const JpegWork w = carve(work_dev, coef_bytes, (n_mcus + ri - 1) / ri);
	JpegHead head;
	head.n = jpeg_head(width, height, planes, quality, restart_interval, head.b);
	const hipStream_t st = static_cast<hipStream_t>(hip_stream);
	if ((rc = transform_run(picture_dev, width, height, planes, quality, w.coef, st))) return rc;
	return entropy_run(w.coef, n_mcus, planes, ri, out_dev, out_room, result_dev, w, &head, true, true, st);
} MDEMOD_API_CATCH

int
mdemod_jpeg_entropy_device(const int16_t *coef_dev, uint64_t n_mcus, uint32_t planes, uint32_t restart_interval, uint8_t *out_dev, uint64_t out_room,
                           uint64_t *result_dev, void *work_dev, uint64_t work_bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_jpeg_entropy_device";
	int rc = jpeg_check_entropy(who, n_mcus, planes, restart_interval);
	if (rc) return rc;
	if ((rc = enc_check_buffers(who, "coefficients", coef_dev, n_mcus * planes * 128, 16, nullptr, 0, out_dev, out_room, result_dev, work_dev, work_bytes,
	                            mdemod_jpeg_entropy_workspace(n_mcus, restart_interval))))
		return rc;
	if ((rc = mdm_select_device(device))) return rc;
	const uint32_t ri = jpeg_interval(restart_interval);
	const JpegWork w = carve(work_dev, 0, (n_mcus + ri - 1) / ri);
	return entropy_run(coef_dev, n_mcus, planes, ri, out_dev, out_room, result_dev, w, nullptr, true, true, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_jpeg_result(const uint64_t *result_dev, uint64_t *bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	return enc_result("mdemod_jpeg_result", result_dev, bytes, device, hip_stream);
} MDEMOD_API_CATCH

int
mdemod_jpeg_encode_host(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval, uint8_t **file,
                        uint64_t *bytes, int device)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_jpeg_encode_host";
	int rc = jpeg_check_picture(who, width, height, planes, quality, restart_interval);
	if (rc) return rc;
	if (!picture || !file || !bytes) REFUSE("%s: the picture, file and bytes are needed", who);
	*file = nullptr; *bytes = 0;
	if ((rc = mdm_select_device(device))) return rc;
	const uint64_t n_mcus = jpeg_mcus(width, height), coef_bytes = n_mcus * planes * 128, area = static_cast<uint64_t>(width) * height * planes;
	const uint32_t ri = jpeg_interval(restart_interval);
	MdmDevMem mem;
	uint8_t *d_picture = nullptr, *d_work = nullptr, *d_out = nullptr;
	uint64_t *d_result = nullptr;
	if ((rc = mem.alloc(&d_picture, area)) || (rc = mem.alloc(&d_work, mdemod_jpeg_workspace(width, height, planes, restart_interval))) || (rc = mem.alloc(&d_result, 2)))
		return rc;
	const JpegWork w = carve(d_work, coef_bytes, (n_mcus + ri - 1) / ri);
	JpegHead head;
	head.n = jpeg_head(width, height, planes, quality, restart_interval, head.b);
	HIP_TRY(hipMemcpyAsync(d_picture, picture, area, hipMemcpyHostToDevice, nullptr));
	if ((rc = transform_run(d_picture, width, height, planes, quality, w.coef, nullptr))) return rc;
	/* the lengths first: the file's size is known before its memory is asked for (the bound is 2 x 208 bytes a block) */
	if ((rc = entropy_run(w.coef, n_mcus, planes, ri, nullptr, 0, d_result, w, &head, true, false, nullptr))) return rc;
	uint64_t r[2] = { 0, 0 };
	HIP_TRY(hipMemcpyAsync(r, d_result, sizeof r, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	mem.release(d_picture);
	if ((rc = mem.alloc(&d_out, r[0]))) return rc;
	if ((rc = entropy_run(w.coef, n_mcus, planes, ri, d_out, r[0], d_result, w, &head, false, true, nullptr))) return rc;
	return enc_download(who, d_out, r[0], file, bytes);
} MDEMOD_API_CATCH

} /* extern "C" */
