/*
 * rs.hip — the transfer-frame layer on the GPU (include/meteor_demod_amd_rs.h): one kernel, and the public entries around it.  The
 * specification is the host model of csrc/rs_host.cpp; the tables are the same compile-time tables (csrc/rs_host.h).
 *
 * rs_decode: one block of 256 threads per CADU, wave c owns codeword c.
 *   In: the row is 256 dwords.  Thread t >= 1 loads dword t: position t - 1 of all four codewords.  It takes the randomiser's dword
 *   off (the sequence laid out over the whole frame: one coalesced dword per thread too), sends each byte through Tinv when the dual
 *   basis is asked for, and scatters the four bytes to four LDS rows of 256 bytes.  192 threads bring the antilog / log tables to LDS.
 *   Syndromes: lane = 32 half + k.  Root k runs Horner's rule over positions 0 .. 127 (half 0) or 128 .. 254 (half 1): per step one
 *   broadcast read of the word and a multiplication by the lane's root, exp[log[acc] + log root].  The halves meet through one
 *   __shfl and a multiplication by root^127.  One __ballot: no syndrome, no work - the wave leaves with corrected = 0.
 *   Otherwise, all in registers and across lanes (no LDS write that another lane of the wave reads back): Berlekamp-Massey in 32
 *   counted steps, lane j holding the terms C_j and B_j (the discrepancy is an xor-reduction over __shfl_xor, the shift of B a
 *   __shfl_up); Omega_k = sum C_j S_(k-j) on lane k; Chien and Forney over positions lane + 64 q, q = 0 .. 3, the 17 terms of
 *   Lambda and the 16 of Omega read across by v_readlane.  The roots are counted by __ballot; only when there are exactly L <= 16
 *   of them do the lanes that hold one xor their value into the word.
 *   Out: after the block's second barrier thread t < 223 gathers position t of the four rows (through T for the dual basis) and stores
 *   dword t of the VCDU; thread 0 stores the report.
 * Every branch between the two barriers is uniform over a wave; no loop's trip count depends on data.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "rs_host.h"
#include "hip_host.h"

#define RS_THREADS 256
#define RS_ROW_DWORDS (MDEMOD_RS_CADU_BYTES / 4)           /* 256 */
#define RS_OUT_DWORDS (MDEMOD_RS_VCDU_BYTES / 4)           /* 223 */

static_assert(offsetof(RsTables, log) == 512 && offsetof(RsTables, pn) == 768, "rs_decode copies exp and log as one run of dwords");
static_assert(sizeof(mdemod_rs_info) == 8 && RS_OUT_DWORDS == RS_K, "a VCDU row is one dword per data position");

__constant__ const RsTables rs_tab = rs_make_tables();

struct alignas(16) RsLds {
	uint8_t  exp[512];
	uint8_t  log[256];
	uint8_t  w[RS_DEPTH][256];                             /* the four words; w[c][255] is 0 */
	uint32_t corrected[RS_DEPTH];
};

/* a alpha^lb, lb < 256 */
__device__ __forceinline__ uint32_t
rs_mul(const RsLds &s, uint32_t a, uint32_t lb)
{
	return a ? s.exp[s.log[a] + lb] : 0u;
}

/* the wave's word has syndromes S (lane k < 32: S_k; 0 elsewhere), not all zero: corrects it in LDS, or leaves it.  Returns what
 * the report says. */
__device__ __forceinline__ uint32_t
rs_fix(RsLds &s, uint8_t *w, uint32_t S, uint32_t lane)
{
	/* ---- Berlekamp-Massey: lane j holds C_j and B_j; L, log b and the discrepancy are the wave's ---- */
	uint32_t C = lane == 0, B = C, L = 0, lb = 0;
	for (uint32_t n = 0; n < RS_ROOTS; n++) {
		B = static_cast<uint32_t>(__shfl_up(static_cast<int>(B), 1));
		if (lane == 0) B = 0;
		const int from = static_cast<int>(n) - static_cast<int>(lane);
		uint32_t sv = static_cast<uint32_t>(__shfl(static_cast<int>(S), from & 63));
		if (from < 0) sv = 0;
		uint32_t term = (C && sv) ? s.exp[s.log[C] + s.log[sv]] : 0u;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) term ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(term), d));
		const uint32_t d = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(term)));
		if (d) {
			const uint32_t ld = s.log[d];
			uint32_t lf = ld + 255u - lb;                      /* log (d / b) */
			if (lf >= 255u) lf -= 255u;
			const uint32_t T = C;
			C ^= rs_mul(s, B, lf);
			if (2 * L <= n) { L = n + 1 - L; B = T; lb = ld; }
		}
	}
	if (L > RS_T) return MDEMOD_RS_FAILED;

	/* ---- Omega_k = sum_j C_j S_(k-j), k < 16, on lane k ---- */
	const uint32_t lC = s.log[C];
	uint32_t om = 0;
#pragma unroll
	for (int j = 0; j <= RS_T; j++) {
		const uint32_t cj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(C), j));
		const uint32_t lcj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lC), j));
		const int from = static_cast<int>(lane) - j;
		uint32_t sv = static_cast<uint32_t>(__shfl(static_cast<int>(S), from & 63));
		if (from < 0) sv = 0;
		if (cj) om ^= rs_mul(s, sv, lcj);
	}
	if (lane >= RS_T) om = 0;
	const uint32_t lOm = s.log[om];

	/* ---- Chien and Forney: positions lane + 64 q ---- */
	uint32_t value[4], roots = 0;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const uint32_t i = lane + 64u * q;
		const uint32_t lx = (RS_PRIM * (254u - min(i, 254u))) % 255u;     /* log X_i */
		const uint32_t step = lx ? 255u - lx : 0u;                         /* log (1 / X_i) */
		uint32_t lam = 0, odd = 0, omv = 0, e = 0;                          /* e = j step mod 255 */
#pragma unroll
		for (int j = 0; j <= RS_T; j++) {
			const uint32_t cj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(C), j));
			const uint32_t lcj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lC), j));
			if (cj) {
				const uint32_t term = s.exp[lcj + e];
				lam ^= term;
				if (j & 1) odd ^= term;
			}
			if (j < RS_T) {
				const uint32_t oj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(om), j));
				const uint32_t loj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lOm), j));
				if (oj) omv ^= s.exp[loj + e];
			}
			e += step;
			if (e >= 255u) e -= 255u;
		}
		const bool root = i < RS_N && lam == 0;
		roots += static_cast<uint32_t>(__popcll(__ballot(root)));
		/* X^(-112) Omega(1 / X) / (x Lambda'(x) at 1 / X) */
		const uint32_t lv = s.log[omv] + 255u - s.log[odd] + (112u * (255u - lx)) % 255u;
		value[q] = (root && omv && odd) ? s.exp[lv % 255u] : 0u;
	}
	if (roots != L) return MDEMOD_RS_FAILED;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const uint32_t i = lane + 64u * q;
		if (value[q]) w[i] ^= static_cast<uint8_t>(value[q]);
	}
	return L;
}

__global__ void __launch_bounds__(RS_THREADS)
rs_decode(const uint32_t *cadu, uint32_t *vcdu, uint32_t *info, uint32_t derandomise, uint32_t dual)
{
	__shared__ RsLds s;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, c = tid >> 6;
	const uint32_t *row = cadu + static_cast<uint64_t>(blockIdx.x) * RS_ROW_DWORDS;

	if (tid < 192) reinterpret_cast<uint32_t *>(s.exp)[tid] = reinterpret_cast<const uint32_t *>(rs_tab.exp)[tid];
	if (tid >= 1) {
		uint32_t d = row[tid];
		if (derandomise) d ^= reinterpret_cast<const uint32_t *>(rs_tab.pn)[tid - 1];
#pragma unroll
		for (int k = 0; k < RS_DEPTH; k++) {
			uint32_t b = (d >> (8 * k)) & 0xFFu;
			if (dual) b = rs_tab.Tinv[b];
			s.w[k][tid - 1] = static_cast<uint8_t>(b);
		}
	} else {
#pragma unroll
		for (int k = 0; k < RS_DEPTH; k++) s.w[k][255] = 0;
	}
	__syncthreads();

	/* ---- syndromes: S_k = w(beta^(112 + k)) on lane k < 32 ---- */
	uint8_t *w = s.w[c];
	const uint32_t half = lane >> 5;
	const uint32_t lroot = (RS_PRIM * (RS_FCR + (lane & 31u))) % 255u;
	uint32_t acc = 0;
	for (uint32_t j = 0; j < 128; j++) {
		const uint32_t r = w[j + 127u * half];
		acc = rs_mul(s, acc, lroot) ^ ((half && j == 0) ? 0u : r);             /* half 1: positions 128 .. 254, one step late */
	}
	const uint32_t low = static_cast<uint32_t>(__shfl(static_cast<int>(acc), (lane + 32u) & 63u));
	uint32_t S = rs_mul(s, acc, (127u * lroot) % 255u) ^ low;
	if (half) S = 0;

	uint32_t corrected = 0;
	if (__ballot(S != 0)) corrected = rs_fix(s, w, S, lane);
	if (lane == 0) s.corrected[c] = corrected;
	__syncthreads();

	if (tid < RS_OUT_DWORDS) {
		uint32_t d = 0;
#pragma unroll
		for (int k = 0; k < RS_DEPTH; k++) {
			uint32_t b = s.w[k][tid];
			if (dual) b = rs_tab.T[b];
			d |= b << (8 * k);
		}
		vcdu[static_cast<uint64_t>(blockIdx.x) * RS_OUT_DWORDS + tid] = d;
	}
	if (tid == 0) {
		uint32_t word = 0, flags = 0;
#pragma unroll
		for (int k = 0; k < RS_DEPTH; k++) {
			word |= s.corrected[k] << (8 * k);
			if (s.corrected[k] == MDEMOD_RS_FAILED) flags |= MDEMOD_RS_UNCORRECTABLE;
		}
		info[2ull * blockIdx.x] = word;
		info[2ull * blockIdx.x + 1] = flags;
	}
}

namespace {

int
rs_run(const mdemod_rs_opts &o, const uint8_t *cadu_dev, uint64_t n, uint8_t *vcdu_dev, mdemod_rs_info *info_dev, hipStream_t st)
{
	if (!n) return MDEMOD_OK;
	if (n > 0x7FFFFFFFull) REFUSE("rs: %llu frames are more than one launch takes", (unsigned long long)n);
	hipLaunchKernelGGL(rs_decode, dim3(static_cast<uint32_t>(n)), dim3(RS_THREADS), 0, st, reinterpret_cast<const uint32_t *>(cadu_dev),
	                   reinterpret_cast<uint32_t *>(vcdu_dev), reinterpret_cast<uint32_t *>(info_dev), o.derandomise, o.dual_basis);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

} /* namespace */

extern "C" {

int
mdemod_rs_decode_device(const mdemod_rs_opts *opts, const uint8_t *cadu_dev, uint64_t n, uint8_t *vcdu_dev, mdemod_rs_info *info_dev, int device,
                        void *hip_stream)
try { MDEMOD_API_ENTER
	mdemod_rs_opts o;
	int rc = rs_settings(opts, o);
	if (rc) return rc;
	if (!n) return MDEMOD_OK;
	if (!cadu_dev || !vcdu_dev || !info_dev) REFUSE("mdemod_rs_decode_device: the CADUs, the VCDUs and the report are needed");
	if ((reinterpret_cast<uintptr_t>(cadu_dev) | reinterpret_cast<uintptr_t>(vcdu_dev) | reinterpret_cast<uintptr_t>(info_dev)) & 3u)
		REFUSE("mdemod_rs_decode_device: the CADUs, the VCDUs and the report must stand at multiples of 4 bytes");
	if (n > 0x7FFFFFFFull) REFUSE("rs: %llu frames are more than one launch takes", (unsigned long long)n);
	const uint64_t in_bytes = n * MDEMOD_RS_CADU_BYTES, out_bytes = n * MDEMOD_RS_VCDU_BYTES, info_bytes = n * sizeof(mdemod_rs_info);
	if (!MdmBuffers().in(cadu_dev, in_bytes).out(vcdu_dev, out_bytes).out(info_dev, info_bytes).apart())
		REFUSE("mdemod_rs_decode_device: the CADUs, the VCDUs and the report intersect (the blocks of one launch would read what others write)");
	rc = mdm_select_device(device);
	if (rc) return rc;
	return rs_run(o, cadu_dev, n, vcdu_dev, info_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_rs_decode_host(const mdemod_rs_opts *opts, const uint8_t *cadu, uint64_t n, uint8_t *vcdu, mdemod_rs_info *info, int device)
try { MDEMOD_API_ENTER
	mdemod_rs_opts o;
	int rc = rs_settings(opts, o);
	if (rc) return rc;
	if (!n) return MDEMOD_OK;
	if (!cadu || !vcdu || !info) REFUSE("mdemod_rs_decode_host: the CADUs, the VCDUs and the report are needed");
	rc = mdm_select_device(device);
	if (rc) return rc;
	hipStream_t st = nullptr;
	const uint64_t P = std::min<uint64_t>(o.piece_frames, n);
	MdmDevMem mem;
	uint8_t *d_cadu = nullptr, *d_vcdu = nullptr;
	mdemod_rs_info *d_info = nullptr;
	if ((rc = mem.alloc(&d_cadu, P * MDEMOD_RS_CADU_BYTES)) || (rc = mem.alloc(&d_vcdu, P * MDEMOD_RS_VCDU_BYTES)) || (rc = mem.alloc(&d_info, P)))
		return rc;
	for (uint64_t at = 0; at < n; at += P) {
		const uint64_t k = std::min<uint64_t>(P, n - at);
		HIP_TRY(hipMemcpyAsync(d_cadu, cadu + at * MDEMOD_RS_CADU_BYTES, k * MDEMOD_RS_CADU_BYTES, hipMemcpyHostToDevice, st));
		rc = rs_run(o, d_cadu, k, d_vcdu, d_info, st);
		if (rc) return rc;
		HIP_TRY(hipMemcpyAsync(vcdu + at * MDEMOD_RS_VCDU_BYTES, d_vcdu, k * MDEMOD_RS_VCDU_BYTES, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(info + at, d_info, k * sizeof(mdemod_rs_info), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
