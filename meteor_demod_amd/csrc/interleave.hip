/*
 * interleave.hip — the 80 k interleaved mode of include/meteor_demod_amd_interleave.h on gfx950: the search for the interleaver's
 * sync word and the gather that strips it, resolves the convention and deinterleaves.  What they compute is pinned by the host
 * model (csrc/interleave_host.cpp); everything is integer arithmetic, and the bytes are the model's.
 *
 * il_candidates: one block of 320 threads per window of 2560 positions (64 periods of 40).  The window's 2560 + 5 symbols are staged
 *   in LDS once (2-byte loads: any symbol alignment; nothing outside soft[0 .. m) is read, and what lies past m is zero in LDS).
 *   Thread (g, r) = (tid / 40, tid % 40) takes phase r in the periods 8 g .. 8 g + 7.  At a position p it forms the four 4-tap sums
 *   A = sum I a, B = sum Q b, C = sum I b, D = sum Q a - two packed int8 dot products each (v_dot4_i32_i8: the weight words carry
 *   the pattern on one rail and zeros on the other) - and the same four at p + 1 (A', B', C', D': the "+1" bin), and adds them to
 *   its eight registers.  The 8 x 40 partial bins meet in LDS; lane r of the first wave adds them up and forms all 24 scores of
 *   its phase from the binned sums alone: s = 0 reads A + B, C - D, A - B, C + D for h = 0, 1, 4, 5, s = 1 reads A + B', C' - D,
 *   A - B', C' + D, s = 2 reads A' + B, C - D', A' - B, C + D', and h = 2, 3, 6, 7 are the negatives.  The argmax runs on one
 *   unsigned key per (r, H), (score + 65536) << 10 | 1023 - (24 r + H): the largest key is the largest score, then the lowest r,
 *   then the lowest H, whatever the order of the reduction (shuffles in the wave).  No atomics.
 *
 * il_deinterleave: the plain gather, one thread per 4 output bytes and one dword store (4 divides 36: a thread's four bits are on
 *   four consecutive branches).  Per byte: k' = k + 36 M b, N = k' / 72, j = k' % 72, the segment of N, the symbol x, and the rail
 *   through H by select and negate.  The segment table is tiny: up to 32 segments travel as kernel arguments (scalar registers;
 *   a linear scan of selects), a longer table lies in device memory and is searched by bisection.  The four loads of a thread go
 *   to four of the 36 regions 36 M bits apart; between the first and the last region lie 35 x 36 M bits (2.9 MB of input at
 *   M = 2048), which the L2 holds while the 36 read pointers pass over it.
 *
 * Every loop's trip count is fixed by the arguments before it begins; no block waits for another.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "hip_host.h"
#include "interleave_host.h"

#define ILC_GROUPS   8u                                   /* 8 groups of 8 periods */
#define ILC_THREADS  (ILC_GROUPS * IL_PERIOD)             /* 320 */
#define ILC_SYMS     (IL_WINDOW + 5u)                     /* 2565 symbols = 5130 bytes: position 2559 + 1, its four taps */
#define ILC_BIAS     65536                                /* |score| <= 64 x 8 x 128 */
#define ILD_THREADS  256
#define IL_SEG_ARG   32u                                  /* segments that travel as kernel arguments */

struct IlcWeights { uint32_t w[4][2]; };                   /* rows A, B, C, D; words: symbols (0, 1) and (2, 3) as bytes I Q I Q */
struct IlSeg { uint64_t x0, n0; uint32_t hyp, pad; };
struct IlSegArg { IlSeg s[IL_SEG_ARG]; };

__device__ __forceinline__ uint32_t
ilc_key(int score, uint32_t rh)
{
	return (static_cast<uint32_t>(score + ILC_BIAS) << 10) | (1023u - rh);
}

/* the score `sc` of hypothesis h (one of 0, 1, 4, 5) at 24 r + 8 s = base: its negative is h + 2's */
__device__ __forceinline__ uint32_t
ilc_vote(uint32_t best, int sc, uint32_t base, uint32_t h)
{
	return max(max(best, ilc_key(sc, base + h)), ilc_key(-sc, base + h + 2));
}

__global__ void __launch_bounds__(ILC_THREADS)
il_candidates(const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand, IlcWeights W)
{
	__shared__ uint16_t sym[ILC_SYMS + 3];
	__shared__ int part[ILC_GROUPS][IL_PERIOD][8];
	const uint32_t tid = threadIdx.x;
	const uint64_t first = static_cast<uint64_t>(blockIdx.x) * IL_WINDOW;          /* (the host launches windows that have a position: first + 4 <= m) */
	const uint64_t left = m - first;
	const uint32_t nsym = left < ILC_SYMS ? static_cast<uint32_t>(left) : ILC_SYMS;
	const uint32_t npos = left - (IL_SYNC - 1) < IL_WINDOW ? static_cast<uint32_t>(left - (IL_SYNC - 1)) : IL_WINDOW;   /* 1 .. 2560 positions */
	const uint16_t *src = reinterpret_cast<const uint16_t *>(soft) + first;        /* (the entry refuses an odd address) */
	for (uint32_t i = tid; i < ILC_SYMS + 3; i += ILC_THREADS) sym[i] = i < nsym ? src[i] : 0;
	__syncthreads();

	const uint32_t r = tid % IL_PERIOD, g = tid / IL_PERIOD;
	int acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };                                      /* A, B, C, D at p; A', B', C', D' at p + 1 */
#pragma unroll
	for (uint32_t k = 0; k < IL_WINDOW / IL_PERIOD / ILC_GROUPS; k++) {
		const uint32_t p = r + IL_PERIOD * (ILC_GROUPS * k + g);                  /* (a wave's 64 threads read consecutive symbols of two periods) */
		if (p < npos) {
			const uint32_t s0 = sym[p], s1 = sym[p + 1], s2 = sym[p + 2], s3 = sym[p + 3], s4 = sym[p + 4];
			const int w01 = static_cast<int>(s0 | (s1 << 16)), w23 = static_cast<int>(s2 | (s3 << 16));
			const int w12 = static_cast<int>(s1 | (s2 << 16)), w34 = static_cast<int>(s3 | (s4 << 16));
#pragma unroll
			for (int x = 0; x < 4; x++) {
				acc[x] = __builtin_amdgcn_sdot4(w01, static_cast<int>(W.w[x][0]), acc[x], false);
				acc[x] = __builtin_amdgcn_sdot4(w23, static_cast<int>(W.w[x][1]), acc[x], false);
				acc[4 + x] = __builtin_amdgcn_sdot4(w12, static_cast<int>(W.w[x][0]), acc[4 + x], false);
				acc[4 + x] = __builtin_amdgcn_sdot4(w34, static_cast<int>(W.w[x][1]), acc[4 + x], false);
			}
		}
	}
#pragma unroll
	for (int x = 0; x < 8; x++) part[g][r][x] = acc[x];
	__syncthreads();
	if (tid >= 64) return;

	uint32_t best = 0;
	if (tid < IL_PERIOD && tid < npos) {                                           /* only a phase that has a position competes */
		int v[8];
#pragma unroll
		for (int x = 0; x < 8; x++) {
			v[x] = 0;
#pragma unroll
			for (uint32_t q = 0; q < ILC_GROUPS; q++) v[x] += part[q][tid][x];
		}
		const int A = v[0], B = v[1], Cc = v[2], D = v[3], A1 = v[4], B1 = v[5], C1 = v[6], D1 = v[7];
		const uint32_t base = 24u * tid;
		best = ilc_vote(best, A + B, base, 0); best = ilc_vote(best, Cc - D, base, 1);
		best = ilc_vote(best, A - B, base, 4); best = ilc_vote(best, Cc + D, base, 5);
		best = ilc_vote(best, A + B1, base + 8, 0); best = ilc_vote(best, C1 - D, base + 8, 1);
		best = ilc_vote(best, A - B1, base + 8, 4); best = ilc_vote(best, C1 + D, base + 8, 5);
		best = ilc_vote(best, A1 + B, base + 16, 0); best = ilc_vote(best, Cc - D1, base + 16, 1);
		best = ilc_vote(best, A1 - B, base + 16, 4); best = ilc_vote(best, Cc + D1, base + 16, 5);
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) best = max(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), d)));
	if (tid == 0) {
		const uint32_t rh = 1023u - (best & 1023u);
		mdemod_frames_candidate c;
		c.position = first + rh / IL_HYPS;
		c.score = static_cast<int32_t>(best >> 10) - ILC_BIAS;
		c.hypothesis = rh % IL_HYPS;
		cand[blockIdx.x] = c;
	}
}

/* the gather.  ARG: the n_seg <= 32 segments are `arg`; otherwise they lie at seg_dev.  step = 36 M; n_words = 18 x the periods
 * written (they may be fewer than P: a caller's shorter buffer); out holds 4 n_words bytes. */
template <bool ARG>
__global__ void __launch_bounds__(ILD_THREADS)
il_deinterleave(const int8_t *soft, uint64_t m, uint64_t step, uint64_t P, uint64_t n_words, uint32_t n_seg, const IlSeg *seg_dev, IlSegArg arg, int8_t *out)
{
	const uint64_t t = static_cast<uint64_t>(blockIdx.x) * ILD_THREADS + threadIdx.x;
	if (t >= n_words) return;
	const uint64_t k0 = 4 * t;
	const uint32_t b0 = static_cast<uint32_t>(k0 % IL_BRANCHES);                   /* 0, 4, .. 32: the four bits are on branches b0 .. b0 + 3 */
	uint32_t word = 0;
#pragma unroll
	for (uint32_t e = 0; e < 4; e++) {
		const uint64_t kp = k0 + e + step * (b0 + e), N = kp / IL_DATA_BITS;
		const uint32_t j = static_cast<uint32_t>(kp - N * IL_DATA_BITS);
		int v = 0;
		if (N < P) {
			uint64_t x0 = 0, n0 = 0;
			uint32_t H = 0;
			if constexpr (ARG) {
				for (uint32_t i = 0; i < n_seg; i++)                                /* (uniform loads; the last segment with N0 <= N stands) */
					if (arg.s[i].n0 <= N) { x0 = arg.s[i].x0; n0 = arg.s[i].n0; H = arg.s[i].hyp; }
			} else {
				uint32_t lo = 0, hi = n_seg;                                        /* seg[lo].n0 <= N < seg[hi].n0 (seg[0].n0 = 0) */
				while (hi - lo > 1) {
					const uint32_t mid = lo + (hi - lo) / 2;
					if (seg_dev[mid].n0 <= N) lo = mid; else hi = mid;
				}
				x0 = seg_dev[lo].x0; n0 = seg_dev[lo].n0; H = seg_dev[lo].hyp;
			}
			const uint64_t x = x0 + IL_PERIOD * (N - n0) + IL_SYNC + (j >> 1);
			/* rail j & 1 of symbol x through H = h + 8 s: I" is rail I' at x (x + 1 for s = 2), Q" is rail Q' at x (x + 1 for s = 1);
			 * I' = si * (swap ? Q : I), Q' = sq * (swap ? I : Q) */
			const uint32_t rail = j & 1u, h = H & 7u, s = H >> 3;
			const bool neg = ((rail ? 0x9Cu : 0xC6u) >> h) & 1u;                   /* sq is -1 for h = 2, 3, 4, 7; si for h = 1, 2, 6, 7 */
			const uint64_t idx = x + (s == (rail ? 1u : 2u) ? 1u : 0u);
			if (idx < m) {
				v = soft[2 * idx + (rail ^ (h & 1u))];
				v = neg ? -v : v;
				v = v > 127 ? 127 : v;
			}
		}
		word |= static_cast<uint32_t>(static_cast<uint8_t>(v)) << (8 * e);
	}
	if ((reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
		reinterpret_cast<uint32_t *>(out)[t] = word;
	} else {
		for (int e = 0; e < 4; e++) out[k0 + e] = static_cast<int8_t>(word >> (8 * e));
	}
}

namespace {

/* the weight words of il_candidates: bytes (I_k, Q_k, I_k+1, Q_k+1) against the pattern on one rail, zeros on the other */
IlcWeights
ilc_weights()
{
	int8_t a[IL_SYNC], b[IL_SYNC];
	il_pattern(a, b);
	IlcWeights W;
	for (int i = 0; i < 2; i++) {
		const int8_t rows[4][4] = { { a[2 * i], 0, a[2 * i + 1], 0 }, { 0, b[2 * i], 0, b[2 * i + 1] },     /* A = sum I a, B = sum Q b */
		                            { b[2 * i], 0, b[2 * i + 1], 0 }, { 0, a[2 * i], 0, a[2 * i + 1] } };   /* C = sum I b, D = sum Q a */
		for (int x = 0; x < 4; x++) {
			uint32_t w = 0;
			for (int k = 0; k < 4; k++) w |= static_cast<uint32_t>(static_cast<uint8_t>(rows[x][k])) << (8 * k);
			W.w[x][i] = w;
		}
	}
	return W;
}

/* one candidate per window of soft_dev[m] into cand_dev[il_windows(m)]; queued on st */
int
il_candidates_run(const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, hipStream_t st)
{
	const uint64_t n_windows = il_windows(m);
	if (!n_windows) return MDEMOD_OK;
	if (reinterpret_cast<uintptr_t>(soft_dev) & 1u) REFUSE("interleave: the symbols stand at an odd address (2-byte alignment is needed)");
	if (n_windows > 0x7FFFFFFFull) REFUSE("interleave: a stream of %llu symbols is more than one launch takes", (unsigned long long)m);
	hipLaunchKernelGGL(il_candidates, dim3(static_cast<uint32_t>(n_windows)), dim3(ILC_THREADS), 0, st, soft_dev, m, cand_dev, ilc_weights());
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* the first `written` periods of the gather of P periods into out_dev; queued on st (and finished, where the table is longer than
 * the kernel's arguments hold).  The segments are checked. */
int
il_deinterleave_run(const mdemod_il_opts &o, const int8_t *soft_dev, uint64_t m, const mdemod_il_segment *segments, uint64_t n_segments, uint64_t P,
                    uint64_t written, int8_t *out_dev, hipStream_t st)
{
	if (!written) return MDEMOD_OK;
	const uint64_t n_words = written * (IL_DATA_BITS / 4), blocks = (n_words + ILD_THREADS - 1) / ILD_THREADS;
	if (blocks > 0x7FFFFFFFull || n_segments > 0x7FFFFFFFull) REFUSE("interleave: %llu periods in %llu segments are more than one launch takes",
	                                                                 (unsigned long long)written, (unsigned long long)n_segments);
	const uint64_t step = static_cast<uint64_t>(IL_BRANCHES) * o.branch_delay;
	const dim3 grid(static_cast<uint32_t>(blocks)), block(ILD_THREADS);
	IlSegArg arg = {};
	if (n_segments <= IL_SEG_ARG) {
		for (uint64_t i = 0; i < n_segments; i++) arg.s[i] = IlSeg{ segments[i].marker_symbol, segments[i].period, segments[i].hypothesis, 0 };
		hipLaunchKernelGGL(il_deinterleave<true>, grid, block, 0, st, soft_dev, m, step, P, n_words, static_cast<uint32_t>(n_segments),
		                   static_cast<const IlSeg *>(nullptr), arg, out_dev);
		HIP_TRY(hipGetLastError());
		return MDEMOD_OK;
	}
	std::vector<IlSeg> table(n_segments);
	for (uint64_t i = 0; i < n_segments; i++) table[i] = IlSeg{ segments[i].marker_symbol, segments[i].period, segments[i].hypothesis, 0 };
	MdmDevMem mem;
	IlSeg *d_table = nullptr;
	const int rc = mem.alloc(&d_table, n_segments);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(d_table, table.data(), n_segments * sizeof(IlSeg), hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(il_deinterleave<false>, grid, block, 0, st, soft_dev, m, step, P, n_words, static_cast<uint32_t>(n_segments),
	                   static_cast<const IlSeg *>(d_table), arg, out_dev);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));                                           /* (the table goes with this call) */
	return MDEMOD_OK;
}

bool
il_apart(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
	const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
	return x + a_bytes <= y || y + b_bytes <= x;
}

/* search, tracker and gather of a stream in device memory into out_dev (the device is selected; *n_segments and *n_periods are 0 on entry) */
int
il_decode(const mdemod_il_opts &o, const int8_t *soft_dev, uint64_t m, int8_t *out_dev, uint64_t out_cap, mdemod_il_segment *segments, uint64_t cap,
          uint64_t *n_segments, uint64_t *n_periods, int32_t *mean_score, hipStream_t st)
{
	const uint64_t n_windows = il_windows(m);
	if (!n_windows) return MDEMOD_OK;
	MdmDevMem mem;
	mdemod_frames_candidate *d_cand = nullptr;
	int rc = mem.alloc(&d_cand, n_windows);
	if (rc) return rc;
	rc = il_candidates_run(soft_dev, m, d_cand, st);
	if (rc) return rc;
	std::vector<mdemod_frames_candidate> cand(n_windows);
	HIP_TRY(hipMemcpyAsync(cand.data(), d_cand, n_windows * sizeof(mdemod_frames_candidate), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if ((rc = il_check_candidates(cand.data(), n_windows, m))) return rc;
	std::vector<mdemod_il_segment> found;
	uint64_t P = 0;
	il_track(o, cand.data(), n_windows, m, found, P);
	*n_segments = found.size();
	*n_periods = P;
	if (mean_score) *mean_score = il_mean_score(cand.data(), n_windows);
	for (uint64_t i = 0; i < found.size() && i < cap; i++) segments[i] = found[i];
	rc = il_deinterleave_run(o, soft_dev, m, found.data(), found.size(), P, std::min<uint64_t>(P, out_cap / IL_BRANCHES), out_dev, st);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(st));
	return MDEMOD_OK;
}

} /* namespace */

extern "C" {

int
mdemod_il_candidates_device(const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	if (!il_windows(m)) return MDEMOD_OK;
	if (!soft_dev || !cand_dev) REFUSE("mdemod_il_candidates_device: the symbols and the candidates are needed");
	const int rc = mdm_select_device(device);
	if (rc) return rc;
	return il_candidates_run(soft_dev, m, cand_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_il_deinterleave_device(const mdemod_il_opts *opts, const int8_t *soft_dev, uint64_t m, const mdemod_il_segment *segments, uint64_t n_segments,
                              uint64_t n_periods, int8_t *out_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	mdemod_il_opts o;
	int rc = il_settings(opts, o);
	if (rc) return rc;
	if ((m && !soft_dev) || (n_segments && !segments) || (n_periods && !out_dev))
		REFUSE("mdemod_il_deinterleave_device: the symbols, the segments and the output are needed");
	if ((rc = il_check_segments(segments, n_segments, n_periods, m))) return rc;
	if (!il_apart(soft_dev, 2 * m, out_dev, IL_DATA_BITS * n_periods)) REFUSE("mdemod_il_deinterleave_device: the input and the output overlap");
	if ((rc = mdm_select_device(device))) return rc;
	return il_deinterleave_run(o, soft_dev, m, segments, n_segments, n_periods, n_periods, out_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_il_decode_device(const mdemod_il_opts *opts, const int8_t *soft_dev, uint64_t m, int8_t *out_dev, uint64_t out_cap, mdemod_il_segment *segments,
                        uint64_t cap, uint64_t *n_segments, uint64_t *n_periods, int32_t *mean_score, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	if (n_segments) *n_segments = 0;
	if (n_periods) *n_periods = 0;
	if (mean_score) *mean_score = 0;
	if (!n_segments || !n_periods || (m && !soft_dev) || (cap && !segments) || (out_cap && !out_dev))
		REFUSE("mdemod_il_decode_device: the symbols, n_segments and n_periods (and the outputs for a capacity > 0) are needed");
	mdemod_il_opts o;
	int rc = il_settings(opts, o);
	if (rc) return rc;
	if (m >> 48) REFUSE("mdemod_il_decode_device: a stream of %llu symbols is more than the layer takes", (unsigned long long)m);
	if (out_cap >> 56 || !il_apart(soft_dev, 2 * m, out_dev, 2 * out_cap)) REFUSE("mdemod_il_decode_device: the input and the output overlap");
	if ((rc = mdm_select_device(device))) return rc;
	return il_decode(o, soft_dev, m, out_dev, out_cap, segments, cap, n_segments, n_periods, mean_score, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_il_decode_host(const mdemod_il_opts *opts, const int8_t *soft, uint64_t m, int8_t *out, uint64_t out_cap, mdemod_il_segment *segments,
                      uint64_t cap, uint64_t *n_segments, uint64_t *n_periods, int32_t *mean_score, int device)
try { MDEMOD_API_ENTER
	if (n_segments) *n_segments = 0;
	if (n_periods) *n_periods = 0;
	if (mean_score) *mean_score = 0;
	if (!n_segments || !n_periods || (m && !soft) || (cap && !segments) || (out_cap && !out))
		REFUSE("mdemod_il_decode_host: the symbols, n_segments and n_periods (and the outputs for a capacity > 0) are needed");
	mdemod_il_opts o;
	int rc = il_settings(opts, o);
	if (rc) return rc;
	if (m >> 48 || out_cap >> 56) REFUSE("mdemod_il_decode_host: a stream of %llu symbols is more than the layer takes", (unsigned long long)m);
	if (!il_windows(m)) return MDEMOD_OK;
	if ((rc = mdm_select_device(device))) return rc;
	hipStream_t st = nullptr;
	/* the output never holds more than the candidates' periods could fill: 36 symbols per 40 and a slip's rounding per window */
	const uint64_t room = std::min<uint64_t>(out_cap / IL_BRANCHES, m / IL_PERIOD + il_windows(m) + 1) * IL_BRANCHES;
	MdmDevMem mem;
	int8_t *d_soft = nullptr, *d_out = nullptr;
	if ((rc = mem.alloc(&d_soft, 2 * m)) || (rc = mem.alloc(&d_out, 2 * room))) return rc;
	HIP_TRY(hipMemcpyAsync(d_soft, soft, 2 * m, hipMemcpyHostToDevice, st));
	rc = il_decode(o, d_soft, m, d_out, room, segments, cap, n_segments, n_periods, mean_score, st);
	if (rc) return rc;
	const uint64_t written = std::min<uint64_t>(*n_periods, room / IL_BRANCHES);
	if (written) HIP_TRY(hipMemcpy(out, d_out, IL_DATA_BITS * written, hipMemcpyDeviceToHost));
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
