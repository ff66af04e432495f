/*
 * frames.hip — the frame layer of include/meteor_demod_amd_frames.h on gfx950: the marker search and the Viterbi decoder.  What
 * they compute is pinned by the host model (csrc/frames_host.cpp); everything is int32, and the bytes are the model's.
 *
 * fr_candidates: one block of 256 threads per window.  The window's 8192 + 32 symbols are staged in LDS (16 448 bytes; 16-byte
 *   loads when the stream is 16-byte aligned, byte loads otherwise; only the 32 symbols two windows share are read twice, nothing
 *   outside soft[0 .. m) is read and what lies past m is zero in LDS).  A thread takes 16 pairs of positions (2q, 2q + 1): the 14 words
 *   (I Q I Q) from symbol 2q + 6 on serve both - the odd position's words are v_alignbit of two neighbours.  The four 26-tap sums
 *   are 13 packed int8 dot products each (v_dot4c_i32_i8: __builtin_amdgcn_sdot4); the weight words carry the pattern so that the
 *   four accumulators ARE the scores of h = 0, 1, 4, 5 (A + B, C - D, A - B, C + D), and h = 2, 3, 6, 7 are their negatives.  The
 *   argmax runs on one unsigned key per (position, h), (score + 8192) << 16 | 0xFFFF - (8 p + h): the largest key is the largest
 *   score, then the lowest p, then the lowest h, whatever the order of the reduction (shuffles in the wave, four words of LDS across
 *   the waves).
 *
 * fr_viterbi: one wavefront per (frame, sub-block), one lane per state s'; four waves share a block and 4 x 12 800 bytes of LDS
 *   (three blocks = 12 waves per CU).  The sub-block's symbols (at most 1280, raw bytes) and its decision words (1280 x 8 bytes)
 *   live in the wave's part.  The two branches into s' carry complementary outputs (both polynomials have the register's top bit),
 *   so the branch metrics are +bm and -bm with bm = cI I + cQ Q: the lane's +-1 constants fold the hypothesis and the outputs.
 *   A step: the predecessors' metrics by two __shfl (ds_bpermute), add, compare, select, __ballot; 64 steps are unrolled: lane i
 *   brings step i's symbol (v_readlane) and keeps its word, and the wave writes 64 words at once.  Traceback: every lane walks the words backwards (the same walk in all of
 *   them), lane c keeps the c-th 32-bit word of the 1024 kept bits, and lanes 0..31 store the 128 bytes.
 *
 * fr_errors: one block per frame re-encodes its 1024 bytes and counts the hard decisions that differ (channel_errors).
 *
 * The link variant (include/meteor_demod_amd_frames_link.h) adds instances beside these; the three kernels above compile to what
 * they compiled to without it.
 * fr_link_candidates<DIFF, SKEW>: the same block per window, four positions 4u .. 4u + 3 per thread and step (fifteen words serve
 *   them and position 4u + 4), the same four accumulators per position.  A, B, C, D follow from them exactly (2A = s0 + s4,
 *   2B = s0 - s4, 2C = s1 + s5, 2D = s5 - s1), and the skewed scores of position p are sums of p's and p + 1's: s = 1 reads
 *   A + B', C' - D, A - B', C' + D and s = 2 A' + B, C - D', A' - B, C + D' (primed: at p + 1).  That is why the LDS tile is one symbol
 *   longer, and why a position needs 33 symbols.  DIFF takes |score| and votes h = 0, 1, 4, 5 only.  The key is
 *   (score + 8192) << 18 | 0x3FFFF - (32 p + H): as independent of the reduction's order as the one above.
 * fr_viterbi<true> / fr_errors<true>: the kernels above with LINK = true.  The skew is resolved where the symbols are staged (each
 *   rail read at its own index, 0 at index m), the NRZ-M is undone at traceback (bit 1 of the state is the bit of the step before),
 *   and the decoder's own bits go to a second buffer, on which fr_errors<true> counts.
 *
 * Every loop's trip count is fixed by the arguments before it begins; no block waits for another.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "frames_device.h"
#include "frames_host.h"
#include "hip_host.h"

#define FRC_THREADS 256
#define FRC_SYMS    (FR_FRAME + FR_SPAN)                   /* 8224 symbols = 16 448 bytes */
#define FRC_PAIRS   (FR_TAPS / 2)                          /* 13 words of two symbols */
#define FRL_SYMS    (FR_FRAME + FR_SPAN + 8)                /* 8232 symbols = 16 464 bytes: a skewed position's 33, the last thread's fifth position */
#define FRL_KEY_LOW 0x3FFFFu                              /* 32 p + H */
#define FRV_WAVES   4
#define FRV_DEC     (FR_STEPS * 8)                         /* bytes of decision words per wave */
#define FRV_WAVE_LDS (FRV_DEC + FR_STEPS * 2)              /* 12 800 */

struct FrcWeights { uint32_t w[4][FRC_PAIRS]; };           /* rows: h = 0, 1, 4, 5 */
struct FrvFrame { uint64_t position; uint32_t hypothesis, pad; };

__device__ __forceinline__ uint32_t
frc_key(int score, uint32_t ph)
{
	return (static_cast<uint32_t>(score + 8192) << 16) | (0xFFFFu - ph);
}

__global__ void __launch_bounds__(FRC_THREADS)
fr_candidates(const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand, FrcWeights W)
{
	__shared__ __align__(16) unsigned char lds[2 * FRC_SYMS];
	__shared__ uint32_t wave_best[FRC_THREADS / 64];
	const uint32_t tid = threadIdx.x;
	const uint64_t first = static_cast<uint64_t>(blockIdx.x) * FR_FRAME;          /* (the host launches windows that have a position: first < m - 32) */
	const uint64_t left = m - first;
	const uint32_t nsym = left < FRC_SYMS ? static_cast<uint32_t>(left) : FRC_SYMS, nbytes = 2 * nsym;
	const uint32_t npos = nsym - FR_SPAN;                                       /* 1 .. 8192 positions */
	const unsigned char *src = reinterpret_cast<const unsigned char *>(soft) + 2 * first;
	uint32_t vec = 0;                                                          /* bytes that go as 16-byte loads */
	if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
		vec = nbytes & ~15u;
		for (uint32_t i = tid; i < vec / 16; i += FRC_THREADS)
			reinterpret_cast<uint4 *>(lds)[i] = reinterpret_cast<const uint4 *>(src)[i];
	}
	for (uint32_t i = vec + tid; i < 2 * FRC_SYMS; i += FRC_THREADS) lds[i] = i < nbytes ? src[i] : 0;
	__syncthreads();

	const uint32_t *words = reinterpret_cast<const uint32_t *>(lds);
	uint32_t best = 0;
	for (uint32_t j = 0; j < FR_FRAME / 2 / FRC_THREADS; j++) {
		const uint32_t q = tid + j * FRC_THREADS;
		uint32_t x[FRC_PAIRS + 1];
#pragma unroll
		for (int i = 0; i <= FRC_PAIRS; i++) x[i] = words[q + FR_LEAD / 2 + i];
#pragma unroll
		for (int odd = 0; odd < 2; odd++) {
			int s0 = 0, s1 = 0, s4 = 0, s5 = 0;
#pragma unroll
			for (int i = 0; i < FRC_PAIRS; i++) {
				const int v = static_cast<int>(odd ? __builtin_amdgcn_alignbit(x[i + 1], x[i], 16) : x[i]);
				s0 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[0][i]), s0, false);
				s1 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[1][i]), s1, false);
				s4 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[2][i]), s4, false);
				s5 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[3][i]), s5, false);
			}
			const uint32_t p = 2 * q + odd;
			if (p < npos) {
				const uint32_t ph = p * 8;
				best = max(best, frc_key(s0, ph + 0)); best = max(best, frc_key(s1, ph + 1));
				best = max(best, frc_key(-s0, ph + 2)); best = max(best, frc_key(-s1, ph + 3));
				best = max(best, frc_key(s4, ph + 4)); best = max(best, frc_key(s5, ph + 5));
				best = max(best, frc_key(-s4, ph + 6)); best = max(best, frc_key(-s5, ph + 7));
			}
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) best = max(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), d)));
	if ((tid & 63) == 0) wave_best[tid >> 6] = best;
	__syncthreads();
	if (tid == 0) {
		for (int i = 1; i < FRC_THREADS / 64; i++) best = max(best, wave_best[i]);
		const uint32_t ph = 0xFFFFu - (best & 0xFFFFu);
		mdemod_frames_candidate c;
		c.position = first + (ph >> 3);
		c.score = static_cast<int32_t>(best >> 16) - 8192;
		c.hypothesis = ph & 7u;
		cand[blockIdx.x] = c;
	}
}

__device__ __forceinline__ uint32_t
frl_key(int score, uint32_t ph)
{
	return (static_cast<uint32_t>(score + 8192) << 18) | (FRL_KEY_LOW - ph);
}

/* the score `sc` of hypothesis h (one of 0, 1, 4, 5) at 32 p + 8 s = base: its negative is h + 2's; DIFF keeps |sc| for h alone */
template <bool DIFF>
__device__ __forceinline__ uint32_t
frl_vote(uint32_t best, int sc, uint32_t base, uint32_t h)
{
	if constexpr (DIFF) return max(best, frl_key(sc < 0 ? -sc : sc, base + h));
	return max(max(best, frl_key(sc, base + h)), frl_key(-sc, base + h + 2));
}

template <bool DIFF, bool SKEW>
__global__ void __launch_bounds__(FRC_THREADS)
fr_link_candidates(const int8_t *soft, uint64_t m, mdemod_frames_candidate *cand, FrcWeights W)
{
	__shared__ __align__(16) unsigned char lds[2 * FRL_SYMS];
	__shared__ uint32_t wave_best[FRC_THREADS / 64];
	constexpr uint32_t SPAN = FR_SPAN + (SKEW ? 1u : 0u);
	const uint32_t tid = threadIdx.x;
	const uint64_t first = static_cast<uint64_t>(blockIdx.x) * FR_FRAME;          /* (the host launches windows that have a position: first < m - SPAN) */
	const uint64_t left = m - first;
	const uint32_t nbytes = 2 * (left < FRL_SYMS ? static_cast<uint32_t>(left) : FRL_SYMS);
	const uint32_t npos = left - SPAN < FR_FRAME ? static_cast<uint32_t>(left - SPAN) : FR_FRAME;   /* 1 .. 8192 positions */
	const unsigned char *src = reinterpret_cast<const unsigned char *>(soft) + 2 * first;
	uint32_t vec = 0;                                                          /* bytes that go as 16-byte loads */
	if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
		vec = nbytes & ~15u;
		for (uint32_t i = tid; i < vec / 16; i += FRC_THREADS)
			reinterpret_cast<uint4 *>(lds)[i] = reinterpret_cast<const uint4 *>(src)[i];
	}
	for (uint32_t i = vec + tid; i < 2 * FRL_SYMS; i += FRC_THREADS) lds[i] = i < nbytes ? src[i] : 0;
	__syncthreads();

	const uint32_t *words = reinterpret_cast<const uint32_t *>(lds);
	uint32_t best = 0;
	for (uint32_t j = 0; j < FR_FRAME / 4 / FRC_THREADS; j++) {
		const uint32_t u = tid + j * FRC_THREADS;
		uint32_t x[FRC_PAIRS + 2];                                             /* symbols 4u + 6 .. 4u + 35 (the last word index: 4111 of 4116) */
#pragma unroll
		for (int i = 0; i < FRC_PAIRS + 2; i++) x[i] = words[2 * u + FR_LEAD / 2 + i];
		int a2 = 0, b2 = 0, c2 = 0, d2 = 0;                                    /* 2A, 2B, 2C, 2D of the position before */
#pragma unroll
		for (int e = 0; e < (SKEW ? 5 : 4); e++) {
			int s0 = 0, s1 = 0, s4 = 0, s5 = 0;
#pragma unroll
			for (int i = 0; i < FRC_PAIRS; i++) {
				const int v = static_cast<int>(e & 1 ? __builtin_amdgcn_alignbit(x[e / 2 + i + 1], x[e / 2 + i], 16) : x[e / 2 + i]);
				s0 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[0][i]), s0, false);
				s1 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[1][i]), s1, false);
				s4 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[2][i]), s4, false);
				s5 = __builtin_amdgcn_sdot4(v, static_cast<int>(W.w[3][i]), s5, false);
			}
			const uint32_t p = 4 * u + e;
			if (e < 4 && p < npos) {
				best = frl_vote<DIFF>(best, s0, p * 32, 0); best = frl_vote<DIFF>(best, s1, p * 32, 1);
				best = frl_vote<DIFF>(best, s4, p * 32, 4); best = frl_vote<DIFF>(best, s5, p * 32, 5);
			}
			if constexpr (SKEW) {
				const int na2 = s0 + s4, nb2 = s0 - s4, nc2 = s1 + s5, nd2 = s5 - s1;
				if (e > 0 && p - 1 < npos) {                                    /* the skewed scores of p - 1: halves of even sums, exact */
					const uint32_t base = (p - 1) * 32;
					best = frl_vote<DIFF>(best, (a2 + nb2) >> 1, base + 8, 0); best = frl_vote<DIFF>(best, (nc2 - d2) >> 1, base + 8, 1);
					best = frl_vote<DIFF>(best, (a2 - nb2) >> 1, base + 8, 4); best = frl_vote<DIFF>(best, (nc2 + d2) >> 1, base + 8, 5);
					best = frl_vote<DIFF>(best, (na2 + b2) >> 1, base + 16, 0); best = frl_vote<DIFF>(best, (c2 - nd2) >> 1, base + 16, 1);
					best = frl_vote<DIFF>(best, (na2 - b2) >> 1, base + 16, 4); best = frl_vote<DIFF>(best, (c2 + nd2) >> 1, base + 16, 5);
				}
				a2 = na2; b2 = nb2; c2 = nc2; d2 = nd2;
			}
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) best = max(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), d)));
	if ((tid & 63) == 0) wave_best[tid >> 6] = best;
	__syncthreads();
	if (tid == 0) {
		for (int i = 1; i < FRC_THREADS / 64; i++) best = max(best, wave_best[i]);
		const uint32_t ph = FRL_KEY_LOW - (best & FRL_KEY_LOW);
		mdemod_frames_candidate c;
		c.position = first + (ph >> 5);
		c.score = static_cast<int32_t>(best >> 18) - 8192;
		c.hypothesis = ph & 31u;
		cand[blockIdx.x] = c;
	}
}

__device__ __forceinline__ int
fr_parity(uint32_t x)
{
	return __builtin_popcount(x) & 1;
}

/* hypothesis h reads (I, Q) as I' = si * (swap ? Q : I), Q' = sq * (swap ? I : Q): frames_host.h's fr_hyp as bit masks */
__device__ __forceinline__ void
fr_hyp_dev(uint32_t h, int &si, int &sq, bool &swap)
{
	si = (0xC6u >> h) & 1u ? -1 : 1;                                           /* h = 1, 2, 6, 7 */
	sq = (0x9Cu >> h) & 1u ? -1 : 1;                                           /* h = 2, 3, 4, 7 */
	swap = (h & 1u) != 0;
}

/* what the LINK instances take besides: nothing for the plain ones */
template <bool LINK> struct FrvLink {};
template <> struct FrvLink<true> { uint8_t *dbits; uint32_t diff; };       /* the decoder's own bits go there; 1: NRZ-M is undone at traceback */
template <bool LINK> struct FreLink {};
template <> struct FreLink<true> { uint64_t m; };

/* the decoder of one (frame, sub-block) per wave.  LINK: the frame's hypothesis is H = h + 8 s. */
template <bool LINK>
__global__ void __launch_bounds__(FRV_WAVES * 64)
fr_viterbi(const int8_t *soft, uint64_t m, const FrvFrame *frames, uint64_t n_units, uint8_t *cadu, [[maybe_unused]] FrvLink<LINK> link)
{
	extern __shared__ __align__(16) unsigned char frv_lds[];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wv = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));   /* (the same in the whole wave: what follows from it stays scalar) */
	uint64_t *dec = reinterpret_cast<uint64_t *>(frv_lds + wv * FRV_WAVE_LDS);
	uint16_t *sym = reinterpret_cast<uint16_t *>(frv_lds + wv * FRV_WAVE_LDS + FRV_DEC);
	const uint64_t unit = static_cast<uint64_t>(blockIdx.x) * FRV_WAVES + wv;
	const bool active = unit < n_units;                                         /* (a whole wave: the last block may have idle ones) */
	const uint64_t f = active ? unit >> 3 : 0;
	const uint32_t k = static_cast<uint32_t>(unit & 7u);
	uint32_t T = 0, off = 0, hyp = 0;
	uint64_t lo = 0;
	if (active) {
		const FrvFrame fr = frames[f];
		const uint64_t s = fr.position + static_cast<uint64_t>(FR_SUB) * k;
		lo = s >= FR_HALO ? s - FR_HALO : 0;
		const uint64_t hi = s + FR_SUB + FR_HALO < m ? s + FR_SUB + FR_HALO : m;
		T = static_cast<uint32_t>(hi - lo);
		off = static_cast<uint32_t>(s - lo);
		hyp = fr.hypothesis;
	}
	if constexpr (LINK) {
		/* s = 1 is (I'[n], Q'[n + 1]) and s = 2 (I'[n + 1], Q'[n]); the rails of I' and Q' are Q and I where h swaps: each rail
		 * of the input is read at its own index, and index m holds 0 */
		const uint32_t s = hyp >> 3, swapped = hyp & 1u;
		const uint32_t dI = (s == 1 && swapped) || (s == 2 && !swapped), dQ = (s == 1 && !swapped) || (s == 2 && swapped);
		hyp &= 7u;
		for (uint32_t t = lane; t < T; t += 64) {
			const uint64_t ni = lo + t + dI, nq = lo + t + dQ;
			const uint8_t i = ni < m ? static_cast<uint8_t>(soft[2 * ni]) : 0, q = nq < m ? static_cast<uint8_t>(soft[2 * nq + 1]) : 0;
			sym[t] = static_cast<uint16_t>(i | (q << 8));
		}
	} else {
		for (uint32_t t = lane; t < T; t += 64) {
			const uint8_t i = static_cast<uint8_t>(soft[2 * (lo + t)]), q = static_cast<uint8_t>(soft[2 * (lo + t) + 1]);
			sym[t] = static_cast<uint16_t>(i | (q << 8));
		}
	}
	__syncthreads();

	/* this lane's state s' = lane; the branch from s' >> 1 has the register s', the one from (s' >> 1) | 32 its complement's outputs */
	const int o1 = fr_parity(lane & 0x4Fu) ? 1 : -1, o2 = fr_parity(lane & 0x6Du) ? 1 : -1;
	int si, sq;
	bool swap;
	fr_hyp_dev(hyp, si, sq, swap);
	const int cI = swap ? o2 * sq : o1 * si, cQ = swap ? o1 * si : o2 * sq;
	const int p0 = static_cast<int>(lane >> 1), p1 = p0 | 32;
	int pm = 0;
	/* one step: the symbol's two bytes in v, the decision word of the wave returned */
	auto step = [&](uint32_t v) -> uint64_t {
		const int I = static_cast<int8_t>(v & 0xFFu), Q = static_cast<int8_t>(v >> 8);
		const int bm = I * cI + Q * cQ;
		const int m0 = __shfl(pm, p0) + bm, m1 = __shfl(pm, p1) - bm;
		const bool second = m1 > m0;
		pm = second ? m1 : m0;
		return __ballot(second);
	};
	/* 64 steps at a time: lane i brings the symbol of step t0 + i (read across by v_readlane) and keeps that step's word */
	uint32_t t0 = 0;
	for (; t0 + 64 <= T; t0 += 64) {
		const int mine_sym = sym[t0 + lane];
		uint64_t keep = 0;
#pragma unroll
		for (int i = 0; i < 64; i++) {
			const uint64_t word = step(static_cast<uint32_t>(__builtin_amdgcn_readlane(mine_sym, i)));
			if (lane == static_cast<uint32_t>(i)) keep = word;
		}
		dec[t0 + lane] = keep;
	}
	if (t0 < T) {                                                                /* a sub-block cut short by the end of the stream */
		uint64_t keep = 0;
		for (uint32_t t = t0; t < T; t++) {
			const uint64_t word = step(sym[t]);
			if (lane == (t & 63u)) keep = word;
		}
		dec[t0 + lane] = keep;                                                    /* (t0 <= 1216: inside the wave's 1280 words) */
	}
	__syncthreads();

	uint32_t key = (static_cast<uint32_t>(pm + (1 << 20)) << 6) | (63u - lane);
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) key = max(key, static_cast<uint32_t>(__shfl_xor(static_cast<int>(key), d)));
	uint32_t state = 63u - (key & 63u);
	uint32_t cur = 0, mine = 0;
	[[maybe_unused]] uint32_t dcur = 0, dmine = 0;
	for (uint32_t t = T; t-- > 0;) {
		const uint32_t j = t - off;
		if (j < FR_SUB) {
			if constexpr (LINK) {
				const uint32_t before = t ? (state >> 1) & link.diff : 0u;              /* (bit 1 of the state: the bit of step t - 1; none before step 0) */
				cur |= ((state ^ before) & 1u) << (((j >> 3) & 3u) * 8u + 7u - (j & 7u));
				dcur |= (state & 1u) << (((j >> 3) & 3u) * 8u + 7u - (j & 7u));
			} else {
				cur |= (state & 1u) << (((j >> 3) & 3u) * 8u + 7u - (j & 7u));
			}
			if ((j & 31u) == 0) {
				if (lane == (j >> 5)) { mine = cur; if constexpr (LINK) dmine = dcur; }
				cur = 0;
				if constexpr (LINK) dcur = 0;
			}
		}
		const uint32_t d = static_cast<uint32_t>(dec[t] >> state) & 1u;
		state = (state >> 1) | (d << 5);
	}
	if (active && lane < FR_SUB / 32) {
		uint8_t *out = cadu + f * MDEMOD_FRAME_BYTES + k * (FR_SUB / 8);
		if ((reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
			reinterpret_cast<uint32_t *>(out)[lane] = mine;
		} else {
			for (int b = 0; b < 4; b++) out[4 * lane + b] = static_cast<uint8_t>(mine >> (8 * b));
		}
		if constexpr (LINK) reinterpret_cast<uint32_t *>(link.dbits + f * MDEMOD_FRAME_BYTES + k * (FR_SUB / 8))[lane] = dmine;   /* (the host's own buffer: aligned) */
	}
}


/* LINK: the hypothesis is H = h + 8 s (each rail read at its own index, 0 at index m), and `cadu` holds the decoder's own bits */
template <bool LINK>
__global__ void __launch_bounds__(256)
fr_errors(const int8_t *soft, const FrvFrame *frames, const uint8_t *cadu, uint32_t *errors, [[maybe_unused]] FreLink<LINK> link)
{
	__shared__ uint32_t wave_sum[4];
	const uint32_t tid = threadIdx.x;
	const FrvFrame fr = frames[blockIdx.x];
	const uint8_t *bytes = cadu + static_cast<uint64_t>(blockIdx.x) * MDEMOD_FRAME_BYTES;
	const uint32_t hyp = LINK ? fr.hypothesis & 7u : fr.hypothesis;
	[[maybe_unused]] const uint32_t skew = fr.hypothesis >> 3;
	[[maybe_unused]] const uint32_t dI = (skew == 1 && (hyp & 1u)) || (skew == 2 && !(hyp & 1u)), dQ = (skew == 1 && !(hyp & 1u)) || (skew == 2 && (hyp & 1u));
	int si, sq;
	bool swap;
	fr_hyp_dev(hyp, si, sq, swap);
	/* 32 info bits per thread; the register comes from the six bits before them (thread 0: from the frame's own first six) */
	uint32_t reg = tid ? bytes[4 * tid - 1] & 0x3Fu : 0u;
	uint32_t count = 0;
	for (uint32_t j = 0; j < 32; j++) {
		const uint32_t n = 32 * tid + j;
		reg = ((reg << 1) | ((bytes[n >> 3] >> (7u - (n & 7u))) & 1u)) & 0x7Fu;
		int I, Q;
		if constexpr (LINK) {
			const uint64_t ni = fr.position + n + dI, nq = fr.position + n + dQ;
			I = ni < link.m ? soft[2 * ni] : 0;
			Q = nq < link.m ? soft[2 * nq + 1] : 0;
		} else {
			I = soft[2 * (fr.position + n)];
			Q = soft[2 * (fr.position + n) + 1];
		}
		const int ip = si * (swap ? Q : I), qp = sq * (swap ? I : Q);
		if (n >= FR_LEAD) {
			count += static_cast<uint32_t>((ip > 0) != (fr_parity(reg & 0x4Fu) != 0));
			count += static_cast<uint32_t>((qp > 0) != (fr_parity(reg & 0x6Du) != 0));
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) count += static_cast<uint32_t>(__shfl_xor(static_cast<int>(count), d));
	if ((tid & 63u) == 0) wave_sum[tid >> 6] = count;
	__syncthreads();
	if (tid == 0) errors[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

namespace {

/* the weight words of the candidates kernels: bytes (I_k, Q_k, I_k+1, Q_k+1) against the pattern (the differential one for `diff`),
 * one row per h = 0, 1, 4, 5 */
FrcWeights
frc_weights(bool diff = false)
{
	int8_t a[FR_TAPS], b[FR_TAPS];
	if (diff) fr_pattern_diff(a, b); else fr_pattern(a, b);
	FrcWeights W;
	for (int i = 0; i < FRC_PAIRS; i++) {
		const int8_t rows[4][4] = { { a[2 * i], b[2 * i], a[2 * i + 1], b[2 * i + 1] },                                             /* A + B */
		                            { b[2 * i], static_cast<int8_t>(-a[2 * i]), b[2 * i + 1], static_cast<int8_t>(-a[2 * i + 1]) },  /* C - D */
		                            { a[2 * i], static_cast<int8_t>(-b[2 * i]), a[2 * i + 1], static_cast<int8_t>(-b[2 * i + 1]) },  /* A - B */
		                            { b[2 * i], a[2 * i], b[2 * i + 1], a[2 * i + 1] } };                                           /* C + D */
		for (int r = 0; r < 4; r++) {
			uint32_t w = 0;
			for (int k = 0; k < 4; k++) w |= static_cast<uint32_t>(static_cast<uint8_t>(rows[r][k])) << (8 * k);
			W.w[r][i] = w;
		}
	}
	return W;
}

} /* namespace */

int
fr_candidates_run(FrMode md, const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, hipStream_t st)
{
	const uint64_t n_windows = fr_mode_windows(m, md);
	if (!n_windows) return MDEMOD_OK;
	if (n_windows > 0x7FFFFFFFull) REFUSE("frames: a stream of %llu symbols is more than one launch takes", (unsigned long long)m);
	const dim3 grid(static_cast<uint32_t>(n_windows)), block(FRC_THREADS);
	if (fr_mode_plain(md)) hipLaunchKernelGGL(fr_candidates, grid, block, 0, st, soft_dev, m, cand_dev, frc_weights());
	else if (!md.skew) hipLaunchKernelGGL((fr_link_candidates<true, false>), grid, block, 0, st, soft_dev, m, cand_dev, frc_weights(true));
	else if (!md.diff) hipLaunchKernelGGL((fr_link_candidates<false, true>), grid, block, 0, st, soft_dev, m, cand_dev, frc_weights(false));
	else hipLaunchKernelGGL((fr_link_candidates<true, true>), grid, block, 0, st, soft_dev, m, cand_dev, frc_weights(true));
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* frames[0 .. n) of soft_dev[m] into cadu_dev; channel_errors into frames[].  Returns after the kernels have finished. */
int
fr_viterbi_run(FrMode md, const int8_t *soft_dev, uint64_t m, mdemod_frame_info *frames, uint64_t n, uint8_t *cadu_dev, hipStream_t st)
{
	if (!n) return MDEMOD_OK;
	if (n > 0x0FFFFFFFull) REFUSE("frames: %llu frames are more than one launch takes", (unsigned long long)n);
	std::vector<FrvFrame> list(n);
	for (uint64_t f = 0; f < n; f++) { list[f].position = frames[f].position; list[f].hypothesis = frames[f].hypothesis; list[f].pad = 0; }
	MdmDevMem mem;
	FrvFrame *d_list = nullptr;
	uint32_t *d_err = nullptr;
	uint8_t *d_bits = nullptr;                                                  /* the link instances: the decoder's own bits */
	int rc;
	if ((rc = mem.alloc(&d_list, n)) || (rc = mem.alloc(&d_err, n))) return rc;
	if (!fr_mode_plain(md) && (rc = mem.alloc(&d_bits, n * MDEMOD_FRAME_BYTES))) return rc;
	HIP_TRY(hipMemcpyAsync(d_list, list.data(), n * sizeof(FrvFrame), hipMemcpyHostToDevice, st));
	const uint64_t units = n * 8;
	const dim3 grid(static_cast<uint32_t>((units + FRV_WAVES - 1) / FRV_WAVES)), block(FRV_WAVES * 64);
	if (fr_mode_plain(md)) {
		HIP_TRY(mdm_launch(fr_viterbi<false>, grid, block, static_cast<size_t>(FRV_WAVES) * FRV_WAVE_LDS, st, soft_dev, m,
		                   static_cast<const FrvFrame *>(d_list), units, cadu_dev, FrvLink<false>{}));
		hipLaunchKernelGGL(fr_errors<false>, dim3(static_cast<uint32_t>(n)), dim3(256), 0, st, soft_dev, static_cast<const FrvFrame *>(d_list),
		                   static_cast<const uint8_t *>(cadu_dev), d_err, FreLink<false>{});
	} else {
		HIP_TRY(mdm_launch(fr_viterbi<true>, grid, block, static_cast<size_t>(FRV_WAVES) * FRV_WAVE_LDS, st, soft_dev, m,
		                   static_cast<const FrvFrame *>(d_list), units, cadu_dev, FrvLink<true>{ d_bits, static_cast<uint32_t>(md.diff) }));
		hipLaunchKernelGGL(fr_errors<true>, dim3(static_cast<uint32_t>(n)), dim3(256), 0, st, soft_dev, static_cast<const FrvFrame *>(d_list),
		                   static_cast<const uint8_t *>(d_bits), d_err, FreLink<true>{ m });
	}
	HIP_TRY(hipGetLastError());
	std::vector<uint32_t> err(n);
	HIP_TRY(hipMemcpyAsync(err.data(), d_err, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (uint64_t f = 0; f < n; f++) frames[f].channel_errors = err[f];
	return MDEMOD_OK;
}

int
fr_decode_device(FrMode md, const mdemod_frames_opts &o, const int8_t *soft_dev, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames, uint64_t cap,
                 uint64_t *n_frames, int device, hipStream_t st)
{
	const uint64_t n_windows = fr_mode_windows(m, md);
	if (!n_windows) return MDEMOD_OK;
	int rc = mdm_select_device(device);
	if (rc) return rc;
	MdmDevMem mem;
	mdemod_frames_candidate *d_cand = nullptr;
	rc = mem.alloc(&d_cand, n_windows);
	if (rc) return rc;
	rc = fr_candidates_run(md, soft_dev, m, d_cand, st);
	if (rc) return rc;
	std::vector<mdemod_frames_candidate> cand(n_windows);
	HIP_TRY(hipMemcpyAsync(cand.data(), d_cand, n_windows * sizeof(mdemod_frames_candidate), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	std::vector<mdemod_frame_info> found;
	(void)fr_track(o, cand.data(), n_windows, m, found);
	*n_frames = found.size();
	const uint64_t n = std::min<uint64_t>(found.size(), cap);
	if (!n) return MDEMOD_OK;
	uint8_t *d_cadu = nullptr;
	rc = mem.alloc(&d_cadu, n * MDEMOD_FRAME_BYTES);
	if (rc) return rc;
	rc = fr_viterbi_run(md, soft_dev, m, found.data(), n, d_cadu, st);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(cadu, d_cadu, n * MDEMOD_FRAME_BYTES, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (uint64_t i = 0; i < n; i++) frames[i] = found[i];
	return MDEMOD_OK;
}

int
fr_decode_host(FrMode md, const mdemod_frames_opts &o, const int8_t *soft, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames, uint64_t cap,
               uint64_t *n_frames, int device)
{
	const uint64_t n_windows = fr_mode_windows(m, md);
	if (!n_windows) return MDEMOD_OK;
	int rc = mdm_select_device(device);
	if (rc) return rc;
	hipStream_t st = nullptr;
	const uint64_t P = o.piece_symbols;
	const uint64_t span = fr_mode_span(md), halo_r = FR_HALO + (md.skew ? 1u : 0u);   /* with skew a rail is read one symbol further on */
	const uint64_t room = std::min<uint64_t>(m, P + FR_FRAME + FR_HALO + halo_r);  /* symbols of the largest piece, halos included */
	MdmDevMem mem;
	int8_t *d_soft = nullptr;
	mdemod_frames_candidate *d_cand = nullptr;
	uint8_t *d_cadu = nullptr;
	if ((rc = mem.alloc(&d_soft, 2 * room)) || (rc = mem.alloc(&d_cand, std::min<uint64_t>(n_windows, P / FR_FRAME)))) return rc;
	/* the candidates: pieces of P symbols from a multiple of 8192, and the 32 (33) symbols the last positions of a piece look ahead */
	std::vector<mdemod_frames_candidate> cand(n_windows);
	for (uint64_t at = 0, done = 0; done < n_windows; at += P) {
		const uint64_t len = std::min<uint64_t>(m - at, P + span), nw = fr_mode_windows(len, md);
		HIP_TRY(hipMemcpyAsync(d_soft, soft + 2 * at, 2 * len, hipMemcpyHostToDevice, st));
		rc = fr_candidates_run(md, d_soft, len, d_cand, st);
		if (rc) return rc;
		HIP_TRY(hipMemcpyAsync(cand.data() + done, d_cand, nw * sizeof(mdemod_frames_candidate), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (uint64_t w = done; w < done + nw; w++) cand[w].position += at;
		done += nw;
	}
	std::vector<mdemod_frame_info> found;
	(void)fr_track(o, cand.data(), n_windows, m, found);
	*n_frames = found.size();
	const uint64_t n = std::min<uint64_t>(found.size(), cap);
	if (!n) return MDEMOD_OK;
	/* the decoding: the frames that fit P + 8192 symbols, from 128 symbols before the first to 128 (129) after the last (where the
	 * stream has them: the piece is clamped where the whole stream would be) */
	const uint64_t most = P / FR_FRAME + 1;
	rc = mem.alloc(&d_cadu, std::min<uint64_t>(n, most) * MDEMOD_FRAME_BYTES);
	if (rc) return rc;
	std::vector<mdemod_frame_info> part;
	for (uint64_t i = 0; i < n;) {
		const uint64_t lo = found[i].position >= FR_HALO ? found[i].position - FR_HALO : 0;
		uint64_t j = i + 1;
		while (j < n && j - i < most && found[j].position + FR_FRAME + halo_r - lo <= room) j++;
		const uint64_t hi = std::min<uint64_t>(m, found[j - 1].position + FR_FRAME + halo_r);
		part.assign(found.begin() + i, found.begin() + j);
		for (mdemod_frame_info &f : part) f.position -= lo;
		HIP_TRY(hipMemcpyAsync(d_soft, soft + 2 * lo, 2 * (hi - lo), hipMemcpyHostToDevice, st));
		rc = fr_viterbi_run(md, d_soft, hi - lo, part.data(), j - i, d_cadu, st);
		if (rc) return rc;
		HIP_TRY(hipMemcpy(cadu + i * MDEMOD_FRAME_BYTES, d_cadu, (j - i) * MDEMOD_FRAME_BYTES, hipMemcpyDeviceToHost));
		for (uint64_t f = i; f < j; f++) found[f].channel_errors = part[f - i].channel_errors;
		i = j;
	}
	for (uint64_t i = 0; i < n; i++) frames[i] = found[i];
	return MDEMOD_OK;
}

extern "C" {

int
mdemod_frames_candidates_device(const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	if (!mdemod_frames_windows(m)) return MDEMOD_OK;
	if (!soft_dev || !cand_dev) REFUSE("mdemod_frames_candidates_device: the symbols and the candidates are needed");
	const int rc = mdm_select_device(device);
	if (rc) return rc;
	return fr_candidates_run(FrMode{ false, false }, soft_dev, m, cand_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_frames_viterbi_device(const int8_t *soft_dev, uint64_t m, mdemod_frame_info *frames, uint64_t n_frames, uint8_t *cadu_dev, int device,
                             void *hip_stream)
try { MDEMOD_API_ENTER
	if (!n_frames) return MDEMOD_OK;
	if (!soft_dev || !frames || !cadu_dev) REFUSE("mdemod_frames_viterbi_device: the symbols, the frames and the output are needed");
	int rc = fr_check_frames(frames, n_frames, m, FrMode{ false, false });
	if (rc) return rc;
	rc = mdm_select_device(device);
	if (rc) return rc;
	return fr_viterbi_run(FrMode{ false, false }, soft_dev, m, frames, n_frames, cadu_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_frames_decode_device(const mdemod_frames_opts *opts, const int8_t *soft_dev, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames,
                            uint64_t cap, uint64_t *n_frames, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	if (!n_frames || (m && !soft_dev) || (cap && (!frames || !cadu)))
		REFUSE("mdemod_frames_decode_device: the symbols, n_frames (and the outputs for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	const int rc = fr_settings(opts, o);
	if (rc) return rc;
	return fr_decode_device(FrMode{ false, false }, o, soft_dev, m, cadu, frames, cap, n_frames, device, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_frames_decode_host(const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m, uint8_t *cadu, mdemod_frame_info *frames,
                          uint64_t cap, uint64_t *n_frames, int device)
try { MDEMOD_API_ENTER
	if (!n_frames || (m && !soft) || (cap && (!frames || !cadu)))
		REFUSE("mdemod_frames_decode_host: the symbols, n_frames (and the outputs for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	const int rc = fr_settings(opts, o);
	if (rc) return rc;
	return fr_decode_host(FrMode{ false, false }, o, soft, m, cadu, frames, cap, n_frames, device);
} MDEMOD_API_CATCH

} /* extern "C" */
