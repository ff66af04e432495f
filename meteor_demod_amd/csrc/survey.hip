/*
 * survey.hip — the survey of include/meteor_demod_amd_survey.h on gfx950: the averaged spectrum of a whole recording, and the
 * confirmation of the detector's candidates (csrc/survey_detect.cpp) by the front end and the recording estimators.
 *
 * sv_spectrum<FMT, LOGN>: N = 2^LOGN points per segment, blocks of T = 256 threads (512 from N = 4096, 1024 at N = 16384).  A
 * segment is transformed by TPS = min(T, N / 4) threads, so a block has S = T / TPS segments in flight (4 at N = 256, 2 at N = 512,
 * else 1), each in its own LDS region.
 * The transform is a decimation-in-frequency radix-4 FFT in place (a last radix-2 pass when LOGN is odd); a thread does
 * B = N / 4 / TPS butterflies per pass, with the four points of a butterfly in registers between its LDS reads and writes:
 *   pass 1    fused into the load: the four samples x[i + q N / 4] come from global memory (consecutive threads, consecutive
 *             samples), are converted and multiplied by the Hann window, and go through the first butterfly before anything
 *             touches the LDS;
 *   middle    LDS -> registers -> LDS, one barrier per pass;
 *   last      fused into the accumulation: the four outputs are squared and added to the thread's accumulators (4 B registers),
 *             which live across all the segments of the block.  Nothing is written back.
 * Twiddles and the window come from one table of N / 8 + 1 entries in LDS (W_N^k for the first octant; the other seven by
 * symmetry; w[n] = 0.5 - 0.5 Re W_N^n): no trigonometric function is evaluated on the device.  An in-place DIF transform
 * leaves X[k] at the digit-reversed position; as only sum |X|^2 is wanted, the accumulators stay in that order and are put in
 * place (and rotated by N / 2: bin 0 = -fs / 2) once, when the block writes its sums.  LDS index p is stored at a swizzled
 * place (SV_PAD: its low five bits XORed with bits 4..6), which takes the late passes' power-of-two strides off a single bank.
 * The table has one float2 of padding per 32 entries (SV_TWI) for the same reason: the passes gather it at strides 4, 16, 64 ...
 * Global memory sees every input byte once, and N floats per part.
 *
 * Determinism: row r's segments are cut into P parts of ceil(count / P) consecutive segments; a part is summed by one group of
 * TPS threads, segment after segment; sv_reduce adds the P parts of a row in ascending order and divides by the count.  P, the
 * grid and every order depend on (n_samples, N, n_rows) only.  No atomics.
 * Built with -ffp-contract=off like the rest of the library: the FMAs are written out.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "demod_internal.h"
#include "hip_host.h"
#include "iq_load.h"
#include "survey_detect.h"

#define SV_BLOCK 256              /* sv_reduce */

/* threads per block of sv_spectrum: a segment of 4096 points or more is spread over more threads, so that no thread does more
 * than four butterflies per pass (its points, twiddles and accumulators stay in registers without spilling) */
constexpr int
sv_threads(int log2n)
{
	return log2n >= 14 ? 1024 : (log2n >= 12 ? 512 : 256);
}

struct SvArgs {
	const void   *iq;
	const float2 *tw;             /* N / 8 + 1 entries: (cos, -sin)(2 pi k / N) */
	float        *partial;        /* [n_rows * P][N] */
	uint64_t      per;            /* segments per row (the last row: the rest) */
	uint64_t      nseg;
	uint32_t      n_rows, P;      /* parts per row: a multiple of the segments in flight per block */
};

/* where entry k of the twiddle table lives in LDS: one float2 of padding per 32, so that the passes' gathers at strides 4, 16, 64 ...
 * (and their doubles and triples) spread over the banks */
#define SV_TWI(k) ((k) + ((k) >> 5))

/* W_N^e = e^{-2 pi i e / N}, 0 <= e < N, from the first octant */
template <int LOGN>
__device__ __forceinline__ float2
sv_tw(const float2 *T, uint32_t e)
{
	constexpr uint32_t N = 1u << LOGN, Q = N / 4;
	const uint32_t quad = e >> (LOGN - 2), r = e & (Q - 1);
	const bool flip = r > N / 8;
	const uint32_t k = flip ? Q - r : r;
	const float2 t = T[SV_TWI(k)];
	float2 w = flip ? make_float2(-t.y, -t.x) : t;
	if (quad & 1) w = make_float2(w.y, -w.x);
	if (quad & 2) w = make_float2(-w.x, -w.y);
	return w;
}

__device__ __forceinline__ float2
sv_cmul(float2 a, float2 w)
{
	return make_float2(__builtin_fmaf(a.x, w.x, -(a.y * w.y)), __builtin_fmaf(a.x, w.y, a.y * w.x));
}

/* the radix-4 DIF butterfly without its twiddles: b_q = sum_r a_r (-i)^{q r} */
__device__ __forceinline__ void
sv_bfly4(float2 &a0, float2 &a1, float2 &a2, float2 &a3)
{
	const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
	const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
	a0 = make_float2(s02.x + s13.x, s02.y + s13.y);
	a2 = make_float2(s02.x - s13.x, s02.y - s13.y);
	a1 = make_float2(d02.x + d13.y, d02.y - d13.x);            /* d02 - i d13 */
	a3 = make_float2(d02.x - d13.y, d02.y + d13.x);            /* d02 + i d13 */
}

/* where LDS index p lives: bits 0..4 swizzled by bits 4..6 (a permutation inside every aligned run of 32 float2, no padding).
 * With it every pass of every size reads (ds_read_b64: 32 lanes over 64 banks) and writes (ds_write_b64: 16 lanes over 32 banks)
 * without a bank conflict: the spans 4 Q = 64 and 16, whose butterflies touch 16 or 4 consecutive points every 64 or 16, would
 * otherwise put 2 and 4 lanes on one bank. */
#define SV_PAD(p) ((p) ^ ((((p) >> 4) & 3) * 5) ^ ((((p) >> 6) & 1) << 4))

template <int FMT, int LOGN>
__global__ void __launch_bounds__(sv_threads(LOGN))
sv_spectrum(SvArgs A)
{
	constexpr int N = 1 << LOGN, Q0 = N / 4, THREADS = sv_threads(LOGN);
	constexpr int TPS = Q0 < THREADS ? Q0 : THREADS, S = THREADS / TPS, B = Q0 / TPS;
	constexpr int PADN = N, NT = N / 8 + 1, NTP = SV_TWI(N / 8) + 1;
	constexpr bool ODD = (LOGN & 1) != 0;
	constexpr int UNR = THREADS == 1024 && B > 2 ? 2 : B;       /* butterflies in flight per thread: 128 registers at 1024 threads */
	extern __shared__ __align__(16) unsigned char sv_lds[];
	float2 *tw = reinterpret_cast<float2 *>(sv_lds);
	const int sub = threadIdx.x / TPS, t = threadIdx.x % TPS;
	float2 *x = reinterpret_cast<float2 *>(sv_lds + (NTP * sizeof(float2) + 15) / 16 * 16) + sub * PADN;
	for (int i = threadIdx.x; i < NT; i += THREADS) tw[SV_TWI(i)] = A.tw[i];
	__syncthreads();

	/* this group's part: `chunk` consecutive segments of its row (the groups of a block share the row, so chunk is uniform) */
	const uint32_t gp = blockIdx.x * S + sub;
	const uint32_t row = gp / A.P, part = gp % A.P;
	const uint64_t row_first = row * A.per;
	const uint64_t cnt = row == A.n_rows - 1 ? A.nseg - row_first : A.per;
	const uint64_t chunk = (cnt + A.P - 1) / A.P;
	const uint64_t seg0 = row_first + part * chunk;
	const uint64_t seg_end = row_first + cnt < seg0 + chunk ? row_first + cnt : seg0 + chunk;

	float acc[4 * B];
#pragma unroll
	for (int i = 0; i < 4 * B; i++) acc[i] = 0.0f;

	for (uint64_t it = 0; it < chunk; it++) {
		const uint64_t seg = seg0 + it;
		const bool active = seg < seg_end;                          /* (uniform over the group, which is whole waves) */
		if (it) __syncthreads();                                    /* the last pass of the segment before has read the LDS */
		/* pass 1: load, convert, window, butterfly of span N */
#pragma unroll UNR
		for (int b = 0; b < B; b++) {
			const int i = t + b * TPS;
			const float2 w1 = sv_tw<LOGN>(tw, i);
			float2 a0 = make_float2(0.0f, 0.0f), a1 = a0, a2 = a0, a3 = a0;
			if (active) {
				const uint64_t at = seg * N + i;
				a0 = md_load_iq<FMT>(A.iq, at);
				a1 = md_load_iq<FMT>(A.iq, at + Q0);
				a2 = md_load_iq<FMT>(A.iq, at + 2 * Q0);
				a3 = md_load_iq<FMT>(A.iq, at + 3 * Q0);
			}
			/* cos(2 pi (i + q N / 4) / N) = c, -s, -c, s with (c, -s) = w1 */
			const float h0 = __builtin_fmaf(-0.5f, w1.x, 0.5f), h1 = __builtin_fmaf(-0.5f, w1.y, 0.5f);
			const float h2 = __builtin_fmaf(0.5f, w1.x, 0.5f), h3 = __builtin_fmaf(0.5f, w1.y, 0.5f);
			a0.x *= h0; a0.y *= h0; a1.x *= h1; a1.y *= h1; a2.x *= h2; a2.y *= h2; a3.x *= h3; a3.y *= h3;
			sv_bfly4(a0, a1, a2, a3);
			x[SV_PAD(i)] = a0;
			x[SV_PAD(i + Q0)] = sv_cmul(a1, w1);
			x[SV_PAD(i + 2 * Q0)] = sv_cmul(a2, sv_tw<LOGN>(tw, 2 * i));
			x[SV_PAD(i + 3 * Q0)] = sv_cmul(a3, sv_tw<LOGN>(tw, 3 * i));
		}
		__syncthreads();
		/* middle passes: span 4 Q, twiddles W_{4Q}^j = W_N^{j N / (4 Q)} */
#pragma unroll
		for (int Q = Q0 / 4; Q > 1; Q /= 4) {
			const int stride = Q0 / Q;
#pragma unroll UNR
			for (int b = 0; b < B; b++) {
				const int i = t + b * TPS;
				const int j = i & (Q - 1);
				const int base = (i - j) * 4 + j;
				float2 a0 = x[SV_PAD(base)], a1 = x[SV_PAD(base + Q)], a2 = x[SV_PAD(base + 2 * Q)], a3 = x[SV_PAD(base + 3 * Q)];
				sv_bfly4(a0, a1, a2, a3);
				const uint32_t e = static_cast<uint32_t>(j * stride);
				x[SV_PAD(base)] = a0;
				x[SV_PAD(base + Q)] = sv_cmul(a1, sv_tw<LOGN>(tw, e));
				x[SV_PAD(base + 2 * Q)] = sv_cmul(a2, sv_tw<LOGN>(tw, 2 * e));
				x[SV_PAD(base + 3 * Q)] = sv_cmul(a3, sv_tw<LOGN>(tw, 3 * e));
			}
			__syncthreads();
		}
		/* last pass (radix 4 of span 4, or two radix-2 of span 2), |X|^2 into the accumulators */
#pragma unroll
		for (int b = 0; b < B; b++) {
			const int pb = 4 * (t + b * TPS);
			float2 a0 = x[SV_PAD(pb)], a1 = x[SV_PAD(pb + 1)], a2 = x[SV_PAD(pb + 2)], a3 = x[SV_PAD(pb + 3)];
			if (ODD) {
				const float2 u0 = make_float2(a0.x + a1.x, a0.y + a1.y), u1 = make_float2(a0.x - a1.x, a0.y - a1.y);
				const float2 u2 = make_float2(a2.x + a3.x, a2.y + a3.y), u3 = make_float2(a2.x - a3.x, a2.y - a3.y);
				a0 = u0; a1 = u1; a2 = u2; a3 = u3;
			} else {
				sv_bfly4(a0, a1, a2, a3);
			}
			acc[4 * b + 0] += __builtin_fmaf(a0.x, a0.x, a0.y * a0.y);
			acc[4 * b + 1] += __builtin_fmaf(a1.x, a1.x, a1.y * a1.y);
			acc[4 * b + 2] += __builtin_fmaf(a2.x, a2.x, a2.y * a2.y);
			acc[4 * b + 3] += __builtin_fmaf(a3.x, a3.x, a3.y * a3.y);
		}
	}

	/* position p holds X[k], k = the digits of p in reverse (most significant digit of p = least significant of k) */
	float *out = A.partial + static_cast<size_t>(gp) * N;
#pragma unroll
	for (int b = 0; b < B; b++) {
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const uint32_t p = 4u * (t + b * TPS) + q;
			uint32_t k = 0, R = 1;
#pragma unroll
			for (int Q = Q0; Q >= (ODD ? 2 : 1); Q /= 4) { k += ((p / Q) & 3u) * R; R *= 4; }
			if (ODD) k += (p & 1u) * R;
			out[(k + N / 2) & (N - 1)] = acc[4 * b + q];
		}
	}
}

/* psd[r][k] = (part 0 + part 1 + ... + part P-1) / count of row r */
__global__ void __launch_bounds__(SV_BLOCK)
sv_reduce(const float *partial, float *psd, uint32_t N, uint32_t P, uint64_t per, uint64_t nseg, uint32_t n_rows)
{
	const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * SV_BLOCK + threadIdx.x;
	if (idx >= static_cast<uint64_t>(n_rows) * N) return;
	const uint32_t r = static_cast<uint32_t>(idx / N), k = static_cast<uint32_t>(idx % N);
	const uint64_t cnt = r == n_rows - 1 ? nseg - r * per : per;
	const float *in = partial + static_cast<size_t>(r) * P * N + k;
	float sum = 0.0f;
	for (uint32_t j = 0; j < P; j++) sum += in[static_cast<size_t>(j) * N];
	psd[idx] = sum / static_cast<float>(cnt);
}

__global__ void
sv_fill_starts(uint64_t *starts, uint64_t pitch, uint64_t skip, uint32_t n)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s < n) starts[s] = s * pitch + skip;
}

namespace {

struct SvGeometry {
	int      log2n;
	uint32_t S;                   /* segments in flight per block */
	uint32_t P;                   /* parts per row */
	uint64_t nseg, per;
	size_t   lds;
};

/* a function of (n_samples, N, n_rows) alone: it fixes who sums what */
void
sv_geometry(uint64_t n_samples, uint32_t N, uint32_t n_rows, SvGeometry &g)
{
	g.log2n = 0;
	while ((1u << g.log2n) < N) g.log2n++;
	const uint32_t threads = static_cast<uint32_t>(sv_threads(g.log2n)), tps = std::min<uint32_t>(threads, N / 4);
	g.S = threads / tps;
	g.nseg = n_samples / N;
	g.per = g.nseg / n_rows;
	const uint64_t most = g.nseg - g.per * (n_rows - 1);                /* the last row's count */
	const uint64_t blocks = N >= 16384 ? 512 : 1024;                    /* in all, about: 2 .. 4 per CU */
	uint64_t P = (blocks * g.S + n_rows - 1) / n_rows;
	P = std::min<uint64_t>(P, (most + 7) / 8);                          /* 8 segments per part or more: the parts' sums stay an eighth of the input */
	P = std::max<uint64_t>(P, 1);
	g.P = static_cast<uint32_t>((P + g.S - 1) / g.S * g.S);
	g.lds = ((SV_TWI(N / 8) + 1) * sizeof(float2) + 15) / 16 * 16 + static_cast<size_t>(g.S) * N * sizeof(float2);
}

template <int FMT>
int
sv_launch_fmt(int log2n, dim3 grid, size_t lds, hipStream_t st, const SvArgs &A)
{
	void (*k)(SvArgs) = nullptr;
	switch (log2n) {
	case 8:  k = sv_spectrum<FMT, 8>; break;
	case 9:  k = sv_spectrum<FMT, 9>; break;
	case 10: k = sv_spectrum<FMT, 10>; break;
	case 11: k = sv_spectrum<FMT, 11>; break;
	case 12: k = sv_spectrum<FMT, 12>; break;
	case 13: k = sv_spectrum<FMT, 13>; break;
	case 14: k = sv_spectrum<FMT, 14>; break;
	default: REFUSE("survey: no spectrum kernel for 2^%d points", log2n);
	}
	HIP_TRY(mdm_launch(k, grid, dim3(sv_threads(log2n)), lds, st, A));
	return MDEMOD_OK;
}

int
sv_spectrum_run(int bps, const void *iq_dev, uint64_t n_samples, uint32_t N, uint32_t n_rows, float *psd_dev, hipStream_t st)
{
	SvGeometry g;
	sv_geometry(n_samples, N, n_rows, g);
	MdmDevMem mem;
	float2 *d_tw = nullptr;
	float *d_part = nullptr;
	int rc = mem.alloc(&d_tw, N / 8 + 1);
	if (rc) return rc;
	rc = mem.alloc(&d_part, static_cast<size_t>(n_rows) * g.P * N);
	if (rc) return rc;
	std::vector<float2> tw(N / 8 + 1);
	for (uint32_t k = 0; k <= N / 8; k++) {
		const double a = 6.283185307179586476925 * k / N;
		tw[k] = make_float2(static_cast<float>(cos(a)), static_cast<float>(-sin(a)));
	}
	HIP_TRY(hipMemcpyAsync(d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, st));
	SvArgs A;
	A.iq = iq_dev; A.tw = d_tw; A.partial = d_part; A.per = g.per; A.nseg = g.nseg; A.n_rows = n_rows; A.P = g.P;
	const dim3 grid(n_rows * (g.P / g.S));
	rc = bps == 8 ? sv_launch_fmt<8>(g.log2n, grid, g.lds, st, A)
	   : bps == 16 ? sv_launch_fmt<16>(g.log2n, grid, g.lds, st, A) : sv_launch_fmt<32>(g.log2n, grid, g.lds, st, A);
	if (rc) return rc;
	const uint64_t cells = static_cast<uint64_t>(n_rows) * N;
	hipLaunchKernelGGL(sv_reduce, dim3(static_cast<uint32_t>((cells + SV_BLOCK - 1) / SV_BLOCK)), dim3(SV_BLOCK), 0, st, d_part, psd_dev, N, g.P,
	                   g.per, g.nseg, n_rows);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));                                   /* (the scratch memory goes with this call) */
	return MDEMOD_OK;
}

int
sv_check_spectrum_args(const mdemod_params *params, const void *iq, uint64_t n_samples, uint32_t N, uint32_t n_rows, const void *out)
{
	if (!params || !iq || !out) REFUSE("survey: params, the samples and the output are needed");
	if (params->bps != 8 && params->bps != 16 && params->bps != 32) REFUSE("survey: %d bits per sample (8, 16 or 32 expected)", params->bps);
	if (!mdemod_survey_fft_size_ok(N)) REFUSE("survey: fft_size %u must be a power of two, %d..%d", N, MDEMOD_SURVEY_MIN_FFT, MDEMOD_SURVEY_MAX_FFT);
	if (n_rows < 1 || n_rows > MDEMOD_SURVEY_MAX_ROWS) REFUSE("survey: n_rows %u must be 1..%d", n_rows, MDEMOD_SURVEY_MAX_ROWS);
	if (n_samples / N < n_rows)
		REFUSE("survey: %llu samples are %llu segments of fft_size %u, fewer than n_rows %u", static_cast<unsigned long long>(n_samples),
		       static_cast<unsigned long long>(n_samples / N), N, n_rows);
	return MDEMOD_OK;
}

/* input samples of a confirmation window: what 2^18 baseband samples and the filter's run-in need, or the whole recording */
uint64_t
sv_window_in(const SurveySettings &s, uint64_t n_samples)
{
	return std::min<uint64_t>(n_samples, ((1ull << 18) + 64) * static_cast<uint64_t>(s.decimation));
}

/* Confirmation: hit k's window is win_in samples of iq_dev from starts[k].  Front end (all hits in one call), clock line,
 * carrier line; the hits get their qualities, `confirmed`, and the refined offset where the carrier line carries it. */
int
sv_confirm(const mdemod_params &params, const SurveySettings &s, std::vector<mdemod_survey_hit> &hits, const void *iq_dev,
           const std::vector<uint64_t> &starts, uint64_t win_in, hipStream_t st)
{
	const uint32_t K = static_cast<uint32_t>(hits.size());
	if (!K) return MDEMOD_OK;
	const uint32_t D = static_cast<uint32_t>(s.decimation);
	const uint64_t n_bb = (win_in + D - 1) / D;
	const uint64_t skip = 2 * MDEMOD_FE_DEFAULT_TAPS_PER_PHASE;          /* the filter's run-in from its zero history */
	if (n_bb < skip + 4096) return MDEMOD_OK;                           /* too short for the estimators: nothing is confirmed */
	uint32_t window = 4096;
	while (window * 2ull <= n_bb - skip && window < (1u << 18)) window *= 2;

	mdemod_params in = params;
	in.n_streams = K;
	std::vector<double> offs(K);
	for (uint32_t k = 0; k < K; k++) offs[k] = hits[k].coarse_offset_hz;
	mdemod_fe_params fp;
	fp.offset_hz = 0.0; fp.decimation = s.decimation; fp.taps_per_phase = 0; fp.offsets_hz = offs.data();
	mdemod_fe *fe = nullptr;
	int rc = mdemod_fe_create(&in, &fp, &fe);
	if (rc) return rc;
	const std::unique_ptr<mdemod_fe, decltype(&mdemod_fe_destroy)> owner(fe, mdemod_fe_destroy);

	MdmDevMem mem;
	uint64_t *d_off = nullptr, *d_starts = nullptr;
	uint32_t *d_cnt = nullptr, *d_nout = nullptr;
	float *d_bb = nullptr, *d_est = nullptr;
	if ((rc = mem.alloc(&d_off, K)) || (rc = mem.alloc(&d_starts, K)) || (rc = mem.alloc(&d_cnt, K)) || (rc = mem.alloc(&d_nout, K)) ||
	    (rc = mem.alloc(&d_bb, 2 * n_bb * K)) || (rc = mem.alloc(&d_est, 4 * static_cast<size_t>(K))))
		return rc;
	const std::vector<uint32_t> cnt(K, static_cast<uint32_t>(win_in));
	HIP_TRY(hipMemcpyAsync(d_off, starts.data(), K * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_cnt, cnt.data(), K * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));
	rc = mdemod_fe_baseband_device(fe, iq_dev, d_off, d_cnt, d_bb, n_bb, static_cast<uint32_t>(n_bb), d_nout, st);
	if (rc) return rc;
	hipLaunchKernelGGL(sv_fill_starts, dim3((K + 63) / 64), dim3(64), 0, st, d_starts, n_bb, skip, K);
	HIP_TRY(hipGetLastError());
	mdemod_params bb = params;
	bb.samplerate = params.samplerate / s.decimation;
	bb.bps = 32;
	float *d_freq = d_est, *d_cq = d_est + K, *d_tf = d_est + 2 * K, *d_kq = d_est + 3 * K;
	rc = mdemod_estimate_carrier(&bb, d_bb, n_bb * K, d_starts, K, window, d_freq, d_cq, st);
	if (rc) return rc;
	rc = mdemod_estimate_clock(&bb, d_bb, n_bb * K, d_starts, d_freq, nullptr, K, window, d_tf, d_kq, st);
	if (rc) return rc;
	std::vector<float> est(4 * static_cast<size_t>(K));
	HIP_TRY(hipMemcpyAsync(est.data(), d_est, est.size() * sizeof(float), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	const double hz_per_rad = params.symrate * (params.oqpsk ? 2.0 : 1.0) / (2 * 3.141592653589793);
	for (uint32_t k = 0; k < K; k++) {
		mdemod_survey_hit &h = hits[k];
		h.carrier_quality = std::isfinite(est[K + k]) ? est[K + k] : 0.0f;
		h.clock_quality = std::isfinite(est[3 * K + k]) ? est[3 * K + k] : 0.0f;
		h.confirmed = h.clock_quality >= s.clock_threshold ? 1 : 0;
		h.refined = h.carrier_quality >= s.carrier_threshold && std::isfinite(est[k]) ? 1 : 0;
		h.offset_hz = h.refined ? h.coarse_offset_hz + est[k] * hz_per_rad : h.coarse_offset_hz;
	}
	std::stable_sort(hits.begin(), hits.end(), [](const mdemod_survey_hit &a, const mdemod_survey_hit &b) {
		if (a.confirmed != b.confirmed) return a.confirmed > b.confirmed;
		return a.psd_snr_db > b.psd_snr_db;
	});
	return MDEMOD_OK;
}

void
sv_give(const std::vector<mdemod_survey_hit> &found, mdemod_survey_hit *hits, uint32_t cap, uint32_t *n_hits)
{
	*n_hits = static_cast<uint32_t>(found.size());
	for (uint32_t i = 0; i < found.size() && i < cap; i++) hits[i] = found[i];
}

} /* namespace */

extern "C" {

int
mdemod_spectrum_device(const mdemod_params *params, const void *iq_dev, uint64_t n_samples, uint32_t fft_size, uint32_t n_rows,
                       float *psd_dev, void *hip_stream)
try { MDEMOD_API_ENTER
	int rc = sv_check_spectrum_args(params, iq_dev, n_samples, fft_size, n_rows, psd_dev);
	if (rc) return rc;
	rc = mdm_select_device(params->device);
	if (rc) return rc;
	return sv_spectrum_run(params->bps, iq_dev, n_samples, fft_size, n_rows, psd_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_survey_device(const mdemod_params *params, const mdemod_survey_opts *opts, const void *iq_dev, uint64_t n_samples,
                     mdemod_survey_hit *hits, uint32_t cap, uint32_t *n_hits, void *hip_stream)
try { MDEMOD_API_ENTER
	if (!params || !iq_dev || !n_hits || (cap && !hits)) REFUSE("mdemod_survey_device: params, the samples, n_hits (and hits for cap > 0) are needed");
	*n_hits = 0;
	SurveySettings s;
	int rc = mdemod_survey_settings(*params, opts, s);
	if (rc) return rc;
	mdemod_fe_params fp;
	fp.offset_hz = 0.0; fp.decimation = s.decimation; fp.taps_per_phase = 0; fp.offsets_hz = nullptr;
	rc = mdemod_fe_design(params, &fp, nullptr, 0, nullptr, nullptr);   /* (a caller's D that does not fit is refused before any work) */
	if (rc) return rc;
	const uint32_t N = s.fft_size;
	const uint64_t nseg = n_samples / N;
	if (nseg == 0) REFUSE("survey: %llu samples are less than one segment of fft_size %u", static_cast<unsigned long long>(n_samples), N);
	const uint32_t rows = static_cast<uint32_t>(std::min<uint64_t>(s.n_rows, nseg));
	rc = mdm_select_device(params->device);
	if (rc) return rc;
	hipStream_t st = static_cast<hipStream_t>(hip_stream);
	MdmDevMem mem;
	float *d_psd = nullptr;
	rc = mem.alloc(&d_psd, static_cast<size_t>(rows) * N);
	if (rc) return rc;
	rc = sv_spectrum_run(params->bps, iq_dev, n_samples, N, rows, d_psd, st);
	if (rc) return rc;
	std::vector<float> psd(static_cast<size_t>(rows) * N);
	HIP_TRY(hipMemcpyAsync(psd.data(), d_psd, psd.size() * sizeof(float), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	std::vector<mdemod_survey_hit> found;
	rc = mdemod_survey_detect_host(*params, s, psd.data(), N, rows, found);
	if (rc) return rc;
	const uint64_t win_in = sv_window_in(s, n_samples), per = nseg / rows;
	std::vector<uint64_t> starts(found.size());
	for (size_t k = 0; k < found.size(); k++)
		starts[k] = std::min<uint64_t>(found[k].best_row * per * N, n_samples - win_in);
	rc = sv_confirm(*params, s, found, iq_dev, starts, win_in, st);
	if (rc) return rc;
	sv_give(found, hits, cap, n_hits);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_survey_host(const mdemod_params *params, const mdemod_survey_opts *opts, const void *iq_host, uint64_t n_samples,
                   mdemod_survey_hit *hits, uint32_t cap, uint32_t *n_hits)
try { MDEMOD_API_ENTER
	if (!params || !iq_host || !n_hits || (cap && !hits)) REFUSE("mdemod_survey_host: params, the samples, n_hits (and hits for cap > 0) are needed");
	*n_hits = 0;
	SurveySettings s;
	int rc = mdemod_survey_settings(*params, opts, s);
	if (rc) return rc;
	mdemod_fe_params fp;
	fp.offset_hz = 0.0; fp.decimation = s.decimation; fp.taps_per_phase = 0; fp.offsets_hz = nullptr;
	rc = mdemod_fe_design(params, &fp, nullptr, 0, nullptr, nullptr);
	if (rc) return rc;
	const uint32_t N = s.fft_size;
	if (n_samples / N == 0) REFUSE("survey: %llu samples are less than one segment of fft_size %u", static_cast<unsigned long long>(n_samples), N);
	rc = mdm_select_device(params->device);
	if (rc) return rc;
	hipStream_t st = nullptr;
	const size_t sb = 2 * static_cast<size_t>(params->bps) / 8;
	const unsigned char *src = static_cast<const unsigned char *>(iq_host);
	/* the spectrum piece by piece: a piece is whole segments, and gives whole rows */
	const uint64_t piece = 1ull << 28;
	const uint64_t usable = n_samples / N * N;
	std::vector<float> psd;
	std::vector<uint64_t> row_start;
	{
		MdmDevMem mem;
		unsigned char *d_in = nullptr;
		float *d_psd = nullptr;
		rc = mem.alloc(&d_in, static_cast<size_t>(std::min(piece, usable)) * sb);
		if (rc) return rc;
		rc = mem.alloc(&d_psd, static_cast<size_t>(s.n_rows) * N);
		if (rc) return rc;
		for (uint64_t at = 0; at < usable; at += piece) {
			const uint64_t len = std::min(piece, usable - at), segs = len / N;
			uint64_t rows = std::max<uint64_t>(1, static_cast<uint64_t>(static_cast<double>(s.n_rows) * len / usable));
			rows = std::min<uint64_t>(std::min<uint64_t>(rows, segs), s.n_rows);
			if (row_start.size() + rows > MDEMOD_SURVEY_MAX_ROWS) rows = 1;
			HIP_TRY(hipMemcpy(d_in, src + at * sb, len * sb, hipMemcpyHostToDevice));
			rc = sv_spectrum_run(params->bps, d_in, len, N, static_cast<uint32_t>(rows), d_psd, st);
			if (rc) return rc;
			const size_t have = psd.size();
			psd.resize(have + rows * N);
			HIP_TRY(hipMemcpy(psd.data() + have, d_psd, rows * N * sizeof(float), hipMemcpyDeviceToHost));
			for (uint64_t r = 0; r < rows; r++) row_start.push_back(at + r * (segs / rows) * N);
		}
	}
	if (row_start.size() > MDEMOD_SURVEY_MAX_ROWS) REFUSE("survey: a recording of this length needs n_rows below %u", s.n_rows);
	std::vector<mdemod_survey_hit> found;
	rc = mdemod_survey_detect_host(*params, s, psd.data(), N, static_cast<uint32_t>(row_start.size()), found);
	if (rc) return rc;
	if (!found.empty()) {
		/* the candidates' windows side by side in device memory */
		const uint64_t win_in = sv_window_in(s, n_samples);
		MdmDevMem mem;
		unsigned char *d_win = nullptr;
		rc = mem.alloc(&d_win, static_cast<size_t>(win_in) * sb * found.size());
		if (rc) return rc;
		std::vector<uint64_t> starts(found.size());
		for (size_t k = 0; k < found.size(); k++) {
			const uint64_t from = std::min<uint64_t>(row_start[found[k].best_row], n_samples - win_in);
			HIP_TRY(hipMemcpy(d_win + k * win_in * sb, src + from * sb, win_in * sb, hipMemcpyHostToDevice));
			starts[k] = k * win_in;
		}
		rc = sv_confirm(*params, s, found, d_win, starts, win_in, st);
		if (rc) return rc;
	}
	sv_give(found, hits, cap, n_hits);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
