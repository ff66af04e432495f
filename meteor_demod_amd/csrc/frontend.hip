/*
 * frontend.hip — the front end of include/meteor_demod_amd_frontend.h on gfx950: convert, mix, low-pass, decimate, for many
 * streams, ragged counts, state carried across calls; then the demodulator of include/meteor_demod_amd.h on the baseband.
 *
 * fe_filter: one block of 256 threads per (stream, tile of T consecutive outputs).  The block stages the mixed samples its tile
 * needs, z[m0 D - (L-1) .. (m0 + T - 1) D], into LDS - from the stream's history (the last L-1 mixed samples of earlier calls)
 * and from this call's input - in polyphase order (row r = index mod D, column = index / D), so that at every tap the threads of
 * a wave read consecutive LDS words.  Output j of the tile is then
 *     y = sum over phases r = 0 .. D-1 (ascending), columns q ascending, of h[q D + r] * z[row r][j + q]
 * one explicit FMA per tap on the (re, im) pair, in that fixed order whatever the tile, the call or the batch slot.  When the
 * span of a tile of 256 outputs does not fit the LDS (large D x taps), G threads share an output: thread g sums a fixed range
 * of phases, and the G partial sums are added in the order g = 0 .. G-1.  T, G and the order depend on the settings only.
 * fe_advance: one block per stream afterwards: the new history (double-buffered: the filter of this call reads the other copy),
 * the absolute index, the output count.
 * The mixer: p(n) = n * step mod 2^32, rounded to 20 bits, e^{j 2 pi p / 2^32} = hi[p >> 10] * lo[p & 1023] from two 1024-entry
 * tables in LDS (computed in double on the host, as synth_core.h's carrier).  No per-sample trig.
 * Built with -ffp-contract=off like the rest of the library: the FMAs are written out, nothing else is fused.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "demod_internal.h"
#include "frontend_design.h"
#include "hip_host.h"
#include "iq_load.h"

#define FE_BLOCK      256
#define FE_SPAN_MAX   6144          /* staged samples per tile at most (48 KiB of z) */
#define FE_TRIG       1024

struct FeConsts {
	int32_t  D, L, H;                /* decimation, taps, history length L - 1 */
	int32_t  T, G, R;                /* outputs per tile, threads per output, outputs per thread */
	int32_t  span, Qp;               /* staged samples, LDS row pitch (float2) */
	int32_t  nq0;                    /* taps of phase 0 (H / D + 1); the other phases have nq0 - 1 (D >= 2) */
	int32_t  mix;                    /* any stream has step != 0 */
	uint32_t dmagic;                 /* floor(2^32 / D) + 1: e / D == umulhi(e, dmagic) for e D < 2^32 (D >= 2) */
	uint32_t n_streams;
	uint32_t tiles;                  /* tiles per stream in the grid */
	uint32_t bb_cap;                 /* outputs per stream at most */
	uint32_t lds_z, lds_h, lds_trig, lds_part;   /* byte offsets */
};

struct FeArgs {
	FeConsts         c;
	const void      *iq;
	const uint64_t  *iq_offset;
	const uint32_t  *n_samples;
	const float     *taps;           /* phase-major: taps[r * nq0 + q] = h[q D + r] */
	const float2    *trig;           /* hi[1024], lo[1024] */
	const uint32_t  *steps;
	uint64_t        *n_abs;
	const float2    *hist_in;        /* [n_streams][H] */
	float2          *hist_out;
	float2          *bb;
	uint64_t         bb_stride;
	uint32_t        *n_out;
};

/* x * e^{j 2 pi p(n) / 2^32}; p rounded to 20 bits */
__device__ __forceinline__ float2
fe_mix(float2 x, uint64_t n, uint32_t step, const float2 *trig)
{
	const uint32_t p = static_cast<uint32_t>(n) * step;
	const uint32_t p20 = ((p + 0x800u) >> 12) & 0xFFFFFu;
	const float2 a = trig[p20 >> 10], b = trig[FE_TRIG + (p20 & 1023u)];
	const float c = a.x * b.x - a.y * b.y, s = a.x * b.y + a.y * b.x;
	return make_float2(x.x * c - x.y * s, x.x * s + x.y * c);
}

__device__ __forceinline__ uint64_t
fe_ceil_div(uint64_t a, uint32_t d)
{
	return (a + d - 1) / d;
}

/* R: outputs per thread (G == 1), summed side by side in the same tap loop - each in its own fixed order, so R changes no byte */
template <int FMT, int R>
__global__ void __launch_bounds__(FE_BLOCK)
fe_filter(FeArgs A)
{
	extern __shared__ __align__(16) unsigned char fe_lds[];
	const FeConsts &c = A.c;
	const uint32_t s = blockIdx.x / c.tiles, tile = blockIdx.x % c.tiles;
	const uint32_t D = static_cast<uint32_t>(c.D);
	const uint32_t n = A.n_samples[s];
	const uint64_t n_abs = A.n_abs[s];
	const uint64_t done = fe_ceil_div(n_abs, D), total = fe_ceil_div(n_abs + n, D);
	const uint64_t n_out = total - done < c.bb_cap ? total - done : c.bb_cap;
	const uint64_t first = static_cast<uint64_t>(tile) * c.T;
	if (first >= n_out) return;                                      /* (uniform: the whole block) */
	const uint32_t step = A.steps[s];
	const bool mix = c.mix && step != 0;
	float2 *z = reinterpret_cast<float2 *>(fe_lds + c.lds_z);
	float *h = reinterpret_cast<float *>(fe_lds + c.lds_h);
	float2 *trig = reinterpret_cast<float2 *>(fe_lds + c.lds_trig);
	const int t = threadIdx.x;
	if (mix)
		for (int i = t; i < 2 * FE_TRIG; i += FE_BLOCK) trig[i] = A.trig[i];
	const int n_h = c.D * c.nq0;
	for (int i = t; i < n_h; i += FE_BLOCK) h[i] = A.taps[i];
	__syncthreads();

	/* stage z[zs .. zs + span) in polyphase order; zs >= n_abs - H because the tile's first output is at or past ceil(n_abs / D) */
	const int64_t zs = static_cast<int64_t>((done + first) * D) - c.H;
	const uint64_t in_off = A.iq_offset[s];
	const float2 *hist = A.hist_in + static_cast<size_t>(s) * c.H;
	for (int e = t; e < c.span; e += FE_BLOCK) {
		const int64_t idx = zs + e;
		float2 v = make_float2(0.0f, 0.0f);
		if (idx >= 0) {
			if (static_cast<uint64_t>(idx) < n_abs) {
				v = hist[c.H - static_cast<int64_t>(n_abs - static_cast<uint64_t>(idx))];
			} else if (static_cast<uint64_t>(idx) < n_abs + n) {
				v = md_load_iq<FMT>(A.iq, in_off + (static_cast<uint64_t>(idx) - n_abs));
				if (mix) v = fe_mix(v, static_cast<uint64_t>(idx), step, trig);
			}
		}
		const uint32_t col = c.D == 1 ? static_cast<uint32_t>(e) : __umulhi(static_cast<uint32_t>(e), c.dmagic);
		z[(e - col * c.D) * c.Qp + col] = v;
	}
	__syncthreads();

	float2 *out = A.bb + s * A.bb_stride;
	if (c.G == 1) {
		float re[R], im[R];
#pragma unroll
		for (int q = 0; q < R; q++) { re[q] = 0.0f; im[q] = 0.0f; }
		for (int r = 0; r < c.D; r++) {
			const int nq = r == 0 ? c.nq0 : c.nq0 - 1;
			const float *hr = h + r * c.nq0;
			const float2 *zr = z + r * c.Qp + t;
#pragma unroll 2
			for (int k = 0; k < nq; k++) {
				const float hk = hr[k];
#pragma unroll
				for (int q = 0; q < R; q++) {
					const float2 v = zr[k + q * FE_BLOCK];
					re[q] = __builtin_fmaf(hk, v.x, re[q]);
					im[q] = __builtin_fmaf(hk, v.y, im[q]);
				}
			}
		}
#pragma unroll
		for (int q = 0; q < R; q++) {
			const uint64_t m = first + t + q * FE_BLOCK;
			if (m < n_out) out[m] = make_float2(re[q], im[q]);
		}
	} else {
		float2 *part = reinterpret_cast<float2 *>(fe_lds + c.lds_part);
		const int j = t / c.G, g = t % c.G;
		const int per = (c.D + c.G - 1) / c.G;
		const int r_lo = g * per, r_hi = r_lo + per < c.D ? r_lo + per : c.D;
		float re = 0.0f, im = 0.0f;
		for (int r = r_lo; r < r_hi; r++) {
			const int nq = r == 0 ? c.nq0 : c.nq0 - 1;
			const float *hr = h + r * c.nq0;
			const float2 *zr = z + r * c.Qp + j;
			for (int k = 0; k < nq; k++) {
				const float hk = hr[k];
				const float2 v = zr[k];
				re = __builtin_fmaf(hk, v.x, re);
				im = __builtin_fmaf(hk, v.y, im);
			}
		}
		part[t] = make_float2(re, im);
		__syncthreads();
		if (g == 0) {
			const uint64_t m = first + j;
			float2 acc = part[t];
			for (int i = 1; i < c.G; i++) { acc.x = acc.x + part[t + i].x; acc.y = acc.y + part[t + i].y; }
			if (m < n_out) out[m] = acc;
		}
	}
}

/* history for the next call, the absolute index, the count: one block per stream, after fe_filter on the same stream */
template <int FMT>
__global__ void __launch_bounds__(FE_BLOCK)
fe_advance(FeArgs A)
{
	__shared__ float2 trig[2 * FE_TRIG];
	const FeConsts &c = A.c;
	const uint32_t s = blockIdx.x;
	const uint32_t D = static_cast<uint32_t>(c.D);
	const uint32_t n = A.n_samples[s];
	const uint64_t n_abs = A.n_abs[s];
	const uint64_t N = n_abs + n;
	const uint32_t step = A.steps[s];
	const bool mix = c.mix && step != 0;
	if (mix)
		for (int i = threadIdx.x; i < 2 * FE_TRIG; i += FE_BLOCK) trig[i] = A.trig[i];
	__syncthreads();
	const float2 *hin = A.hist_in + static_cast<size_t>(s) * c.H;
	float2 *hout = A.hist_out + static_cast<size_t>(s) * c.H;
	const uint64_t in_off = A.iq_offset[s];
	for (int i = threadIdx.x; i < c.H; i += FE_BLOCK) {
		const int64_t idx = static_cast<int64_t>(N) - c.H + i;
		float2 v = make_float2(0.0f, 0.0f);
		if (idx >= 0) {
			if (static_cast<uint64_t>(idx) < n_abs) {
				v = hin[c.H - static_cast<int64_t>(n_abs - static_cast<uint64_t>(idx))];
			} else {
				v = md_load_iq<FMT>(A.iq, in_off + (static_cast<uint64_t>(idx) - n_abs));
				if (mix) v = fe_mix(v, static_cast<uint64_t>(idx), step, trig);
			}
		}
		hout[i] = v;
	}
	__syncthreads();                                                /* every thread has read n_abs */
	if (threadIdx.x == 0) {
		const uint64_t produced = fe_ceil_div(N, D) - fe_ceil_div(n_abs, D);
		A.n_out[s] = static_cast<uint32_t>(produced < c.bb_cap ? produced : c.bb_cap);
		A.n_abs[s] = N;
	}
}

__global__ void
fe_fill_rows(uint64_t *off, uint64_t pitch, uint32_t n_streams)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s < n_streams) off[s] = s * pitch;
}

struct mdemod_fe {
	mdemod_params  input;
	FeDesign       design;
	FeConsts       c;
	size_t         lds_bytes;
	mdemod_ctx    *inner;
	float         *d_taps;
	float2        *d_trig;
	uint32_t      *d_steps;
	uint64_t      *d_n_abs;
	float2        *d_hist[2];
	int            parity;          /* which history copy the next call reads */
	/* mdemod_fe_process_device / _host: the baseband rows (grow only) */
	float2        *d_bb;
	uint64_t       bb_stride;
	uint64_t      *d_bb_off;
	uint32_t      *d_bb_cnt;
	/* mdemod_fe_process_host: input staging */
	void          *d_in;
	size_t         in_bytes;
	uint64_t      *d_in_off;
	uint32_t      *d_in_cnt;
	MdmDevMem      mem;
};

namespace {

/* tile geometry: 256 outputs per block (512 / 1024 when they fit), else G threads per output; the span always fits FE_SPAN_MAX */
void
fe_plan(const FeDesign &d, bool mix, FeConsts &c, size_t &lds)
{
	memset(&c, 0, sizeof(c));
	c.D = d.decimation;
	c.L = static_cast<int32_t>(d.n_taps);
	c.H = c.L - 1;
	c.nq0 = c.H / c.D + 1;
	c.mix = mix ? 1 : 0;
	c.G = 0;
	for (int R = 4; R >= 1 && !c.G; R /= 2)
		if ((FE_BLOCK * R - 1) * c.D + c.L <= FE_SPAN_MAX) { c.G = 1; c.R = R; c.T = FE_BLOCK * R; }
	for (int G = 2; G <= FE_BLOCK && !c.G; G *= 2)
		if (G <= c.D && (FE_BLOCK / G - 1) * c.D + c.L <= FE_SPAN_MAX) { c.G = G; c.R = 1; c.T = FE_BLOCK / G; }
	c.span = (c.T - 1) * c.D + c.L;
	c.dmagic = static_cast<uint32_t>(0x100000000ull / static_cast<uint32_t>(c.D) + 1);
	c.Qp = ((c.span + c.D - 1) / c.D) | 1;
	size_t off = 0;
	c.lds_z = static_cast<uint32_t>(off);    off += static_cast<size_t>(c.D) * c.Qp * sizeof(float2);
	c.lds_h = static_cast<uint32_t>(off);    off += (static_cast<size_t>(c.D) * c.nq0 * sizeof(float) + 15) / 16 * 16;
	c.lds_trig = static_cast<uint32_t>(off); off += mix ? 2 * FE_TRIG * sizeof(float2) : 0;
	c.lds_part = static_cast<uint32_t>(off); off += c.G > 1 ? FE_BLOCK * sizeof(float2) : 0;
	lds = off;
}

int
fe_reset_state(mdemod_fe *fe, hipStream_t st)
{
	const size_t n = fe->input.n_streams;
	HIP_TRY(hipMemsetAsync(fe->d_n_abs, 0, n * sizeof(uint64_t), st));
	HIP_TRY(hipMemsetAsync(fe->d_hist[0], 0, n * (fe->c.H ? fe->c.H : 1) * sizeof(float2), st));
	fe->parity = 0;
	return MDEMOD_OK;
}

/* fe_create: the tables and the zero state, on a private stream that is waited for */
int
fe_upload(mdemod_fe *fe, const std::vector<float> &taps, const std::vector<float2> &trig)
{
	MdmStream own;
	HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
	HIP_TRY(hipMemcpyAsync(fe->d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, own.s));
	HIP_TRY(hipMemcpyAsync(fe->d_trig, trig.data(), trig.size() * sizeof(float2), hipMemcpyHostToDevice, own.s));
	HIP_TRY(hipMemcpyAsync(fe->d_steps, fe->design.steps.data(), fe->design.steps.size() * sizeof(uint32_t), hipMemcpyHostToDevice, own.s));
	const int rc = fe_reset_state(fe, own.s);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(own.s));
	return MDEMOD_OK;
}

int
fe_create(const mdemod_params *input, const mdemod_fe_params *p, bool with_inner, mdemod_fe **out)
{
	if (!input || !p || !out || input->n_streams == 0) { mdm_note_error("mdemod_fe_create: input, fe, out and at least one stream are needed"); return MDEMOD_ERR_PARAM; }
	*out = nullptr;
	FeDesign d;
	int rc = mdemod_fe_design_host(*input, *p, d);
	if (rc) return rc;
	mdemod_fe *fe = new mdemod_fe();
	fe->input = *input;
	fe->design = d;
	bool mix = false;
	for (uint32_t s : d.steps) mix = mix || s != 0;
	fe_plan(d, mix, fe->c, fe->lds_bytes);
	fe->c.n_streams = input->n_streams;
#define FE_CREATE_TRY(expr) do { rc = (expr); if (rc) { mdemod_fe_destroy(fe); return rc; } } while (0)
	if (with_inner) {
		mdemod_params ip = *input;
		ip.samplerate = d.samplerate_out;
		ip.bps = 32;
		FE_CREATE_TRY(mdemod_create(&ip, &fe->inner));             /* (its refusals pass through with their own text) */
	}
	FE_CREATE_TRY(mdm_select_device(input->device));
	const size_t n = input->n_streams, H = fe->c.H ? fe->c.H : 1;
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_taps, static_cast<size_t>(fe->c.D) * fe->c.nq0));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_trig, 2 * FE_TRIG));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_steps, n));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_n_abs, n));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_hist[0], n * H));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_hist[1], n * H));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_bb_off, n));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_bb_cnt, n));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_in_off, n));
	FE_CREATE_TRY(fe->mem.alloc(&fe->d_in_cnt, n));
	/* phase-major taps, zero where a phase has one tap fewer; the mixer's tables in double, rounded once */
	std::vector<float> ht(static_cast<size_t>(fe->c.D) * fe->c.nq0, 0.0f);
	for (int r = 0; r < fe->c.D; r++)
		for (int q = 0; q < fe->c.nq0; q++)
			if (q * fe->c.D + r < fe->c.L) ht[static_cast<size_t>(r) * fe->c.nq0 + q] = d.taps[q * fe->c.D + r];
	std::vector<float2> trig(2 * FE_TRIG);
	for (int i = 0; i < FE_TRIG; i++) {
		const double a = 6.283185307179586476925 * i / 1024.0, b = 6.283185307179586476925 * i / 1048576.0;
		trig[i] = make_float2(static_cast<float>(cos(a)), static_cast<float>(sin(a)));
		trig[FE_TRIG + i] = make_float2(static_cast<float>(cos(b)), static_cast<float>(sin(b)));
	}
	FE_CREATE_TRY(fe_upload(fe, ht, trig));
#undef FE_CREATE_TRY
	*out = fe;
	return MDEMOD_OK;
}

int
fe_launch(mdemod_fe *fe, const void *iq, const uint64_t *off, const uint32_t *cnt, float2 *bb, uint64_t bb_stride, uint32_t bb_cap,
          uint32_t *n_out, hipStream_t st)
{
	FeArgs A;
	memset(&A, 0, sizeof(A));
	A.c = fe->c;
	A.c.bb_cap = bb_cap;
	A.c.tiles = bb_cap ? (bb_cap + fe->c.T - 1) / fe->c.T : 1;
	A.iq = iq; A.iq_offset = off; A.n_samples = cnt;
	A.taps = fe->d_taps; A.trig = fe->d_trig; A.steps = fe->d_steps; A.n_abs = fe->d_n_abs;
	A.hist_in = fe->d_hist[fe->parity]; A.hist_out = fe->d_hist[fe->parity ^ 1];
	A.bb = bb; A.bb_stride = bb_stride; A.n_out = n_out;
	const uint64_t blocks = static_cast<uint64_t>(A.c.tiles) * fe->c.n_streams;
	if (blocks > 0x7FFFFFFFull) { mdm_note_error("front end: %llu blocks in one call: fewer streams or a smaller bb_cap", static_cast<unsigned long long>(blocks)); return MDEMOD_ERR_PARAM; }
	const int fmt = fe->input.bps;
	if (bb_cap) {
		void (*kfn)(FeArgs) = nullptr;
#define FE_PICK(F) (fe->c.R == 4 ? fe_filter<F, 4> : (fe->c.R == 2 ? fe_filter<F, 2> : fe_filter<F, 1>))
		kfn = fmt == 8 ? FE_PICK(8) : (fmt == 16 ? FE_PICK(16) : FE_PICK(32));
#undef FE_PICK
		HIP_TRY(mdm_launch(kfn, dim3(static_cast<uint32_t>(blocks)), dim3(FE_BLOCK), fe->lds_bytes, st, A));
	}
	if (fmt == 8) hipLaunchKernelGGL(fe_advance<8>, dim3(fe->c.n_streams), dim3(FE_BLOCK), 0, st, A);
	else if (fmt == 16) hipLaunchKernelGGL(fe_advance<16>, dim3(fe->c.n_streams), dim3(FE_BLOCK), 0, st, A);
	else hipLaunchKernelGGL(fe_advance<32>, dim3(fe->c.n_streams), dim3(FE_BLOCK), 0, st, A);
	HIP_TRY(hipGetLastError());
	fe->parity ^= 1;
	return MDEMOD_OK;
}

/* the baseband rows of the process calls: at least `outputs` per stream */
int
fe_grow_bb(mdemod_fe *fe, uint64_t outputs, hipStream_t st)
{
	const uint64_t want = (outputs + 63) / 64 * 64;
	if (fe->d_bb && fe->bb_stride >= want) return MDEMOD_OK;
	if (fe->d_bb) {
		HIP_TRY(hipStreamSynchronize(st));                           /* (a call still queued may read the old rows) */
		fe->mem.release(fe->d_bb);
		fe->d_bb = nullptr;
	}
	int rc = fe->mem.alloc(&fe->d_bb, want * fe->c.n_streams);
	if (rc) return rc;
	fe->bb_stride = want;
	hipLaunchKernelGGL(fe_fill_rows, dim3((fe->c.n_streams + 255) / 256), dim3(256), 0, st, fe->d_bb_off, want, fe->c.n_streams);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

} /* namespace */

extern "C" {

int
mdemod_fe_create(const mdemod_params *input, const mdemod_fe_params *fe, mdemod_fe **out)
try { MDEMOD_API_ENTER
	return fe_create(input, fe, true, out);
} MDEMOD_API_CATCH

void
mdemod_fe_destroy(mdemod_fe *fe)
{
	if (!fe) return;
	(void)hipSetDevice(fe->input.device);
	if (fe->inner) mdemod_destroy(fe->inner);
	delete fe;                                                      /* (with everything fe->mem holds) */
}

int
mdemod_fe_reset(mdemod_fe *fe, void *hip_stream)
try { MDEMOD_API_ENTER
	if (!fe) return MDEMOD_ERR_PARAM;
	int rc = mdm_select_device(fe->input.device);
	if (rc) return rc;
	rc = fe_reset_state(fe, static_cast<hipStream_t>(hip_stream));
	if (rc) return rc;
	return fe->inner ? mdemod_reset(fe->inner, hip_stream) : MDEMOD_OK;
} MDEMOD_API_CATCH

mdemod_ctx *
mdemod_fe_demodulator(mdemod_fe *fe)
{
	return fe ? fe->inner : nullptr;
}

uint64_t
mdemod_fe_max_outputs(const mdemod_fe *fe, uint64_t n_samples)
{
	if (!fe) return 0;
	return (n_samples + fe->c.D - 1) / fe->c.D;
}

int
mdemod_fe_baseband_device(mdemod_fe *fe, const void *iq_dev, const uint64_t *iq_offset_dev, const uint32_t *n_samples_dev,
                          float *bb_dev, uint64_t bb_stride, uint32_t bb_cap, uint32_t *n_out_dev, void *hip_stream)
try { MDEMOD_API_ENTER
	if (!fe || !iq_dev || !iq_offset_dev || !n_samples_dev || !bb_dev || !n_out_dev) { mdm_note_error("mdemod_fe_baseband_device: a pointer is NULL"); return MDEMOD_ERR_PARAM; }
	if (bb_cap > bb_stride) { mdm_note_error("mdemod_fe_baseband_device: bb_cap %u exceeds the row pitch %llu", bb_cap, static_cast<unsigned long long>(bb_stride)); return MDEMOD_ERR_PARAM; }
	int rc = mdm_select_device(fe->input.device);
	if (rc) return rc;
	return fe_launch(fe, iq_dev, iq_offset_dev, n_samples_dev, reinterpret_cast<float2 *>(bb_dev), bb_stride, bb_cap, n_out_dev,
	                 static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_fe_process_device(mdemod_fe *fe, const void *iq_dev, const uint64_t *iq_offset_dev, const uint32_t *n_samples_dev,
                         uint32_t max_samples, int8_t *soft_dev, uint64_t soft_stride_symbols, uint32_t soft_cap_symbols,
                         void *hip_stream)
try { MDEMOD_API_ENTER
	if (!fe || !fe->inner || !iq_dev || !iq_offset_dev || !n_samples_dev || !soft_dev) { mdm_note_error("mdemod_fe_process_device: a pointer is NULL"); return MDEMOD_ERR_PARAM; }
	if (soft_cap_symbols > soft_stride_symbols) { mdm_note_error("mdemod_fe_process_device: soft capacity beyond the row pitch"); return MDEMOD_ERR_PARAM; }
	int rc = mdm_select_device(fe->input.device);
	if (rc) return rc;
	hipStream_t st = static_cast<hipStream_t>(hip_stream);
	const uint64_t outs = mdemod_fe_max_outputs(fe, max_samples);
	rc = fe_grow_bb(fe, outs, st);
	if (rc) return rc;
	rc = fe_launch(fe, iq_dev, iq_offset_dev, n_samples_dev, fe->d_bb, fe->bb_stride, static_cast<uint32_t>(outs), fe->d_bb_cnt, st);
	if (rc) return rc;
	return mdemod_process_device(fe->inner, fe->d_bb, fe->d_bb_off, fe->d_bb_cnt, soft_dev, soft_stride_symbols, soft_cap_symbols, hip_stream);
} MDEMOD_API_CATCH

int
mdemod_fe_process_host(mdemod_fe *fe, const void *const *iq_host, const uint32_t *n_samples,
                       int8_t *const *soft_host, const uint32_t *soft_cap, uint32_t *n_symbols)
try { MDEMOD_API_ENTER
	if (!fe || !fe->inner || !iq_host || !n_samples || !soft_host || !soft_cap || !n_symbols) { mdm_note_error("mdemod_fe_process_host: a pointer is NULL"); return MDEMOD_ERR_PARAM; }
	int rc = mdm_select_device(fe->input.device);
	if (rc) return rc;
	/* plain and synchronous: the blocks side by side in one device buffer, the front end, the baseband back to the host, and the
	   inner context's own host path on it (8 / D bytes per input sample come back: a fraction of what went in for D >= 2) */
	const uint32_t ns = fe->c.n_streams;
	const size_t sb = 2 * static_cast<size_t>(fe->input.bps) / 8;
	std::vector<uint64_t> off(ns);
	uint64_t total = 0;
	uint32_t most = 0;
	for (uint32_t s = 0; s < ns; s++) {
		if (n_samples[s] && !iq_host[s]) { mdm_note_error("mdemod_fe_process_host: stream %u has samples and no buffer", s); return MDEMOD_ERR_PARAM; }
		off[s] = total;
		total += n_samples[s];
		if (n_samples[s] > most) most = n_samples[s];
	}
	hipStream_t st = nullptr;
	HIP_TRY(hipDeviceSynchronize());
	if (total * sb > fe->in_bytes) {
		if (fe->d_in) { fe->mem.release(fe->d_in); fe->d_in = nullptr; fe->in_bytes = 0; }
		unsigned char *p = nullptr;
		rc = fe->mem.alloc(&p, total * sb);
		if (rc) return rc;
		fe->d_in = p;
		fe->in_bytes = total * sb;
	}
	for (uint32_t s = 0; s < ns; s++)
		if (n_samples[s]) HIP_TRY(hipMemcpy(static_cast<unsigned char *>(fe->d_in) + off[s] * sb, iq_host[s], n_samples[s] * sb, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(fe->d_in_off, off.data(), ns * sizeof(uint64_t), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(fe->d_in_cnt, n_samples, ns * sizeof(uint32_t), hipMemcpyHostToDevice));
	const uint64_t outs = mdemod_fe_max_outputs(fe, most);
	rc = fe_grow_bb(fe, outs, st);
	if (rc) return rc;
	rc = fe_launch(fe, fe->d_in ? fe->d_in : fe->d_bb, fe->d_in_off, fe->d_in_cnt, fe->d_bb, fe->bb_stride, static_cast<uint32_t>(outs), fe->d_bb_cnt, st);
	if (rc) return rc;
	std::vector<uint32_t> cnt(ns);
	HIP_TRY(hipMemcpy(cnt.data(), fe->d_bb_cnt, ns * sizeof(uint32_t), hipMemcpyDeviceToHost));
	std::vector<float> bb(static_cast<size_t>(fe->bb_stride) * 2 * ns);
	std::vector<const void *> rows(ns);
	for (uint32_t s = 0; s < ns; s++) {
		float *row = bb.data() + static_cast<size_t>(s) * fe->bb_stride * 2;
		if (cnt[s]) HIP_TRY(hipMemcpy(row, fe->d_bb + static_cast<size_t>(s) * fe->bb_stride, cnt[s] * sizeof(float2), hipMemcpyDeviceToHost));
		rows[s] = row;
	}
	return mdemod_process_host(fe->inner, rows.data(), cnt.data(), soft_host, soft_cap, n_symbols);
} MDEMOD_API_CATCH

int
mdemod_fe_demodulate_recording_host(const mdemod_params *input, const mdemod_fe_params *fe_params, const mdemod_recording_opts *opts,
                                    const void *iq_host, uint64_t n_samples, int8_t *soft_host, uint64_t soft_cap_symbols,
                                    mdemod_recording_report *report)
try { MDEMOD_API_ENTER
	if (!input || !fe_params || !opts || (!iq_host && n_samples) || !soft_host || !report) { mdm_note_error("mdemod_fe_demodulate_recording_host: a pointer is NULL"); return MDEMOD_ERR_PARAM; }
	mdemod_params one = *input;
	one.n_streams = 1;
	mdemod_fe_params fp = *fe_params;
	fp.offsets_hz = nullptr;
	mdemod_fe *fe = nullptr;
	int rc = fe_create(&one, &fp, false, &fe);
	if (rc) return rc;
	/* (the buffers below live in the front end's own list: they go with it, on every way out) */
	const std::unique_ptr<mdemod_fe, decltype(&mdemod_fe_destroy)> owner(fe, mdemod_fe_destroy);
	const size_t sb = 2 * static_cast<size_t>(input->bps) / 8;
	const uint64_t n_bb = mdemod_fe_max_outputs(fe, n_samples);
	/* the input in pieces of 2^26 samples (one device buffer, reused), the baseband of the whole recording in one */
	const uint64_t piece = n_samples < (1ull << 26) ? (n_samples ? n_samples : 1) : (1ull << 26);
	unsigned char *d_in = nullptr;
	float2 *d_bb = nullptr;
	int8_t *d_soft = nullptr;
	if ((rc = fe->mem.alloc(&d_in, piece * sb)) || (rc = fe->mem.alloc(&d_bb, n_bb)) || (rc = fe->mem.alloc(&d_soft, soft_cap_symbols * 2)))
		return rc;
	hipStream_t st = nullptr;
	uint64_t done = 0, produced = 0;
	while (done < n_samples) {
		const uint32_t n = static_cast<uint32_t>(n_samples - done < piece ? n_samples - done : piece);
		HIP_TRY(hipMemcpy(d_in, static_cast<const unsigned char *>(iq_host) + done * sb, n * sb, hipMemcpyHostToDevice));
		const uint64_t zero = 0;
		HIP_TRY(hipMemcpy(fe->d_in_off, &zero, sizeof(zero), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(fe->d_in_cnt, &n, sizeof(n), hipMemcpyHostToDevice));
		const uint64_t outs = mdemod_fe_max_outputs(fe, n);
		rc = fe_launch(fe, d_in, fe->d_in_off, fe->d_in_cnt, d_bb + produced, outs, static_cast<uint32_t>(outs), fe->d_bb_cnt, st);
		if (rc) return rc;
		uint32_t got = 0;
		HIP_TRY(hipMemcpy(&got, fe->d_bb_cnt, sizeof(got), hipMemcpyDeviceToHost));
		produced += got;
		done += n;
	}
	mdemod_params ip = one;
	ip.samplerate = fe->design.samplerate_out;
	ip.bps = 32;
	rc = mdemod_demodulate_recording(&ip, opts, d_bb, produced, d_soft, soft_cap_symbols, report, nullptr);
	if (rc) return rc;
	HIP_TRY(hipMemcpy(soft_host, d_soft, report->n_symbols * 2, hipMemcpyDeviceToHost));
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
