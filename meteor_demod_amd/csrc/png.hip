/*
 * png.hip — the PNG encoder on the GPU (include/meteor_demod_amd_png.h): png_filter, png_deflate, png_offsets, png_place, and the
 * public entries around them.  The specification is the host model of csrc/png_host.cpp; the filters, the parse, the code lengths and
 * the header of a block are the model's own functions (csrc/png_host.h).
 *
 * png_filter: one block of 256 threads per row, in tiles of 1024 pixels.  A tile of the row and of the row above comes into LDS with
 *   the pixel to its left, neighbouring lanes taking neighbouring pixels, the mask already as the alpha byte behind the planes; a
 *   filtered byte is then four LDS reads.  Filter 5 sums the five costs over the row first (a shuffle reduction per wave, five LDS
 *   adds per wave), chooses, and goes over the tiles again (a row of one tile stays in LDS).  The filtered stream goes to the workspace.
 * png_deflate: one block of 256 threads per segment, the segment in LDS.  A thread owns 128 consecutive bytes of a 32 KiB segment (its part stands at
 *   a pitch of chunk + 4 bytes, an odd number of words, so that the lanes of a wave read different banks).  The last run start at or
 *   before a part (a max scan) and the first at or after it (a min scan from the right) give every thread the run it enters in and
 *   the end of the run it leaves in; png_token then says what stands at each of its places.  Three walks over the part: the counts
 *   (LDS adds) and the Adler sums; the bits, whose scan gives the part's bit offset; the packing into the LDS image of the chunk by
 *   ds_or, bits gathering in a 64-bit register.  Between them the code: the leaves' order by counting (a thread per symbol), the tree
 *   and its limit by thread 0 (png_code_lengths, the model's function), the canonical codes a thread per symbol, the run-length coding
 *   of the lengths and the code-length code by thread 0.  The chunk's CRC-32: a thread takes a slice with a register of 0, multiplies
 *   by x^(8 n) for the n bytes behind its slice, and the products are XORed.  The chunk leaves as whole words into the segment's
 *   slot of the workspace.
 *   LDS: the segment at its pitch (33 792 bytes for 32 KiB), the image (32 KiB + 32), 10 KiB of tables: 75 KiB, two blocks a CU.
 * png_offsets: one block runs the encoders' offset scan (csrc/encoder_device.h) over the lengths: the total, whether it fits; it sums
 *   the segments' Adler parts and stores the file's head, the Adler chunk and IEND.  No global atomics anywhere.
 * png_place: a block per segment copies the chunk from its slot to its offset.
 * The check of the entries' pointers, mdemod_png_result and the host entry's download are the JPEG encoder's too (csrc/encoder_device.h).
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "png_host.h"
#include "encoder_device.h"

#define PF_THREADS 256
#define PF_TILE    1024                           /* pixels of a tile */
#define PD_THREADS 256
#define PP_THREADS 256

__device__ const PngCrcTable PNG_CRC_DEV = png_make_crc();
__device__ const PngCrcPowers PNG_POW_DEV = png_make_powers();
constexpr uint32_t PNG_IDAT_REGISTER = png_idat_register();

/* ---- filter ---- */
struct PngFilter {
	const uint8_t *picture, *valid;
	uint8_t *filtered;
	uint32_t width, height, filter;
};

template <int PLANES, bool MASK>
__global__ void __launch_bounds__(PF_THREADS)
png_filter(PngFilter a)
{
	constexpr uint32_t CH = PLANES + (MASK ? 1 : 0);
	__shared__ uint8_t cur[(PF_TILE + 1) * CH], prv[(PF_TILE + 1) * CH];
	__shared__ uint32_t sums[5];
	const uint32_t y = blockIdx.x, tid = threadIdx.x;
	const size_t row = static_cast<size_t>(y) * a.width;
	uint8_t *to = a.filtered + static_cast<size_t>(y) * (1u + a.width * CH);
	const uint32_t n_tiles = (a.width + PF_TILE - 1) / PF_TILE;
	if (tid < 5) sums[tid] = 0;
	/* the pixels x0 - 1 .. x0 + n - 1 of this row and the one above into the places 0 .. n; what is outside the picture is 0 */
	auto load = [&](uint32_t x0, uint32_t n) {
		for (uint32_t j = tid; j <= n; j += PF_THREADS) {
			const bool in = x0 + j > 0;
			const size_t x = row + x0 + j - 1;                                       /* (used only when `in`) */
#pragma unroll
			for (uint32_t c = 0; c < CH; c++) {
				uint32_t vc = 0, vp = 0;
				if (in) {
					if (c < PLANES) {
						vc = a.picture[x * PLANES + c];
						if (y) vp = a.picture[(x - a.width) * PLANES + c];
					} else {
						vc = a.valid[x] ? 255u : 0u;
						if (y) vp = a.valid[x - a.width] ? 255u : 0u;
					}
				}
				cur[j * CH + c] = static_cast<uint8_t>(vc);
				prv[j * CH + c] = static_cast<uint8_t>(vp);
			}
		}
	};
	uint32_t f = a.filter;
	const bool adapt = f == MDEMOD_PNG_FILTER_ADAPT;
	if (adapt) {
		uint32_t s[5] = { 0, 0, 0, 0, 0 };
		for (uint32_t t = 0; t < n_tiles; t++) {
			const uint32_t x0 = t * PF_TILE, n = min(static_cast<uint32_t>(PF_TILE), a.width - x0);
			__syncthreads();
			load(x0, n);
			__syncthreads();
			for (uint32_t o = tid; o < n * CH; o += PF_THREADS) {
				const uint32_t x = cur[CH + o], l = cur[o], u = prv[CH + o], ul = prv[o];
#pragma unroll
				for (uint32_t g = 0; g < 5; g++) s[g] += png_cost(png_filter_byte(g, x, l, u, ul));
			}
		}
#pragma unroll
		for (uint32_t g = 0; g < 5; g++) {
			uint32_t v = s[g];
			for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
			if ((tid & 63u) == 0) atomicAdd(&sums[g], v);
		}
		__syncthreads();
		uint32_t all[5];
#pragma unroll
		for (uint32_t g = 0; g < 5; g++) all[g] = sums[g];
		f = png_choose(all);
	}
	for (uint32_t t = 0; t < n_tiles; t++) {
		const uint32_t x0 = t * PF_TILE, n = min(static_cast<uint32_t>(PF_TILE), a.width - x0);
		if (!adapt || n_tiles > 1) {
			__syncthreads();
			load(x0, n);
			__syncthreads();
		}
		uint8_t *out = to + 1 + static_cast<size_t>(x0) * CH;
		for (uint32_t o = tid; o < n * CH; o += PF_THREADS) out[o] = static_cast<uint8_t>(png_filter_byte(f, cur[CH + o], cur[o], prv[CH + o], prv[o]));
	}
	if (tid == 0) to[0] = static_cast<uint8_t>(f);
}

/* ---- deflate ---- */
struct PngDeflate {
	const uint8_t *bytes;                         /* at a multiple of 4 bytes */
	uint64_t n_bytes;
	uint8_t *slots;                               /* [n_seg][slot_bytes] */
	uint32_t *seg_len;                            /* [n_seg] */
	uint32_t *adler;                              /* [n_seg][2]: the sum of the bytes, and what the segment adds to the second sum */
	uint32_t seg_bytes, slot_bytes, n_seg, chunk; /* chunk: bytes of a thread, a multiple of 8 */
};

/* bits from bit `pos` of the image on; a word of the image holds its first bit lowest */
struct PngPack {
	uint32_t *img;
	uint64_t acc;
	uint32_t fill, w;
	__device__ __forceinline__ void open(uint32_t *image, uint32_t pos) { img = image; acc = 0; fill = pos & 31u; w = pos >> 5; }
	__device__ __forceinline__ void put(uint32_t bits, uint32_t count)
	{
		acc |= static_cast<uint64_t>(bits) << fill;
		fill += count;
		if (fill >= 32u) {
			atomicOr(img + w, static_cast<uint32_t>(acc));
			w++;
			acc >>= 32;
			fill -= 32u;
		}
	}
	__device__ __forceinline__ void close() { if (fill) atomicOr(img + w, static_cast<uint32_t>(acc)); }
};

/* an inclusive scan over the block's threads in the order of idx; every thread calls it */
template <class Op>
__device__ __forceinline__ uint32_t
png_block_scan(uint32_t *buf, uint32_t idx, uint32_t v, uint32_t identity, Op op)
{
	buf[idx] = v;
	__syncthreads();
	for (uint32_t d = 1; d < PD_THREADS; d <<= 1) {
		const uint32_t o = idx >= d ? buf[idx - d] : identity;
		__syncthreads();
		buf[idx] = op(buf[idx], o);
		__syncthreads();
	}
	return buf[idx];
}

/* f(byte, token) for every token that begins in the thread's part [lo, hi): mine holds its bytes, `start` is where the run at lo
 * began and `end_after` where the run that reaches hi ends */
template <class F>
__device__ __forceinline__ void
png_walk(const uint8_t *mine, uint32_t lo, uint32_t hi, uint32_t start, uint32_t end_after, F &&f)
{
	uint32_t p = lo, s = start;
	while (p < hi) {
		const uint32_t v = mine[p - lo];
		uint32_t q = p + 1;
		while (q < hi && mine[q - lo] == v) q++;
		const uint32_t L = (q < hi ? q : end_after) - s;
		for (uint32_t x = p; x < q; x++) {
			const uint32_t t = png_token(x - s, L);
			if (t) f(v, t);
		}
		p = q;
		s = q;
	}
}

/* r x^(8 n) */
__device__ __forceinline__ uint32_t
png_crc_shift(uint32_t r, uint32_t n, const uint32_t *powers)
{
	for (uint32_t k = 0; n; k++, n >>= 1)
		if (n & 1u) r = png_gf_mul(r, powers[k]);
	return r;
}

__global__ void __launch_bounds__(PD_THREADS)
png_deflate(PngDeflate a)
{
	extern __shared__ uint32_t lds[];             /* the segment at its pitch, then the image of the chunk */
	__shared__ uint32_t count[PNG_LL_ROOM], w[2 * PNG_LL_ROOM], num[16], clcount[PNG_CL], crc_tab[256], powers[32], scan_a[PD_THREADS], scan_b[PD_THREADS];
	__shared__ uint16_t code[PNG_LL_ROOM], order[PNG_LL_ROOM], up[2 * PNG_LL_ROOM], tok[PNG_LL_ROOM], clcode[PNG_CL + 1], clorder[PNG_CL + 1];
	__shared__ uint8_t len[PNG_LL_ROOM + 4], cllen[PNG_CL + 1];
	__shared__ uint32_t n_leaves, n_cl, hlit_s, n_tok_s, hbits_s, crc_s, adler_a, adler_b;

	const uint32_t tid = threadIdx.x, seg = blockIdx.x;
	const uint64_t at = static_cast<uint64_t>(seg) * a.seg_bytes;
	const uint32_t n = a.n_bytes - at < a.seg_bytes ? static_cast<uint32_t>(a.n_bytes - at) : a.seg_bytes;
	const bool last = seg + 1 == a.n_seg;
	const uint32_t c = a.chunk, pitch = c + 4;
	uint8_t *segb = reinterpret_cast<uint8_t *>(lds);
	uint32_t *image = lds + PD_THREADS * pitch / 4;
	uint8_t *imgb = reinterpret_cast<uint8_t *>(image);
	const uint32_t image_words = (a.seg_bytes + 32) / 4;

	/* the segment in, the tables cleared */
	const uint8_t *src = a.bytes + at;
	for (uint32_t g = tid; g < n / 4; g += PD_THREADS) {
		const uint32_t p = 4 * g;
		*reinterpret_cast<uint32_t *>(segb + p + 4 * (p / c)) = reinterpret_cast<const uint32_t *>(src)[g];
	}
	for (uint32_t p = (n & ~3u) + tid; p < n; p += PD_THREADS) segb[p + 4 * (p / c)] = src[p];
	for (uint32_t i = tid; i < image_words; i += PD_THREADS) image[i] = 0;
	for (uint32_t i = tid; i < PNG_LL_ROOM; i += PD_THREADS) { count[i] = 0; len[i] = 0; }
	crc_tab[tid] = PNG_CRC_DEV.t[tid];
	if (tid < 32) powers[tid] = PNG_POW_DEV.p[tid];
	if (tid < PNG_CL) { clcount[tid] = 0; cllen[tid] = 0; }
	if (tid == 0) { n_leaves = 0; n_cl = 0; crc_s = 0; adler_a = 0; adler_b = 0; }
	__syncthreads();

	/* the thread's part, the run it enters in and the end of the run it leaves in */
	const uint32_t lo = min(tid * c, n), hi = min(lo + c, n);
	const uint8_t *mine = segb + tid * pitch;
	const bool live = lo < hi;
	uint32_t first_brk = 0xFFFFFFFFu, last_brk = 0;                                  /* (the last one + 1; 0: none) */
	bool brk_lo = false;
	if (live) {
		brk_lo = lo == 0 || mine[0] != segb[(lo - 1) + 4 * ((lo - 1) / c)];
		if (brk_lo) { first_brk = lo; last_brk = lo + 1; }
		for (uint32_t p = lo + 1; p < hi; p++)
			if (mine[p - lo] != mine[p - lo - 1]) {
				if (first_brk == 0xFFFFFFFFu) first_brk = p;
				last_brk = p + 1;
			}
	}
	png_block_scan(scan_a, tid, last_brk, 0u, [](uint32_t x, uint32_t y) { return max(x, y); });
	png_block_scan(scan_b, PD_THREADS - 1 - tid, first_brk, 0xFFFFFFFFu, [](uint32_t x, uint32_t y) { return min(x, y); });
	uint32_t start = lo, end_after = n;
	if (live) {
		if (!brk_lo) start = scan_a[tid - 1] - 1;                                    /* (tid > 0, and place 0 begins a run) */
		if (tid + 1 < PD_THREADS) end_after = min(scan_b[PD_THREADS - 2 - tid], n);
	}

	/* the counts and the Adler sums */
	if (live) {
		png_walk(mine, lo, hi, start, end_after, [&](uint32_t byte, uint32_t t) {
			uint32_t eb, ev;
			atomicAdd(&count[t == 1 ? byte : 257 + png_length_symbol(t, &eb, &ev)], 1u);
		});
		uint32_t sa = 0, sb = 0;
		for (uint32_t p = lo; p < hi; p++) { const uint32_t v = mine[p - lo]; sa += v; sb += (hi - p) * v; }
		atomicAdd(&adler_a, sa);
		atomicAdd(&adler_b, (sb + (n - hi) * sa) % PNG_ADLER);
	}
	if (tid == 0) atomicAdd(&count[PNG_EOB], 1u);
	__syncthreads();

	/* the leaves in order */
	for (uint32_t s = tid; s < PNG_LL; s += PD_THREADS)
		if (count[s]) {
			uint32_t rank = 0;
			for (uint32_t j = 0; j < PNG_LL; j++) rank += count[j] && png_before(count, j, s);
			order[rank] = static_cast<uint16_t>(s);
			atomicAdd(&n_leaves, 1u);
		}
	__syncthreads();
	if (tid == 0) png_code_lengths(count, order, n_leaves, 15, len, w, up, num);
	__syncthreads();
	for (uint32_t s = tid; s < PNG_LL; s += PD_THREADS) code[s] = static_cast<uint16_t>(png_code_of(len, PNG_LL, s));

	/* the bits of the part's tokens, and where they begin */
	uint32_t bits = 0;
	if (live) png_walk(mine, lo, hi, start, end_after, [&](uint32_t byte, uint32_t t) { bits += png_token_bits(byte, t, len); });
	const uint32_t incl = png_block_scan(scan_a, tid, bits, 0u, [](uint32_t x, uint32_t y) { return x + y; });
	const uint32_t data_bits = scan_a[PD_THREADS - 1];

	/* the lengths as a sequence, and its code */
	if (tid == 0) {
		uint32_t hlit = PNG_LL;
		while (hlit > 257 && !len[hlit - 1]) hlit--;
		len[hlit] = 1;                                                               /* the distance code */
		hlit_s = hlit;
		n_tok_s = png_rle(len, hlit + 1, tok, clcount);
	}
	__syncthreads();
	if (tid < PNG_CL && clcount[tid]) {
		uint32_t rank = 0;
		for (uint32_t j = 0; j < PNG_CL; j++) rank += clcount[j] && png_before(clcount, j, tid);
		clorder[rank] = static_cast<uint16_t>(tid);
		atomicAdd(&n_cl, 1u);
	}
	__syncthreads();
	if (tid == 0) png_code_lengths(clcount, clorder, n_cl, 7, cllen, w, up, num);
	__syncthreads();
	if (tid < PNG_CL) clcode[tid] = static_cast<uint16_t>(png_code_of(cllen, PNG_CL, tid));
	if (tid == 0) hbits_s = png_header_bits(tok, n_tok_s, cllen);
	__syncthreads();

	/* dynamic or stored; the payload into the image behind the chunk's length and type */
	const uint32_t hbits = hbits_s, total_bits = hbits + data_bits + len[PNG_EOB] + 3u;
	const uint32_t dynamic = (total_bits + 7u) / 8u + 4u;
	const bool stored = dynamic > n + 5u;
	const uint32_t payload = stored ? n + 5u : dynamic;
	if (stored) {
		for (uint32_t p = lo; p < hi; p++) imgb[13 + p] = mine[p - lo];
	} else {
		if (live) {
			PngPack pack;
			pack.open(image, 64u + hbits + incl - bits);
			png_walk(mine, lo, hi, start, end_after, [&](uint32_t byte, uint32_t t) { png_put_token(pack, byte, t, len, code); });
			pack.close();
		}
		if (tid == 0) {
			PngPack pack;
			pack.open(image, 64u);
			png_put_header(pack, hlit_s, tok, n_tok_s, cllen, clcode);
			pack.close();
			pack.open(image, 64u + hbits + data_bits);
			pack.put(code[PNG_EOB], len[PNG_EOB]);
			pack.put(last ? 1u : 0u, 3);                                             /* the empty stored block */
			pack.close();
		}
	}
	__syncthreads();
	if (tid == 0) {
		imgb[0] = static_cast<uint8_t>(payload >> 24); imgb[1] = static_cast<uint8_t>(payload >> 16);
		imgb[2] = static_cast<uint8_t>(payload >> 8); imgb[3] = static_cast<uint8_t>(payload);
		imgb[4] = 'I'; imgb[5] = 'D'; imgb[6] = 'A'; imgb[7] = 'T';
		if (stored) {
			imgb[8] = last ? 1 : 0;
			imgb[9] = static_cast<uint8_t>(n & 255u); imgb[10] = static_cast<uint8_t>(n >> 8);
			imgb[11] = static_cast<uint8_t>(~n & 255u); imgb[12] = static_cast<uint8_t>((~n >> 8) & 255u);
		} else {
			imgb[8 + payload - 2] = 0xFF; imgb[8 + payload - 1] = 0xFF;             /* (the two 00 before them are there) */
		}
	}
	__syncthreads();

	/* the CRC of the type and the payload: a slice per thread */
	{
		const uint32_t k = (payload + PD_THREADS - 1) / PD_THREADS, from = min(tid * k, payload), to = min(from + k, payload);
		uint32_t r = 0;
		for (uint32_t p = from; p < to; p++) r = crc_tab[(r ^ imgb[8 + p]) & 255u] ^ (r >> 8);
		if (from < to) r = png_crc_shift(r, payload - to, powers);
		if (tid == 0) r ^= png_crc_shift(PNG_IDAT_REGISTER, payload, powers);
		if (r) atomicXor(&crc_s, r);
	}
	__syncthreads();
	if (tid == 0) {
		const uint32_t crc = crc_s ^ 0xFFFFFFFFu;
		uint8_t *e = imgb + 8 + payload;
		e[0] = static_cast<uint8_t>(crc >> 24); e[1] = static_cast<uint8_t>(crc >> 16); e[2] = static_cast<uint8_t>(crc >> 8); e[3] = static_cast<uint8_t>(crc);
		a.seg_len[seg] = payload + 12u;
		a.adler[2 * seg] = adler_a % PNG_ADLER;
		const uint64_t behind = (a.n_bytes - (at + n)) % PNG_ADLER;
		a.adler[2 * seg + 1] = static_cast<uint32_t>((adler_b + behind * (adler_a % PNG_ADLER)) % PNG_ADLER);
	}
	__syncthreads();
	uint32_t *slot = reinterpret_cast<uint32_t *>(a.slots + static_cast<size_t>(seg) * a.slot_bytes);
	for (uint32_t i = tid; i < (payload + 12u + 3u) / 4u; i += PD_THREADS) slot[i] = image[i];
}

/* ---- offsets ---- */
struct PngEnds {
	uint32_t n;                                   /* bytes before the first segment; with them the file ends in the Adler chunk and IEND */
	uint8_t head[MDEMOD_PNG_HEAD + 1];
};

__global__ void __launch_bounds__(ENC_SCAN_THREADS)
png_offsets(const uint32_t *seg_len, const uint32_t *adler, uint64_t *seg_off, uint32_t n_seg, uint64_t n_bytes, uint8_t *out, uint64_t out_room, uint64_t *result,
            PngEnds ends)
{
	__shared__ uint32_t sum_a, sum_b;
	const uint32_t tid = threadIdx.x;
	if (tid == 0) { sum_a = 0; sum_b = 0; }
	const uint64_t total = enc_scan_offsets(seg_len, seg_off, n_seg, 0u, ends.n) + (ends.n ? MDEMOD_PNG_TAIL : 0u);
	const bool fits = total <= out_room;
	if (tid == 0) { seg_off[n_seg] = total; result[0] = total; result[1] = fits; }
	if (!fits || !ends.n) return;                                                 /* (uniform) */
	uint32_t my_a = 0, my_b = 0;
	for (uint32_t i = tid; i < n_seg; i += ENC_SCAN_THREADS) { my_a = (my_a + adler[2 * i]) % PNG_ADLER; my_b = (my_b + adler[2 * i + 1]) % PNG_ADLER; }
	__syncthreads();
	atomicAdd(&sum_a, my_a);
	atomicAdd(&sum_b, my_b);
	for (uint32_t i = tid; i < ends.n; i += ENC_SCAN_THREADS) out[i] = ends.head[i];
	__syncthreads();
	if (tid) return;
	const uint32_t s1 = (1u + sum_a) % PNG_ADLER, s2 = static_cast<uint32_t>((n_bytes % PNG_ADLER + sum_b) % PNG_ADLER);
	uint8_t t[MDEMOD_PNG_TAIL] = { 0, 0, 0, 4, 'I', 'D', 'A', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82 };
	t[8] = static_cast<uint8_t>(s2 >> 8); t[9] = static_cast<uint8_t>(s2); t[10] = static_cast<uint8_t>(s1 >> 8); t[11] = static_cast<uint8_t>(s1);
	uint32_t r = 0xFFFFFFFFu;
	for (int i = 4; i < 12; i++) {
		r ^= t[i];
		for (int k = 0; k < 8; k++) r = (r & 1u) ? (r >> 1) ^ PNG_POLY : r >> 1;
	}
	r ^= 0xFFFFFFFFu;
	t[12] = static_cast<uint8_t>(r >> 24); t[13] = static_cast<uint8_t>(r >> 16); t[14] = static_cast<uint8_t>(r >> 8); t[15] = static_cast<uint8_t>(r);
	for (int i = 0; i < MDEMOD_PNG_TAIL; i++) out[total - MDEMOD_PNG_TAIL + i] = t[i];
}

/* ---- place ---- */
__global__ void __launch_bounds__(PP_THREADS)
png_place(const uint8_t *slots, uint32_t slot_bytes, const uint32_t *seg_len, const uint64_t *seg_off, uint32_t n_seg, uint8_t *out, uint64_t out_room)
{
	if (seg_off[n_seg] > out_room) return;                                        /* (uniform) it does not fit: nothing is written */
	const uint32_t seg = blockIdx.x, n = seg_len[seg];
	const uint8_t *from = slots + static_cast<size_t>(seg) * slot_bytes;
	uint8_t *to = out + seg_off[seg];
	for (uint32_t i = threadIdx.x; i < n; i += PP_THREADS) to[i] = from[i];
}

namespace {

struct PngWork {
	uint8_t *filtered, *slots;
	uint64_t *seg_off;
	uint32_t *seg_len, *adler;
};

/* the workspace's parts: the filtered stream (when it holds one), the slots, the offsets, the lengths, the Adler sums */
PngWork
carve(void *work, uint64_t filtered_bytes, uint64_t n_seg, uint32_t slot_bytes)
{
	uint8_t *p = static_cast<uint8_t *>(work);
	PngWork w;
	w.filtered = p;
	p += (filtered_bytes + 15) & ~15ull;
	w.slots = p;
	p += (n_seg * slot_bytes + 7) & ~7ull;
	w.seg_off = reinterpret_cast<uint64_t *>(p);
	p += (n_seg + 1) * 8;
	w.seg_len = reinterpret_cast<uint32_t *>(p);
	p += n_seg * 4;
	w.adler = reinterpret_cast<uint32_t *>(p);
	return w;
}

int
filter_run(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint8_t *filtered, hipStream_t st)
{
	PngFilter a;
	memset(&a, 0, sizeof a);
	a.picture = picture; a.valid = valid; a.filtered = filtered; a.width = width; a.height = height; a.filter = filter;
	const dim3 grid(height), block(PF_THREADS);
	if (planes == 3 && valid) hipLaunchKernelGGL((png_filter<3, true>), grid, block, 0, st, a);
	else if (planes == 3) hipLaunchKernelGGL((png_filter<3, false>), grid, block, 0, st, a);
	else if (valid) hipLaunchKernelGGL((png_filter<1, true>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((png_filter<1, false>), grid, block, 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* the segments' chunks of bytes[n_bytes] to out; ends: the file's, or NULL for the chunks alone */
int
deflate_run(const uint8_t *bytes, uint64_t n_bytes, uint32_t seg_bytes, uint8_t *out, uint64_t out_room, uint64_t *result, const PngWork &w, const PngEnds *ends, hipStream_t st)
{
	PngDeflate a;
	memset(&a, 0, sizeof a);
	a.bytes = bytes; a.n_bytes = n_bytes; a.slots = w.slots; a.seg_len = w.seg_len; a.adler = w.adler;
	a.seg_bytes = seg_bytes; a.slot_bytes = png_slot_bytes(seg_bytes); a.n_seg = static_cast<uint32_t>(png_segments(n_bytes, seg_bytes));
	a.chunk = (seg_bytes / PD_THREADS + 7u) & ~7u;
	const size_t lds = static_cast<size_t>(PD_THREADS) * (a.chunk + 4) + seg_bytes + 32;
	HIP_TRY(mdm_launch(png_deflate, dim3(a.n_seg), dim3(PD_THREADS), lds, st, a));
	PngEnds none;
	memset(&none, 0, sizeof none);
	hipLaunchKernelGGL(png_offsets, dim3(1), dim3(ENC_SCAN_THREADS), 0, st, w.seg_len, w.adler, w.seg_off, a.n_seg, n_bytes, out, out_room, result, ends ? *ends : none);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(png_place, dim3(a.n_seg), dim3(PP_THREADS), 0, st, w.slots, a.slot_bytes, w.seg_len, w.seg_off, a.n_seg, out, out_room);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

int
encode_run(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment, uint8_t *out, uint64_t out_room,
           uint64_t *result, void *work, hipStream_t st)
{
	const uint32_t sb = png_segment_bytes(segment);
	const uint64_t n = png_filtered_bytes(width, height, png_channels(planes, valid != nullptr));
	const PngWork w = carve(work, n, png_segments(n, sb), png_slot_bytes(sb));
	PngEnds ends;
	memset(&ends, 0, sizeof ends);
	ends.n = MDEMOD_PNG_HEAD;
	png_head(width, height, planes, valid != nullptr, ends.head);
	const int rc = filter_run(picture, valid, width, height, planes, filter, w.filtered, st);
	if (rc) return rc;
	return deflate_run(w.filtered, n, sb, out, out_room, result, w, &ends, st);
}

} /* namespace */

extern "C" {

int
mdemod_png_encode_device(const uint8_t *picture_dev, const uint8_t *valid_dev, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment,
                         uint8_t *out_dev, uint64_t out_room, uint64_t *result_dev, void *work_dev, uint64_t work_bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_png_encode_device";
	int rc = png_check_picture(who, width, height, planes, filter, segment);
	if (rc) return rc;
	const uint64_t area = static_cast<uint64_t>(width) * height;
	if ((rc = enc_check_buffers(who, "bytes", picture_dev, area * planes, 1, valid_dev, area, out_dev, out_room, result_dev, work_dev, work_bytes,
	                            mdemod_png_workspace(width, height, planes, valid_dev != nullptr, segment))))
		return rc;
	if ((rc = mdm_select_device(device))) return rc;
	return encode_run(picture_dev, valid_dev, width, height, planes, filter, segment, out_dev, out_room, result_dev, work_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_png_deflate_device(const uint8_t *bytes_dev, uint64_t n_bytes, uint32_t segment, uint8_t *out_dev, uint64_t out_room, uint64_t *result_dev, void *work_dev,
                          uint64_t work_bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_png_deflate_device";
	int rc = png_check_bytes(who, n_bytes, segment);
	if (rc) return rc;
	if ((rc = enc_check_buffers(who, "bytes", bytes_dev, n_bytes, 16, nullptr, 0, out_dev, out_room, result_dev, work_dev, work_bytes, mdemod_png_deflate_workspace(n_bytes, segment))))
		return rc;
	if ((rc = mdm_select_device(device))) return rc;
	const uint32_t sb = png_segment_bytes(segment);
	const PngWork w = carve(work_dev, 0, png_segments(n_bytes, sb), png_slot_bytes(sb));
	return deflate_run(bytes_dev, n_bytes, sb, out_dev, out_room, result_dev, w, nullptr, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_png_result(const uint64_t *result_dev, uint64_t *bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	return enc_result("mdemod_png_result", result_dev, bytes, device, hip_stream);
} MDEMOD_API_CATCH

int
mdemod_png_encode_host(const uint8_t *picture, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t filter, uint32_t segment, uint8_t **file,
                       uint64_t *bytes, int device)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_png_encode_host";
	int rc = png_check_picture(who, width, height, planes, filter, segment);
	if (rc) return rc;
	if (!picture || !file || !bytes) REFUSE("%s: the picture, file and bytes are needed", who);
	*file = nullptr; *bytes = 0;
	if ((rc = mdm_select_device(device))) return rc;
	const uint64_t area = static_cast<uint64_t>(width) * height, room = mdemod_png_bound(width, height, planes, valid != nullptr, segment);
	MdmDevMem mem;
	uint8_t *d_picture = nullptr, *d_valid = nullptr, *d_work = nullptr, *d_out = nullptr;
	uint64_t *d_result = nullptr;
	if ((rc = mem.alloc(&d_picture, area * planes)) || (rc = mem.alloc(&d_work, mdemod_png_workspace(width, height, planes, valid != nullptr, segment))) ||
	    (rc = mem.alloc(&d_out, room)) || (rc = mem.alloc(&d_result, 2)))
		return rc;
	HIP_TRY(hipMemcpyAsync(d_picture, picture, area * planes, hipMemcpyHostToDevice, nullptr));
	if (valid) {
		if ((rc = mem.alloc(&d_valid, area))) return rc;
		HIP_TRY(hipMemcpyAsync(d_valid, valid, area, hipMemcpyHostToDevice, nullptr));
	}
	if ((rc = encode_run(d_picture, d_valid, width, height, planes, filter, segment, d_out, room, d_result, d_work, nullptr))) return rc;
	uint64_t r[2] = { 0, 0 };
	HIP_TRY(hipMemcpyAsync(r, d_result, sizeof r, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	if (!r[1]) { mdm_note_error("%s: the file of %llu bytes passed its bound of %llu", who, static_cast<unsigned long long>(r[0]), static_cast<unsigned long long>(room)); return MDEMOD_ERR_OVERFLOW; }
	return enc_download(who, d_out, r[0], file, bytes);
} MDEMOD_API_CATCH

} /* extern "C" */
