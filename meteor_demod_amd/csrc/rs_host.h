/*
 * rs_host.h — host side of the transfer-frame layer (include/meteor_demod_amd_rs.h): the tables of the field, the randomiser and
 * the dual basis (derived here, at compile time, for the host model and the kernel alike), the option check and the host model of
 * the kernel.  Free of the GPU runtime (the CPU fuzz test builds csrc/rs_host.cpp with gcc's sanitizers).
 */
#ifndef MDEMOD_RS_HOST_H
#define MDEMOD_RS_HOST_H

#include "../../include/meteor_demod_amd_rs.h"

#define RS_N        255               /* bytes of a codeword */
#define RS_K        223               /* of them data */
#define RS_ROOTS    32                /* parity bytes = roots of the generator = syndromes */
#define RS_T        16
#define RS_DEPTH    4                 /* interleaved codewords of a frame */
#define RS_POLY     0x187u
#define RS_FCR      112               /* the roots are beta^(RS_FCR + k), k = 0 .. 31, with */
#define RS_PRIM     11                /* beta = alpha^RS_PRIM */
#define RS_CODED    (RS_N * RS_DEPTH) /* 1020 bytes after the marker */

#ifdef __cplusplus

/* the shift-and-xor product: the definition of the field (the tables below are derived from it) */
constexpr uint8_t
rs_gf_mul(uint8_t a, uint8_t b)
{
	uint32_t acc = 0, x = a;
	for (int i = 0; i < 8; i++) {
		if (b & (1u << i)) acc ^= x;
		x <<= 1;
		if (x & 0x100u) x ^= RS_POLY;
	}
	return static_cast<uint8_t>(acc);
}

struct alignas(16) RsTables {
	uint8_t exp[512];                 /* alpha^i for i < 510 (the period is 255: a sum of two logarithms needs no reduction) */
	uint8_t log[256];                 /* log[alpha^i] = i for i < 255; log[0] is 0 and never used */
	uint8_t pn[RS_CODED];             /* the randomiser's sequence over a whole frame: four periods of 255 */
	uint8_t T[256], Tinv[256];        /* the dual basis: T after decoding, Tinv before */
	uint8_t gen[RS_ROOTS + 1];        /* the generator, x^0 .. x^32 */
};

constexpr RsTables
rs_make_tables()
{
	RsTables t{};
	uint8_t x = 1;
	for (int i = 0; i < 255; i++) {
		t.exp[i] = x; t.exp[i + 255] = x;
		t.log[x] = static_cast<uint8_t>(i);
		x = rs_gf_mul(x, 2);
	}
	t.exp[510] = t.exp[0]; t.exp[511] = t.exp[1];
	uint32_t reg = 0xFFu;
	for (int i = 0; i < 255; i++) {
		uint32_t byte = 0;
		for (int b = 0; b < 8; b++) {
			byte = (byte << 1) | (reg >> 7);
			const uint32_t fb = ((reg >> 7) ^ (reg >> 4) ^ (reg >> 2) ^ reg) & 1u;
			reg = ((reg << 1) | fb) & 0xFFu;
		}
		for (int p = 0; p < RS_DEPTH; p++) t.pn[i + 255 * p] = static_cast<uint8_t>(byte);
	}
	const uint8_t tal[8] = { 0x8d, 0xef, 0xec, 0x86, 0xfa, 0x99, 0xaf, 0x7b };
	for (int i = 0; i < 256; i++) {
		uint8_t v = 0;
		for (int j = 0; j < 8; j++)
			if (i & (1 << j)) v ^= tal[7 - j];
		t.T[i] = v;
	}
	for (int i = 0; i < 256; i++) t.Tinv[t.T[i]] = static_cast<uint8_t>(i);
	/* g(x) = prod (x - beta^(112 + k)) */
	t.gen[0] = 1;
	for (int k = 0; k < RS_ROOTS; k++) {
		const uint8_t root = t.exp[(RS_PRIM * (RS_FCR + k)) % 255];
		for (int j = k + 1; j > 0; j--) t.gen[j] = static_cast<uint8_t>(t.gen[j - 1] ^ rs_gf_mul(t.gen[j], root));
		t.gen[0] = rs_gf_mul(t.gen[0], root);
	}
	return t;
}

/* opts (NULL = defaults) checked: MDEMOD_OK or MDEMOD_ERR_PARAM with the text noted; piece_frames 0 becomes 8192 */
int  rs_settings(const mdemod_rs_opts *opts, mdemod_rs_opts &out);

extern "C" {
#endif

/* ---- the host model: what the kernel of csrc/rs.hip must compute, byte for byte (exported for the tests) ---- */

/* pn[255] := one period of the randomiser's sequence */
void mdemod_rs_model_pn(uint8_t *pn);
/* gen[33] := the generator's coefficients, x^0 first */
void mdemod_rs_model_generator(uint8_t *gen);
/* T[256], Tinv[256] := the dual-basis tables */
void mdemod_rs_model_dual(uint8_t *T, uint8_t *Tinv);
/* parity[32] := the parity of data[223] (conventional representation) */
void mdemod_rs_model_parity(const uint8_t *data, uint8_t *parity);
/* vcdu[892] into cadu[1024]: the marker, the four parities, the interleave, and per options the dual basis and the randomiser */
int  mdemod_rs_model_encode(const mdemod_rs_opts *opts, const uint8_t *vcdu, uint8_t *cadu);
/* cadu[n][1024] into vcdu[n][892] and info[n] */
int  mdemod_rs_model_decode(const mdemod_rs_opts *opts, const uint8_t *cadu, uint64_t n, uint8_t *vcdu, mdemod_rs_info *info);

#ifdef __cplusplus
}
#endif
#endif
