/*
 * rs_host.cpp — host side of the transfer-frame layer (include/meteor_demod_amd_rs.h): the option check, the header fields, and
 * the host model of the kernel of csrc/rs.hip (mdemod_rs_model_*: the kernel's specification, written for reading, one core, no
 * tricks).  Free of the GPU runtime.
 */
#include <cstring>

#include "rs_host.h"
#include "mdemod_internal_api.h"

namespace {

constexpr RsTables TAB = rs_make_tables();
const uint8_t MARKER[4] = { 0x1A, 0xCF, 0xFC, 0x1D };

inline uint8_t mul(uint8_t a, uint8_t b) { return rs_gf_mul(a, b); }
/* alpha^e for any e >= 0 */
inline uint8_t alpha_pow(uint32_t e) { return TAB.exp[e % 255u]; }
inline uint8_t inverse(uint8_t a) { return TAB.exp[(255u - TAB.log[a]) % 255u]; }          /* a != 0 */

/* the parity of data[223]: the remainder of data(x) x^32 by the generator, reg[0] the coefficient of x^31 */
void
parity_of(const uint8_t *data, uint8_t *reg)
{
	memset(reg, 0, RS_ROOTS);
	for (int i = 0; i < RS_K; i++) {
		const uint8_t fb = data[i] ^ reg[0];
		for (int j = 0; j < RS_ROOTS - 1; j++) reg[j] = reg[j + 1] ^ mul(fb, TAB.gen[RS_ROOTS - 1 - j]);
		reg[RS_ROOTS - 1] = mul(fb, TAB.gen[0]);
	}
}

/* One word w[0 .. 254], w[0] the coefficient of x^254.  Returns the number of bytes changed (0 .. 16), or 255 with w untouched.
 *
 * With X_i = beta^(254 - i) the locator number of position i, an error pattern e has the syndromes S_k = sum e_i X_i^(112 + k).
 * Berlekamp-Massey finds the shortest recurrence Lambda (length L) that generates S_0 .. S_31.  The word is within 16 of a codeword
 * exactly when L <= 16 and Lambda has L roots among the 255 inverse locator numbers (the argument); then the roots name
 * the positions and Forney's formula e_i = X_i^(1 - 112) Omega(1 / X_i) / Lambda'(1 / X_i) the values, Omega = S Lambda mod x^32. */
uint32_t
decode_word(uint8_t *w)
{
	uint8_t S[RS_ROOTS];
	bool clean = true;
	for (int k = 0; k < RS_ROOTS; k++) {
		const uint8_t x = alpha_pow(RS_PRIM * (RS_FCR + k));
		uint8_t acc = 0;
		for (int i = 0; i < RS_N; i++) acc = mul(acc, x) ^ w[i];               /* Horner: w(x) */
		S[k] = acc;
		clean = clean && acc == 0;
	}
	if (clean) return 0;

	/* Berlekamp-Massey: C the recurrence so far, B the one before the last change of length (times x^m, by a shift per step) */
	uint8_t C[RS_ROOTS + 2] = { 1 }, B[RS_ROOTS + 2] = { 1 }, T[RS_ROOTS + 2];
	uint32_t L = 0;
	uint8_t b = 1;
	for (uint32_t n = 0; n < RS_ROOTS; n++) {
		for (int j = RS_ROOTS + 1; j > 0; j--) B[j] = B[j - 1];
		B[0] = 0;
		uint8_t d = 0;
		for (uint32_t j = 0; j <= L && j <= n; j++) d ^= mul(C[j], S[n - j]);
		if (d == 0) continue;
		const uint8_t f = mul(d, inverse(b));
		memcpy(T, C, sizeof T);
		for (int j = 0; j < RS_ROOTS + 2; j++) C[j] ^= mul(f, B[j]);
		if (2 * L <= n) { L = n + 1 - L; memcpy(B, T, sizeof B); b = d; }
	}
	if (L > RS_T) return MDEMOD_RS_FAILED;

	uint8_t omega[RS_T] = { 0 };
	for (uint32_t k = 0; k < RS_T; k++)
		for (uint32_t j = 0; j <= k && j <= L; j++) omega[k] ^= mul(C[j], S[k - j]);

	/* Chien: every position; at a root, Forney's value */
	uint32_t roots = 0;
	int at[RS_T];
	uint8_t value[RS_T];
	for (int i = 0; i < RS_N; i++) {
		const uint32_t lx = (RS_PRIM * (254u - i)) % 255u;                      /* log X_i */
		const uint8_t xinv = alpha_pow(255u - lx);
		uint8_t lam = 0, odd = 0, p = 1;                                        /* Lambda(1 / X), x Lambda'(x) there, (1 / X)^j */
		for (uint32_t j = 0; j <= L; j++) {
			const uint8_t term = mul(C[j], p);
			lam ^= term;
			if (j & 1u) odd ^= term;
			p = mul(p, xinv);
		}
		if (lam != 0) continue;
		if (roots == RS_T) return MDEMOD_RS_FAILED;                            /* (more roots than the degree: not reached) */
		uint8_t om = 0;
		p = 1;
		for (uint32_t k = 0; k < RS_T; k++) { om ^= mul(omega[k], p); p = mul(p, xinv); }
		/* X^(1 - 112) Omega / Lambda' = X^(-112) Omega / (x Lambda'(x)) at x = 1 / X */
		at[roots] = i;
		value[roots] = (om && odd) ? mul(mul(om, inverse(odd)), alpha_pow(255u * 112u - 112u * lx)) : 0;
		roots++;
	}
	if (roots != L) return MDEMOD_RS_FAILED;
	for (uint32_t r = 0; r < roots; r++) w[at[r]] ^= value[r];
	return L;
}

} /* namespace */

int
rs_settings(const mdemod_rs_opts *opts, mdemod_rs_opts &out)
{
	mdemod_rs_default_opts(&out);
	if (opts) out = *opts;
	if (out.derandomise > 1) REFUSE("rs: derandomise is %u (0 or 1)", out.derandomise);
	if (out.dual_basis > 1) REFUSE("rs: dual_basis is %u (0 or 1)", out.dual_basis);
	if (out.piece_frames > MDEMOD_RS_MAX_PIECE)
		REFUSE("rs: piece_frames is %llu (0 for the default, or at most %u)", (unsigned long long)out.piece_frames, MDEMOD_RS_MAX_PIECE);
	if (!out.piece_frames) out.piece_frames = MDEMOD_RS_DEFAULT_PIECE;
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_rs_default_opts(mdemod_rs_opts *opts)
{
	if (!opts) return;
	opts->derandomise = 1;
	opts->dual_basis = 0;
	opts->piece_frames = 0;
}

void
mdemod_rs_vcdu_header(const uint8_t *vcdu, mdemod_rs_header *out)
{
	if (!vcdu || !out) return;
	out->version = vcdu[0] >> 6;
	out->spacecraft = ((vcdu[0] & 0x3Fu) << 2) | (vcdu[1] >> 6);
	out->vcid = vcdu[1] & 0x3Fu;
	out->counter = (static_cast<uint32_t>(vcdu[2]) << 16) | (static_cast<uint32_t>(vcdu[3]) << 8) | vcdu[4];
}

void mdemod_rs_model_pn(uint8_t *pn) { memcpy(pn, TAB.pn, 255); }
void mdemod_rs_model_generator(uint8_t *gen) { memcpy(gen, TAB.gen, RS_ROOTS + 1); }
void mdemod_rs_model_dual(uint8_t *T, uint8_t *Tinv) { memcpy(T, TAB.T, 256); memcpy(Tinv, TAB.Tinv, 256); }
void mdemod_rs_model_parity(const uint8_t *data, uint8_t *parity) { parity_of(data, parity); }

int
mdemod_rs_model_encode(const mdemod_rs_opts *opts, const uint8_t *vcdu, uint8_t *cadu)
try { MDEMOD_API_ENTER
	if (!vcdu || !cadu) REFUSE("mdemod_rs_model_encode: the VCDU and the CADU are needed");
	mdemod_rs_opts o;
	const int rc = rs_settings(opts, o);
	if (rc) return rc;
	memcpy(cadu, MARKER, 4);
	uint8_t *body = cadu + 4;
	for (int c = 0; c < RS_DEPTH; c++) {
		uint8_t word[RS_N];
		for (int i = 0; i < RS_K; i++) {
			const uint8_t v = vcdu[RS_DEPTH * i + c];
			word[i] = o.dual_basis ? TAB.Tinv[v] : v;
		}
		parity_of(word, word + RS_K);
		for (int i = 0; i < RS_N; i++) body[RS_DEPTH * i + c] = o.dual_basis ? TAB.T[word[i]] : word[i];
	}
	if (o.derandomise)
		for (int i = 0; i < RS_CODED; i++) body[i] ^= TAB.pn[i];
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_rs_model_decode(const mdemod_rs_opts *opts, const uint8_t *cadu, uint64_t n, uint8_t *vcdu, mdemod_rs_info *info)
try { MDEMOD_API_ENTER
	if (!n) return MDEMOD_OK;
	if (!cadu || !vcdu || !info) REFUSE("mdemod_rs_model_decode: the CADUs, the VCDUs and the report are needed");
	mdemod_rs_opts o;
	const int rc = rs_settings(opts, o);
	if (rc) return rc;
	for (uint64_t f = 0; f < n; f++) {
		const uint8_t *body = cadu + f * MDEMOD_RS_CADU_BYTES + 4;
		uint8_t *out = vcdu + f * MDEMOD_RS_VCDU_BYTES;
		info[f].flags = 0;
		for (int c = 0; c < RS_DEPTH; c++) {
			uint8_t word[RS_N];
			for (int i = 0; i < RS_N; i++) {
				uint8_t v = body[RS_DEPTH * i + c];
				if (o.derandomise) v ^= TAB.pn[RS_DEPTH * i + c];
				word[i] = o.dual_basis ? TAB.Tinv[v] : v;
			}
			const uint32_t corrected = decode_word(word);
			info[f].corrected[c] = static_cast<uint8_t>(corrected);
			if (corrected == MDEMOD_RS_FAILED) info[f].flags |= MDEMOD_RS_UNCORRECTABLE;
			for (int i = 0; i < RS_K; i++) out[RS_DEPTH * i + c] = o.dual_basis ? TAB.T[word[i]] : word[i];
		}
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
