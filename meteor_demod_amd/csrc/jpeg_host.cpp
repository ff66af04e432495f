/*
 * jpeg_host.cpp — host side of the JPEG encoder (include/meteor_demod_amd_jpeg.h): the argument checks, the sizes, the head of a
 * file, and the host model of the kernels of csrc/jpeg.hip (mdemod_jpeg_model_*: the rule of csrc/jpeg_host.h as plain loops, one
 * block and one bit after the other).  Free of the GPU runtime.
 */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_host.h"
#include "encoder_host.h"

namespace {

constexpr JpegCodes CODES = jpeg_make_codes();
constexpr JpegUnzig UNZIG = jpeg_make_unzig();

/* the bits of one segment, one after the other; the bytes with their 00s come out of flush() */
struct BitWriter {
	std::vector<uint8_t> &out;
	uint64_t acc = 0;
	uint32_t cnt = 0;
	explicit BitWriter(std::vector<uint8_t> &o) : out(o) {}
	void byte(uint32_t b) { out.push_back(static_cast<uint8_t>(b)); if (b == 0xFFu) out.push_back(0); }
	void put(uint32_t bits, uint32_t count)
	{
		acc = (acc << count) | bits;
		cnt += count;
		while (cnt >= 8) { cnt -= 8; byte(static_cast<uint32_t>(acc >> cnt) & 255u); }
	}
	void flush() { if (cnt) put((1u << (8 - cnt)) - 1u, 8 - cnt); }
};

struct HostSrc {
	const int16_t *p;
	void load8(int g, int16_t *w) const { memcpy(w, p + 8 * g, 16); }
};

void
model_block(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t bx, uint32_t by, uint32_t c, const uint8_t *q, int16_t *coef)
{
	int32_t t[64], R[8], col[8];
	for (uint32_t y = 0; y < 8; y++) {
		int32_t f[8];
		const uint32_t i = by * 8 + y < height ? by * 8 + y : height - 1;
		for (uint32_t x = 0; x < 8; x++) {
			const uint32_t j = bx * 8 + x < width ? bx * 8 + x : width - 1;
			const uint8_t *p = picture + (static_cast<size_t>(i) * width + j) * planes;
			f[x] = (planes == 1 ? p[0] : jpeg_ycc(static_cast<int>(c), p[0], p[1], p[2])) - 128;
		}
		jpeg_line(f, t + 8 * y);
	}
	for (uint32_t u = 0; u < 8; u++) {
		for (uint32_t y = 0; y < 8; y++) col[y] = t[8 * y + u];
		jpeg_column(col, R);
		for (uint32_t v = 0; v < 8; v++) {
			const uint32_t n = 8 * v + u;
			coef[UNZIG.at[n]] =static_cast<int16_t>(jpeg_level(R[v], q[n], n == 0));
		}
	}
}

/* the segments and the markers between them, appended to out */
void
model_segments(const int16_t *coef, uint64_t n_mcus, uint32_t planes, uint32_t ri, std::vector<uint8_t> &out)
{
	const uint64_t n_seg = (n_mcus + ri - 1) / ri;
	for (uint64_t s = 0; s < n_seg; s++) {
		BitWriter w(out);
		int32_t pred[3] = { 0, 0, 0 };
		const uint64_t end = (s + 1) * ri < n_mcus ? (s + 1) * ri : n_mcus;
		for (uint64_t m = s * ri; m < end; m++)
			for (uint32_t c = 0; c < planes; c++) {
				const HostSrc src{ coef + (m * planes + c) * 64 };
				pred[c] = jpeg_code_block(CODES.dc[c != 0], CODES.ac[c != 0], src, pred[c], w);
			}
		w.flush();
		if (s + 1 < n_seg) { out.push_back(0xFF); out.push_back(static_cast<uint8_t>(0xD0 + (s & 7))); }
	}
}

} /* namespace */

int
jpeg_check_picture(const char *who, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval)
{
	if (planes != 1 && planes != 3) REFUSE("%s: planes must be 1 or 3, not %u", who, planes);
	if (width < 1 || width > MDEMOD_JPEG_MAX_WIDTH) REFUSE("%s: width %u is outside 1 .. %d", who, width, MDEMOD_JPEG_MAX_WIDTH);
	if (height < 1 || height > MDEMOD_JPEG_MAX_HEIGHT) REFUSE("%s: height %u is outside 1 .. %d", who, height, MDEMOD_JPEG_MAX_HEIGHT);
	if (quality < 1 || quality > 100) REFUSE("%s: quality %u is outside 1 .. 100", who, quality);
	if (restart_interval > MDEMOD_JPEG_MAX_RESTART) REFUSE("%s: restart interval %u is outside 0 .. %d", who, restart_interval, MDEMOD_JPEG_MAX_RESTART);
	return MDEMOD_OK;
}

int
jpeg_check_entropy(const char *who, uint64_t n_mcus, uint32_t planes, uint32_t restart_interval)
{
	if (planes != 1 && planes != 3) REFUSE("%s: planes must be 1 or 3, not %u", who, planes);
	if (n_mcus < 1 || n_mcus > JPEG_MAX_MCUS) REFUSE("%s: %llu MCUs are outside 1 .. 2^21", who, static_cast<unsigned long long>(n_mcus));
	if (restart_interval > MDEMOD_JPEG_MAX_RESTART) REFUSE("%s: restart interval %u is outside 0 .. %d", who, restart_interval, MDEMOD_JPEG_MAX_RESTART);
	return MDEMOD_OK;
}

uint32_t
jpeg_head(uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval, uint8_t *head)
{
	uint8_t q[128];
	jpeg_quant_tables(quality, q);
	uint32_t n = 0;
	auto b = [&](uint32_t v) { head[n++] = static_cast<uint8_t>(v); };
	auto w = [&](uint32_t v) { b(v >> 8); b(v & 255u); };
	const uint32_t tabs = planes == 3 ? 2 : 1;
	w(0xFFD8);
	w(0xFFE0); w(16); b('J'); b('F'); b('I'); b('F'); b(0); w(0x0101); b(0); w(1); w(1); b(0); b(0);
	w(0xFFDB); w(2 + 65 * tabs);
	for (uint32_t t = 0; t < tabs; t++) {
		b(t);
		for (int k = 0; k < 64; k++) b(q[64 * t + IMG_ZIGZAG[k]]);
	}
	w(0xFFC0); w(8 + 3 * planes); b(8); w(height); w(width); b(planes);
	for (uint32_t c = 0; c < planes; c++) { b(c + 1); b(0x11); b(c ? 1 : 0); }
	w(0xFFC4); w(2 + 208 * tabs);
	for (uint32_t t = 0; t < tabs; t++) {
		const uint8_t *dc_bits = t ? JPEG_DC_BITS_C : IMG_DC_BITS, *ac_bits = t ? JPEG_AC_BITS_C : IMG_AC_BITS, *ac_val = t ? JPEG_AC_VAL_C : IMG_AC_VAL;
		b(t);
		for (int i = 0; i < 16; i++) b(dc_bits[i]);
		for (int i = 0; i < 12; i++) b(i);
		b(0x10 | t);
		for (int i = 0; i < 16; i++) b(ac_bits[i]);
		for (int i = 0; i < 162; i++) b(ac_val[i]);
	}
	w(0xFFDD); w(4); w(jpeg_interval(restart_interval));
	w(0xFFDA); w(6 + 2 * planes); b(planes);
	for (uint32_t c = 0; c < planes; c++) { b(c + 1); b(c ? 0x11 : 0x00); }
	b(0); b(63); b(0);
	return n;
}

extern "C" {

uint64_t
mdemod_jpeg_entropy_bound(uint64_t n_mcus, uint32_t planes, uint32_t restart_interval)
{
	if ((planes != 1 && planes != 3) || restart_interval > MDEMOD_JPEG_MAX_RESTART || n_mcus < 1 || n_mcus > JPEG_MAX_MCUS) return 0;
	const uint64_t ri = jpeg_interval(restart_interval);
	return 2ull * MDEMOD_JPEG_BLOCK_BYTES * n_mcus * planes + 2ull * ((n_mcus + ri - 1) / ri);
}

uint64_t
mdemod_jpeg_bound(uint32_t width, uint32_t height, uint32_t planes, uint32_t restart_interval)
{
	if (width < 1 || width > MDEMOD_JPEG_MAX_WIDTH || height < 1 || height > MDEMOD_JPEG_MAX_HEIGHT) return 0;
	const uint64_t e = mdemod_jpeg_entropy_bound(jpeg_mcus(width, height), planes, restart_interval);
	return e ? e + (planes == 3 ? MDEMOD_JPEG_HEAD_COLOUR : MDEMOD_JPEG_HEAD_GREY) : 0;
}

uint64_t
mdemod_jpeg_entropy_workspace(uint64_t n_mcus, uint32_t restart_interval)
{
	if (restart_interval > MDEMOD_JPEG_MAX_RESTART || n_mcus < 1 || n_mcus > JPEG_MAX_MCUS) return 0;
	const uint64_t ri = jpeg_interval(restart_interval), n_seg = (n_mcus + ri - 1) / ri;
	return (n_seg + 1) * 8 + ((n_seg * 4 + 15) & ~15ull);                  /* an offset and a length per segment */
}

uint64_t
mdemod_jpeg_workspace(uint32_t width, uint32_t height, uint32_t planes, uint32_t restart_interval)
{
	if (!mdemod_jpeg_bound(width, height, planes, restart_interval)) return 0;
	const uint64_t n = jpeg_mcus(width, height);
	return n * planes * 128 + mdemod_jpeg_entropy_workspace(n, restart_interval);
}

void mdemod_jpeg_free(uint8_t *file) { free(file); }

int
mdemod_jpeg_model_tables(uint32_t quality, uint8_t *q, uint8_t *bits, uint8_t *vals, uint8_t *zigzag, int32_t *m)
try { MDEMOD_API_ENTER
	if (quality < 1 || quality > 100) REFUSE("mdemod_jpeg_model_tables: quality %u is outside 1 .. 100", quality);
	if (q) jpeg_quant_tables(quality, q);
	if (bits) {
		memcpy(bits, IMG_DC_BITS, 16); memcpy(bits + 16, IMG_AC_BITS, 16);
		memcpy(bits + 32, JPEG_DC_BITS_C, 16); memcpy(bits + 48, JPEG_AC_BITS_C, 16);
	}
	if (vals) {
		memset(vals, 0, 4 * 162);
		for (int i = 0; i < 12; i++) vals[i] = vals[2 * 162 + i] = static_cast<uint8_t>(i);
		memcpy(vals + 162, IMG_AC_VAL, 162); memcpy(vals + 3 * 162, JPEG_AC_VAL_C, 162);
	}
	if (zigzag) memcpy(zigzag, IMG_ZIGZAG, 64);
	if (m)
		for (int x = 0; x < 8; x++)
			for (int u = 0; u < 8; u++) m[8 * x + u] = img_m(x, u);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

void
mdemod_jpeg_model_fdct(const uint8_t *samples, int32_t *R)
{
	int32_t t[64], col[8], out[8];
	for (int y = 0; y < 8; y++) {
		int32_t f[8];
		for (int x = 0; x < 8; x++) f[x] = static_cast<int32_t>(samples[8 * y + x]) - 128;
		jpeg_line(f, t + 8 * y);
	}
	for (int u = 0; u < 8; u++) {
		for (int y = 0; y < 8; y++) col[y] = t[8 * y + u];
		jpeg_column(col, out);
		for (int v = 0; v < 8; v++) R[8 * v + u] = out[v];
	}
}

int
mdemod_jpeg_model_coefficients(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, int16_t *coef)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_jpeg_model_coefficients";
	const int rc = jpeg_check_picture(who, width, height, planes, quality, 0);
	if (rc) return rc;
	if (!picture || !coef) REFUSE("%s: the picture and the coefficients are needed", who);
	uint8_t q[128];
	jpeg_quant_tables(quality, q);
	const uint32_t mx = (width + 7) / 8, my = (height + 7) / 8;
	for (uint32_t by = 0; by < my; by++)
		for (uint32_t bx = 0; bx < mx; bx++)
			for (uint32_t c = 0; c < planes; c++)
				model_block(picture, width, height, planes, bx, by, c, q + (c ? 64 : 0), coef + ((static_cast<size_t>(by) * mx + bx) * planes + c) * 64);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_jpeg_model_entropy(const int16_t *coef, uint64_t n_mcus, uint32_t planes, uint32_t restart_interval, uint8_t *out, uint64_t out_room, uint64_t *bytes)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_jpeg_model_entropy";
	const int rc = jpeg_check_entropy(who, n_mcus, planes, restart_interval);
	if (rc) return rc;
	if (!coef || (!out && out_room)) REFUSE("%s: the coefficients and the output are needed", who);
	std::vector<uint8_t> file;
	model_segments(coef, n_mcus, planes, jpeg_interval(restart_interval), file);
	return enc_give(who, file, out, out_room, bytes);
} MDEMOD_API_CATCH

int
mdemod_jpeg_model_encode(const uint8_t *picture, uint32_t width, uint32_t height, uint32_t planes, uint32_t quality, uint32_t restart_interval, uint8_t *out,
                         uint64_t out_room, uint64_t *bytes)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_jpeg_model_encode";
	int rc = jpeg_check_picture(who, width, height, planes, quality, restart_interval);
	if (rc) return rc;
	if (!picture || (!out && out_room)) REFUSE("%s: the picture and the output are needed", who);
	const uint64_t n_mcus = jpeg_mcus(width, height);
	std::vector<int16_t> coef(n_mcus * planes * 64);
	if ((rc = mdemod_jpeg_model_coefficients(picture, width, height, planes, quality, coef.data()))) return rc;
	std::vector<uint8_t> file(JPEG_HEAD_ROOM);
	file.resize(jpeg_head(width, height, planes, quality, restart_interval, file.data()));
	model_segments(coef.data(), n_mcus, planes, jpeg_interval(restart_interval), file);
	file.push_back(0xFF); file.push_back(0xD9);
	return enc_give(who, file, out, out_room, bytes);
} MDEMOD_API_CATCH

} /* extern "C" */
