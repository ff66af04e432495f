/*
 * image_host.cpp — host side of the image layer (include/meteor_demod_amd_image.h): the option check, the placement, the pieces of
 * the host entry, the synthetic sender, and the host model of the kernels of csrc/image.hip (mdemod_image_model_*: one core, the
 * walk and the packet decoder of csrc/image_host.h over plain arrays).  Free of the GPU runtime.
 */
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "image_host.h"
#include "mdemod_internal_api.h"

namespace {

constexpr ImgTables TAB = img_make_tables();
constexpr ImgCodes CODES = img_make_codes();

struct HostBlk {
	int32_t *c;
	int32_t get(uint32_t i) const { return c[i]; }
	void set(uint32_t i, int32_t v) const { c[i] = v; }
};
struct HostQt {
	uint16_t *q;
	uint32_t get(uint32_t i) const { return q[i]; }
	void set(uint32_t i, uint32_t v) const { q[i] = static_cast<uint16_t>(v); }
};
struct HostOut {
	uint8_t *strip;
	void put(uint32_t k, int y, uint32_t lo, uint32_t hi) const
	{
		uint8_t *p = strip + 112 * y + 8 * k;
		for (int i = 0; i < 4; i++) { p[i] = static_cast<uint8_t>(lo >> (8 * i)); p[4 + i] = static_cast<uint8_t>(hi >> (8 * i)); }
	}
};

int
model_find(const mdemod_image_opts &o, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, std::vector<mdemod_packet> &desc)
{
	mdemod_packet row[MDEMOD_IMAGE_MAX_PER_FRAME];
	for (uint64_t f = 0; f < n; f++) {
		const uint32_t c = img_walk(vcdu, info, n, f, o.vcid, row, MDEMOD_IMAGE_MAX_PER_FRAME);
		desc.insert(desc.end(), row, row + c);
	}
	return MDEMOD_OK;
}

void
model_decode(const uint8_t *vcdu, uint64_t n, const mdemod_packet *desc, uint64_t n_desc, uint8_t *strips, mdemod_strip_info *sinfo)
{
	for (uint64_t i = 0; i < n_desc; i++) {
		int32_t blk[64];
		uint16_t qt[64];
		sinfo[i] = img_decode_packet(TAB, vcdu, n, desc[i], HostBlk{ blk }, HostQt{ qt }, HostOut{ strips + i * MDEMOD_IMAGE_STRIP_BYTES });
	}
}

int
model_piece(void *, const mdemod_image_opts &o, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t k, std::vector<mdemod_packet> &desc,
            std::vector<mdemod_strip_info> &sinfo, std::vector<uint8_t> &strips)
{
	model_find(o, vcdu, info, k, desc);
	sinfo.resize(desc.size());
	strips.resize(desc.size() * MDEMOD_IMAGE_STRIP_BYTES);
	model_decode(vcdu, k, desc.data(), desc.size(), strips.data(), sinfo.data());
	return MDEMOD_OK;
}

struct BitWriter {
	uint8_t *out;
	uint64_t cap, bits;
	bool full;
	void put(uint32_t value, uint32_t count)
	{
		for (uint32_t i = count; i-- > 0;) {
			const uint64_t at = bits >> 3;
			if (at >= cap) { full = true; return; }
			if (!(bits & 7)) out[at] = 0;
			out[at] |= static_cast<uint8_t>(((value >> i) & 1u) << (7 - (bits & 7)));
			bits++;
		}
	}
};

uint32_t category(int32_t v) { uint32_t a = static_cast<uint32_t>(v < 0 ? -v : v), s = 0; while (a) { s++; a >>= 1; } return s; }
uint32_t extra_of(int32_t v, uint32_t s) { return static_cast<uint32_t>(v >= 0 ? v : v + (1 << s) - 1); }

} /* namespace */

int
img_settings(const mdemod_image_opts *opts, mdemod_image_opts &out)
{
	mdemod_image_default_opts(&out);
	if (opts) out = *opts;
	if (out.vcid > 63) REFUSE("image: vcid is %u (0 .. 63)", out.vcid);
	if (out.period == 0) REFUSE("image: period is 0 (packets per strip row: 43)");
	for (int k = 0; k < 3; k++) {
		if (out.apids[k] < 64 || out.apids[k] > 69) REFUSE("image: apids[%d] is %u (the image channels are apid 64 .. 69)", k, out.apids[k]);
		for (int j = 0; j < k; j++)
			if (out.apids[j] == out.apids[k]) REFUSE("image: apids names %u twice (apid repeated)", out.apids[k]);
	}
	if (out.piece_frames > MDEMOD_RS_MAX_PIECE)
		REFUSE("image: piece_frames is %llu (0 for the default, or at most %u)", (unsigned long long)out.piece_frames, MDEMOD_RS_MAX_PIECE);
	if (!out.piece_frames) out.piece_frames = MDEMOD_RS_DEFAULT_PIECE;
	return MDEMOD_OK;
}

int
img_decode_pieces(const mdemod_image_opts &o, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, mdemod_image_result *out, img_piece_fn piece,
                  void *ctx)
{
	memset(out, 0, sizeof *out);
	std::vector<mdemod_packet> desc, d;
	std::vector<mdemod_strip_info> sinfo, si;
	std::vector<uint8_t> strips, st;
	const uint64_t P = o.piece_frames;
	for (uint64_t at = 0; at < n; at += P) {
		const uint64_t own = P < n - at ? P : n - at;
		const uint64_t k = own + MDEMOD_IMAGE_OVERLAP < n - at ? own + MDEMOD_IMAGE_OVERLAP : n - at;
		d.clear(); si.clear(); st.clear();
		const int rc = piece(ctx, o, vcdu + at * IMG_VCDU, info ? info + at : nullptr, k, d, si, st);
		if (rc) return rc;
		for (size_t i = 0; i < d.size(); i++) {
			if (d[i].start >= own * IMG_ZONE) break;                                /* (stream order) the next piece's own */
			mdemod_packet p = d[i];
			p.start += static_cast<uint32_t>(at * IMG_ZONE);
			desc.push_back(p);
			sinfo.push_back(si[i]);
			strips.insert(strips.end(), st.begin() + i * MDEMOD_IMAGE_STRIP_BYTES, st.begin() + (i + 1) * MDEMOD_IMAGE_STRIP_BYTES);
		}
	}
	const size_t m = desc.size();
	out->n_packets = m;
	out->desc = static_cast<mdemod_packet *>(malloc((m ? m : 1) * sizeof(mdemod_packet)));
	out->sinfo = static_cast<mdemod_strip_info *>(malloc((m ? m : 1) * sizeof(mdemod_strip_info)));
	out->strips = static_cast<uint8_t *>(malloc((m ? m : 1) * MDEMOD_IMAGE_STRIP_BYTES));
	out->place = static_cast<mdemod_placement *>(malloc((m ? m : 1) * sizeof(mdemod_placement)));
	if (!out->desc || !out->sinfo || !out->strips || !out->place) { mdemod_image_free(out); return MDEMOD_ERR_NOMEM; }
	if (m) {
		memcpy(out->desc, desc.data(), m * sizeof(mdemod_packet));
		memcpy(out->sinfo, sinfo.data(), m * sizeof(mdemod_strip_info));
		memcpy(out->strips, strips.data(), m * MDEMOD_IMAGE_STRIP_BYTES);
	}
	int rc = mdemod_image_place(&o, out->desc, out->sinfo, m, out->place, &out->summary);
	if (rc) { mdemod_image_free(out); return rc; }
	const uint64_t rows = out->summary.rows;
	if (rows) {
		for (int k = 0; k < 3; k++) {
			out->image[k] = static_cast<uint8_t *>(calloc(rows * 8 * MDEMOD_IMAGE_WIDTH, 1));
			out->filled[k] = static_cast<uint8_t *>(calloc(rows * MDEMOD_IMAGE_CELLS, 1));
			if (!out->image[k] || !out->filled[k]) { mdemod_image_free(out); return MDEMOD_ERR_NOMEM; }
		}
		for (size_t i = 0; i < m; i++) {
			const mdemod_placement &p = out->place[i];
			if (p.channel < 0) continue;
			uint8_t *to = out->image[p.channel] + (static_cast<uint64_t>(p.row) * 8) * MDEMOD_IMAGE_WIDTH + 112u * p.cell;
			for (int y = 0; y < 8; y++) memcpy(to + static_cast<uint64_t>(y) * MDEMOD_IMAGE_WIDTH, out->strips + i * MDEMOD_IMAGE_STRIP_BYTES + 112 * y, 112);
			uint8_t &cell = out->filled[p.channel][static_cast<uint64_t>(p.row) * MDEMOD_IMAGE_CELLS + p.cell];
			if (!cell) out->summary.cells_filled++;
			cell = 1;
		}
	}
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_image_default_opts(mdemod_image_opts *opts)
{
	if (!opts) return;
	opts->vcid = 5;
	opts->period = 43;
	opts->apids[0] = 64; opts->apids[1] = 65; opts->apids[2] = 66;
	opts->reserved = 0;
	opts->piece_frames = 0;
}

void
mdemod_image_free(mdemod_image_result *out)
{
	if (!out) return;
	free(out->desc); free(out->sinfo); free(out->strips); free(out->place);
	for (int k = 0; k < 3; k++) { free(out->image[k]); free(out->filled[k]); }
	memset(out, 0, sizeof *out);
}

int
mdemod_image_place(const mdemod_image_opts *opts, const mdemod_packet *desc, const mdemod_strip_info *sinfo, uint64_t n_desc, mdemod_placement *place,
                   mdemod_place_summary *summary)
try { MDEMOD_API_ENTER
	mdemod_image_opts o;
	const int rc = img_settings(opts, o);
	if (rc) return rc;
	if (n_desc && (!desc || !sinfo)) REFUSE("mdemod_image_place: the descriptors and the reports are needed");
	mdemod_place_summary s;
	memset(&s, 0, sizeof s);
	s.packets = n_desc;
	bool anchored = false, have_prev = false, have_last = false;
	int64_t first = 0, wraps = 0;
	uint32_t prev = 0, last = 0, top = 0;
	for (uint64_t i = 0; i < n_desc; i++) {
		const mdemod_packet &d = desc[i];
		const mdemod_strip_info &r = sinfo[i];
		mdemod_placement p = { -1, 0, 0, 0 };
		if (d.apid >= 64 && d.apid <= 70) {
			if (have_last && d.seq != ((last + 1u) & 0x3FFFu)) s.seq_gaps++;
			have_last = true;
			last = d.seq;
		}
		const bool image = d.apid >= 64 && d.apid <= 69 && !(r.flags & (MDEMOD_STRIP_NOT_IMAGE | MDEMOD_STRIP_OUTSIDE));
		if (image) s.per_apid[d.apid - 64]++;
		int slot = -1;
		for (int k = 0; k < 3; k++)
			if (o.apids[k] == d.apid) slot = k;
		if (image && slot >= 0 && !(r.flags & MDEMOD_STRIP_BAD_HEADER)) {
			if (!anchored && r.flags == 0) {
				anchored = true;
				first = static_cast<int64_t>(d.seq) - 14 * slot - r.mcun / 14;
			}
			if (!anchored) s.dropped++;
			else {
				if (have_prev && d.seq < prev) wraps++;
				have_prev = true;
				prev = d.seq;
				const int64_t row = (static_cast<int64_t>(d.seq) + 16384 * wraps - first) / static_cast<int64_t>(o.period);
				if (row >= MDEMOD_IMAGE_MAX_ROWS) s.dropped++;
				else {
					p.channel = slot;
					p.row = static_cast<uint32_t>(row);
					p.cell = r.mcun / 14u;
					s.placed++;
					if (r.flags & MDEMOD_STRIP_TRUNCATED) s.truncated++;
					if (p.row + 1 > top) top = p.row + 1;
				}
			}
		}
		if (place) place[i] = p;
	}
	s.first = first;
	s.rows = top;
	s.anchored = anchored;
	if (summary) *summary = s;
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_image_model_find(const mdemod_image_opts *opts, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, mdemod_packet *desc, uint64_t cap,
                        uint64_t *total)
try { MDEMOD_API_ENTER
	mdemod_image_opts o;
	const int rc = img_settings(opts, o);
	if (rc) return rc;
	if (!total) REFUSE("mdemod_image_model_find: the total is needed");
	*total = 0;
	if (!n) return MDEMOD_OK;
	if (!vcdu || (cap && !desc)) REFUSE("mdemod_image_model_find: the VCDUs and the descriptors are needed");
	if (n > IMG_MAX_FRAMES) REFUSE("image: %llu frames are more than one batch takes (2^20)", (unsigned long long)n);
	std::vector<mdemod_packet> all;
	model_find(o, vcdu, info, n, all);
	*total = all.size();
	const uint64_t k = all.size() < cap ? all.size() : cap;
	if (k) memcpy(desc, all.data(), k * sizeof(mdemod_packet));
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_image_model_decode(const mdemod_image_opts *opts, const uint8_t *vcdu, uint64_t n, const mdemod_packet *desc, uint64_t n_desc, uint8_t *strips,
                          mdemod_strip_info *sinfo)
try { MDEMOD_API_ENTER
	mdemod_image_opts o;
	const int rc = img_settings(opts, o);
	if (rc) return rc;
	if (!n_desc) return MDEMOD_OK;
	if ((n && !vcdu) || !desc || !strips || !sinfo) REFUSE("mdemod_image_model_decode: the VCDUs, the descriptors, the strips and the reports are needed");
	if (n > IMG_MAX_FRAMES) REFUSE("image: %llu frames are more than one batch takes (2^20)", (unsigned long long)n);
	model_decode(vcdu, n, desc, n_desc, strips, sinfo);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

void
mdemod_image_model_quant(uint32_t q, uint16_t *out)
{
	for (uint32_t i = 0; i < 64; i++) out[i] = static_cast<uint16_t>(img_quant(TAB, q, i));
}

void
mdemod_image_model_idct(const int32_t *in, uint8_t *out)
{
	int32_t t[64];
	for (int y = 0; y < 8; y++)
		for (int u = 0; u < 8; u++) {
			int32_t sum = 0;
			for (int v = 0; v < 8; v++) {
				const int32_t c = in[8 * v + u] < -2048 ? -2048 : in[8 * v + u] > 2047 ? 2047 : in[8 * v + u];
				sum += img_m(y, v) * c;
			}
			t[8 * y + u] = (sum + 2048) >> 12;
		}
	for (int y = 0; y < 8; y++)
		for (int x = 0; x < 8; x++) {
			int32_t A = 0, B = 0;
			for (int u = 0; u < 8; u++) {
				A += img_m(x, u) * (t[8 * y + u] >> 9);
				B += img_m(x, u) * (t[8 * y + u] & 511);
			}
			const int32_t R = A + ((B + 256) >> 9);
			const int32_t p = 128 + ((R + 32768) >> 16);
			out[8 * y + x] = static_cast<uint8_t>(p < 0 ? 0 : p > 255 ? 255 : p);
		}
}

void
mdemod_image_model_tables(uint8_t *bits, uint8_t *dc_val, uint8_t *ac_val, uint8_t *zigzag, uint8_t *std_q, int32_t *m)
{
	memcpy(bits, IMG_DC_BITS, 16);
	memcpy(bits + 16, IMG_AC_BITS, 16);
	memcpy(dc_val, TAB.dc_val, 12);
	memcpy(ac_val, TAB.ac_val, 162);
	memcpy(zigzag, TAB.zigzag, 64);
	memcpy(std_q, TAB.std_q, 64);
	for (int x = 0; x < 8; x++)
		for (int u = 0; u < 8; u++) m[8 * x + u] = img_m(x, u);
}

int64_t
mdemod_image_model_encode_packet(const uint8_t *strip, uint32_t q, uint32_t mcun, uint32_t apid, uint32_t seq, uint32_t day, uint32_t ms, uint32_t us,
                                 uint8_t *out, uint64_t cap)
try { MDEMOD_API_ENTER
	if (!strip || !out) REFUSE("mdemod_image_model_encode_packet: the strip and the packet are needed");
	if (q > 255 || mcun > 255 || apid > 2047 || seq > 16383 || day > 65535 || us > 65535)
		REFUSE("mdemod_image_model_encode_packet: a field does not fit (q %u, mcun %u, apid %u, seq %u, day %u, us %u)", q, mcun, apid, seq, day, us);
	if (cap < IMG_HEAD + 1) REFUSE("mdemod_image_model_encode_packet: room for %llu bytes is less than a packet's head", (unsigned long long)cap);
	uint16_t qt[64];
	mdemod_image_model_quant(q, qt);
	BitWriter w = { out + IMG_HEAD, cap - IMG_HEAD, 0, false };
	const double pi = 3.14159265358979323846;
	double cs[8][8];                                                              /* cos((2 x + 1) u pi / 16) */
	for (int x = 0; x < 8; x++)
		for (int u = 0; u < 8; u++) cs[x][u] = cos((2 * x + 1) * u * pi / 16);
	int32_t pred = 0;
	for (int k = 0; k < MDEMOD_IMAGE_MCUS; k++) {
		int32_t coef[64];                                                         /* zigzag order */
		for (int z = 0; z < 64; z++) {
			const int v = TAB.zigzag[z] / 8, u = TAB.zigzag[z] % 8;
			double sum = 0;
			for (int y = 0; y < 8; y++)
				for (int x = 0; x < 8; x++) sum += (strip[112 * y + 8 * k + x] - 128.0) * cs[x][u] * cs[y][v];
			sum *= 0.25 * (u ? 1.0 : sqrt(0.5)) * (v ? 1.0 : sqrt(0.5));
			int32_t c = static_cast<int32_t>(lround(sum / qt[TAB.zigzag[z]]));
			coef[z] = c < -1023 ? -1023 : c > 1023 ? 1023 : c;           /* categories 10 (AC) and, for a difference of two, 11 (DC) */
		}
		const int32_t diff = coef[0] - pred;
		pred = coef[0];
		uint32_t s = category(diff);
		w.put(CODES.dc_code[s], CODES.dc_size[s]);
		w.put(extra_of(diff, s), s);
		int run = 0;
		for (int z = 1; z < 64; z++) {
			if (!coef[z]) { run++; continue; }
			for (; run >= 16; run -= 16) w.put(CODES.ac_code[0xF0], CODES.ac_size[0xF0]);
			s = category(coef[z]);
			w.put(CODES.ac_code[(run << 4) | s], CODES.ac_size[(run << 4) | s]);
			w.put(extra_of(coef[z], s), s);
			run = 0;
		}
		if (run) w.put(CODES.ac_code[0], CODES.ac_size[0]);
	}
	if (w.full) REFUSE("mdemod_image_model_encode_packet: the packet does not fit %llu bytes", (unsigned long long)cap);
	const uint64_t len = IMG_HEAD + (w.bits + 7) / 8;
	if (len > IMG_MAX_LEN) REFUSE("mdemod_image_model_encode_packet: the packet is %llu bytes (at most 65542)", (unsigned long long)len);
	const uint8_t head[IMG_HEAD] = {
		static_cast<uint8_t>(0x08 | (apid >> 8)), static_cast<uint8_t>(apid), static_cast<uint8_t>(0xC0 | (seq >> 8)), static_cast<uint8_t>(seq),
		static_cast<uint8_t>((len - 7) >> 8), static_cast<uint8_t>(len - 7),
		static_cast<uint8_t>(day >> 8), static_cast<uint8_t>(day), static_cast<uint8_t>(ms >> 24), static_cast<uint8_t>(ms >> 16), static_cast<uint8_t>(ms >> 8),
		static_cast<uint8_t>(ms), static_cast<uint8_t>(us >> 8), static_cast<uint8_t>(us), static_cast<uint8_t>(mcun), 0, 0, 0xFF, 0xF0, static_cast<uint8_t>(q) };
	memcpy(out, head, IMG_HEAD);
	return static_cast<int64_t>(len);
} MDEMOD_API_CATCH

int
mdemod_image_model_host(const mdemod_image_opts *opts, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, mdemod_image_result *out)
try { MDEMOD_API_ENTER
	mdemod_image_opts o;
	const int rc = img_settings(opts, o);
	if (rc) return rc;
	if (!out || (n && !vcdu)) REFUSE("mdemod_image_model_host: the VCDUs and the result are needed");
	if (n > 4 * static_cast<uint64_t>(IMG_MAX_FRAMES)) REFUSE("image: %llu frames are more than a stream position counts (2^22)", (unsigned long long)n);
	return img_decode_pieces(o, vcdu, info, n, out, model_piece, nullptr);
} MDEMOD_API_CATCH

} /* extern "C" */
