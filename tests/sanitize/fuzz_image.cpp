/*
 * fuzz_image.cpp — the host side of the image layer (csrc/image_host.cpp) under ASan + UBSan (tests/test_image_sanitize.py): batches
 * of 1 .. 6 VCDUs multiplexed here from the synthetic sender's packets, then left alone, mutated in a few bytes, or replaced by
 * random bytes under valid frame headers; random options (some out of range: refused with MDEMOD_ERR_PARAM and a text); the
 * descriptors the model finds and descriptors drawn at random (most point outside the batch: reported, never followed); the pieces
 * of the host entry's model path; the placement of random reports.  Every buffer is exactly as long as the interface says and
 * comes from the heap, so that one byte too far is a report.  What comes back is checked against the rules that hold for any
 * input.  Prints one JSON line.
 * Usage: fuzz_image <cases> <seed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/meteor_demod_amd_image.h"
#include "../../meteor_demod_amd/csrc/image_host.h"

static long bad = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); bad++; } while (0)

template <class T> static std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

int
main(int argc, char **argv)
{
	const long cases = argc > 1 ? atol(argv[1]) : 400;
	std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
	long accepted = 0, refused = 0, truncated = 0, outside = 0, decoded = 0, placed = 0, pieces = 0;
	for (long i = 0; i < cases; i++) {
		mdemod_image_opts o;
		mdemod_image_default_opts(&o);
		if (rng() & 1) { o.apids[0] = 64 + rng() % 2; o.apids[1] = 66 + rng() % 2; o.apids[2] = 68 + rng() % 2; }
		if (rng() & 1) o.period = 1 + static_cast<uint32_t>(rng() % 100);
		o.piece_frames = rng() % 5;
		bool broken = false;
		if (rng() % 10 == 0) {
			broken = true;
			switch (rng() % 5) {
			case 0: o.vcid = 64 + static_cast<uint32_t>(rng() % 1000); break;
			case 1: o.period = 0; break;
			case 2: o.apids[rng() % 3] = rng() & 1 ? 63 : 70 + static_cast<uint32_t>(rng() % 2000); break;
			case 3: o.apids[1] = o.apids[0]; break;
			default: o.piece_frames = (1ull << 20) + 1 + rng() % 1000; break;
			}
		}
		/* ---- the batch ---- */
		std::vector<uint8_t> stream;
		uint8_t strip[MDEMOD_IMAGE_STRIP_BYTES];
		std::vector<size_t> heads;
		const size_t want_frames = 1 + rng() % 6;
		uint32_t seq = static_cast<uint32_t>(rng() % 16384);
		while (stream.size() < want_frames * IMG_ZONE) {
			const int kind = static_cast<int>(rng() % 4);
			const uint8_t base = static_cast<uint8_t>(rng());
			for (int k = 0; k < MDEMOD_IMAGE_STRIP_BYTES; k++) strip[k] = kind == 0 ? static_cast<uint8_t>(rng()) : kind == 1 ? base : static_cast<uint8_t>(base + k % 112 + 3 * (k / 112));
			uint8_t packet[4096];
			const int64_t len = mdemod_image_model_encode_packet(strip, static_cast<uint32_t>(rng() % 101), 14 * static_cast<uint32_t>(rng() % 14),
			                                                      64 + static_cast<uint32_t>(rng() % 7), seq++ & 16383u, 1, 2, 3, packet, sizeof packet);
			if (len < 21 || len > 4096) { FAIL("case %ld: the sender returned %lld: %s", i, (long long)len, mdemod_last_error()); break; }
			heads.push_back(stream.size());
			stream.insert(stream.end(), packet, packet + len);
		}
		while (stream.size() % IMG_ZONE) {                                         /* idle fill */
			size_t room = IMG_ZONE - stream.size() % IMG_ZONE;
			if (room < 7) room += IMG_ZONE;
			heads.push_back(stream.size());
			const uint8_t h[6] = { 0x07, 0xFF, 0xC0, 0, static_cast<uint8_t>((room - 7) >> 8), static_cast<uint8_t>(room - 7) };
			stream.insert(stream.end(), h, h + 6);
			stream.insert(stream.end(), room - 6, 0x55);
		}
		const uint64_t n = stream.size() / IMG_ZONE;
		auto vcdu = exact<uint8_t>(n * IMG_VCDU);
		auto info = exact<mdemod_rs_info>(n);
		const uint32_t c0 = static_cast<uint32_t>(rng()) & 0xFFFFFFu;
		const int mode = static_cast<int>(rng() % 4);                               /* 0, 1: as sent; 2: mutated; 3: random under valid headers */
		for (uint64_t f = 0; f < n; f++) {
			uint8_t *v = vcdu.get() + f * IMG_VCDU;
			const uint32_t c = (c0 + f) & 0xFFFFFFu;
			uint32_t fhp = MDEMOD_IMAGE_NO_HEADER;
			for (size_t h : heads)
				if (h >= f * IMG_ZONE && h < (f + 1) * IMG_ZONE) { fhp = static_cast<uint32_t>(h - f * IMG_ZONE); break; }
			const uint8_t head[10] = { 0x40, 0x05, static_cast<uint8_t>(c >> 16), static_cast<uint8_t>(c >> 8), static_cast<uint8_t>(c), 0, 0, 0,
			                           static_cast<uint8_t>(fhp >> 8), static_cast<uint8_t>(fhp) };
			memcpy(v, head, 10);
			memcpy(v + 10, stream.data() + f * IMG_ZONE, IMG_ZONE);
			if (mode == 3) {
				for (int k = 10; k < IMG_VCDU; k++) v[k] = static_cast<uint8_t>(rng());
				const uint32_t p = static_cast<uint32_t>(rng() % 900);
				v[8] = static_cast<uint8_t>(p >> 8); v[9] = static_cast<uint8_t>(p);
			}
			info[f].flags = rng() % 9 == 0 ? MDEMOD_RS_UNCORRECTABLE : 0;
			memset(info[f].corrected, 0, 4);
		}
		if (mode == 2)
			for (int k = 0, m = 1 + static_cast<int>(rng() % 12); k < m; k++) vcdu[rng() % (n * IMG_VCDU)] ^= static_cast<uint8_t>(1 + rng() % 255);
		const mdemod_rs_info *ip = rng() & 1 ? info.get() : nullptr;

		/* ---- find ---- */
		uint64_t total = ~0ull;
		const uint64_t cap_all = MDEMOD_IMAGE_MAX_PER_FRAME * n;
		auto all = exact<mdemod_packet>(cap_all);
		int rc = mdemod_image_model_find(&o, vcdu.get(), ip, n, all.get(), cap_all, &total);
		if (broken) {
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: options out of range gave rc %d, text '%s'", i, rc, mdemod_last_error());
			mdemod_image_result res;
			rc = mdemod_image_model_host(&o, vcdu.get(), ip, n, &res);
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: the host entry took options out of range (rc %d)", i, rc);
			rc = mdemod_image_place(&o, all.get(), nullptr, 0, nullptr, nullptr);
			if (rc != MDEMOD_ERR_PARAM || !*mdemod_last_error()) FAIL("case %ld: the placement took options out of range (rc %d)", i, rc);
			refused++;
			continue;
		}
		if (rc != MDEMOD_OK || total > cap_all) { FAIL("case %ld: find gave rc %d, total %llu: %s", i, rc, (unsigned long long)total, mdemod_last_error()); continue; }
		if (mode < 2 && !ip && total != heads.size()) FAIL("case %ld: %llu of %zu packets of an undamaged batch", i, (unsigned long long)total, heads.size());
		accepted += static_cast<long>(total);
		/* a buffer of exactly min(total, cap) descriptors */
		const uint64_t cap = total ? rng() % (total + 1) : 0;
		auto some = exact<mdemod_packet>(cap);
		uint64_t again = 0;
		rc = mdemod_image_model_find(&o, vcdu.get(), ip, n, some.get(), cap, &again);
		if (rc != MDEMOD_OK || again != total || (cap && memcmp(some.get(), all.get(), cap * sizeof(mdemod_packet)))) FAIL("case %ld: cap %llu changes the list", i, (unsigned long long)cap);
		for (uint64_t k = 0; k < total; k++) {
			const mdemod_packet &d = all[k];
			if (d.length < 7 || d.length > 65542 || static_cast<uint64_t>(d.start) + d.length > n * IMG_ZONE || d.apid > 2047 || d.seq > 16383 || d.flags > 7 ||
			    (k && d.start < all[k - 1].start + all[k - 1].length))
				FAIL("case %ld: descriptor %llu breaks the rules (start %u, length %u)", i, (unsigned long long)k, d.start, d.length);
		}

		/* ---- decode: the found descriptors, then random ones ---- */
		for (int round = 0; round < 2; round++) {
			const uint64_t m = round ? 1 + rng() % 8 : total;
			auto desc = exact<mdemod_packet>(m);
			for (uint64_t k = 0; k < m; k++) {
				if (!round) { desc[k] = all[k]; continue; }
				desc[k].start = static_cast<uint32_t>(rng() & 1 ? rng() % (n * IMG_ZONE + 100) : rng());
				desc[k].length = static_cast<uint32_t>(rng() & 1 ? rng() % 3000 : rng());
				desc[k].apid = static_cast<uint16_t>(60 + rng() % 14);
				desc[k].seq = static_cast<uint16_t>(rng());
				desc[k].flags = static_cast<uint32_t>(rng() % 8);
			}
			auto strips = exact<uint8_t>(m * MDEMOD_IMAGE_STRIP_BYTES);
			auto sinfo = exact<mdemod_strip_info>(m);
			memset(strips.get(), 0xEE, m * MDEMOD_IMAGE_STRIP_BYTES);
			rc = mdemod_image_model_decode(&o, vcdu.get(), n, desc.get(), m, strips.get(), sinfo.get());
			if (rc != MDEMOD_OK) { if (m) FAIL("case %ld: decode refused: %s", i, mdemod_last_error()); continue; }
			for (uint64_t k = 0; k < m; k++) {
				const mdemod_strip_info &s = sinfo[k];
				const uint8_t *px = strips.get() + k * MDEMOD_IMAGE_STRIP_BYTES;
				const bool out_of_batch = desc[k].length < 7 || desc[k].length > 65542 || static_cast<uint64_t>(desc[k].start) + desc[k].length > n * IMG_ZONE;
				if (out_of_batch != (s.flags == MDEMOD_STRIP_OUTSIDE)) FAIL("case %ld: descriptor %llu outside %d, flags %u", i, (unsigned long long)k, out_of_batch, s.flags);
				if (s.mcus > 14 || ((s.flags & MDEMOD_STRIP_TRUNCATED) != 0) != (s.mcus < 14 && !(s.flags & (MDEMOD_STRIP_OUTSIDE | MDEMOD_STRIP_NOT_IMAGE))))
					FAIL("case %ld: strip %llu: %u blocks, flags %u", i, (unsigned long long)k, s.mcus, s.flags);
				if (s.bits_used > 8ull * desc[k].length) FAIL("case %ld: strip %llu used %u bits of %u bytes", i, (unsigned long long)k, s.bits_used, desc[k].length);
				for (int y = 0; y < 8; y++)
					for (int x = 8 * s.mcus; x < 112; x++)
						if (px[112 * y + x]) { FAIL("case %ld: strip %llu is not zero behind block %u", i, (unsigned long long)k, s.mcus); y = 8; break; }
				if (s.flags & MDEMOD_STRIP_TRUNCATED) truncated++;
				if (s.flags & MDEMOD_STRIP_OUTSIDE) outside++;
				if (!s.flags) decoded++;
			}
			/* ---- placement of these reports ---- */
			auto place = exact<mdemod_placement>(m);
			mdemod_place_summary sum;
			rc = mdemod_image_place(&o, desc.get(), sinfo.get(), m, place.get(), &sum);
			if (rc != MDEMOD_OK) { if (m) FAIL("case %ld: place refused: %s", i, mdemod_last_error()); continue; }
			for (uint64_t k = 0; k < m; k++)
				if (place[k].channel >= 0) {
					placed++;
					if (place[k].channel > 2 || place[k].row >= sum.rows || place[k].cell >= MDEMOD_IMAGE_CELLS || sum.rows > MDEMOD_IMAGE_MAX_ROWS)
						FAIL("case %ld: placement %llu out of the picture", i, (unsigned long long)k);
				}
		}

		/* ---- the host entry's model path: the pieces equal one batch ---- */
		mdemod_image_result res;
		rc = mdemod_image_model_host(&o, vcdu.get(), ip, n, &res);
		if (rc != MDEMOD_OK) { FAIL("case %ld: the host entry refused: %s", i, mdemod_last_error()); continue; }
		if (res.n_packets != total || (total && memcmp(res.desc, all.get(), total * sizeof(mdemod_packet)))) FAIL("case %ld: pieces of %llu frames change the list", i, (unsigned long long)o.piece_frames);
		if (res.summary.rows > 64) { /* a mutated sequence count may ask for a tall picture: allowed, only bounded */
			if (res.summary.rows > MDEMOD_IMAGE_MAX_ROWS) FAIL("case %ld: %u rows", i, res.summary.rows);
		}
		pieces++;
		mdemod_image_free(&res);
	}
	printf("{\"ok\": %s, \"cases\": %ld, \"accepted\": %ld, \"refused\": %ld, \"truncated\": %ld, \"outside\": %ld, \"decoded\": %ld, \"placed\": %ld, \"pieces\": %ld, \"bad\": %ld}\n",
	       bad ? "false" : "true", cases, accepted, refused, truncated, outside, decoded, placed, pieces, bad);
	return bad ? 1 : 0;
}
