/*
 * buffers.h — the byte ranges of a device entry and the one rule about them: every output apart from every input and from every
 * other output (the blocks of a launch would read what others write).  Free of the GPU runtime.
 */
#ifndef MDEMOD_BUFFERS_H
#define MDEMOD_BUFFERS_H

#include <cstdint>
#include <vector>

/* Do two byte ranges overlap?  A range that is not there (NULL, or no bytes) overlaps nothing. */
inline bool
mdm_ranges_intersect(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
	const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
	return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

/* What an entry reads (in) and what it writes (out; a buffer it reads and writes is an output).  Inputs may alias each other. */
struct MdmBuffers {
	struct Range { const void *p; uint64_t bytes; };
	std::vector<Range> ins, outs;

	MdmBuffers &in(const void *p, uint64_t bytes) { ins.push_back({ p, bytes }); return *this; }
	MdmBuffers &out(const void *p, uint64_t bytes) { outs.push_back({ p, bytes }); return *this; }

	bool apart() const
	{
		for (size_t o = 0; o < outs.size(); o++) {
			for (const Range &i : ins)
				if (mdm_ranges_intersect(outs[o].p, outs[o].bytes, i.p, i.bytes)) return false;
			for (size_t j = 0; j < o; j++)
				if (mdm_ranges_intersect(outs[o].p, outs[o].bytes, outs[j].p, outs[j].bytes)) return false;
		}
		return true;
	}
};

#endif
