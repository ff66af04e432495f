/*
 * buffers_test.cpp — stand-alone check of csrc/buffers.h (MdmBuffers: every output apart from every input and from every other
 * output), built with ASan + UBSan by tests/test_buffers_sanitize.py.  The ranges are never dereferenced: they are offsets into one
 * array that exists.  Prints one JSON line; the exit status is the number of wrong answers (at most 100).
 */
#include <cstdio>
#include <cstdint>

#include "buffers.h"

static int bad = 0, checks = 0;

static void
expect(const char *what, bool got, bool want)
{
	checks++;
	if (got != want) { bad++; fprintf(stderr, "%s: apart() is %d, not %d\n", what, got, want); }
}

int
main()
{
	static uint8_t mem[1 << 16];
	uint8_t *const A = mem + 4096, *const B = mem + 16384, *const C = mem + 32768;

	expect("nothing at all", MdmBuffers().apart(), true);
	expect("one output", MdmBuffers().out(A, 100).apart(), true);
	expect("an output far from an input", MdmBuffers().in(A, 100).out(B, 100).apart(), true);
	/* an output against an input: the same range, one inside the other, either order of the calls */
	expect("an output that is an input", MdmBuffers().in(A, 100).out(A, 100).apart(), false);
	expect("an output inside an input", MdmBuffers().in(A, 1000).out(A + 10, 5).apart(), false);
	expect("an input inside an output", MdmBuffers().out(A, 1000).in(A + 10, 5).apart(), false);
	/* an output against a second output */
	expect("two outputs that are one", MdmBuffers().out(A, 100).out(A, 100).apart(), false);
	expect("the third output in the first", MdmBuffers().in(C, 8).out(A, 100).out(B, 100).out(A + 99, 100).apart(), false);
	expect("three outputs apart", MdmBuffers().in(C, 8).out(A, 100).out(B, 100).out(A + 100, 100).apart(), true);
	/* inputs may alias */
	expect("two inputs that are one", MdmBuffers().in(A, 100).in(A, 100).in(A + 50, 100).out(B, 100).apart(), true);
	/* a range that is not there joins nothing */
	expect("a NULL output", MdmBuffers().in(A, 100).out(nullptr, 100).apart(), true);
	expect("a NULL input", MdmBuffers().in(nullptr, ~0ull).out(A, 100).apart(), true);
	expect("an empty output in an input", MdmBuffers().in(A, 100).out(A + 10, 0).apart(), true);
	expect("an empty input in an output", MdmBuffers().in(A + 10, 0).out(A, 100).apart(), true);
	expect("an empty output in an output", MdmBuffers().out(A, 100).out(A + 10, 0).apart(), true);
	expect("NULL and empty among real ones", MdmBuffers().in(nullptr, 0).out(nullptr, 0).in(A, 16).out(B, 16).out(A, 0).apart(), true);
	/* ranges that only touch */
	expect("an input ends where an output starts", MdmBuffers().in(A, 100).out(A + 100, 100).apart(), true);
	expect("an output ends where an input starts", MdmBuffers().out(A, 100).in(A + 100, 100).apart(), true);
	expect("an output ends where an output starts", MdmBuffers().out(A, 100).out(A + 100, 100).apart(), true);
	/* one byte of overlap at either end */
	expect("the last byte of an input", MdmBuffers().in(A, 100).out(A + 99, 100).apart(), false);
	expect("the first byte of an input", MdmBuffers().in(A + 99, 100).out(A, 100).apart(), false);
	expect("the last byte of an output", MdmBuffers().out(A, 100).out(A + 99, 100).apart(), false);
	expect("the first byte of an output", MdmBuffers().out(A + 99, 100).out(A, 100).apart(), false);
	expect("ranges of one byte, the same", MdmBuffers().in(A, 1).out(A, 1).apart(), false);
	expect("ranges of one byte, neighbours", MdmBuffers().in(A, 1).out(A + 1, 1).apart(), true);

	/* dozens of inputs, as mosaic builds: 8 passes of 8 ranges, aliasing each other, and three outputs behind them */
	for (int hit = -1; hit < 64; hit++) {
		MdmBuffers b;
		for (int k = 0; k < 64; k++) b.in(mem + 128 * k, 192);                  /* (each reaches into the next) */
		b.in(nullptr, 64).in(mem, 0);
		b.out(B, 1000).out(B + 1000, 1000).out(B + 2000, 1000);
		expect("64 inputs, the outputs behind them", b.apart(), true);
		if (hit < 0) continue;
		b.out(mem + 128 * hit + 191, 1);                                        /* the last byte of input `hit` */
		expect("64 inputs, a fourth output in one of them", b.apart(), false);
	}
	{
		MdmBuffers b;
		for (int k = 0; k < 64; k++) b.in(mem + 128 * k, 128);
		b.out(mem + 128 * 64, 128);                                              /* touches the last input */
		expect("64 inputs, an output that touches the last", b.apart(), true);
		b.in(mem + 128 * 65 - 1, 1);
		expect("a 65th input on the output's last byte", b.apart(), false);
	}
	printf("{\"ok\": %s, \"checks\": %d, \"bad\": %d}\n", bad ? "false" : "true", checks, bad);
	return bad > 100 ? 100 : bad;
}
