/*
 * pll_flags.h — the lock detector's flag arithmetic and the sweep's turn-round (pll.c:117-128) as a pure integer mapping on the
 * packed flag word (demod_device.h: md_pll_update_packed).  Plain integer functions, host and device, so the mapping and the
 * predicate that lets a whole wave skip it are checked on the CPU (tests/test_pll_flags_host.py).
 *
 * fl: bit 0 locked, bit 1 locked_once, bit 2 updown > 0 (the layout of the state array).  below = err < 85, above = err > 105 (0 / 1;
 * they exclude each other).  The frequency case is where freq stands AFTER the sweep's +-1e-6 step and BEFORE the clamp: inside
 * (-fmax, fmax), >= fmax, or <= -fmax (a NaN compares false both times: inside).
 */
#ifndef MDEMOD_PLL_FLAGS_H
#define MDEMOD_PLL_FLAGS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PLL_FLAGS_HD __host__ __device__
#else
#define PLL_FLAGS_HD
#endif

enum { PLL_FREQ_INSIDE = 0, PLL_FREQ_HIGH = 1, PLL_FREQ_LOW = 2 };

struct PllFlagStep { uint32_t fl, first, changed; };      /* first: bit 1 set = the first lock ever; changed: bit 0 set = `locked` flipped */

/* `locked` after pll.c:117-123, which is what the sweep (pll.c:125) asks: a locked loop stays locked unless err is above 105, an
 * unlocked one locks when err is below 85.  Equal to bit 0 of pll_flags_step(...).fl for every input. */
PLL_FLAGS_HD constexpr bool
pll_flags_locked_after(uint32_t fl, uint32_t below, uint32_t above)
{
	return (fl & 1u) ? !(above & 1u) : (below & 1u) != 0;
}

/* Can the symbol change anything in fl, or report a lock event?  False: pll_flags_step is the identity with first = changed = 0. */
PLL_FLAGS_HD constexpr bool
pll_flags_event(uint32_t fl, uint32_t below, uint32_t above, int freq_case)
{
	return ((below & ~fl & 1u) | (above & fl & 1u)) != 0 || freq_case != PLL_FREQ_INSIDE;
}

PLL_FLAGS_HD constexpr PllFlagStep
pll_flags_step(uint32_t fl, uint32_t below, uint32_t above, int freq_case)
{
	/* pll.c:117-123: lock below 85, unlock above 105 */
	const uint32_t lock_now = below & (fl ^ 1u);                            /* bit 0: locks on this symbol            */
	const uint32_t unlock_now = above & fl;                                 /* bit 0: unlocks on this symbol          */
	const uint32_t lock2 = lock_now + lock_now;                             /* the same in bit 1                      */
	const uint32_t first = lock2 ^ (lock2 & fl);                            /* bit 1: locks and never had before      */
	fl = fl | lock_now | lock2;                                             /* locked = locked_once = 1               */
	fl = fl ^ (fl & unlock_now);                                            /* locked = 0                             */
	/* pll.c:126-127: turn round at +-fmax */
	fl = freq_case == PLL_FREQ_HIGH ? (fl & ~4u) : (freq_case == PLL_FREQ_LOW ? (fl | 4u) : fl);
	return PllFlagStep{ fl, first, lock_now | unlock_now };
}

#endif
