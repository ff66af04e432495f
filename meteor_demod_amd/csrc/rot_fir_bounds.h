/*
 * rot_fir_bounds.h — which edge half-chunks of the std window's FIR a whole wave may skip (demod_kernel_rot.hip: WinF::fir; the
 * assembly that takes the flags: gen_rotwin_asm.py).  Plain integer functions, host and device, so the mapping is checked on the
 * CPU (tests/test_rot_fir_bounds.py).
 *
 * A lane at alignment a (0..15) has its 65 taps in slots a .. a + 64 of the 80-slot window; half-chunk h is slots 4h .. 4h + 3.
 * The wave votes with three lane masks, m4 = lanes with a >= 4, m8 = a >= 8, m12 = a >= 12 (over the lanes that are in the firing:
 * `ex`, the exec mask there).  They are nested, so
 *     q_lo = min over the lanes of a / 4 = how many of the masks are all of ex,
 *     q_hi = max over the lanes of a / 4 = how many of the masks have a lane at all.
 */
#ifndef MDEMOD_ROT_FIR_BOUNDS_H
#define MDEMOD_ROT_FIR_BOUNDS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROT_FIR_HD __host__ __device__
#else
#define ROT_FIR_HD
#endif

struct RotFirQ { int q_lo, q_hi; };

ROT_FIR_HD constexpr RotFirQ
rot_fir_q(uint64_t ex, uint64_t m4, uint64_t m8, uint64_t m12)
{
	/* (nested masks: counting them is finding the first one that fails - written as selects between constants, which stay on the
	 * scalar unit; a sum of three 0/1 comparisons went through the vector unit and back) */
	return RotFirQ{ m4 != ex ? 0 : (m8 != ex ? 1 : (m12 != ex ? 2 : 3)), m4 == 0 ? 0 : (m8 == 0 ? 1 : (m12 == 0 ? 2 : 3)) };
}

/* bits 0, 1, 2: slots 0..3, 4..7, 8..11 are in front of every lane's first tap; bits 3, 4, 5: slots from 76, 72, 68 on are behind
 * every lane's last (slot a + 64) */
ROT_FIR_HD constexpr int
rot_fir_flags(int q_lo, int q_hi)
{
	return ((1 << q_lo) - 1) | (((1 << (3 - q_hi)) - 1) << 3);
}

#endif
