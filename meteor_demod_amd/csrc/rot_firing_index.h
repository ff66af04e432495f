/*
 * rot_firing_index.h — the two pieces of integer bookkeeping a firing of the rotating-window kernels (rotwin_body.h) does per
 * symbol, as pure mappings: where the symbol goes in the lane's output ring, and which entry of the symbol clock's position table
 * the next firing reads.  Plain integer functions, host and device, so both are checked on the CPU (tests/test_rot_firing_index.py).
 *
 * Output ring.  A lane's ring holds RING symbols of 2 bytes in RING / 8 groups of 16 bytes, laid out [group][thread]: symbol k of
 * the ring is at byte  (k & 7) * 2 + (k >> 3) * BLOCK * 16  behind the lane's base (rot_ring_off).  The offset has two fields, bits
 * 1..3 and the bits from log2(BLOCK * 16) on, and the bits between them belong to nobody: with the gap filled, adding 2 carries out
 * of the low field straight into the high one, and masking with the two fields drops the filler and wraps the ring (rot_ring_step).
 * An offset's gap bits are zero, so filling them is an addition too: one add of GAP + 2 and one mask per symbol, and the ring is
 * full when the offset is back at 0.
 *
 * Clock table.  An entry is 16 bytes; the firing reads entry isub * 4 + j, j = how many of the first three checked steps stayed below
 * the threshold = !c1 + !c2 + !c3 (c_i: step i reached it).  The clock's increment is positive, so "reached" is monotone,
 * c1 => c2 => c3: mdemod_set_state and mdemod_set_clock_seeds (demod_api.cpp: clock_in_domain) refuse a clock word below
 * t_center - t_maxdev or a NaN, timing.c:80-86 (md_timing_update) clamps it to that range on every symbol, and a context's centre
 * is positive.  For the four monotone patterns the sum is the select cascade of rot_clock_sel, whose operands are constants; the
 * kernel carries isub scaled by the size of a table row (ROT_CLOCK_ROW_SHIFT) and reads at isub_scaled + rot_clock_sel(...).  The
 * LDS copy of the table holds the scaled isub in its third word (rot_clock_entry_scaled; the table in memory, mdemod_clock_table,
 * stays as it is).
 */
#ifndef MDEMOD_ROT_FIRING_INDEX_H
#define MDEMOD_ROT_FIRING_INDEX_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROT_IDX_HD __host__ __device__
#else
#define ROT_IDX_HD
#endif

/* ---- output ring ---- */

ROT_IDX_HD constexpr bool
rot_ring_geometry_ok(uint32_t ring, uint32_t block)
{
	return (ring == 16u || ring == 32u) && (block == 256u || block == 512u);
}

/* byte offset of a group of 8 symbols: BLOCK lanes x 16 bytes */
ROT_IDX_HD constexpr uint32_t
rot_ring_group_bytes(uint32_t block)
{
	return block * 16u;
}

/* the two fields of an offset, and the bits between them */
ROT_IDX_HD constexpr uint32_t
rot_ring_keep(uint32_t ring, uint32_t block)
{
	return 14u | ((ring / 8u - 1u) * rot_ring_group_bytes(block));
}

ROT_IDX_HD constexpr uint32_t
rot_ring_gap(uint32_t block)
{
	return rot_ring_group_bytes(block) - 16u;
}

/* where symbol number k of a call goes (k: any count, taken modulo RING) */
ROT_IDX_HD constexpr uint32_t
rot_ring_off(uint32_t k, uint32_t ring, uint32_t block)
{
	return ((k & 7u) * 2u) + (((k & (ring - 1u)) >> 3) * rot_ring_group_bytes(block));
}

/* which symbol of the ring an offset is: the inverse of rot_ring_off on 0..RING-1 */
ROT_IDX_HD constexpr uint32_t
rot_ring_count(uint32_t off, uint32_t block)
{
	return ((off >> 1) & 7u) | ((off / rot_ring_group_bytes(block)) << 3);
}

/* the offset of the next symbol; 0: the ring is full.  ((off | GAP) + 2) & KEEP, with the OR written as the addition it is for an
 * offset (gap bits zero) so that it folds into the constant */
ROT_IDX_HD constexpr uint32_t
rot_ring_step(uint32_t off, uint32_t ring, uint32_t block)
{
	return (off + (rot_ring_gap(block) + 2u)) & rot_ring_keep(ring, block);
}

/* ---- clock table ---- */

enum { ROT_CLOCK_ROW_SHIFT = 6 };       /* one isub = four entries of 16 bytes */

/* 16 * (!c1 + !c2 + !c3) for c1 => c2 => c3 */
ROT_IDX_HD constexpr uint32_t
rot_clock_sel(bool c1, bool c2, bool c3)
{
	return c1 ? 0u : (c2 ? 16u : (c3 ? 32u : 48u));
}

/* the third word of an entry as the LDS copy holds it, and back */
ROT_IDX_HD constexpr int32_t
rot_clock_entry_scaled(int32_t isub)
{
	return (int32_t)((uint32_t)isub << ROT_CLOCK_ROW_SHIFT);
}

ROT_IDX_HD constexpr int32_t
rot_clock_entry_unscaled(int32_t isub_scaled)
{
	return isub_scaled >> ROT_CLOCK_ROW_SHIFT;
}

#endif
