/*
 * sun_host.h — what the host model (csrc/sun_host.cpp, g++) and the kernel (csrc/sun.hip) of the sun layer
 * (include/meteor_demod_amd_sun.h) share, written once: the gain of a pixel from the four nodes of its cell and the corrected byte.
 * The check that is independent of this file is tests/sun_ref.py.  Free of the GPU runtime.
 */
#ifndef MDEMOD_SUN_HOST_H
#define MDEMOD_SUN_HOST_H

#include <cstddef>
#include <cstring>

#include "../../include/meteor_demod_amd_map.h"
#include "../../include/meteor_demod_amd_sun.h"

/* the pass of the public header is the map layer's, field for field */
static_assert(sizeof(mdemod_sun_orbit) == sizeof(mdemod_map_tle) && offsetof(mdemod_sun_orbit, epoch_sec) == offsetof(mdemod_map_tle, epoch_sec) &&
              offsetof(mdemod_sun_orbit, mean_motion) == offsetof(mdemod_map_tle, mean_motion), "mdemod_sun_orbit is the map layer's element set");
static_assert(sizeof(mdemod_sun_timing) == sizeof(mdemod_map_timing) && offsetof(mdemod_sun_timing, date) == offsetof(mdemod_map_timing, date) &&
              offsetof(mdemod_sun_timing, lines) == offsetof(mdemod_map_timing, lines), "mdemod_sun_timing is the map layer's line times");
static_assert(sizeof(mdemod_sun_pass_opts) == sizeof(mdemod_map_opts) && offsetof(mdemod_sun_pass_opts, time_offset) == offsetof(mdemod_map_opts, time_offset) &&
              offsetof(mdemod_sun_pass_opts, side) == offsetof(mdemod_map_opts, side) && offsetof(mdemod_sun_pass_opts, date) == offsetof(mdemod_map_opts, date) &&
              offsetof(mdemod_sun_pass_opts, piece_lines) == offsetof(mdemod_map_opts, piece_lines), "mdemod_sun_pass_opts is the map layer's options");

/* a copy of *from as its twin; NULL stays NULL (the map layer says what is missing) */
template <typename To, typename From>
inline const To *sun_twin(const From *from, To &to) { if (!from) return nullptr; memcpy(&to, from, sizeof to); return &to; }

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SUN_HD __host__ __device__ __forceinline__
#else
#define SUN_HD inline
#endif

#define SUN_WIDTH      1568u                       /* pixels of a line (MDEMOD_IMAGE_WIDTH)                          */
#define SUN_ROW_BYTES  (8u * SUN_WIDTH)            /* bytes of a strip row of one slot                               */

SUN_HD bool sun_missing(uint32_t g00, uint32_t g10, uint32_t g01, uint32_t g11)
{
	return g00 == MDEMOD_SUN_NO_NODE || g10 == MDEMOD_SUN_NO_NODE || g01 == MDEMOD_SUN_NO_NODE || g11 == MDEMOD_SUN_NO_NODE;
}

/* the two columns of nodes of a cell at line p of the strip row: (8 - p) G0 + p G1 */
SUN_HD uint32_t sun_down(uint32_t g0, uint32_t g1, uint32_t p) { return (8u - p) * g0 + p * g1; }
/* g of column q of the cell from the two: the header's sum, in the order (16 - q) left + q right */
SUN_HD uint32_t sun_across(uint32_t left, uint32_t right, uint32_t q) { return ((16u - q) * left + q * right + 64u) >> 7; }
/* t of the header: the corrected value before it is held at 255 */
SUN_HD uint32_t sun_scaled(uint32_t v, uint32_t g) { return (v * g + 32768u) >> 16; }

/* The arguments of the apply entries: MDEMOD_OK, or MDEMOD_ERR_PARAM with the text noted.  `saturated`: the model's counts, which
 * the device entry has in its workspace. */
int  sun_check_apply(const char *who, const uint8_t *const image[3], uint8_t *const out[3], uint32_t slot_mask, uint32_t rows, const uint32_t *gain,
                     const void *work, uint64_t work_bytes, bool has_work);
/* What mdemod_sun_correct_host does before the device: checks, line times, nodes (gain: (rows + 1) x 99 words of the caller's) and
 * the slot mask of the APIDs into summary->slot_mask. */
int  sun_prepare(const char *who, const mdemod_sun_opts *sun_opts, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_orbit *orbit, uint8_t *const image[3],
                 const uint32_t apids[3], uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, uint32_t *gain,
                 mdemod_sun_summary *summary);

extern "C" {

/* ---- the host model: what the kernel of csrc/sun.hip must compute, byte for byte (exported for the tests) ---- */

/* The slots of slot_mask of image[3] (host memory) through gain[rows + 1][99] into out[3] (out[k] may be image[k]); saturated[3]
 * (may be NULL) receives the counts, 0 for a slot that is not selected. */
int  mdemod_sun_model_apply(const uint8_t *const image[3], uint8_t *const out[3], uint32_t slot_mask, uint32_t rows, const uint32_t *gain, uint64_t saturated[3]);
/* mdemod_sun_correct_host with the model in the kernel's place (no device). */
int  mdemod_sun_model_host(const mdemod_sun_opts *sun_opts, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_orbit *orbit, uint8_t *const image[3],
                           const uint32_t apids[3], uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc,
                           mdemod_sun_summary *summary);

}

#endif
