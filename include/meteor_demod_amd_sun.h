/*
 * meteor_demod_amd_sun.h — the visible channels normalised by the sun's zenith angle: the counts of a reflective channel fall with
 * the cosine of the zenith angle of the sun at the ground, and this layer takes that factor out of the swath pictures
 * (include/meteor_demod_amd_image.h: uint8 [8 rows][1568] per slot) before any derived picture is made of them, so that the picture,
 * map, mosaic and polar layers take corrected buffers as they are.  The sun's position and the grid of gain nodes are host code in
 * double precision; the gain is applied on the GPU.  The apply is stated in integers; its specification is a host model
 * (csrc/sun_host.cpp, exported as mdemod_sun_model_apply): GPU bytes and counts equal model bytes and counts.  `>>` is a floor, and
 * values are 32-bit unless stated otherwise.
 *
 *   sun         host, double.  date = days since 1970-01-01, utc = seconds of that day (any real number: it may be negative or
 *               above 86 400).  n = (date - 10 957) + (utc - 43 200) / 86 400, the days since J2000.0.  L = 280.460 + 0.9856474 n,
 *               g = 357.528 + 0.9856003 n, lambda = L + 1.915 sin g + 0.020 sin 2g, eps = 23.439 - 0.0000004 n, all in degrees.
 *               The inertial unit vector to the sun is (cos lambda, cos eps sin lambda, sin eps sin lambda).
 *   Earth-fixed the map layer's rotation (include/meteor_demod_amd_map.h, orbit): x' = x cos G + y sin G, y' = -x sin G + y cos G,
 *               z' = z with G = (280.46061837 + 360.98564736629 n) mod 360 degrees and the same n: both layers share one Earth
 *               rotation.  mdemod_sun_position gives this vector.
 *   cos z       at a ground point of geodetic latitude lat and longitude lon (degrees): the dot product of that vector with the
 *               geodetic normal (cos lat cos lon, cos lat sin lon, sin lat).  The sun's parallax, the refraction and the height of
 *               the ground are left out.
 *   nodes       a picture of `rows` strip rows has the gain nodes (a, b), a = 0 .. rows, b = 0 .. 98: uint32 [rows + 1][99].  Node
 *               (a, b) sits at line 8 a, column 16 b: the last row and the last column of nodes lie one past the picture.  Its
 *               latitude and longitude are the map layer's forward geolocation (`look` in its header); the UTC of its line is the
 *               map layer's too, s0 + y row_period / 8 - time_offset on the date that layer resolves.  A node that is not visible
 *               (NaN from the geolocation: possible when scan_deg exceeds about 124 degrees) is MDEMOD_SUN_NO_NODE.
 *   gain        c = cos z at the node, cl = cos(limit_deg), cr = cos(ref_deg): G = floor(65 536 cr / max(c, cl) + 0.5).  limit_deg
 *               60 .. 89 (default 85): beyond it the gain grows no further, and the night stays dark.  ref_deg 0 .. 80 (default
 *               45): the zenith angle at which the counts stay as they are.  It is fixed, and not taken from the pass, so that every
 *               pass of a mosaic lands on one scale.  Within these ranges G <= 65 536 / cos 89 < 2^22.
 *   apply       the kernel.  Pixel (y, x) of a slot: a = y >> 3, p = y & 7, b = x >> 4, q = x & 15; G00 = G[a][b], G10 = G[a + 1][b],
 *               G01 = G[a][b + 1], G11 = G[a + 1][b + 1].  One of the four MDEMOD_SUN_NO_NODE: the pixel's byte is copied unchanged.
 *               Otherwise g = ((8 - p)(16 - q) G00 + p (16 - q) G10 + (8 - p) q G01 + p q G11 + 64) >> 7, and for every selected
 *               slot with byte v: t = (v g + 32 768) >> 16, out = min(255, t).  The weights sum to 128: with G < 2^22 the sum is
 *               below 2^29 + 64 and v g below 2^30; nothing needs 64 bits.  (A table with words of 2^22 and more that are not the
 *               marker is applied in the same 32-bit arithmetic, wrapping; the model does the same.)  An unfilled cell holds 0
 *               and stays 0: the `filled` masks are neither read nor changed.
 *   slots       slot_mask, 1 .. 7: bit k selects slot k.  Only selected slots are read, corrected and written; of the others not
 *               even the pointers are looked at.  The host entry and the CLI select the slots whose APID is 64, 65 or 66, the
 *               reflective channels; a thermal channel's counts do not depend on the sun and stay as decoded.
 *   saturated   per selected slot, the number of pixels with t > 255.  The kernel leaves per-block partial counts in the
 *               workspace, uint32 [rows][3] (one block per strip row; 0 for a slot that is not selected), and the host adds them:
 *               no global atomics, and the total is exact.
 *   in place    out[k] may be image[k] itself.  Nothing else may intersect: no output another output, another slot's input, the
 *               gain table or the workspace.
 *   refused     MDEMOD_ERR_PARAM, text in mdemod_last_error, nothing written: rows outside 1 .. 8192, a slot mask outside 1 .. 7, a
 *               missing pointer of a selected slot, of the table or of the workspace, a pointer that is no multiple of 4 bytes, a
 *               workspace below mdemod_sun_workspace(rows), ranges that intersect other than in place, limit_deg or ref_deg out of
 *               range or not a number, and whatever the map layer refuses of the orbit, the line times and its options.
 *
 *   to be confirmed off air   no recording stands behind this layer yet.  The first passes with a low sun confirm or replace: that
 *               the counts are proportional to the radiance with a dark level of zero (a dark level d wants (v - d) g + d), that
 *               45 degrees is a sensible reference (mid-latitude passes around noon should keep their brightness), and that APIDs
 *               64 .. 66 are the reflective channels of the sender in use (a sender that switches a thermal channel onto one of
 *               them wants that slot left out: `slots=` in Python).
 */
#ifndef METEOR_DEMOD_AMD_SUN_H
#define METEOR_DEMOD_AMD_SUN_H

#include "meteor_demod_amd_picture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_SUN_NO_NODE     0xFFFFFFFFu
#define MDEMOD_SUN_NODE_COLS   99         /* 1568 / 16 + 1                                                                        */
#define MDEMOD_SUN_MAX_ROWS    8192       /* the map layer's                                                                      */
#define MDEMOD_SUN_MIN_LIMIT   60.0
#define MDEMOD_SUN_MAX_LIMIT   89.0
#define MDEMOD_SUN_MAX_REF     80.0

/* The orbit, the line times and the options of a pass are the map layer's (include/meteor_demod_amd_map.h): its element set as its
 * TLE parser fills it, its line times as its time fit leaves them, and its options.  They are repeated here field for field, as
 * the mosaic layer repeats them, so that this header stands without that one; a pointer to the map layer's struct may be passed
 * as a pointer to its twin here (the library copies the bytes and asserts at compile time that the layouts are the same). */
typedef struct {
	uint32_t norad;               /* catalogue number                                                                                 */
	int32_t  epoch_day;           /* days since 1970-01-01 of the epoch                                                               */
	double   epoch_sec;           /* seconds of that day                                                                              */
	double   inclination_deg, raan_deg, eccentricity, argp_deg, mean_anomaly_deg;
	double   mean_motion;         /* revolutions per day                                                                              */
} mdemod_sun_orbit;

typedef struct {
	double   row_period;          /* seconds per strip row                                                                            */
	double   s0;                  /* onboard seconds of the day of line 0                                                             */
	int32_t  date;                /* days since 1970-01-01, or INT32_MIN: the date nearest the epoch                                  */
	uint32_t rows_fit, placed, lines;
} mdemod_sun_timing;

typedef struct {
	double   scan_deg;            /* 110.0: the full scan angle, 1 .. 130                                                             */
	double   px_per_deg;          /* (the map's scale: not used here)                                                                 */
	double   time_offset;         /* 10 800.0: onboard clock minus UTC in seconds                                                     */
	double   row_period;          /* 8 / 6.5: seconds per strip row where the stamps cannot say                                       */
	int32_t  side;                /* +1 or -1                                                                                         */
	int32_t  date;                /* days since 1970-01-01, or INT32_MIN                                                              */
	uint32_t stretch, clip_low, clip_high, piece_lines;   /* (the map's: checked as that layer checks them, not used here)            */
} mdemod_sun_pass_opts;

typedef struct {
	double   limit_deg;           /* 85.0: the zenith angle beyond which the gain grows no further, 60 .. 89                          */
	double   ref_deg;             /* 45.0: the zenith angle whose counts stay as they are, 0 .. 80                                    */
	uint32_t reserved[4];         /* 0                                                                                                */
} mdemod_sun_opts;

typedef struct {
	double   zenith_min, zenith_max;  /* degrees, over the visible nodes (both 0 when there is none)                                  */
	uint32_t nodes;               /* (rows + 1) x 99                                                                                  */
	uint32_t missing;             /* nodes that are MDEMOD_SUN_NO_NODE                                                                */
	uint32_t at_limit;            /* visible nodes with cos z < cos(limit_deg)                                                        */
	uint32_t slot_mask;           /* the slots that were corrected (mdemod_sun_correct_host; 0 from mdemod_sun_nodes)                 */
	int32_t  date;                /* the date that was used, days since 1970-01-01                                                    */
	uint32_t reserved;
	uint64_t saturated[3];        /* per slot: pixels that t > 255 held at 255 (mdemod_sun_correct_host)                              */
} mdemod_sun_summary;

/* limit_deg 85, ref_deg 45. */
void mdemod_sun_default_opts(mdemod_sun_opts *opts);

/* Host only: the Earth-fixed unit vector to the sun at second `utc` of day `date`. */
int  mdemod_sun_position(int32_t date, double utc, double out[3]);

/* Host only: out[k] = cos z at (lat[k], lon[k]) (degrees) at second utc[k] of day `date`. */
int  mdemod_sun_cos_zenith(int32_t date, const double *utc, const double *lat, const double *lon, uint64_t n, double *out);

/* Host only: the gain nodes gain[rows + 1][99] of a pass (pass_opts, sun_opts NULL: the defaults).  *summary (may be NULL) receives
 * the zenith range, the counts of nodes and the date. */
int  mdemod_sun_nodes(const mdemod_sun_orbit *orbit, const mdemod_sun_timing *timing, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_opts *sun_opts,
                      uint32_t rows, uint32_t *gain, mdemod_sun_summary *summary);

/* Bytes of workspace for a picture of `rows` strip rows (12 bytes a strip row); 0 for rows out of range. */
uint64_t mdemod_sun_workspace(uint32_t rows);

/* The slots of slot_mask of image_dev through gain_dev[rows + 1][99] into out_dev (out_dev[k] may be image_dev[k]), the partial
 * counts into work_dev[work_bytes].  Device memory at multiples of 4 bytes.  Queued on hip_stream of `device`; asynchronous.  Nothing
 * outside the selected inputs and the table is read, nothing outside the selected outputs and the first mdemod_sun_workspace(rows)
 * bytes of the workspace is written. */
int  mdemod_sun_apply_device(const uint8_t *const image_dev[3], uint8_t *const out_dev[3], uint32_t slot_mask, uint32_t rows, const uint32_t *gain_dev,
                             void *work_dev, uint64_t work_bytes, int device, void *hip_stream);

/* Pictures in host memory, in place: the line times from the packets' placements and reports (the map layer's time fit), the nodes, and
 * the slots k whose apids[k] is 64, 65 or 66 through the kernel on `device`.  Synchronous.  rows = 0, or no such slot: nothing to
 * do.  *summary (may be NULL) receives everything. */
int  mdemod_sun_correct_host(const mdemod_sun_opts *sun_opts, const mdemod_sun_pass_opts *pass_opts, const mdemod_sun_orbit *orbit, uint8_t *const image[3],
                             const uint32_t apids[3], uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc,
                             mdemod_sun_summary *summary, int device);

#ifdef __cplusplus
}
#endif
#endif
