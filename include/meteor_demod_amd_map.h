/*
 * meteor_demod_amd_map.h — from swath pictures (include/meteor_demod_amd_image.h), the onboard time stamps of their packets and a
 * two-line element set to a north-up picture on a regular latitude / longitude grid (EPSG:4326), contrast-stretched as the picture
 * layer does it (include/meteor_demod_amd_picture.h).  Orbit, time fit, geolocation and the grid of nodes are host code in double
 * precision; the warp runs on the GPU.  The specification of the kernel is a host model in integer arithmetic
 * (csrc/map_host.cpp, exported as mdemod_map_model_*): GPU bytes equal model bytes.
 *
 *   constants   mu = 398600.4418 km^3/s^2, Re = 6378.137 km, f = 1 / 298.257223563 (b = Re (1 - f), e^2 = f (2 - f)),
 *               J2 = 1.08262668e-3.  Angles in radians inside, degrees at the interface.
 *   TLE         two lines of 69 characters, an optional name line before them; columns counted from 1.  Line 1: '1' in column 1,
 *               catalogue number 3 .. 7, epoch year 19 .. 20 (below 57: 20yy, otherwise 19yy), epoch day of the year with
 *               fraction 21 .. 32 (1.0 is 1 January 0 h), checksum 69.  Line 2: '2' in column 1, catalogue number 3 .. 7,
 *               inclination 9 .. 16, RAAN 18 .. 25, eccentricity 27 .. 33 (a decimal point before it), argument of perigee
 *               35 .. 42, mean anomaly 44 .. 51 (all degrees), mean motion 53 .. 63 (revolutions per day), checksum 69.  A
 *               checksum is the sum of the digits of columns 1 .. 68 plus one per '-', modulo 10.  In a text with several sets the
 *               first is taken, or the one with the catalogue number asked for.  Refused (MDEMOD_ERR_PARAM, text in
 *               mdemod_last_error): a line 1 or 2 shorter than 69 characters, a line 1 not followed by a line 2 (or a line 2
 *               without its line 1), catalogue numbers that differ or are not numbers, a wrong checksum, a field that is not a
 *               number or out of range (inclination 0 .. 180, eccentricity below 1, mean motion 0.5 .. 20), no set with the
 *               number asked for.
 *   orbit       a circular orbit with the secular J2 terms.  THIS IS NOT SGP4.  n = mean motion in rad/s, a = (mu / n^2)^(1/3),
 *               k = 1.5 J2 (Re / a)^2 n.  With dt seconds since the epoch: Omega = Omega0 - k cos i dt,
 *               u = omega0 + M0 + (n + 0.5 k (5 cos^2 i - 1)) dt.  Inertial unit vectors
 *                 r = ( cos Omega cos u - sin Omega sin u cos i,  sin Omega cos u + cos Omega sin u cos i, sin u sin i)
 *                 v = (-cos Omega sin u - sin Omega cos u cos i, -sin Omega sin u + cos Omega cos u cos i, cos u sin i)
 *                 h = r x v = (sin Omega sin i, -cos Omega sin i, cos i);   the satellite sits at a r.
 *               Inertial to Earth-fixed: x' = x cos g + y sin g, y' = -x sin g + y cos g, z' = z with
 *               g = (280.46061837 + 360.98564736629 d) mod 360 degrees, d = days since J2000.0 (2000-01-01 12 h) formed as
 *               (whole days) + (seconds of the day - 43 200) / 86 400.
 *               Left out: the eccentricity (the satellite is up to 2 a e before or behind along the track: 7 to 15 km for this
 *               family, e about 0.0005 .. 0.001), the short-period terms of J2, the difference between TEME and true of date,
 *               and the attitude of the spacecraft.
 *   look        pixel (y, x): line y, column x, both may be fractional and outside the picture.  theta = (x - 783.5) D,
 *               D = scan_deg / 1568 in radians (the picture layer's D).  look = -cos theta r + side sin theta h at the line's time,
 *               side = +1 or -1.  The ray satellite + t look against (x^2 + y^2) / Re^2 + z^2 / b^2 = 1 in Earth-fixed
 *               coordinates: the nearer root; no real root, or a root behind the satellite: not visible (NaN).  For the point:
 *               lat = atan2(z, (1 - e^2) hypot(x, y)), lon = atan2(y, x).
 *   line times  from the placed packets (channel >= 0), in list order: the point (row, s), s = ms / 1000 + us / 1e6, 86 400 added
 *               or taken where s differs from the first point's by more than 43 200 (midnight).  Each row is represented by
 *               its first placed packet; over the rows in ascending order, row_period is the median of
 *               (s_b - s_a) / (row_b - row_a) of neighbouring rows (the mean of the two middle values of an even count).
 *               Fewer than two rows: opts.row_period.  s0 is the median of s - row row_period over all placed packets, reduced
 *               to 0 .. 86 400 (whole days taken off).  Line y
 *               has the onboard time s0 + y row_period / 8, and UTC = date + that - time_offset.  date counts days from
 *               1970-01-01; MDEMOD_MAP_DATE_AUTO is the date that puts line lines / 2 nearest the TLE's epoch.
 *   grid        sy = px_per_deg (1 .. 1000) pixels per degree of latitude, sx = max(1, round(sy cos lat_mid)) per degree of
 *               longitude, lat_mid the middle of the latitude range.  The range is that of the swath's border: lines 0, 8, 16 ..
 *               and the last, columns 0, 16, 32 .. and 1567, along the four edges.  Longitudes relative to that of pixel
 *               ((lines - 1) / 2, 783.5), wrapped to +-180.  lat_top = ceil(max lat sy) / sy, lon_left = floor(min lon sx) / sx,
 *               H = ceil((lat_top - min lat) sy), W = ceil((max lon - lon_left) sx) rounded up to a multiple of 4.  Pixel
 *               (i, j), row i, column j, has its centre at lat_top - (i + 0.5) / sy and lon_left + (j + 0.5) / sx.  Refused: a
 *               border sample that is not visible or beyond 85 degrees of latitude (a polar pass wants another projection),
 *               W > 8192 or H > 16 384 (the text names a scale that fits), more than 8192 strip rows.
 *   nodes       int32 [ceil(H / 16) + 1][ceil(W / 16) + 1][2]: node (a, b) holds X = round(256 x), Y = round(256 y) of the
 *               source pixel that sees the centre of output pixel (16 a, 16 b), solved up to 5 degrees of scan angle beyond
 *               either edge and 120 s before line 0 and after the last line.  Both words MDEMOD_MAP_NO_NODE where the point is
 *               not visible, beyond that margin, or the solve does not converge.
 *   warp        integers; >> is a floor; as if in 64 bits.  Output pixel (i, j): cell (i >> 4, j >> 4), p = i & 15, q = j & 15,
 *               X00 the node (i >> 4, j >> 4), X10 one node down, X01 one to the right, X11 both.  A missing corner: the pixel
 *               is empty.  X = ((16 - p)(16 - q) X00 + p (16 - q) X10 + (16 - p) q X01 + p q X11 + 128) >> 8, Y likewise.
 *               Empty unless 0 <= X <= 1567 * 256 and 0 <= Y <= (8 rows - 1) * 256.  ix = X >> 8, fx = X & 255,
 *               ix2 = min(ix + 1, 1567); iy, fy, iy2 likewise with 8 rows - 1.  Tap (y, x) of slot s is filled when
 *               filled_s[y / 8][x / 112] != 0.  Along line iy (and iy2): both taps filled: (a (256 - fx) + b fx + 128) >> 8; one:
 *               its value; none: the line does not count.  Across the lines the same rule with fy.  No line counts: the byte
 *               is 0, the table is not applied, the plane's valid bit stays clear; otherwise the byte is lut[p][v].  Empty
 *               pixels are 0 in every plane and in valid.
 *   outputs     out uint8 [H][W][planes], planes 1 or 3, select[p] the slot of plane p; valid uint8 [H][W], optional, bit p:
 *               plane p had a filled tap.
 *   world file  six lines: 1 / sx, 0, 0, -1 / sy, lon_left + 0.5 / sx, lat_top - 0.5 / sy.
 *
 *   to be confirmed off air   no recording stands behind this layer yet.  The first geolocated pass with coastlines confirms or
 *               replaces: the time offset (10 800 s: the onboard clock is taken to run on Moscow time), that a packet's stamp is
 *               the time of its strip row's first line, the sign of `side` (which way the mirror turns), the line rate (6.5 lines
 *               per second, the fallback of the fit), and whether column 783.5 is the nadir.
 */
#ifndef METEOR_DEMOD_AMD_MAP_H
#define METEOR_DEMOD_AMD_MAP_H

#include "meteor_demod_amd_picture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_MAP_NODE_STEP     16
#define MDEMOD_MAP_NO_NODE       INT32_MIN
#define MDEMOD_MAP_MAX_WIDTH     8192
#define MDEMOD_MAP_MAX_HEIGHT    16384
#define MDEMOD_MAP_MAX_ROWS      8192
#define MDEMOD_MAP_DEFAULT_PIECE 1024
#define MDEMOD_MAP_DATE_AUTO     INT32_MIN
#define MDEMOD_MAP_MAX_LAT       85.0
#define MDEMOD_MAP_SCAN_MARGIN   5.0      /* degrees of scan angle a node is solved beyond either edge                            */
#define MDEMOD_MAP_TIME_MARGIN   120.0    /* seconds before the first and after the last line                                    */

typedef struct {
	uint32_t norad;               /* catalogue number                                                                                 */
	int32_t  epoch_day;           /* days since 1970-01-01 of the epoch                                                               */
	double   epoch_sec;           /* seconds of that day                                                                              */
	double   inclination_deg, raan_deg, eccentricity, argp_deg, mean_anomaly_deg;
	double   mean_motion;         /* revolutions per day                                                                              */
} mdemod_map_tle;

typedef struct {
	double   scan_deg;            /* 110.0: the full scan angle, 1 .. 130                                                             */
	double   px_per_deg;          /* 100.0: 1 .. 1000                                                                                 */
	double   time_offset;         /* 10 800.0: onboard clock minus UTC in seconds, -86 400 .. 86 400                                  */
	double   row_period;          /* 8 / 6.5: seconds per strip row where the stamps cannot say (0.1 .. 10)                           */
	int32_t  side;                /* +1 or -1                                                                                         */
	int32_t  date;                /* days since 1970-01-01, or MDEMOD_MAP_DATE_AUTO                                                   */
	uint32_t stretch;             /* 1; 0: identity tables                                                                            */
	uint32_t clip_low, clip_high; /* 5 and 5 permille, as in the picture layer                                                        */
	uint32_t piece_lines;         /* mdemod_map_compose_host makes bands of this many output lines: 0 = 1024, a multiple of 16        */
} mdemod_map_opts;

typedef struct {
	double   row_period;          /* seconds per strip row                                                                            */
	double   s0;                  /* onboard seconds of the day of line 0                                                             */
	int32_t  date;                /* opts.date (MDEMOD_MAP_DATE_AUTO is resolved against a TLE by mdemod_map_date)                    */
	uint32_t rows_fit;            /* rows the period rests on (below 2: the fallback)                                                 */
	uint32_t placed;              /* placed packets s0 rests on                                                                       */
	uint32_t lines;               /* 8 x (the largest placed row + 1)                                                                 */
} mdemod_map_timing;

typedef struct {
	uint32_t width, height;       /* W, H                                                                                             */
	uint32_t sx;                  /* pixels per degree of longitude                                                                   */
	uint32_t node_rows, node_cols;
	int32_t  date;                /* the date that was used                                                                           */
	double   sy;                  /* pixels per degree of latitude                                                                    */
	double   lat_top, lon_left;   /* the outer edges of pixel (0, 0), degrees; lon_left in -180 .. 180                                */
	int32_t *nodes;               /* [node_rows][node_cols][2]: X, Y                                                                  */
} mdemod_map_nodes;

/* What mdemod_map_compose_host returns: pixels, valid are malloc'ed, and mdemod_map_free gives them back. */
typedef struct {
	uint32_t width, height, planes, sx;
	double   sy, lat_top, lon_left;
	mdemod_map_timing timing;     /* date resolved                                                                                    */
	double   utc0;                /* UTC seconds of day `timing.date` of line 0 (may be negative or above 86 400)                     */
	uint32_t lo[3], hi[3];        /* the stretch limits of each plane                                                                 */
	uint64_t valid_pixels;        /* non-zero bytes of valid                                                                          */
	uint8_t *pixels;              /* [height][width][planes]                                                                          */
	uint8_t *valid;               /* [height][width]                                                                                  */
} mdemod_map_result;

/* scan 110, 100 px/deg, offset 10 800, row_period 8 / 6.5, side +1, date auto, stretch 1, clips 5 and 5, piece_lines 0. */
void mdemod_map_default_opts(mdemod_map_opts *opts);

/* Host only.  text: a NUL-terminated TLE file; norad 0: the first set. */
int  mdemod_map_parse_tle(const char *text, uint32_t norad_or_0, mdemod_map_tle *tle);

/* Host only: the line times from the placed packets.  No placed packet: MDEMOD_ERR_PARAM. */
int  mdemod_map_fit_time(const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const mdemod_map_opts *opts,
                         mdemod_map_timing *timing);

/* Host only: *date := timing->date, or for MDEMOD_MAP_DATE_AUTO the date nearest the TLE's epoch. */
int  mdemod_map_date(const mdemod_map_tle *orbit, const mdemod_map_timing *timing, const mdemod_map_opts *opts, int32_t *date);

/* Host only, the forward function: pixel (y[k], x[k]) to lat[k], lon[k] in degrees, NaN where not visible. */
int  mdemod_map_geolocate(const mdemod_map_tle *orbit, const mdemod_map_timing *timing, const mdemod_map_opts *opts, const double *y, const double *x,
                          uint64_t n, double *lat, double *lon);

/* Host only: the grid and its nodes for a picture of `lines` lines (a multiple of 8).  *grid is overwritten; mdemod_map_grid_free. */
int  mdemod_map_grid(const mdemod_map_tle *orbit, const mdemod_map_timing *timing, const mdemod_map_opts *opts, uint32_t lines, mdemod_map_nodes *grid);
void mdemod_map_grid_free(mdemod_map_nodes *grid);

/* The slots select[0 .. planes - 1] (host memory, each 0 .. 2, planes 1 or 3) through nodes_dev[ceil(height / 16) + 1][ceil(width / 16) + 1][2]
 * and lut_dev[planes][256] into out_dev[height][width][planes] and, unless NULL, valid_dev[height][width].  width is a multiple of 4,
 * 4 .. 8192, height at most 16 384, rows at most 65 536.  Device memory; everything but the masks at multiples of 4 bytes; only the
 * selected slots' pointers are looked at.  Queued on hip_stream of `device`; asynchronous.  rows = 0 or height = 0 is nothing to
 * do.  Nothing outside the inputs is read and nothing outside the outputs is written.  MDEMOD_ERR_PARAM (text in mdemod_last_error)
 * for a missing or misaligned pointer, a size out of range, or outputs that intersect inputs. */
int  mdemod_map_warp_device(const uint8_t *const image_dev[3], const uint8_t *const filled_dev[3], uint32_t rows, const uint32_t *select, uint32_t planes,
                            const uint8_t *lut_dev, const int32_t *nodes_dev, uint32_t width, uint32_t height, uint8_t *out_dev, uint8_t *valid_dev,
                            int device, void *hip_stream);

/* Pictures and masks in host memory, the packets' placements and reports (what mdemod_image_result holds) and a TLE to the finished
 * map.  Synchronous.  The time fit, the grid, the stretch tables (the picture layer's histogram on the device over the selected
 * slots and its table on the host), the selected slots copied whole, the output in bands of opts->piece_lines lines: the result is byte for byte
 * that of one batch.  *out is overwritten; mdemod_map_free(out) afterwards. */
int  mdemod_map_compose_host(const mdemod_map_opts *opts, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3],
                             uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select,
                             uint32_t planes, mdemod_map_result *out, int device);
void mdemod_map_free(mdemod_map_result *out);

#ifdef __cplusplus
}
#endif
#endif
