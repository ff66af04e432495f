/*
 * meteor_demod_amd_polar.h — 1 to 8 passes on one polar stereographic grid.  Every pass is what the mosaic layer
 * (include/meteor_demod_amd_mosaic.h) takes: swath pictures and masks of three slots, the placements and reports of its packets, and
 * a two-line element set as text with a catalogue number.  Time fit, date, orbit, look, node rule, warp rule, tap rule, blend and
 * stretch are those layers', word for word; what is new is the grid, which is metres on a plane instead of degrees, and that the
 * nodes are solved on the GPU (polar_nodes, csrc/polar.hip) into the buffers the blend kernel reads.  The latitude / longitude grid
 * refuses a pass beyond 85 degrees of latitude; this one takes the pole inside the swath.
 *
 *   projection  polar stereographic on WGS-84 with a standard parallel (Snyder 21-33 .. 21-41; "variant B" of the EPSG guidance
 *               note 7-2, with false origins 0).  a = 6 378 137 m, f = 1 / 298.257223563, e^2 = f (2 - f).  With phi_c = |lat_ts|:
 *                 t(phi) = tan(pi/4 - phi/2) / ((1 - e sin phi) / (1 + e sin phi))^(e/2),  m_c = cos phi_c / sqrt(1 - e^2 sin^2 phi_c),
 *                 rho = a m_c t(phi) / t(phi_c)      (phi_c = 90 degrees: the limit, rho = 2 a t(phi) / sqrt((1+e)^(1+e) (1-e)^(1-e))).
 *               pole +1 (north): E = rho sin(lam - lam0), N = -rho cos(lam - lam0).  pole -1 (south): the same with phi -> -phi and
 *               N = +rho cos(lam - lam0).  Inverse: rho = hypot(E, N), t = rho t(phi_c) / (a m_c), then
 *               phi <- pi/2 - 2 atan(t ((1 - e sin phi) / (1 + e sin phi))^(e/2)) from phi = pi/2 - 2 atan t until the change is below
 *               1e-14, at most 10 rounds; lam = lam0 + atan2(E, -N) in the north, atan2(E, N) in the south; rho = 0 is the pole
 *               with lam = lam0.  Check value (the guidance note's example): lat_ts -71, lam0 70 E, the point 75 S 120 E gives
 *               E = 1 255 380.79 m, N = 1 053 389.56 m.
 *   options     the map layer's scan_deg, time_offset, row_period, side, clip_low, clip_high, piece_lines with its defaults and
 *               ranges; stretch (0 none, 1 joint, 2 per pass) and blend (feather, best) as in the mosaic; metres_per_pixel 1000
 *               (100 .. 100 000); pole 0: the sign of the latitude of pass 0's pixel ((lines_0 - 1) / 2, 783.5), +1 or -1 forces it;
 *               lat_ts_deg 70, a magnitude in 0 < .. <= 90 whose sign comes from the pole; lon0_deg NaN: the longitude of that
 *               centre pixel rounded to a whole degree (floor(lon + 0.5), 180 becoming -180), otherwise -360 .. 360;
 *               nodes_on_host 1: mdemod_polar_compose_host solves the nodes on the host.
 *   frame       res = metres_per_pixel.  The border samples of every pass are the map header's (lines 0, 8, .. and the last, columns
 *               0, 16, .. and 1567); they are projected and their bounding box taken over all passes.  E_left = floor(min E / res) res,
 *               N_top = ceil(max N / res) res, W = ceil((max E - E_left) / res) rounded up to a multiple of 4 (at least 4),
 *               H = ceil((N_top - min N) / res) (at least 1).  Pixel (i, j) has its centre at E_left + (j + 0.5) res,
 *               N_top - (i + 0.5) res.  Refused (MDEMOD_ERR_PARAM, text in mdemod_last_error): a border sample that does not see the
 *               Earth; a border sample in the other hemisphere (such a pass wants the latitude / longitude grid); W > 8192 or
 *               H > 16 384 (the text names a resolution that fits); the map layer's other refusals (options, element sets, packets,
 *               more than 8192 strip rows).
 *   nodes       the map header's: per pass int32 [ceil(H / 16) + 1][ceil(W / 16) + 1][2], X = round(256 x), Y = round(256 y) of the
 *               source pixel that sees the centre of output pixel (16 a, 16 b), up to 5 degrees of scan angle beyond either edge and
 *               120 s before line 0 and after the last line; both words MDEMOD_POLAR_NO_NODE where there is none.  The centre's
 *               (E, N) goes through the inverse above to (lat, lon), and from there the solve is the map layer's one-dimensional
 *               Newton: on the host the map layer's own code, on the device the same formulas in double (12 steps at most, seed
 *               from the pass's table of r(t) every 8 s).  The two agree as far as two libms do: at every node both are missing, or
 *               both present within 1 unit in X and in Y, or exactly one is present and lies within 2 units of an edge of the
 *               margin (256 (-120 s / line period), 256 (lines - 1 + 120 s / line period), 256 (783.5 +- (scan / 2 + 5) / (scan / 1568))).
 *   picture     the mosaic header's blend, stretch, outputs (pixels, valid, cover) with these nodes; the kernel is the mosaic's.
 *   world file  six lines: res, 0, 0, -res, E_left + res / 2, N_top - res / 2.
 *   .prj        WKT 1: PROJCS["WGS 84 / Polar Stereographic", GEOGCS["WGS 84", DATUM["WGS_1984", SPHEROID["WGS 84", 6378137,
 *               298.257223563]], PRIMEM["Greenwich", 0], UNIT["degree", 0.0174532925199433]], PROJECTION["Polar_Stereographic"],
 *               PARAMETER["latitude_of_origin", signed lat_ts], PARAMETER["central_meridian", lam0], PARAMETER["false_easting", 0],
 *               PARAMETER["false_northing", 0], UNIT["metre", 1]].
 *   graticule   the meridians and parallels at multiples of step degrees that cross the picture, as polylines in degrees.  The
 *               extent in latitude and longitude (relative to lam0) is that of the picture's edge pixels every 16 pixels, inverted;
 *               with the pole inside the picture the full circle of longitudes and the pole itself.  A parallel has a vertex every
 *               step (at most every 5) degrees of longitude, a meridian two.  step 0: the smallest of 1, 2, 5, 10, 15, 30 whose
 *               parallels stand at least 128 pixels apart at the middle of the latitude extent, 30 if none.  No labels.
 *   vertices    polylines in degrees to fixed point: X = floor(256 ((E - E_left) / res - 0.5) + 0.5), Y = floor(256 ((N_top - N) / res
 *               - 0.5) + 0.5), saturated to int32; pixel centres stand at multiples of 256: the overlay layer's points, for its cut,
 *               bin and draw.  A segment is bisected in (lon, lat), the short way round in longitude, until the projected midpoint
 *               lies within 64 units (a quarter pixel) of the chord's midpoint, or 12 levels deep: a parallel becomes an
 *               arc.  A vertex in the other hemisphere (latitude times pole <= 0) ends the polyline there; the next vertex on this
 *               side begins another.  Lines of fewer than two vertices are dropped.
 *
 *   to be confirmed   everything the map header lists.  The .prj text was written from the WKT 1 specification; no GDAL or PROJ was
 *               at hand to read it back, so whether a GIS takes the parameter names as they stand (some readers want
 *               "standard_parallel_1" for the latitude of true scale) is open until a file is opened in one.
 */
#ifndef METEOR_DEMOD_AMD_POLAR_H
#define METEOR_DEMOD_AMD_POLAR_H

#include "meteor_demod_amd_picture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDEMOD_POLAR_MAX_PASSES 8
#define MDEMOD_POLAR_FEATHER    0
#define MDEMOD_POLAR_BEST       1
#define MDEMOD_POLAR_DATE_AUTO  INT32_MIN
#define MDEMOD_POLAR_NO_NODE    INT32_MIN
#define MDEMOD_POLAR_MAX_WIDTH  8192
#define MDEMOD_POLAR_MAX_HEIGHT 16384
#define MDEMOD_POLAR_MIN_RES    100.0
#define MDEMOD_POLAR_MAX_RES    100000.0
#define MDEMOD_POLAR_CHORD_TOP  64        /* units of 1 / 256 pixel a bisected chord may stand off its arc                         */
#define MDEMOD_POLAR_MAX_LEVELS 12

typedef enum { MDEMOD_POLAR_STEREOGRAPHIC = 0 } mdemod_polar_projection;

typedef struct {
	double   scan_deg;            /* 110.0: the full scan angle, 1 .. 130                                                             */
	double   time_offset;         /* 10 800.0: onboard clock minus UTC in seconds, -86 400 .. 86 400                                  */
	double   row_period;          /* 8 / 6.5: seconds per strip row where the stamps cannot say (0.1 .. 10)                           */
	double   metres_per_pixel;    /* 1000.0: 100 .. 100 000                                                                           */
	double   lat_ts_deg;          /* 70.0: the magnitude of the standard parallel, 0 < .. <= 90                                       */
	double   lon0_deg;            /* NaN: pass 0's centre longitude rounded to a degree; otherwise -360 .. 360                        */
	int32_t  side;                /* +1 or -1                                                                                         */
	int32_t  pole;                /* 0: from pass 0's centre pixel; +1 north, -1 south                                                */
	uint32_t stretch;             /* 1: joint; 0: identity tables; 2: per pass                                                        */
	uint32_t clip_low, clip_high; /* 5 and 5 permille, as in the picture layer                                                        */
	uint32_t piece_lines;         /* mdemod_polar_compose_host makes bands of this many output lines: 0 = 1024, a multiple of 16      */
	uint32_t blend;               /* MDEMOD_POLAR_FEATHER or MDEMOD_POLAR_BEST                                                        */
	uint32_t nodes_on_host;       /* 0: the nodes are solved on the device; 1: on the host                                            */
	uint32_t projection;          /* MDEMOD_POLAR_STEREOGRAPHIC                                                                       */
	uint32_t reserved;
} mdemod_polar_opts;

/* One pass, host memory: the fields of the mosaic layer's pass. */
typedef struct {
	const char    *tle_text;      /* NUL-terminated                                                                                   */
	uint32_t       norad;         /* 0: the text's first set                                                                          */
	int32_t        date;          /* days since 1970-01-01, or MDEMOD_POLAR_DATE_AUTO                                                 */
	const uint8_t *image[3];      /* [8 rows][1568] each; only the selected slots are looked at                                       */
	const uint8_t *filled[3];     /* [rows][14] each                                                                                  */
	uint32_t       rows;
	uint32_t       reserved;
	const mdemod_placement  *place;
	const mdemod_strip_info *sinfo;
	uint64_t       n_desc;
} mdemod_polar_pass;

typedef struct {
	double   row_period;          /* seconds per strip row                                                                            */
	double   s0;                  /* onboard seconds of the day of line 0                                                             */
	int32_t  date;                /* the date that was used                                                                           */
	uint32_t rows_fit;            /* rows the period rests on (below 2: the fallback)                                                 */
	uint32_t placed;              /* placed packets s0 rests on                                                                       */
	uint32_t lines;               /* 8 rows                                                                                           */
} mdemod_polar_timing;

typedef struct {
	uint32_t width, height;       /* W, H                                                                                             */
	uint32_t node_rows, node_cols;
	int32_t  pole;                /* +1 or -1                                                                                         */
	uint32_t projection;
	double   res;                 /* metres per pixel                                                                                 */
	double   e_left, n_top;       /* the outer edges of pixel (0, 0), metres                                                          */
	double   lat_ts_deg;          /* signed                                                                                           */
	double   lon0_deg;            /* -180 .. 180                                                                                      */
} mdemod_polar_frame;

/* What the node kernel is told of one pass, made on the host (mdemod_polar_grid).  Angles in radians, times in UTC seconds of the
 * pass's date.  Omega, u and the sidereal angle g are linear in t: their values at table_t0, reduced to one turn, and their rates,
 * so that sines and cosines are taken of small arguments.  table: r (Earth-fixed unit vector to the satellite) at
 * table_t0 + 8 k seconds, malloc'ed. */
typedef struct {
	double   a;                   /* km                                                                                               */
	double   cos_i, sin_i;
	double   raan, u, g;          /* at table_t0                                                                                      */
	double   raan_rate, u_rate, g_rate;
	double   table_t0;
	double   sec_lo, sec_hi;      /* line 0 minus 120 s, the last line plus 120 s                                                     */
	double   theta_max;           /* scan / 2 + 5 degrees, in radians                                                                 */
	double   s0, line_period, time_offset;
	double   step;                /* radians per column                                                                               */
	int32_t  side;
	uint32_t table_n;
	double  *table;               /* [table_n][3]                                                                                     */
} mdemod_polar_solver;

typedef struct {
	mdemod_polar_frame  frame;
	uint32_t            n;        /* passes                                                                                           */
	uint32_t            reserved;
	mdemod_polar_timing timing[MDEMOD_POLAR_MAX_PASSES];
	mdemod_polar_solver solver[MDEMOD_POLAR_MAX_PASSES];
	int32_t            *nodes[MDEMOD_POLAR_MAX_PASSES];     /* each [node_rows][node_cols][2]: X, Y; solved on the host              */
} mdemod_polar_nodes;

/* What mdemod_polar_compose_host returns: pixels, valid, cover and nodes[k] are malloc'ed, and mdemod_polar_free gives them back. */
typedef struct {
	mdemod_polar_frame  frame;
	uint32_t planes, n, blend;
	uint32_t nodes_on_host;       /* where nodes[] were solved                                                                        */
	mdemod_polar_timing timing[MDEMOD_POLAR_MAX_PASSES];
	double   utc0[MDEMOD_POLAR_MAX_PASSES];           /* UTC seconds of day timing[k].date of pass k's line 0                          */
	uint32_t lo[MDEMOD_POLAR_MAX_PASSES][3], hi[MDEMOD_POLAR_MAX_PASSES][3];    /* the stretch limits of each pass and plane          */
	uint64_t covered[MDEMOD_POLAR_MAX_PASSES];        /* pixels with cover bit k                                                       */
	uint64_t valid_pixels;        /* non-zero bytes of valid                                                                          */
	uint64_t overlap_pixels;      /* bytes of cover with two or more bits                                                             */
	uint8_t *pixels;              /* [height][width][planes]                                                                          */
	uint8_t *valid;               /* [height][width]                                                                                  */
	uint8_t *cover;               /* [height][width]                                                                                  */
	int32_t *nodes[MDEMOD_POLAR_MAX_PASSES];          /* the nodes the picture was made through                                        */
} mdemod_polar_result;

/* polylines in degrees; lon, lat, first are malloc'ed, and mdemod_polar_lines_free gives them back */
typedef struct {
	double   *lon, *lat;          /* [n_points]                                                                                       */
	uint32_t *first;              /* [n_lines + 1]                                                                                    */
	uint32_t  n_lines, n_points;
	double    step_deg;           /* the step that was used                                                                           */
} mdemod_polar_lines;

/* polylines in fixed point, laid out as the overlay layer's points; mdemod_polar_points_free */
typedef struct {
	int32_t  *x, *y;              /* [n_points]                                                                                       */
	uint32_t *first;              /* [n_lines + 1]                                                                                    */
	uint32_t  n_lines, n_points;
} mdemod_polar_points;

/* how a layer of lines is drawn: the overlay layer's style, field for field */
typedef struct {
	uint32_t half_width;          /* in 1/256 pixel, 0 .. 2048: 128 is a line of one pixel                                            */
	uint32_t opacity;             /* 0 .. 256                                                                                         */
	uint8_t  colour[3];
	uint8_t  inside_only;         /* draw only where valid is not 0                                                                   */
} mdemod_polar_style;

/* what mdemod_polar_draw_host has done */
typedef struct {
	uint64_t pieces[4];           /* pieces kept per style                                                                            */
	uint64_t tiles;               /* tiles of 32 x 32 pixels with an item                                                             */
	uint64_t items;
} mdemod_polar_drawn;

/* scan 110, offset 10 800, row_period 8 / 6.5, 1000 m, lat_ts 70, lon0 NaN, side +1, pole 0, stretch 1, clips 5 and 5, piece_lines 0,
 * blend 0, nodes_on_host 0, stereographic. */
void mdemod_polar_default_opts(mdemod_polar_opts *opts);

/* Host only, the projection by itself: pole +1 or -1, lat_ts_deg a magnitude, degrees and metres.  A point in the other hemisphere
 * projects to where the formulas put it (far out). */
int  mdemod_polar_forward(int32_t pole, double lat_ts_deg, double lon0_deg, const double *lat, const double *lon, uint64_t n, double *e, double *north);
int  mdemod_polar_inverse(int32_t pole, double lat_ts_deg, double lon0_deg, const double *e, const double *north, uint64_t n, double *lat, double *lon);

/* Host only: the frame, every pass's line times with the date resolved, its solver constants and its nodes solved on the host.
 * *grid is overwritten; mdemod_polar_grid_free. */
int  mdemod_polar_grid(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, mdemod_polar_nodes *grid);
void mdemod_polar_grid_free(mdemod_polar_nodes *grid);

/* The bytes of device memory mdemod_polar_nodes_device wants as work_dev for these passes (their tables), 0 for none. */
uint64_t mdemod_polar_nodes_work_bytes(const mdemod_polar_solver *solvers, uint32_t n);

/* frame and solvers[n] (host memory, n at most 8) into nodes_dev[k][node_rows][node_cols][2] for every k (host array of device
 * pointers at multiples of 4 bytes), node_rows = ceil(height / 16) + 1 and node_cols likewise, width 1 .. 8192, height 1 .. 16 384.
 * work_dev: device memory of at least mdemod_polar_nodes_work_bytes at a multiple of 8 bytes; the tables are copied there on the
 * stream.  One launch, queued on hip_stream of `device`; asynchronous.  n = 0 is nothing to do.  Nothing outside work_dev and the
 * nodes is written.  MDEMOD_ERR_PARAM (text in mdemod_last_error) for a missing or misaligned pointer, a size or a constant out of
 * range, a table that is missing, work_bytes too small, or buffers that intersect; nothing is written then. */
int  mdemod_polar_nodes_device(const mdemod_polar_frame *frame, const mdemod_polar_solver *solvers, uint32_t n, int32_t *const *nodes_dev, void *work_dev,
                               uint64_t work_bytes, int device, void *hip_stream);

/* Passes in host memory to the finished picture.  Synchronous.  The time fits, the frame, the nodes on the device (on the host with
 * opts->nodes_on_host), the stretch tables by the mosaic's rules (the picture layer's histogram on the device), the mosaic layer's
 * blend kernel, the output in bands of opts->piece_lines lines: byte for byte that of one batch.  *out is overwritten;
 * mdemod_polar_free(out) afterwards. */
int  mdemod_polar_compose_host(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                               mdemod_polar_result *out, int device);
void mdemod_polar_free(mdemod_polar_result *out);

/* Host only: the graticule of a picture; step_deg 0 is automatic.  *lines is overwritten; mdemod_polar_lines_free. */
int  mdemod_polar_graticule(const mdemod_polar_frame *frame, double step_deg, mdemod_polar_lines *lines);
void mdemod_polar_lines_free(mdemod_polar_lines *lines);

/* Host only: polylines in degrees (lon, lat, first[n_lines + 1]) to fixed point on this frame.  *points is overwritten;
 * mdemod_polar_points_free. */
int  mdemod_polar_vertices(const mdemod_polar_frame *frame, const double *lon, const double *lat, const uint32_t *first, uint32_t n_lines,
                           mdemod_polar_points *points);
void mdemod_polar_points_free(mdemod_polar_points *points);

/* Fixed-point polylines drawn onto a picture in host memory, pixels[height][width][planes] in place, through the overlay layer as it
 * stands: its cut per layer (layer l has the style style_of[l]), its bins, its draw kernel on the whole picture; styles as the
 * overlay header defines them (half_width in 1/256 pixel up to 2048, opacity up to 256, at most 4).  valid may be NULL unless a
 * style has inside_only; report may be NULL.  width a multiple of 4.  Synchronous. */
int  mdemod_polar_draw_host(const mdemod_polar_points *const *layers, const uint32_t *style_of, uint32_t n_layers, const mdemod_polar_style *styles, uint32_t n_styles,
                            uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid, mdemod_polar_drawn *report, int device);

/* The six lines of the world file and the .prj text of a frame into text[size], NUL-terminated; MDEMOD_ERR_PARAM where it does not fit. */
int  mdemod_polar_world_file(const mdemod_polar_frame *frame, char *text, uint64_t size);
int  mdemod_polar_prj(const mdemod_polar_frame *frame, char *text, uint64_t size);

#ifdef __cplusplus
}
#endif
#endif
