/*
 * map_host.h — what csrc/map_host.cpp (host: TLE, orbit, time fit, geolocation, node grid, the model, the bands of the whole-map
 * entry) and csrc/map.hip (the kernel and the device entries) share: the option check, the bands with a backend in the kernel's
 * place, and the model's entries, exported for the tests.  Free of the GPU runtime.
 */
#ifndef MDEMOD_MAP_HOST_H
#define MDEMOD_MAP_HOST_H

#include <cstddef>
#include <vector>

#include "../../include/meteor_demod_amd_map.h"
#include "picture_host.h"

#define MAP_STEP       MDEMOD_MAP_NODE_STEP
#define MAP_X_TOP      (PIC_LAST * 256)           /* the largest X inside the picture */

/* opts (NULL: the defaults) checked and completed (piece_lines 0 -> 1024); MDEMOD_ERR_PARAM with a text otherwise */
int  map_settings(const mdemod_map_opts *opts, mdemod_map_opts &out);

/* rows, select, planes, width and height of a warp call; MDEMOD_ERR_PARAM with a text */
int  map_check_warp(const char *who, uint32_t rows, const uint32_t *select, uint32_t planes, uint32_t width, uint32_t height);

inline uint32_t map_node_count(uint32_t pixels) { return (pixels + MAP_STEP - 1) / MAP_STEP + 1; }

/* what stands in the kernel's place in the whole-map entry.  begin: the selected slots (the others NULL), whole, and the nodes;
 * histogram: of those slots; band: `height` lines from node row `node_row` on into host memory.  All synchronous. */
struct MapBackend {
	virtual int begin(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const mdemod_map_nodes &grid, uint32_t planes,
	                  uint32_t piece_lines) = 0;
	virtual int histogram(uint32_t *hist) = 0;
	virtual int tables(const uint8_t *lut, uint32_t planes) = 0;
	virtual int band(const uint32_t *select, uint32_t planes, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid) = 0;
	virtual ~MapBackend() {}
};

int  map_compose_bands(const mdemod_map_opts &o, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                       const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select, uint32_t planes,
                       mdemod_map_result *out, MapBackend &backend);

/* the argument checks that mdemod_map_compose_host and the model's host entry share */
int  map_check_compose(const char *who, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                       const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select, uint32_t planes,
                       mdemod_map_result *out);

/* What mdemod_map_grid is made of, shared with the mosaic layer (csrc/mosaic_host.cpp): the swath's border samples with their
 * refusals, the grid's frame from a range of latitudes and longitudes, and the nodes of a pass on a prescribed frame.  Longitudes
 * of a range are relative to lon_c and wrapped to +-180; a fresh MapRange is empty and every border widens it. */
struct MapRange { double lat_lo = 1.0e9, lat_hi = -1.0e9, lon_lo = 1.0e9, lon_hi = -1.0e9; };
struct MapFrame { double sy, sx, lat_top, left; uint32_t width, height; };      /* left: lon_left before it is wrapped to -180 .. 180 */

int  map_check_pass(const char *who, const mdemod_map_tle *tle, const mdemod_map_timing *timing);
int  map_check_lines(uint32_t lines);
int  map_resolve_date(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, uint32_t lines, int32_t &date);
/* the longitude of pixel ((lines - 1) / 2, 783.5) */
int  map_swath_centre(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, double &lon_c);
int  map_swath_border(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, double lon_c,
                      MapRange &range);
int  map_frame(const mdemod_map_opts &o, const MapRange &range, double lon_c, MapFrame &f);
double map_frame_lon_left(const MapFrame &f);
/* nodes[map_node_count(f.height)][map_node_count(f.width)][2] of this pass */
void map_nodes_on(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, const MapFrame &f,
                  int32_t *nodes);

/* What other projections (csrc/polar_host.cpp) take from this layer: the nodes of a pass at prescribed points (degrees; a point
 * that is not finite has no node) by the solver map_nodes_on uses, the forward function of one pixel, and the solver's constants
 * for a solver elsewhere: the angles of the orbit and of the Earth at the table's start (reduced to one turn) with their rates in
 * rad/s, the table of r every table_step seconds from table_t0 on, the margins in UTC seconds and in scan angle. */
void map_nodes_at(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, const double *lat,
                  const double *lon, size_t n, int32_t *nodes);
bool map_forward(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, double y, double x, double &lat, double &lon);
struct MapSolver {
	double a, ci, si, raan_dot, u_dot, g_dot, raan_t0, u_t0, g_t0, table_t0, table_step, sec_lo, sec_hi, theta_max, s0, line_period, offset, step;
	int side;
	std::vector<double> table;                   /* [entries][3] */
};
void map_solver_of(const mdemod_map_tle &tle, const mdemod_map_timing &tm, const mdemod_map_opts &o, int32_t date, uint32_t lines, MapSolver &s);

extern "C" {

/* the model of map_warp: host memory, the same rule */
int  mdemod_map_model_warp(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes,
                           const uint8_t *lut, const int32_t *nodes, uint32_t width, uint32_t height, uint8_t *out, uint8_t *valid);
/* mdemod_map_compose_host with the model in the kernel's place (no device) */
int  mdemod_map_model_host(const mdemod_map_opts *opts, const mdemod_map_tle *tle, const uint8_t *const image[3], const uint8_t *const filled[3],
                           uint32_t rows, const mdemod_placement *place, const mdemod_strip_info *sinfo, uint64_t n_desc, const uint32_t *select,
                           uint32_t planes, mdemod_map_result *out);

}

#endif
