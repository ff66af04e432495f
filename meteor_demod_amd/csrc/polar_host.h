/*
 * polar_host.h — what csrc/polar_host.cpp (host: projection, frame, host nodes, graticule, vertices, the model, the bands) and
 * csrc/polar.hip (the node kernel and the device entries) share.  The passes, the tables, the bands and the blend are the mosaic
 * layer's (csrc/mosaic_host.h), the solver is the map layer's (csrc/map_host.h).  Free of the GPU runtime.
 */
#ifndef MDEMOD_POLAR_HOST_H
#define MDEMOD_POLAR_HOST_H

#include "../../include/meteor_demod_amd_polar.h"
#include "mosaic_host.h"
#include "polar_proj.h"

#define POLAR_MAX MDEMOD_POLAR_MAX_PASSES

static_assert(MDEMOD_POLAR_NO_NODE == MDEMOD_MAP_NO_NODE && POLAR_MAX == MOSAIC_MAX, "the nodes go to the mosaic layer's blend as they are");

/* opts (NULL: the defaults) checked and completed (piece_lines 0 -> 1024); MDEMOD_ERR_PARAM with a text otherwise */
int  polar_settings(const mdemod_polar_opts *opts, mdemod_polar_opts &out);

/* a frame that somebody hands in: sizes, node counts, pole, resolution, parallel and meridian in range */
int  polar_check_frame(const char *who, const mdemod_polar_frame *frame);
PolarProj polar_proj_of(const mdemod_polar_frame &frame);

/* the argument checks that mdemod_polar_compose_host and the model's host entry share */
int  polar_check_compose(const char *who, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes, mdemod_polar_result *out);

/* mdemod_polar_grid: on `given` instead of the passes' own frame unless NULL; the nodes solved only with host_nodes (they are
 * allocated either way) */
int  polar_grid_make(const char *who, const mdemod_polar_opts &o, const mdemod_polar_pass *passes, uint32_t n, const mdemod_polar_frame *given, bool host_nodes,
                     mdemod_polar_nodes *grid);

/* the mosaic layer's tables and bands on this grid with `backend` in the kernel's place; grid's nodes move into *out */
int  polar_compose(const mdemod_polar_opts &o, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes, mdemod_polar_nodes &grid,
                   mdemod_polar_result *out, MosaicBackend &backend);

extern "C" {

/* mdemod_polar_grid on a frame that is given: the host solver */
int  mdemod_polar_model_nodes(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, const mdemod_polar_frame *frame, mdemod_polar_nodes *grid);
/* mdemod_polar_compose_host with host nodes and the mosaic layer's model blend (no device) */
int  mdemod_polar_model_host(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                             mdemod_polar_result *out);

}

#endif
