/*
 * mosaic_host.h — what csrc/mosaic_host.cpp (host: the common grid, the tables, the model, the bands of the whole-mosaic entry) and
 * csrc/mosaic.hip (the kernel and the device entries) share: the option check, the argument checks, the bands with a backend in the
 * kernel's place, and the model's entries, exported for the tests.  Free of the GPU runtime.
 */
#ifndef MDEMOD_MOSAIC_HOST_H
#define MDEMOD_MOSAIC_HOST_H

#include <memory>

#include "../../include/meteor_demod_amd_mosaic.h"
#include "map_host.h"

#define MOSAIC_MAX      MDEMOD_MOSAIC_MAX_PASSES
#define MOSAIC_W_TOP    784                        /* the largest weight */

/* the warp is the map layer's, on the device (csrc/warp_device.h) and in the model (csrc/warp_model.h): one word for "no node" */
static_assert(MDEMOD_MOSAIC_NO_NODE == MDEMOD_MAP_NO_NODE, "a pass's nodes are tested against the map layer's MDEMOD_MAP_NO_NODE");

/* opts (NULL: the defaults) checked and completed (piece_lines 0 -> 1024); MDEMOD_ERR_PARAM with a text otherwise */
int  mosaic_settings(const mdemod_mosaic_opts *opts, mdemod_mosaic_opts &out);

/* n, select, planes, blend, width, height and every pass's rows of a blend call; MDEMOD_ERR_PARAM with a text */
int  mosaic_check_blend(const char *who, const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend,
                        uint32_t width, uint32_t height);
/* the selected slots, the tables and the nodes of every pass that is not empty are there */
int  mosaic_check_sources(const char *who, const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes);

/* the argument checks that mdemod_mosaic_compose_host and the model's host entry share */
int  mosaic_check_compose(const char *who, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes, mdemod_mosaic_result *out);

/* what stands in the kernel's place in the whole-mosaic entry.  begin: every pass's selected slots (the others NULL), whole, and
 * the nodes; histogram: of pass k's slots; tables: [n][planes][256]; band: `height` lines from node row `node_row` on into host
 * memory.  All synchronous. */
struct MosaicBackend {
	virtual int begin(const mdemod_mosaic_pass *passes, const mdemod_mosaic_nodes &grid, uint32_t planes, uint32_t piece_lines) = 0;
	virtual int histogram(uint32_t k, uint32_t *hist) = 0;
	virtual int tables(const uint8_t *lut, uint32_t planes) = 0;
	virtual int band(const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid,
	                 uint8_t *cover) = 0;
	virtual ~MosaicBackend() {}
};

/* the model in the kernel's place: host memory, the blend of mdemod_mosaic_model_blend */
std::unique_ptr<MosaicBackend> mosaic_model_backend();

int  mosaic_compose_bands(const mdemod_mosaic_opts &o, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                          mdemod_mosaic_result *out, MosaicBackend &backend);

/* mosaic_compose_bands behind its grid: tables, bands and counts on a grid that is given (its width, height, node counts, n, timing
 * and whatever of nodes the backend's begin wants); another projection's grid (csrc/polar_host.cpp) comes in here. */
int  mosaic_bands_on(const mdemod_mosaic_opts &o, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                     const mdemod_mosaic_nodes &grid, mdemod_mosaic_result *out, MosaicBackend &backend);

extern "C" {

/* the model of mosaic_blend: host memory, the same rule */
int  mdemod_mosaic_model_blend(const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width,
                               uint32_t height, uint8_t *out, uint8_t *valid, uint8_t *cover);
/* mdemod_mosaic_compose_host with the model in the kernel's place (no device) */
int  mdemod_mosaic_model_host(const mdemod_mosaic_opts *opts, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                              mdemod_mosaic_result *out);

}

#endif
