/*
 * mosaic_device.h — the kernel of csrc/mosaic.hip in the whole-picture entries: the backend that mdemod_mosaic_compose_host hands to
 * the bands (csrc/mosaic_host.h), shared with the other projection that blends through the same bands (csrc/polar.hip).  The members
 * are defined in csrc/mosaic.hip.
 */
#ifndef MDEMOD_MOSAIC_DEVICE_H
#define MDEMOD_MOSAIC_DEVICE_H

#include "mosaic_host.h"
#include "hip_host.h"

/* every pass's slots and nodes up once, one band down at a time, on the null stream */
struct MosaicDeviceBackend : MosaicBackend {
	MdmDevMem mem;
	uint8_t *d_image[MOSAIC_MAX][3] = {}, *d_filled[MOSAIC_MAX][3] = {}, *d_lut = nullptr, *d_out = nullptr, *d_valid = nullptr, *d_cover = nullptr;
	int32_t *d_nodes[MOSAIC_MAX] = {};
	uint32_t *d_hist = nullptr;
	uint32_t rows[MOSAIC_MAX] = {}, n = 0, width = 0, node_cols = 0, planes = 0;
	size_t node_words = 0;
	int device;
	explicit MosaicDeviceBackend(int dev) : device(dev) {}

	int begin(const mdemod_mosaic_pass *passes, const mdemod_mosaic_nodes &grid, uint32_t pl, uint32_t piece_lines) override;
	int histogram(uint32_t k, uint32_t *hist) override;
	int tables(const uint8_t *lut, uint32_t pl) override;
	int band(const uint32_t *select, uint32_t pl, uint32_t blend, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid, uint8_t *cover) override;

	/* begin's one open step: the nodes of the n passes into d_nodes[] (allocated, node_words words each), queued on the null stream.
	 * Here grid.nodes[k] is uploaded; a projection that solves its nodes on the device launches that instead. */
	virtual int nodes_in(const mdemod_mosaic_nodes &grid);
};

#endif
