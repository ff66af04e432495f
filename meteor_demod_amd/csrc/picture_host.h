/*
 * picture_host.h — what csrc/picture_host.cpp (host: options, column map, tables, the model, the pieces of the whole-picture entry)
 * and csrc/picture.hip (the kernels and the device entries) share: the option check, the pieces with a backend in the kernels'
 * place, and the model's entries, exported for the tests.  Free of the GPU runtime.
 */
#ifndef MDEMOD_PICTURE_HOST_H
#define MDEMOD_PICTURE_HOST_H

#include "../../include/meteor_demod_amd_picture.h"

#define PIC_SRC_W      MDEMOD_IMAGE_WIDTH         /* 1568 */
#define PIC_CELL_W     112
#define PIC_CELLS      MDEMOD_IMAGE_CELLS
#define PIC_LAST       (PIC_SRC_W - 1)
#define PIC_LINE_BYTES (8ull * PIC_SRC_W)         /* one strip row of one slot */

/* opts (NULL: the defaults) checked and completed (piece_rows 0 -> 1024); MDEMOD_ERR_PARAM with a text otherwise */
int  pic_settings(const mdemod_picture_opts *opts, mdemod_picture_opts &out);

/* rows, select and planes of a render / compose call; MDEMOD_ERR_PARAM with a text */
int  pic_check_select(const char *who, uint32_t rows, const uint32_t *select, uint32_t planes);

/* the selected slots' pictures and masks are there; MDEMOD_ERR_PARAM with a text */
int  pic_check_slots(const char *who, const uint8_t *const image[3], const uint8_t *const filled[3], const uint32_t *select, uint32_t planes);

/* what stands in the kernels' place in the whole-picture entry: the histograms of one piece (NULL slots stay zero) and the render
 * of one piece, both synchronous, host memory in and out */
struct PicBackend {
	virtual int histogram(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, uint32_t *hist) = 0;
	virtual int render(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes,
	                   const uint8_t *lut, const uint32_t *map, uint32_t width, uint8_t *out, uint8_t *valid) = 0;
	virtual ~PicBackend() {}
};

int  pic_compose_pieces(const mdemod_picture_opts &o, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                        const uint32_t *select, uint32_t planes, mdemod_picture_result *out, PicBackend &backend);

extern "C" {

/* the model of picture_histogram: host memory, the same rule */
int  mdemod_picture_model_histogram(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, uint32_t *hist);
/* the model of picture_render */
int  mdemod_picture_model_render(const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows, const uint32_t *select, uint32_t planes,
                                 const uint8_t *lut, const uint32_t *map, uint32_t width, uint8_t *out, uint8_t *valid);
/* mdemod_picture_compose_host with the model in the kernels' place (no device) */
int  mdemod_picture_model_host(const mdemod_picture_opts *opts, const uint8_t *const image[3], const uint8_t *const filled[3], uint32_t rows,
                               const uint32_t *select, uint32_t planes, mdemod_picture_result *out);

}

#endif
