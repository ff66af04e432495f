/*
 * overlay.hip — the overlay layer on the GPU (include/meteor_demod_amd_overlay.h): overlay_draw, and the public entries around it.
 * The specification is the host model of csrc/overlay_host.cpp.
 *
 * overlay_draw: one block of 256 threads per tile of 32 x 32 pixels, a thread owns 4 neighbouring pixels of one line (the layout of
 *   map_warp, csrc/map.hip), so that the picture, valid and mask are read and written in whole dwords.  The tile's first and last
 *   item are uniform: a block whose tile has no item returns before it loads or stores a pixel.  The tile's pieces are staged
 *   through LDS in chunks of 256 records of 32 bytes (thread t fetches item t of the chunk); then every lane reads the same record,
 *   which is a broadcast, and works the rule out for its 4 pixels: the two products of the first pixel, and an addition per further
 *   pixel (256 tx, 256 ty).  The bins hold only pieces of at most 64 pixels per axis within reach of the tile, so the products stay
 *   below 2^31 and 32-bit arithmetic gives the model's 64-bit values (csrc/overlay_host.cpp: check_pieces).  The items of a tile
 *   ascend in style, so a thread keeps the maximum of one style only, 4 words; when the style changes, and after the last item, that
 *   style is blended into the bytes the thread holds: the styles meet a pixel in ascending order, as the rule asks.  The maximum is
 *   free of order, there is no atomic, and nothing but the arguments decides a byte.  A style's numbers come from the kernel
 *   arguments by a uniform index: scalar loads.  An item that is no index into the pieces, or a piece whose style is none, is staged
 *   as a record that covers nothing.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "overlay_host.h"
#include "hip_host.h"

#define OVERLAY_THREADS 256
#define OVERLAY_CHUNK   256                      /* records staged at a time */

struct OverlayStyle {
	int32_t w128;                                 /* half width + 128 */
	uint32_t opacity;
	uint32_t colour;                              /* plane p in bits 8 p .. 8 p + 7 */
	uint32_t inside_only;
};

struct OverlayDraw {
	const mdemod_overlay_piece *pieces;
	const uint32_t *tile_first;                   /* of the band's first tile row */
	const uint32_t *items;
	uint8_t *pixels;                              /* of the band's first line */
	const uint8_t *valid;
	uint8_t *mask;
	uint32_t n_pieces, n_items, n_styles;
	uint32_t width, height, tiles_x;
	uint32_t line0;                               /* the band's first line in the picture the bins were made for */
	OverlayStyle style[OVERLAY_MAX_STYLES];
};

/* style s with the maxima `top` onto the thread's 4 pixels */
template <int PLANES>
__device__ __forceinline__ void
overlay_blend(const OverlayStyle &st, uint32_t s, const int32_t (&top)[4], uint32_t inside, uint32_t (&bytes)[4 * PLANES], uint32_t &bits)
{
#pragma unroll
	for (int q = 0; q < 4; q++) {
		int32_t a = min(top[q], 256);
		if (st.inside_only && !((inside >> (8 * q)) & 255u)) a = 0;
		if (a <= 0) continue;
		bits |= (1u << s) << (8 * q);
		const uint32_t o = (static_cast<uint32_t>(a) * st.opacity + 128u) >> 8;
#pragma unroll
		for (int p = 0; p < PLANES; p++) {
			uint32_t &b = bytes[PLANES * q + p];
			b = (b * (256u - o) + ((st.colour >> (8 * p)) & 255u) * o + 128u) >> 8;
		}
	}
}

template <int PLANES>
__global__ void __launch_bounds__(OVERLAY_THREADS)
overlay_draw(OverlayDraw a)
{
	__shared__ __attribute__((aligned(16))) int32_t rec[OVERLAY_CHUNK * 8];
	const uint32_t tile = blockIdx.y * a.tiles_x + blockIdx.x;
	const uint32_t from = a.tile_first[tile], to = min(a.tile_first[tile + 1], a.n_items);
	if (from >= to) return;                                                    /* (uniform: the whole block) */
	constexpr int ACROSS = OVERLAY_TILE / 4;
	const uint32_t t = threadIdx.x;
	const uint32_t i = blockIdx.y * OVERLAY_TILE + t / ACROSS, j0 = blockIdx.x * OVERLAY_TILE + 4 * (t % ACROSS);
	const bool live = i < a.height && j0 < a.width;
	const size_t at = static_cast<size_t>(i) * a.width + j0;
	uint32_t bytes[4 * PLANES], bits = 0, inside = 0x01010101u;
#pragma unroll
	for (int c = 0; c < 4 * PLANES; c++) bytes[c] = 0;
	if (live) {
		const uint32_t *px = reinterpret_cast<const uint32_t *>(a.pixels + at * PLANES);
#pragma unroll
		for (int d = 0; d < PLANES; d++) {
			const uint32_t w = px[d];
#pragma unroll
			for (int b = 0; b < 4; b++) bytes[4 * d + b] = (w >> (8 * b)) & 255u;
		}
		if (a.valid) inside = *reinterpret_cast<const uint32_t *>(a.valid + at);
	}
	const int32_t px0 = static_cast<int32_t>(256u * j0), py = static_cast<int32_t>(256u * (a.line0 + i));
	int32_t top[4] = { 0, 0, 0, 0 };
	uint32_t cur = 0;                                                          /* the style `top` belongs to */
	for (uint32_t base = from; base < to; base += OVERLAY_CHUNK) {
		const uint32_t n = min(static_cast<uint32_t>(OVERLAY_CHUNK), to - base);
		__syncthreads();                                                       /* (the chunk before has been read) */
		if (t < n) {
			const uint32_t k = a.items[base + t];
			int32_t w[8] = { 0, 0, 0, 0, 0, -1, 0, 0 };                         /* style -1: covers nothing */
			if (k < a.n_pieces) {
				const int32_t *g = reinterpret_cast<const int32_t *>(a.pieces + k);
#pragma unroll
				for (int c = 0; c < 6; c++) w[c] = g[c];
				if (static_cast<uint32_t>(w[5]) >= a.n_styles) w[5] = -1;
			}
			*reinterpret_cast<int4 *>(rec + 8 * t) = make_int4(w[0], w[1], w[2], w[3]);
			*reinterpret_cast<int4 *>(rec + 8 * t + 4) = make_int4(w[4], w[5], 0, 0);
		}
		__syncthreads();
		for (uint32_t r = 0; r < n; r++) {
			const int4 p = *reinterpret_cast<const int4 *>(rec + 8 * r);
			const int2 q = *reinterpret_cast<const int2 *>(rec + 8 * r + 4);
			const int32_t style = __builtin_amdgcn_readfirstlane(q.y);
			if (style < 0) continue;
			if (static_cast<uint32_t>(style) != cur) {
				if (live) overlay_blend<PLANES>(a.style[cur], cur, top, inside, bytes, bits);
#pragma unroll
				for (int c = 0; c < 4; c++) top[c] = 0;
				cur = static_cast<uint32_t>(style);
			}
			const int32_t w128 = a.style[cur].w128;
			const uint32_t tx = static_cast<uint32_t>(p.z), ty = static_cast<uint32_t>(p.w);
			const uint32_t dx = static_cast<uint32_t>(px0) - static_cast<uint32_t>(p.x), dy = static_cast<uint32_t>(py) - static_cast<uint32_t>(p.y);
			uint32_t al = tx * dx + ty * dy, cr = tx * dy - ty * dx;
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const int32_t along = static_cast<int32_t>(al) >> 14;
				const int32_t perp = static_cast<int32_t>(static_cast<uint32_t>(abs(static_cast<int32_t>(cr))) >> 14);
				const int32_t d = max(max(perp, -along), max(along - q.x, 0));
				top[c] = max(top[c], w128 - d);
				al += 256u * tx;
				cr -= 256u * ty;
			}
		}
	}
	if (!live) return;
	overlay_blend<PLANES>(a.style[cur], cur, top, inside, bytes, bits);
	uint32_t *out = reinterpret_cast<uint32_t *>(a.pixels + at * PLANES);
#pragma unroll
	for (int d = 0; d < PLANES; d++) out[d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | (bytes[4 * d + 3] << 24);
	if (a.mask) *reinterpret_cast<uint32_t *>(a.mask + at) = bits;
}

namespace {

/* `height` lines from line `line0` of the picture the bins were made for; tile_first of that line's tile row */
int
draw_run(const mdemod_overlay_piece *pieces_dev, uint64_t n_pieces, const uint32_t *tile_first_dev, const uint32_t *items_dev, uint64_t n_items,
         const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t line0, uint32_t height, uint32_t planes, uint8_t *pixels_dev,
         const uint8_t *valid_dev, uint8_t *mask_dev, hipStream_t st)
{
	if (!height) return MDEMOD_OK;
	if (mask_dev) HIP_TRY(hipMemsetAsync(mask_dev, 0, static_cast<size_t>(height) * width, st));
	if (!n_pieces || !n_items) return MDEMOD_OK;
	OverlayDraw a;
	memset(&a, 0, sizeof a);
	a.pieces = pieces_dev; a.tile_first = tile_first_dev; a.items = items_dev; a.pixels = pixels_dev; a.valid = valid_dev; a.mask = mask_dev;
	a.n_pieces = static_cast<uint32_t>(n_pieces); a.n_items = static_cast<uint32_t>(n_items); a.n_styles = n_styles;
	a.width = width; a.height = height; a.tiles_x = overlay_tiles(width); a.line0 = line0;
	for (uint32_t s = 0; s < n_styles; s++) {
		a.style[s].w128 = static_cast<int32_t>(styles[s].half_width) + 128;
		a.style[s].opacity = styles[s].opacity;
		a.style[s].colour = planes == 3 ? styles[s].colour[0] | styles[s].colour[1] << 8 | styles[s].colour[2] << 16 : styles[s].colour[0];
		a.style[s].inside_only = styles[s].inside_only != 0;
	}
	const dim3 grid(a.tiles_x, overlay_tiles(height));
	if (planes == 3) hipLaunchKernelGGL(overlay_draw<3>, grid, dim3(OVERLAY_THREADS), 0, st, a);
	else hipLaunchKernelGGL(overlay_draw<1>, grid, dim3(OVERLAY_THREADS), 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* the kernel in the whole-picture entries: pieces and bins up once, one band up and down at a time, on the null stream.  The device
 * is taken when the bands begin: a refusal of the arguments comes first and touches no device. */
struct DeviceBackend : OverlayBackend {
	MdmDevMem mem;
	int device;
	explicit DeviceBackend(int dev) : device(dev) {}
	mdemod_overlay_piece *d_pieces = nullptr;
	uint32_t *d_first = nullptr, *d_items = nullptr;
	uint8_t *d_pixels = nullptr, *d_valid = nullptr, *d_mask = nullptr;
	const mdemod_overlay_style *styles = nullptr;
	uint64_t n_pieces = 0, n_items = 0;
	uint32_t n_styles = 0, width = 0, planes = 0, tiles_x = 0;

	int begin(const mdemod_overlay_pieces &p, const mdemod_overlay_bins &b, const mdemod_overlay_style *st, uint32_t ns, uint32_t w, uint32_t pl, uint32_t piece_lines,
	          bool with_valid, bool with_mask) override
	{
		int rc = mdm_select_device(device);
		if (rc) return rc;
		styles = st; n_styles = ns; width = w; planes = pl; tiles_x = b.tiles_x; n_pieces = p.n; n_items = b.n_items;
		const size_t tiles = static_cast<size_t>(b.tiles_x) * b.tiles_y;
		if ((rc = mem.alloc(&d_pieces, p.n)) || (rc = mem.alloc(&d_first, tiles + 1)) || (rc = mem.alloc(&d_items, b.n_items)) ||
		    (rc = mem.alloc(&d_pixels, static_cast<size_t>(piece_lines) * w * pl)))
			return rc;
		if (with_valid && (rc = mem.alloc(&d_valid, static_cast<size_t>(piece_lines) * w))) return rc;
		if (with_mask && (rc = mem.alloc(&d_mask, static_cast<size_t>(piece_lines) * w))) return rc;
		if (p.n) HIP_TRY(hipMemcpyAsync(d_pieces, p.piece, p.n * sizeof(mdemod_overlay_piece), hipMemcpyHostToDevice, nullptr));
		HIP_TRY(hipMemcpyAsync(d_first, b.tile_first, (tiles + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
		if (b.n_items) HIP_TRY(hipMemcpyAsync(d_items, b.items, b.n_items * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int band(uint32_t tile_row, uint32_t height, uint8_t *pixels, const uint8_t *valid, uint8_t *mask) override
	{
		const size_t area = static_cast<size_t>(height) * width;
		HIP_TRY(hipMemcpyAsync(d_pixels, pixels, area * planes, hipMemcpyHostToDevice, nullptr));
		if (valid) HIP_TRY(hipMemcpyAsync(d_valid, valid, area, hipMemcpyHostToDevice, nullptr));
		const int rc = draw_run(d_pieces, n_pieces, d_first + static_cast<size_t>(tile_row) * tiles_x, d_items, n_items, styles, n_styles, width, OVERLAY_TILE * tile_row,
		                        height, planes, d_pixels, valid ? d_valid : nullptr, mask ? d_mask : nullptr, nullptr);
		if (rc) return rc;
		HIP_TRY(hipMemcpyAsync(pixels, d_pixels, area * planes, hipMemcpyDeviceToHost, nullptr));
		if (mask) HIP_TRY(hipMemcpyAsync(mask, d_mask, area, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}
};

} /* namespace */

int
overlay_draw_points_device(const mdemod_overlay_points *const *layers, const uint32_t *style_of, uint32_t n_layers, const mdemod_overlay_style *styles, uint32_t n_styles,
                           uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid, mdemod_overlay_report *report, int device)
{
	DeviceBackend dev(device);
	return overlay_draw_points(layers, style_of, n_layers, styles, n_styles, width, height, planes, pixels, valid, nullptr, 0, report, dev);
}

extern "C" {

int
mdemod_overlay_draw_device(const mdemod_overlay_piece *pieces_dev, uint64_t n_pieces, const uint32_t *tile_first_dev, const uint32_t *items_dev, uint64_t n_items,
                           const mdemod_overlay_style *styles, uint32_t n_styles, uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels_dev,
                           const uint8_t *valid_dev, uint8_t *mask_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_overlay_draw_device";
	int rc = overlay_check_draw(who, styles, n_styles, width, height, planes, pixels_dev, valid_dev);
	if (rc) return rc;
	if (!height) return MDEMOD_OK;
	if (n_pieces >= (1ull << 31) || n_items >= (1ull << 31)) REFUSE("%s: more than 2^31 pieces or items", who);
	if (n_pieces && n_items && (!pieces_dev || !tile_first_dev || !items_dev)) REFUSE("%s: the pieces and the bins are needed", who);
	const bool draws = n_pieces && n_items;
	uintptr_t low = reinterpret_cast<uintptr_t>(pixels_dev) | reinterpret_cast<uintptr_t>(valid_dev) | reinterpret_cast<uintptr_t>(mask_dev);
	if (draws) low |= reinterpret_cast<uintptr_t>(pieces_dev) | reinterpret_cast<uintptr_t>(tile_first_dev) | reinterpret_cast<uintptr_t>(items_dev);
	if (low & 3u) REFUSE("%s: the pieces, the bins, the picture, valid and mask must stand at multiples of 4 bytes", who);
	const uint64_t area = static_cast<uint64_t>(height) * width;
	const uint64_t tiles = static_cast<uint64_t>(overlay_tiles(width)) * overlay_tiles(height);
	MdmBuffers b;
	b.out(pixels_dev, area * planes).out(mask_dev, area).in(valid_dev, area);
	if (draws) b.in(pieces_dev, n_pieces * sizeof(mdemod_overlay_piece)).in(tile_first_dev, (tiles + 1) * sizeof(uint32_t)).in(items_dev, n_items * sizeof(uint32_t));
	if (!b.apart()) REFUSE("%s: the outputs and the inputs intersect (the blocks of one launch would read what others write)", who);
	if ((rc = mdm_select_device(device))) return rc;
	return draw_run(pieces_dev, n_pieces, tile_first_dev, items_dev, n_items, styles, n_styles, width, 0, height, planes, pixels_dev, valid_dev, mask_dev,
	                static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_overlay_draw_host(const mdemod_overlay_geo *geo, const mdemod_overlay_layer *layers, uint32_t n_layers, const mdemod_overlay_style *styles, uint32_t n_styles,
                         uint32_t planes, uint8_t *pixels, const uint8_t *valid, uint8_t *mask, uint32_t piece_lines, mdemod_overlay_report *report, int device)
try { MDEMOD_API_ENTER
	DeviceBackend dev(device);
	return overlay_draw_bands("mdemod_overlay_draw_host", geo, layers, n_layers, styles, n_styles, planes, pixels, valid, mask, piece_lines, report, dev);
} MDEMOD_API_CATCH

} /* extern "C" */
