/*
 * polar.hip — the polar layer on the GPU (include/meteor_demod_amd_polar.h): polar_nodes, and the public entries around it.  The
 * picture itself is made by the mosaic layer's blend kernel through its exported entry (mdemod_mosaic_blend_device); there is no
 * second warp or blend here.
 *
 * polar_nodes: one thread per node, blockIdx.y the pass, all passes in one launch.  Everything is double: the node's (E, N) through
 *   the inverse projection (csrc/polar_proj.h, the host's own formulas) to (phi, lam), the geodetic point G, the seed from the
 *   pass's table of r(t) every 8 s (the entry with the largest G . r), at most 12 Newton steps on G . v(t) = 0 with the map layer's
 *   frame formulas, the visibility and margin checks, theta by atan2, the rounding to int32.  The map layer's solver
 *   (csrc/map_host.cpp: Inverse::solve) is the specification, statement by statement; the two differ where the device's libm and
 *   glibc differ in the last place (the rule of agreement is in the header).  Omega, u and the sidereal angle arrive as values at the
 *   table's start plus rates, and times run from the table's start, so sines and cosines see arguments of a few radians.  The pass
 *   constants travel by value in the kernel arguments and are indexed by blockIdx.y, which is uniform: scalar loads.  The table is
 *   read at uniform addresses by every lane.  A node is written with two ordinary dword stores into the buffer the blend reads.
 *   This file is compiled without FMA contraction (-ffp-contract=off, as the whole library): the Newton loop does not depend on
 *   what the compiler would fuse.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "polar_host.h"
#include "hip_host.h"
#include "../../include/meteor_demod_amd_overlay.h"

#define POLAR_THREADS   256
#define POLAR_RE        6378.137                        /* km: the map layer's constants */
#define POLAR_B         (POLAR_RE * (1.0 - POLAR_F))
#define POLAR_TABLE_STEP 8.0
#define POLAR_NEWTON_MAX 12
#define POLAR_TABLE_TOP (1u << 20)

/* one pass; times (tau) in seconds from the table's start */
struct PolarPassArgs {
	double a, ci, si, raan, u, g, raan_rate, u_rate, g_rate;
	double tau_lo, tau_hi, theta_max, y_bias, line_period, step;
	const double *table;
	int32_t *nodes;
	uint32_t table_n;
	int32_t side;
};

struct PolarNodesArgs {
	PolarPassArgs pass[POLAR_MAX];
	PolarProj proj;
	double e_left, n_top, res;
	uint32_t node_rows, node_cols;
};

struct PolarFrame3 { double r[3], v[3], h[3]; };

/* the map layer's frame_at with the angles linear in tau */
__device__ __forceinline__ void
polar_frame_at(const PolarPassArgs &p, double tau, PolarFrame3 &f)
{
	const double raan = p.raan + p.raan_rate * tau, u = p.u + p.u_rate * tau, g = p.g + p.g_rate * tau;
	const double cO = cos(raan), sO = sin(raan), cu = cos(u), su = sin(u), cg = cos(g), sg = sin(g);
	const double r[3] = { cO * cu - sO * su * p.ci, sO * cu + cO * su * p.ci, su * p.si };
	const double v[3] = { -cO * su - sO * cu * p.ci, -sO * su + cO * cu * p.ci, cu * p.si };
	const double h[3] = { sO * p.si, -cO * p.si, p.ci };
	f.r[0] = r[0] * cg + r[1] * sg; f.r[1] = -r[0] * sg + r[1] * cg; f.r[2] = r[2];
	f.v[0] = v[0] * cg + v[1] * sg; f.v[1] = -v[0] * sg + v[1] * cg; f.v[2] = v[2];
	f.h[0] = h[0] * cg + h[1] * sg; f.h[1] = -h[0] * sg + h[1] * cg; f.h[2] = h[2];
}

__device__ __forceinline__ double polar_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* the source pixel that sees (phi, lam); false: no node */
__device__ __forceinline__ bool
polar_solve(const PolarPassArgs &p, double phi, double lam, double &y, double &x)
{
	const double sp = sin(phi), cp = cos(phi), N = POLAR_RE / sqrt(1.0 - POLAR_E2 * sp * sp);
	const double G[3] = { N * cp * cos(lam), N * cp * sin(lam), N * (1.0 - POLAR_E2) * sp };
	uint32_t best = 0;
	double most = -1.0e30;
	for (uint32_t k = 0; k < p.table_n; k++) {
		const double d = polar_dot(G, p.table + 3 * static_cast<size_t>(k));
		if (d > most) { most = d; best = k; }
	}
	double tau = POLAR_TABLE_STEP * static_cast<double>(best);
	PolarFrame3 f;
	bool done = false;
	for (int it = 0; it < POLAR_NEWTON_MAX && !done; it++) {
		polar_frame_at(p, tau, f);
		const double zxv[3] = { -f.v[1], f.v[0], 0.0 };
		const double slope = -p.u_rate * polar_dot(G, f.r) - p.g_rate * polar_dot(G, zxv);
		if (!(fabs(slope) > 1.0e-9)) return false;
		double dt = -polar_dot(G, f.v) / slope;
		if (!isfinite(dt)) return false;
		dt = dt > 60.0 ? 60.0 : dt < -60.0 ? -60.0 : dt;
		tau += dt;
		done = fabs(dt) < 1.0e-7;
		if (tau < p.tau_lo - 600.0 || tau > p.tau_hi + 600.0) return false;
	}
	if (!done || tau < p.tau_lo || tau > p.tau_hi) return false;
	polar_frame_at(p, tau, f);
	double D[3];
	for (int k = 0; k < 3; k++) D[k] = G[k] - p.a * f.r[k];
	const double normal[3] = { G[0] / (POLAR_RE * POLAR_RE), G[1] / (POLAR_RE * POLAR_RE), G[2] / (POLAR_B * POLAR_B) };
	if (!(polar_dot(D, normal) < 0.0)) return false;
	const double theta = atan2(p.side * polar_dot(D, f.h), -polar_dot(D, f.r));
	if (!(fabs(theta) <= p.theta_max)) return false;
	y = (tau + p.y_bias) / p.line_period;
	x = theta / p.step + 783.5;
	return true;
}

__global__ void __launch_bounds__(POLAR_THREADS)
polar_nodes(PolarNodesArgs a)
{
	const uint32_t at = blockIdx.x * POLAR_THREADS + threadIdx.x, count = a.node_rows * a.node_cols;
	if (at >= count) return;
	const PolarPassArgs &p = a.pass[blockIdx.y];
	const uint32_t row = at / a.node_cols, col = at % a.node_cols;
	double phi, lam, y, x;
	polar_inverse(a.proj, a.e_left + (MAP_STEP * col + 0.5) * a.res, a.n_top - (MAP_STEP * row + 0.5) * a.res, phi, lam);
	int32_t X = MDEMOD_POLAR_NO_NODE, Y = MDEMOD_POLAR_NO_NODE;
	if (polar_solve(p, phi, lam, y, x)) {
		const double fx = floor(256.0 * x + 0.5), fy = floor(256.0 * y + 0.5);
		if (fabs(fx) < 2.0e9 && fabs(fy) < 2.0e9) { X = static_cast<int32_t>(fx); Y = static_cast<int32_t>(fy); }
	}
	int32_t *node = p.nodes + 2 * static_cast<size_t>(at);
	node[0] = X;
	node[1] = Y;
}

namespace {

#define REFUSE(...) do { mdm_note_error(__VA_ARGS__); return MDEMOD_ERR_PARAM; } while (0)

uint64_t
table_bytes(const mdemod_polar_solver &s)
{
	return 3ull * s.table_n * sizeof(double);
}

int
check_solver(const char *who, const mdemod_polar_solver &s, uint32_t k)
{
	const double nums[] = { s.a, s.cos_i, s.sin_i, s.raan, s.u, s.g, s.raan_rate, s.u_rate, s.g_rate, s.table_t0, s.sec_lo, s.sec_hi, s.theta_max, s.s0, s.line_period,
	                        s.time_offset, s.step };
	for (double v : nums)
		if (!std::isfinite(v)) REFUSE("%s: a constant of pass %u is not a number", who, k);
	if (!(s.line_period > 0.0) || !(s.step > 0.0) || !(s.a > 0.0)) REFUSE("%s: the line period, the column step and the radius of pass %u must be positive", who, k);
	if (s.side != 1 && s.side != -1) REFUSE("%s: the scan side of pass %u is %d (1 or -1)", who, k, s.side);
	if (!s.table || !s.table_n) REFUSE("%s: the table of pass %u is needed", who, k);
	if (s.table_n > POLAR_TABLE_TOP) REFUSE("%s: the table of pass %u has %u entries (at most %u)", who, k, s.table_n, POLAR_TABLE_TOP);
	return MDEMOD_OK;
}

/* the tables to work_dev and the launch; everything was checked */
int
nodes_run(const mdemod_polar_frame &f, const mdemod_polar_solver *solvers, uint32_t n, int32_t *const *nodes_dev, void *work_dev, hipStream_t st)
{
	if (!n) return MDEMOD_OK;
	PolarNodesArgs a;
	memset(&a, 0, sizeof a);
	uint8_t *work = static_cast<uint8_t *>(work_dev);
	for (uint32_t k = 0; k < n; k++) {
		const mdemod_polar_solver &s = solvers[k];
		PolarPassArgs &p = a.pass[k];
		p.a = s.a; p.ci = s.cos_i; p.si = s.sin_i; p.raan = s.raan; p.u = s.u; p.g = s.g; p.raan_rate = s.raan_rate; p.u_rate = s.u_rate; p.g_rate = s.g_rate;
		p.tau_lo = s.sec_lo - s.table_t0; p.tau_hi = s.sec_hi - s.table_t0; p.theta_max = s.theta_max;
		p.y_bias = s.table_t0 + s.time_offset - s.s0; p.line_period = s.line_period; p.step = s.step;
		p.table = reinterpret_cast<const double *>(work); p.nodes = nodes_dev[k]; p.table_n = s.table_n; p.side = s.side;
		/* (pageable host memory: the runtime has taken the bytes when the call returns) */
		HIP_TRY(hipMemcpyAsync(work, s.table, table_bytes(s), hipMemcpyHostToDevice, st));
		work += table_bytes(s);
	}
	a.proj = polar_proj_of(f);
	a.e_left = f.e_left; a.n_top = f.n_top; a.res = f.res; a.node_rows = f.node_rows; a.node_cols = f.node_cols;
	const uint32_t count = f.node_rows * f.node_cols;
	hipLaunchKernelGGL(polar_nodes, dim3((count + POLAR_THREADS - 1) / POLAR_THREADS, n), dim3(POLAR_THREADS), 0, st, a);
	HIP_TRY(hipGetLastError());
	return MDEMOD_OK;
}

/* the whole-picture entry: every pass's slots up once, the nodes made here (or brought up), one band down at a time through the
 * mosaic layer's blend entry, on the null stream */
struct DeviceBackend : MosaicBackend {
	MdmDevMem mem;
	uint8_t *d_image[POLAR_MAX][3] = {}, *d_filled[POLAR_MAX][3] = {}, *d_lut = nullptr, *d_out = nullptr, *d_valid = nullptr, *d_cover = nullptr, *d_work = nullptr;
	int32_t *d_nodes[POLAR_MAX] = {};
	uint32_t *d_hist = nullptr;
	uint32_t rows[POLAR_MAX] = {}, n = 0, width = 0, node_cols = 0, planes = 0;
	size_t node_words = 0;
	const mdemod_polar_nodes &polar;
	bool on_host;
	int device;
	DeviceBackend(int dev, const mdemod_polar_nodes &grid, bool host_nodes) : polar(grid), on_host(host_nodes), device(dev) {}

	int begin(const mdemod_mosaic_pass *passes, const mdemod_mosaic_nodes &grid, uint32_t pl, uint32_t piece_lines) override
	{
		int rc;
		n = grid.n; width = grid.width; node_cols = grid.node_cols; planes = pl;
		node_words = 2 * static_cast<size_t>(grid.node_rows) * grid.node_cols;
		for (uint32_t k = 0; k < n; k++) {
			rows[k] = passes[k].rows;
			for (int s = 0; s < 3; s++) {
				if (!passes[k].image[s]) continue;
				if ((rc = mem.alloc(&d_image[k][s], rows[k] * PIC_LINE_BYTES)) || (rc = mem.alloc(&d_filled[k][s], static_cast<size_t>(rows[k]) * PIC_CELLS))) return rc;
				HIP_TRY(hipMemcpyAsync(d_image[k][s], passes[k].image[s], rows[k] * PIC_LINE_BYTES, hipMemcpyHostToDevice, nullptr));
				HIP_TRY(hipMemcpyAsync(d_filled[k][s], passes[k].filled[s], static_cast<size_t>(rows[k]) * PIC_CELLS, hipMemcpyHostToDevice, nullptr));
			}
			if ((rc = mem.alloc(&d_nodes[k], node_words))) return rc;
			if (on_host) HIP_TRY(hipMemcpyAsync(d_nodes[k], grid.nodes[k], node_words * sizeof(int32_t), hipMemcpyHostToDevice, nullptr));
		}
		if (!on_host) {
			if ((rc = mem.alloc(&d_work, static_cast<size_t>(mdemod_polar_nodes_work_bytes(polar.solver, n))))) return rc;
			if ((rc = nodes_run(polar.frame, polar.solver, n, d_nodes, d_work, nullptr))) return rc;
		}
		if ((rc = mem.alloc(&d_lut, static_cast<size_t>(POLAR_MAX) * 3 * 256)) || (rc = mem.alloc(&d_hist, 3 * 256)) ||
		    (rc = mem.alloc(&d_out, static_cast<size_t>(piece_lines) * width * planes)) || (rc = mem.alloc(&d_valid, static_cast<size_t>(piece_lines) * width)) ||
		    (rc = mem.alloc(&d_cover, static_cast<size_t>(piece_lines) * width)))
			return rc;
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int histogram(uint32_t k, uint32_t *hist) override
	{
		const int rc = mdemod_picture_histogram_device(d_image[k], d_filled[k], rows[k], d_hist, device, nullptr);
		if (rc) return rc;
		HIP_TRY(hipMemcpyAsync(hist, d_hist, 3 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int tables(const uint8_t *lut, uint32_t pl) override
	{
		HIP_TRY(hipMemcpyAsync(d_lut, lut, static_cast<size_t>(n) * pl * 256, hipMemcpyHostToDevice, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	int band(const uint32_t *select, uint32_t pl, uint32_t blend, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid, uint8_t *cover) override
	{
		mdemod_mosaic_source src[POLAR_MAX];
		memset(src, 0, sizeof src);
		for (uint32_t k = 0; k < n; k++) {
			for (int s = 0; s < 3; s++) { src[k].image[s] = d_image[k][s]; src[k].filled[s] = d_filled[k][s]; }
			src[k].lut = d_lut + static_cast<size_t>(k) * pl * 256;
			src[k].nodes = d_nodes[k] + 2 * static_cast<size_t>(node_row) * node_cols;
			src[k].rows = rows[k];
		}
		const int rc = mdemod_mosaic_blend_device(src, n, select, pl, blend, width, height, d_out, d_valid, d_cover, device, nullptr);
		if (rc) return rc;
		HIP_TRY(hipMemcpyAsync(out, d_out, static_cast<size_t>(height) * width * pl, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipMemcpyAsync(valid, d_valid, static_cast<size_t>(height) * width, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipMemcpyAsync(cover, d_cover, static_cast<size_t>(height) * width, hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}

	/* the nodes the picture was made through, for the result */
	int fetch(int32_t *const *nodes)
	{
		for (uint32_t k = 0; k < n; k++) HIP_TRY(hipMemcpyAsync(nodes[k], d_nodes[k], node_words * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return MDEMOD_OK;
	}
};

} /* namespace */

extern "C" {

uint64_t
mdemod_polar_nodes_work_bytes(const mdemod_polar_solver *solvers, uint32_t n)
{
	uint64_t sum = 0;
	for (uint32_t k = 0; solvers && k < n && k < POLAR_MAX; k++) sum += table_bytes(solvers[k]);
	return sum;
}

int
mdemod_polar_nodes_device(const mdemod_polar_frame *frame, const mdemod_polar_solver *solvers, uint32_t n, int32_t *const *nodes_dev, void *work_dev,
                          uint64_t work_bytes, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_polar_nodes_device";
	int rc = polar_check_frame(who, frame);
	if (rc) return rc;
	if (n > POLAR_MAX) REFUSE("%s: %u passes are more than a polar picture takes (8)", who, n);
	if (!n) return MDEMOD_OK;
	if (!solvers || !nodes_dev) REFUSE("%s: the passes and their node buffers are needed", who);
	for (uint32_t k = 0; k < n; k++)
		if ((rc = check_solver(who, solvers[k], k))) return rc;
	const uint64_t need = mdemod_polar_nodes_work_bytes(solvers, n), node_bytes = 8ull * frame->node_rows * frame->node_cols;
	if (!work_dev) REFUSE("%s: the work buffer is needed", who);
	if (work_bytes < need) REFUSE("%s: the work buffer has %llu bytes, the tables take %llu", who, static_cast<unsigned long long>(work_bytes), static_cast<unsigned long long>(need));
	if (reinterpret_cast<uintptr_t>(work_dev) & 7u) REFUSE("%s: the work buffer must stand at a multiple of 8 bytes", who);
	for (uint32_t k = 0; k < n; k++) {
		if (!nodes_dev[k]) REFUSE("%s: the node buffer of pass %u is needed", who, k);
		if (reinterpret_cast<uintptr_t>(nodes_dev[k]) & 3u) REFUSE("%s: the node buffers must stand at multiples of 4 bytes", who);
	}
	bool hit = false;
	for (uint32_t k = 0; k < n; k++) {
		hit = hit || mdm_ranges_intersect(nodes_dev[k], node_bytes, work_dev, need);
		for (uint32_t j = 0; j < k; j++) hit = hit || mdm_ranges_intersect(nodes_dev[k], node_bytes, nodes_dev[j], node_bytes);
	}
	if (hit) REFUSE("%s: the node buffers and the work buffer intersect", who);
	if ((rc = mdm_select_device(device))) return rc;
	return nodes_run(*frame, solvers, n, nodes_dev, work_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_polar_draw_host(const mdemod_polar_points *const *layers, const uint32_t *style_of, uint32_t n_layers, const mdemod_polar_style *styles, uint32_t n_styles,
                       uint32_t width, uint32_t height, uint32_t planes, uint8_t *pixels, const uint8_t *valid, mdemod_polar_drawn *report, int device)
try { MDEMOD_API_ENTER
	const char *who = "mdemod_polar_draw_host";
	static_assert(sizeof(mdemod_polar_points) == sizeof(mdemod_overlay_points) && offsetof(mdemod_polar_points, first) == offsetof(mdemod_overlay_points, first) &&
	              offsetof(mdemod_polar_points, n_points) == offsetof(mdemod_overlay_points, n_points) && sizeof(mdemod_polar_style) == sizeof(mdemod_overlay_style) &&
	              offsetof(mdemod_polar_style, inside_only) == offsetof(mdemod_overlay_style, inside_only), "points and styles go to the overlay layer as they are");
	if (report) memset(report, 0, sizeof *report);
	if (n_layers && (!layers || !style_of)) REFUSE("%s: the layers and their styles are needed", who);
	if (!styles || !n_styles || n_styles > MDEMOD_OVERLAY_MAX_STYLES) REFUSE("%s: %u styles (1 .. 4)", who, n_styles);
	if (!pixels) REFUSE("%s: the picture is needed", who);
	if (planes != 1 && planes != 3) REFUSE("%s: %u planes (1 or 3)", who, planes);
	const mdemod_overlay_style *st = reinterpret_cast<const mdemod_overlay_style *>(styles);
	mdemod_overlay_pieces pieces;
	mdemod_overlay_bins bins;
	memset(&pieces, 0, sizeof pieces);
	memset(&bins, 0, sizeof bins);
	struct Keep { mdemod_overlay_pieces *p; mdemod_overlay_bins *b; ~Keep() { mdemod_overlay_pieces_free(p); mdemod_overlay_bins_free(b); } } keep{ &pieces, &bins };
	int rc;
	for (uint32_t l = 0; l < n_layers; l++) {
		if (!layers[l]) REFUSE("%s: layer %u is missing", who, l);
		if (style_of[l] >= n_styles) REFUSE("%s: layer %u has style %u of %u", who, l, style_of[l], n_styles);
		const uint64_t before = pieces.n;
		if ((rc = mdemod_overlay_cut(reinterpret_cast<const mdemod_overlay_points *>(layers[l]), style_of[l], st[style_of[l]].half_width, width, height, &pieces))) return rc;
		if (report) report->pieces[style_of[l]] += pieces.n - before;
	}
	if ((rc = mdemod_overlay_bin(pieces.piece, pieces.n, st, n_styles, width, height, &bins))) return rc;
	const uint64_t tiles = static_cast<uint64_t>(bins.tiles_x) * bins.tiles_y;
	if (report) {
		report->items = bins.n_items;
		for (uint64_t t = 0; t < tiles; t++) report->tiles += bins.tile_first[t + 1] != bins.tile_first[t];
	}
	if ((rc = mdm_select_device(device))) return rc;
	MdmDevMem mem;
	mdemod_overlay_piece *d_pieces = nullptr;
	uint32_t *d_first = nullptr, *d_items = nullptr;
	uint8_t *d_pixels = nullptr, *d_valid = nullptr;
	const size_t area = static_cast<size_t>(height) * width;
	if ((rc = mem.alloc(&d_pieces, pieces.n)) || (rc = mem.alloc(&d_first, tiles + 1)) || (rc = mem.alloc(&d_items, bins.n_items)) || (rc = mem.alloc(&d_pixels, area * planes)) ||
	    (valid && (rc = mem.alloc(&d_valid, area))))
		return rc;
	if (pieces.n) HIP_TRY(hipMemcpyAsync(d_pieces, pieces.piece, pieces.n * sizeof *d_pieces, hipMemcpyHostToDevice, nullptr));
	HIP_TRY(hipMemcpyAsync(d_first, bins.tile_first, (tiles + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
	if (bins.n_items) HIP_TRY(hipMemcpyAsync(d_items, bins.items, bins.n_items * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
	if (area) HIP_TRY(hipMemcpyAsync(d_pixels, pixels, area * planes, hipMemcpyHostToDevice, nullptr));
	if (valid && area) HIP_TRY(hipMemcpyAsync(d_valid, valid, area, hipMemcpyHostToDevice, nullptr));
	if ((rc = mdemod_overlay_draw_device(d_pieces, pieces.n, d_first, d_items, bins.n_items, st, n_styles, width, height, planes, d_pixels, d_valid, nullptr, device, nullptr)))
		return rc;
	if (area) HIP_TRY(hipMemcpyAsync(pixels, d_pixels, area * planes, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_polar_compose_host(const mdemod_polar_opts *opts, const mdemod_polar_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                          mdemod_polar_result *out, int device)
try { MDEMOD_API_ENTER
	if (out) memset(out, 0, sizeof *out);                                      /* (a refusal leaves nothing to free) */
	mdemod_polar_opts o;
	int rc = polar_settings(opts, o);
	if (rc) return rc;
	if ((rc = polar_check_compose("mdemod_polar_compose_host", passes, n, select, planes, out))) return rc;
	mdemod_polar_nodes grid;
	if ((rc = polar_grid_make("mdemod_polar_compose_host", o, passes, n, nullptr, o.nodes_on_host != 0, &grid))) return rc;
	struct Keep { mdemod_polar_nodes *g; ~Keep() { mdemod_polar_grid_free(g); } } keep{ &grid };
	if ((rc = mdm_select_device(device))) return rc;
	DeviceBackend dev(device, grid, o.nodes_on_host != 0);
	if ((rc = polar_compose(o, passes, n, select, planes, grid, out, dev))) return rc;
	if (!o.nodes_on_host && (rc = dev.fetch(out->nodes))) { mdemod_polar_free(out); return rc; }
	return MDEMOD_OK;
} MDEMOD_API_CATCH

} /* extern "C" */
