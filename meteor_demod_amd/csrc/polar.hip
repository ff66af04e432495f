/*
 * polar.hip — the polar layer on the GPU (include/meteor_demod_amd_polar.h): polar_nodes, and the public entries around it.  The
 * picture itself is made by the mosaic layer's blend kernel through that layer's own device backend (csrc/mosaic_device.h), and the
 * lines are drawn by the overlay layer's banded draw (csrc/overlay_host.h: overlay_draw_points_device); there is no second warp,
 * blend or draw here.
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
#include "mosaic_device.h"
#include "overlay_host.h"

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

/* the whole-picture entry: the mosaic layer's backend (csrc/mosaic_device.h: slots up once, tables, one band down at a time through
 * its blend) with the nodes made on the device, in the backend's own memory, unless they come from the host */
struct DeviceBackend : MosaicDeviceBackend {
	const mdemod_polar_nodes &polar;
	bool on_host;
	DeviceBackend(int dev, const mdemod_polar_nodes &grid, bool host_nodes) : MosaicDeviceBackend(dev), polar(grid), on_host(host_nodes) {}

	int nodes_in(const mdemod_mosaic_nodes &grid) override
	{
		if (on_host) return MosaicDeviceBackend::nodes_in(grid);
		uint8_t *d_work = nullptr;
		const int rc = mem.alloc(&d_work, static_cast<size_t>(mdemod_polar_nodes_work_bytes(polar.solver, n)));
		return rc ? rc : nodes_run(polar.frame, polar.solver, n, d_nodes, d_work, nullptr);
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
	MdmBuffers b;
	b.out(work_dev, need);
	for (uint32_t k = 0; k < n; k++) b.out(nodes_dev[k], node_bytes);
	if (!b.apart()) REFUSE("%s: the node buffers and the work buffer intersect", who);
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
	int rc = overlay_check_draw(who, st, n_styles, width, height, planes, pixels, valid);
	if (rc) return rc;
	for (uint32_t l = 0; l < n_layers; l++) {
		if (!layers[l]) REFUSE("%s: layer %u is missing", who, l);
		if (style_of[l] >= n_styles) REFUSE("%s: layer %u has style %u of %u", who, l, style_of[l], n_styles);
	}
	mdemod_overlay_report drawn;
	if ((rc = overlay_draw_points_device(reinterpret_cast<const mdemod_overlay_points *const *>(layers), style_of, n_layers, st, n_styles, width, height, planes, pixels, valid,
	                                     &drawn, device)))
		return rc;
	if (report) {
		memcpy(report->pieces, drawn.pieces, sizeof report->pieces);
		report->tiles = drawn.tiles;
		report->items = drawn.items;
	}
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
