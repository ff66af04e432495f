/*
 * mosaic_host.cpp — host side of the mosaic layer (include/meteor_demod_amd_mosaic.h): the common grid of several passes out of the
 * map layer's pieces (csrc/map_host.h: border samples, frame, nodes on a prescribed frame), the stretch tables, the bands of the
 * whole-mosaic entry, and the host model of the kernel of csrc/mosaic.hip (mdemod_mosaic_model_*: the blend as a plain loop over
 * the warp's model, which is the map layer's: csrc/warp_model.h).  Free of the GPU runtime.
 */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mosaic_host.h"
#include "mdemod_internal_api.h"
#include "warp_model.h"

namespace {

void
model_blend(const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width, uint32_t height,
            uint8_t *out, uint8_t *valid, uint8_t *cover)
{
	const uint32_t nc = map_node_count(width);
	for (uint32_t i = 0; i < height; i++)
		for (uint32_t j = 0; j < width; j++) {
			uint64_t sum[3] = { 0, 0, 0 }, weight[3] = { 0, 0, 0 };
			uint32_t best[3] = { 0, 0, 0 };
			uint8_t seen = 0, from = 0;
			for (uint32_t k = 0; k < n; k++) {
				const mdemod_mosaic_source &s = sources[k];
				int64_t X, Y;
				if (!s.rows || !warp_model_point(s.nodes, nc, s.rows, i, j, X, Y)) continue;       /* an empty pass, or nothing of it here */
				const int64_t y_top = (8ll * s.rows - 1) * 256;
				int64_t e = X < MAP_X_TOP - X ? X : MAP_X_TOP - X;
				e = Y < e ? Y : e;
				e = y_top - Y < e ? y_top - Y : e;
				const uint64_t w = 1 + static_cast<uint64_t>(e >> 8);
				for (uint32_t p = 0; p < planes; p++) {
					uint32_t v;
					if (!warp_model_value(s.image[select[p]], s.filled[select[p]], s.rows, X, Y, v)) continue;
					const uint64_t b = s.lut[256 * p + v];
					if (blend == MDEMOD_MOSAIC_FEATHER) { sum[p] += w * b; weight[p] += w; from |= static_cast<uint8_t>(1u << k); }
					else if (w > weight[p]) { sum[p] = b; weight[p] = w; best[p] = k; }
					seen |= static_cast<uint8_t>(1u << p);
				}
			}
			uint8_t *px = out + (static_cast<size_t>(i) * width + j) * planes;
			for (uint32_t p = 0; p < planes; p++)
				px[p] = !weight[p] ? 0 : blend == MDEMOD_MOSAIC_FEATHER ? static_cast<uint8_t>((sum[p] + (weight[p] >> 1)) / weight[p]) : static_cast<uint8_t>(sum[p]);
			if (blend == MDEMOD_MOSAIC_BEST)
				for (uint32_t p = 0; p < planes; p++)
					if (weight[p]) from |= static_cast<uint8_t>(1u << best[p]);
			if (valid) valid[static_cast<size_t>(i) * width + j] = seen;
			if (cover) cover[static_cast<size_t>(i) * width + j] = from;
		}
}

mdemod_map_opts
map_opts_of(const mdemod_mosaic_opts &o, int32_t date)
{
	mdemod_map_opts m;
	mdemod_map_default_opts(&m);
	m.scan_deg = o.scan_deg; m.px_per_deg = o.px_per_deg; m.time_offset = o.time_offset; m.row_period = o.row_period;
	m.side = o.side; m.date = date; m.stretch = o.stretch ? 1 : 0; m.clip_low = o.clip_low; m.clip_high = o.clip_high; m.piece_lines = o.piece_lines;
	return m;
}

struct ModelBackend : MosaicBackend {
	mdemod_mosaic_source src[MOSAIC_MAX];
	const uint8_t *lut = nullptr;
	uint32_t n = 0, width = 0, nc = 0;
	int begin(const mdemod_mosaic_pass *passes, const mdemod_mosaic_nodes &grid, uint32_t, uint32_t) override
	{
		n = grid.n; width = grid.width; nc = grid.node_cols;
		memset(src, 0, sizeof src);
		for (uint32_t k = 0; k < n; k++) {
			for (int s = 0; s < 3; s++) { src[k].image[s] = passes[k].image[s]; src[k].filled[s] = passes[k].filled[s]; }
			src[k].nodes = grid.nodes[k];
			src[k].rows = passes[k].rows;
		}
		return MDEMOD_OK;
	}
	int histogram(uint32_t k, uint32_t *hist) override { return mdemod_picture_model_histogram(src[k].image, src[k].filled, src[k].rows, hist); }
	int tables(const uint8_t *t, uint32_t planes) override
	{
		for (uint32_t k = 0; k < n; k++) src[k].lut = t + static_cast<size_t>(k) * planes * 256;
		return MDEMOD_OK;
	}
	int band(const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t node_row, uint32_t height, uint8_t *out, uint8_t *valid, uint8_t *cover) override
	{
		mdemod_mosaic_source at[MOSAIC_MAX];
		for (uint32_t k = 0; k < n; k++) { at[k] = src[k]; at[k].nodes += 2 * static_cast<size_t>(node_row) * nc; }
		model_blend(at, n, select, planes, blend, width, height, out, valid, cover);
		return MDEMOD_OK;
	}
};

} /* namespace */

std::unique_ptr<MosaicBackend> mosaic_model_backend() { return std::unique_ptr<MosaicBackend>(new ModelBackend); }

int
mosaic_settings(const mdemod_mosaic_opts *opts, mdemod_mosaic_opts &out)
{
	mdemod_mosaic_default_opts(&out);
	if (opts) out = *opts;
	/* the fields shared with the map layer are checked by the map layer, with its texts */
	const mdemod_map_opts m = map_opts_of(out, MDEMOD_MAP_DATE_AUTO);
	mdemod_map_opts done;
	const int rc = map_settings(&m, done);
	if (rc) return rc;
	if (out.stretch > 2) REFUSE("mosaic: stretch is %u (0: none, 1: joint, 2: per pass)", out.stretch);
	if (out.blend > MDEMOD_MOSAIC_BEST) REFUSE("mosaic: blend is %u (0: feather, 1: best)", out.blend);
	out.piece_lines = done.piece_lines;
	return MDEMOD_OK;
}

int
mosaic_check_blend(const char *who, const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width,
                   uint32_t height)
{
	if (n > MOSAIC_MAX) REFUSE("%s: %u passes are more than a mosaic takes (8)", who, n);
	if (n && !sources) REFUSE("%s: the passes are needed", who);
	if (blend > MDEMOD_MOSAIC_BEST) REFUSE("%s: blend is %u (0: feather, 1: best)", who, blend);
	uint32_t most = 0;
	for (uint32_t k = 0; k < n; k++) most = sources[k].rows > most ? sources[k].rows : most;
	return map_check_warp(who, most, select, planes, width, height);
}

int
mosaic_check_sources(const char *who, const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes)
{
	for (uint32_t k = 0; k < n; k++) {
		if (!sources[k].rows) continue;
		for (uint32_t p = 0; p < planes; p++)
			if (!sources[k].image[select[p]] || !sources[k].filled[select[p]]) REFUSE("%s: the picture and the mask of slot %u of pass %u are needed", who, select[p], k);
		if (!sources[k].lut || !sources[k].nodes) REFUSE("%s: the tables and the nodes of pass %u are needed", who, k);
	}
	return MDEMOD_OK;
}

int
mosaic_check_compose(const char *who, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes, mdemod_mosaic_result *out)
{
	int rc;
	if (!out) REFUSE("%s: the result is needed", who);
	if (!n) REFUSE("%s: no pass: a mosaic takes 1 .. 8", who);
	if (n > MOSAIC_MAX) REFUSE("%s: %u passes are more than a mosaic takes (1 .. 8)", who, n);
	if (!passes) REFUSE("%s: the passes are needed", who);
	if ((rc = pic_check_select(who, 0, select, planes))) return rc;
	for (uint32_t k = 0; k < n; k++) {
		const mdemod_mosaic_pass &p = passes[k];
		if (!p.tle_text) REFUSE("%s: the element set of pass %u is needed", who, k);
		if (!p.rows) REFUSE("%s: pass %u has no strip rows: it cannot be put on a map", who, k);
		if (p.rows > MDEMOD_MAP_MAX_ROWS) REFUSE("%s: the %u strip rows of pass %u are more than a map takes (8192)", who, p.rows, k);
		if ((rc = pic_check_slots(who, p.image, p.filled, select, planes))) return rc;
		if (p.n_desc && (!p.place || !p.sinfo)) REFUSE("%s: the placements and the reports of the packets of pass %u are needed", who, k);
	}
	return MDEMOD_OK;
}

int
mosaic_compose_bands(const mdemod_mosaic_opts &o, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                     mdemod_mosaic_result *out, MosaicBackend &backend)
{
	memset(out, 0, sizeof *out);
	mdemod_mosaic_nodes grid;
	const int rc = mdemod_mosaic_grid(&o, passes, n, &grid);
	if (rc) return rc;
	struct Keep { mdemod_mosaic_nodes *g; ~Keep() { mdemod_mosaic_grid_free(g); } } keep{ &grid };
	return mosaic_bands_on(o, passes, n, select, planes, grid, out, backend);
}

int
mosaic_bands_on(const mdemod_mosaic_opts &o, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                const mdemod_mosaic_nodes &grid, mdemod_mosaic_result *out, MosaicBackend &backend)
{
	int rc;
	memset(out, 0, sizeof *out);
	out->width = grid.width; out->height = grid.height; out->planes = planes; out->sx = grid.sx; out->n = n; out->blend = o.blend;
	out->sy = grid.sy; out->lat_top = grid.lat_top; out->lon_left = grid.lon_left;
	for (uint32_t k = 0; k < n; k++) {
		out->timing[k] = grid.timing[k];
		out->utc0[k] = grid.timing[k].s0 - o.time_offset;
	}
	/* only the selected slots are looked at */
	std::vector<mdemod_mosaic_pass> chosen(passes, passes + n);
	for (uint32_t k = 0; k < n; k++) {
		for (int s = 0; s < 3; s++) chosen[k].image[s] = chosen[k].filled[s] = nullptr;
		for (uint32_t p = 0; p < planes; p++) { chosen[k].image[select[p]] = passes[k].image[select[p]]; chosen[k].filled[select[p]] = passes[k].filled[select[p]]; }
	}
	const uint32_t P = o.piece_lines < grid.height ? o.piece_lines : (grid.height + MAP_STEP - 1) / MAP_STEP * MAP_STEP;
	if ((rc = backend.begin(chosen.data(), grid, planes, P))) return rc;
	/* the tables: [n][planes][256] */
	std::vector<uint32_t> hist(static_cast<size_t>(n) * 3 * 256, 0), joint(3 * 256, 0);
	if (o.stretch)
		for (uint32_t k = 0; k < n; k++) {
			if ((rc = backend.histogram(k, hist.data() + static_cast<size_t>(k) * 768))) return rc;
			for (uint32_t p = 0; p < planes; p++)
				for (int v = 0; v < 256; v++) joint[256 * p + v] += hist[static_cast<size_t>(k) * 768 + 256 * select[p] + v];
		}
	std::vector<uint8_t> lut(static_cast<size_t>(n) * planes * 256);
	for (uint32_t k = 0; k < n; k++)
		for (uint32_t p = 0; p < planes; p++) {
			uint8_t *t = lut.data() + (static_cast<size_t>(k) * planes + p) * 256;
			uint32_t lim[2] = { 0, 255 };
			if (o.stretch) {
				const uint32_t *h = o.stretch == 1 ? joint.data() + 256 * p : hist.data() + static_cast<size_t>(k) * 768 + 256 * select[p];
				if ((rc = mdemod_picture_lut(h, o.clip_low, o.clip_high, t, lim))) return rc;
			} else {
				for (int v = 0; v < 256; v++) t[v] = static_cast<uint8_t>(v);
			}
			out->lo[k][p] = lim[0];
			out->hi[k][p] = lim[1];
		}
	if ((rc = backend.tables(lut.data(), planes))) return rc;
	const size_t W = grid.width, H = grid.height;
	out->pixels = static_cast<uint8_t *>(malloc(H * W * planes));
	out->valid = static_cast<uint8_t *>(malloc(H * W));
	out->cover = static_cast<uint8_t *>(malloc(H * W));
	if (!out->pixels || !out->valid || !out->cover) { mdemod_mosaic_free(out); return MDEMOD_ERR_NOMEM; }
	for (uint32_t at = 0; at < H; at += P) {
		rc = backend.band(select, planes, o.blend, at / MAP_STEP, P < H - at ? P : static_cast<uint32_t>(H - at), out->pixels + at * W * planes, out->valid + at * W,
		                  out->cover + at * W);
		if (rc) { mdemod_mosaic_free(out); return rc; }
	}
	for (size_t i = 0; i < H * W; i++) {
		const uint8_t c = out->cover[i];
		out->valid_pixels += out->valid[i] != 0;
		out->overlap_pixels += (c & (c - 1)) != 0;
		for (uint32_t k = 0; k < n; k++) out->covered[k] += (c >> k) & 1u;
	}
	return MDEMOD_OK;
}

extern "C" {

void
mdemod_mosaic_default_opts(mdemod_mosaic_opts *opts)
{
	if (!opts) return;
	opts->scan_deg = 110.0;
	opts->px_per_deg = 100.0;
	opts->time_offset = 10800.0;
	opts->row_period = 8.0 / 6.5;
	opts->side = 1;
	opts->stretch = 1;
	opts->clip_low = 5;
	opts->clip_high = 5;
	opts->piece_lines = 0;
	opts->blend = MDEMOD_MOSAIC_FEATHER;
}

void
mdemod_mosaic_grid_free(mdemod_mosaic_nodes *grid)
{
	if (!grid) return;
	for (int k = 0; k < MOSAIC_MAX; k++) free(grid->nodes[k]);
	memset(grid, 0, sizeof *grid);
}

void
mdemod_mosaic_free(mdemod_mosaic_result *out)
{
	if (!out) return;
	free(out->pixels); free(out->valid); free(out->cover);
	memset(out, 0, sizeof *out);
}

int
mdemod_mosaic_grid(const mdemod_mosaic_opts *opts, const mdemod_mosaic_pass *passes, uint32_t n, mdemod_mosaic_nodes *grid)
try { MDEMOD_API_ENTER
	if (!grid) REFUSE("mdemod_mosaic_grid: the grid is needed");
	memset(grid, 0, sizeof *grid);
	mdemod_mosaic_opts o;
	int rc = mosaic_settings(opts, o);
	if (rc) return rc;
	if (!n) REFUSE("mdemod_mosaic_grid: no pass: a mosaic takes 1 .. 8");
	if (n > MOSAIC_MAX) REFUSE("mdemod_mosaic_grid: %u passes are more than a mosaic takes (1 .. 8)", n);
	if (!passes) REFUSE("mdemod_mosaic_grid: the passes are needed");
	mdemod_map_tle tle[MOSAIC_MAX];
	mdemod_map_timing tm[MOSAIC_MAX];
	mdemod_map_opts mo[MOSAIC_MAX];
	int32_t date[MOSAIC_MAX];
	for (uint32_t k = 0; k < n; k++) {
		const mdemod_mosaic_pass &p = passes[k];
		if (!p.tle_text) REFUSE("mdemod_mosaic_grid: the element set of pass %u is needed", k);
		if (p.n_desc && (!p.place || !p.sinfo)) REFUSE("mdemod_mosaic_grid: the placements and the reports of the packets of pass %u are needed", k);
		if (p.date != MDEMOD_MOSAIC_DATE_AUTO && (p.date < -1000000 || p.date > 1000000))
			REFUSE("mosaic: the date of pass %u is day %d since 1970 (or auto)", k, p.date);
		mo[k] = map_opts_of(o, p.date);
		if ((rc = mdemod_map_parse_tle(p.tle_text, p.norad, &tle[k])) || (rc = mdemod_map_fit_time(p.place, p.sinfo, p.n_desc, &mo[k], &tm[k])) ||
		    (rc = map_check_pass("mdemod_mosaic_grid", &tle[k], &tm[k])) || (rc = map_check_lines(8 * p.rows)) ||
		    (rc = map_resolve_date(tle[k], tm[k], mo[k], 8 * p.rows, date[k])))
			return rc;
	}
	double lon_c;
	MapRange range;
	MapFrame f;
	if ((rc = map_swath_centre(tle[0], tm[0], mo[0], date[0], 8 * passes[0].rows, lon_c))) return rc;
	for (uint32_t k = 0; k < n; k++)
		if ((rc = map_swath_border(tle[k], tm[k], mo[k], date[k], 8 * passes[k].rows, lon_c, range))) return rc;
	if ((rc = map_frame(mo[0], range, lon_c, f))) return rc;
	grid->width = f.width; grid->height = f.height;
	grid->sx = static_cast<uint32_t>(f.sx); grid->sy = f.sy;
	grid->lat_top = f.lat_top;
	grid->lon_left = map_frame_lon_left(f);
	grid->node_rows = map_node_count(f.height); grid->node_cols = map_node_count(f.width);
	grid->n = n;
	const size_t count = static_cast<size_t>(grid->node_rows) * grid->node_cols;
	for (uint32_t k = 0; k < n; k++) {
		grid->nodes[k] = static_cast<int32_t *>(malloc(count * 2 * sizeof(int32_t)));
		if (!grid->nodes[k]) { mdemod_mosaic_grid_free(grid); return MDEMOD_ERR_NOMEM; }
		map_nodes_on(tle[k], tm[k], mo[k], date[k], 8 * passes[k].rows, f, grid->nodes[k]);
		mdemod_mosaic_timing &t = grid->timing[k];
		t.row_period = tm[k].row_period; t.s0 = tm[k].s0; t.date = date[k]; t.rows_fit = tm[k].rows_fit; t.placed = tm[k].placed; t.lines = 8 * passes[k].rows;
	}
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_mosaic_model_blend(const mdemod_mosaic_source *sources, uint32_t n, const uint32_t *select, uint32_t planes, uint32_t blend, uint32_t width,
                          uint32_t height, uint8_t *out, uint8_t *valid, uint8_t *cover)
try { MDEMOD_API_ENTER
	int rc = mosaic_check_blend("mdemod_mosaic_model_blend", sources, n, select, planes, blend, width, height);
	if (rc) return rc;
	if (!n || !height) return MDEMOD_OK;
	if ((rc = mosaic_check_sources("mdemod_mosaic_model_blend", sources, n, select, planes))) return rc;
	if (!out) REFUSE("mdemod_mosaic_model_blend: the picture is needed");
	model_blend(sources, n, select, planes, blend, width, height, out, valid, cover);
	return MDEMOD_OK;
} MDEMOD_API_CATCH

int
mdemod_mosaic_model_host(const mdemod_mosaic_opts *opts, const mdemod_mosaic_pass *passes, uint32_t n, const uint32_t *select, uint32_t planes,
                         mdemod_mosaic_result *out)
try { MDEMOD_API_ENTER
	if (out) memset(out, 0, sizeof *out);                                      /* (a refusal leaves nothing to free) */
	mdemod_mosaic_opts o;
	int rc = mosaic_settings(opts, o);
	if (rc) return rc;
	if ((rc = mosaic_check_compose("mdemod_mosaic_model_host", passes, n, select, planes, out))) return rc;
	ModelBackend model;
	return mosaic_compose_bands(o, passes, n, select, planes, out, model);
} MDEMOD_API_CATCH

} /* extern "C" */
