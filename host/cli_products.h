/*
 * cli_products.h - what meteor_demod_amd makes of a finished output file: the frames, the transfer frames, the pictures, the maps and
 * the mosaic, each writer with its line on stdout.  Every writer takes the file's request (struct vcdu_req, cli_opts.h): the options,
 * the GPU and the run's JPEG count.  Part of host/meteor_demod_amd.c, which includes it; not a translation unit of its own.
 */
/* <s_name without .s><ext> in a new string (NULL: out of memory) */
static char *
beside(const char *s_name, const char *ext)
{
	const size_t name_len = strlen(s_name);
	char *out = malloc(name_len + strlen(ext) + 1);
	if (!out) return NULL;
	strcpy(out, s_name);
	if (name_len > 2 && !strcmp(s_name + name_len - 2, ".s")) out[name_len - 2] = 0;
	strcat(out, ext);
	return out;
}

/* --equalise: a derived picture in place under its own mask (valid_step lines of the picture per line of the mask), before lines are
 * drawn on a copy of it and before it is written, and its line on stdout.  Nothing without the option.  0, or the exit status. */
static int
equalise_picture(const char *name, uint8_t *pixels, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t valid_step, const struct vcdu_req *req)
{
	if (!req->equalise.clip_percent || !height || !width) return 0;
	mdemod_equalise_opts eo;
	mdemod_equalise_summary es;
	mdemod_equalise_default_opts(&eo);
	eo.tile = req->equalise.tile; eo.clip_percent = req->equalise.clip_percent; eo.amount = req->equalise.amount; eo.valid_step = valid_step;
	const int rc = mdemod_equalise_host(&eo, pixels, valid, width, height, planes, &es, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--equalise: %s: %s\n", name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	printf("%s: equalised: tile %u, clip %g, %u x %u tiles, %u empty\n", name, eo.tile, eo.clip_percent / 100.0, es.nx, es.ny, es.empty_tiles);
	return 0;
}

/* One picture of the program, pixels[height][width][planes], into `name`, which ends in ".pgm" or ".ppm": as that binary P5 / P6
 * file, or with --jpeg encoded on the GPU into the same name ending in ".jpg" (`name` is changed), with one line on stdout that names
 * the file.  `what` is the option the messages begin with.  0, or the exit status. */
static int
write_picture(const char *what, char *name, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t planes, const struct vcdu_req *req)
{
	const size_t bytes = (size_t)height * width * planes;
	uint8_t *file = NULL;
	uint64_t file_bytes = 0;
	if (req->jpeg_quality) {
		const int rc = mdemod_jpeg_encode_host(pixels, width, height, planes, req->jpeg_quality, 0, &file, &file_bytes, req->device);
		if (rc != MDEMOD_OK) { fprintf(stderr, "--jpeg: %s: %s\n", name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
		memcpy(name + strlen(name) - 3, "jpg", 3);
	}
	FILE *o = fopen(name, "wb");
	if (!o) { fprintf(stderr, "%s: could not open %s\n", what, name); if (file) mdemod_jpeg_free(file); return 1; }
	int short_write;
	if (req->jpeg_quality) short_write = fwrite(file, 1, file_bytes, o) != file_bytes;
	else short_write = fprintf(o, "P%d\n%u %u\n255\n", planes == 3 ? 6 : 5, width, height) < 0 || (bytes && fwrite(pixels, 1, bytes, o) != bytes);
	if (req->jpeg_quality) mdemod_jpeg_free(file);
	if ((fclose(o) != 0) | short_write) { fprintf(stderr, "%s: writing %s failed: the picture is incomplete\n", what, name); return 1; }
	if (req->jpeg_quality) {
		printf("%s: JPEG quality %u: %u x %u x %u, %llu bytes of %llu\n", name, req->jpeg_quality, width, height, planes, (unsigned long long)file_bytes,
		       (unsigned long long)bytes);
		req->jpeg->files++; req->jpeg->bytes_in += bytes; req->jpeg->bytes_out += file_bytes;
	}
	return 0;
}

/* got[k] set where slot k of an image result received a strip (several results add up); whether any slot did */
static int
slots_received(const mdemod_image_result *res, int got[3])
{
	int any = 0;
	for (int k = 0; k < 3; k++)
		for (uint64_t c = 0; c < (uint64_t)res->summary.rows * MDEMOD_IMAGE_CELLS; c++)
			if (res->filled[k][c]) { got[k] = any = 1; break; }
	return any;
}

/* The pictures a product makes of the slots that received a strip: with --composite one of three planes (the slots given, or auto:
 * 321 with strips in all three channels, 221 with strips in the first two), otherwise a grey one per channel.  The next choice into
 * select, *planes and tag ("321", or the channel's APID); *slot is 0 before the first.  1, 0 after the last, -1 where --composite auto
 * finds neither. */
static int
next_choice(const struct vcdu_req *req, const int got[3], int *slot, uint32_t select[3], uint32_t *planes, char tag[16])
{
	if (req->composite) {
		if (*slot) return 0;
		*slot = 3;
		for (int k = 0; k < 3; k++) select[k] = req->comp[k];
		if (req->composite == 2) {
			if (got[0] && got[1] && got[2]) { select[0] = 2; select[1] = 1; select[2] = 0; }
			else if (got[0] && got[1]) { select[0] = 1; select[1] = 1; select[2] = 0; }
			else return -1;
		}
		*planes = 3;
		snprintf(tag, 16, "%u%u%u", (unsigned)select[0] + 1, (unsigned)select[1] + 1, (unsigned)select[2] + 1);
		return 1;
	}
	while (*slot < 3 && !got[*slot]) (*slot)++;
	if (*slot >= 3) return 0;
	select[0] = (uint32_t)*slot;
	*planes = 1;
	snprintf(tag, 16, "%u", (unsigned)req->apids[(*slot)++]);
	return 1;
}

/* `text` into the file `name`.  `what` is the option the messages begin with, `tail` what a failed write adds.  0, or 1. */
static int
write_text(const char *what, const char *name, const char *text, const char *tail)
{
	FILE *o = fopen(name, "w");
	if (!o) { fprintf(stderr, "%s: could not open %s\n", what, name); return 1; }
	if ((fputs(text, o) < 0) | (fclose(o) != 0)) { fprintf(stderr, "%s: writing %s failed%s\n", what, name, tail); return 1; }
	return 0;
}

/* --rectify / --composite: the pictures of one file through the picture layer.  One <apid>_rect.pgm per channel that received a
 * strip (--rectify), one <abc>.ppm and its line (--composite).  0, or the exit status. */
static int
picture_files(const char *s_name, const mdemod_image_result *res, const struct vcdu_req *req)
{
	const uint32_t rows = res->summary.rows;
	const uint8_t *image[3] = { res->image[0], res->image[1], res->image[2] }, *filled[3] = { res->filled[0], res->filled[1], res->filled[2] };
	int got[3] = { 0, 0, 0 }, code = 0;
	slots_received(res, got);
	mdemod_picture_opts po;
	mdemod_picture_default_opts(&po);
	po.rectify = req->rectify ? 1 : 0;
	if (req->altitude_km != 0.0) po.altitude_km = req->altitude_km;
	if (req->scan_deg != 0.0) po.scan_deg = req->scan_deg;
	for (int k = 0; k < 3 && !code && req->rectify; k++) {
		if (!got[k]) continue;
		const uint32_t select[1] = { (uint32_t)k };
		mdemod_picture_result pic;
		const int rc = mdemod_picture_compose_host(&po, image, filled, rows, select, 1, &pic, req->device);
		if (rc != MDEMOD_OK) { fprintf(stderr, "--rectify: %s: %s\n", s_name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
		char ext[32];
		snprintf(ext, sizeof ext, "_%u_rect.pgm", (unsigned)req->apids[k]);
		char *name = beside(s_name, ext);
		if (!name) { fprintf(stderr, "--rectify: could not open the picture\n"); code = 1; }
		else if (!(code = equalise_picture(name, pic.pixels, pic.valid, pic.width, pic.lines, 1, 8, req)))
			code = write_picture("--rectify", name, pic.pixels, pic.width, pic.lines, 1, req);
		free(name);
		mdemod_picture_free(&pic);
	}
	if (code || !req->composite) return code;
	uint32_t select[3], planes;
	char tag[16], *base = beside(s_name, "");
	int slot = 0;
	if (next_choice(req, got, &slot, select, &planes, tag) < 0) {
		printf("%s: no composite (--composite auto wants strips in all three channels, or in the first two)\n", base ? base : s_name);
		free(base);
		return 0;
	}
	mdemod_picture_result pic;
	const int rc = mdemod_picture_compose_host(&po, image, filled, rows, select, 3, &pic, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--composite: %s: %s\n", s_name, why_of(rc)); free(base); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	char ext[32];
	snprintf(ext, sizeof ext, "_%s.ppm", tag);
	char *name = beside(s_name, ext);
	if (!name) { fprintf(stderr, "--composite: could not open the picture\n"); code = 1; }
	else if (!(code = equalise_picture(name, pic.pixels, pic.valid, pic.width, pic.lines, 3, 8, req)))
		code = write_picture("--composite", name, pic.pixels, pic.width, pic.lines, 3, req);
	if (!code)
		printf("%s: composite %s: %u x %u%s; stretch R %u .. %u, G %u .. %u, B %u .. %u; %.1f %% of pixels valid\n", base ? base : s_name,
		       tag, pic.width, pic.lines, req->rectify ? " rectified" : "",
		       pic.lo[0], pic.hi[0], pic.lo[1], pic.hi[1], pic.lo[2], pic.hi[2],
		       rows ? 100.0 * (double)pic.valid_cells / ((double)rows * pic.width) : 0.0);
	free(name); free(base);
	mdemod_picture_free(&pic);
	return code;
}

/* "yyyy-mm-ddThh:mm:ss.sss" of second `utc0` of day `date` since 1970-01-01 (utc0 may be negative or above 86 400) */
static void
utc_text(char out[64], int32_t date, double utc0)
{
	const double total = (double)date * 86400.0 + utc0, day = floor(total / 86400.0), sec = total - day * 86400.0;
	int y; unsigned m, d;
	civil_from_days((int64_t)day, &y, &m, &d);
	snprintf(out, 64, "%04d-%02u-%02uT%02d:%02d:%06.3f", y, m, d, (int)(sec / 3600.0), (int)(fmod(sec, 3600.0) / 60.0), fmod(sec, 60.0));
}

/* what follows "first lines" in the line of a picture of n passes: " <time>Z, <time>Z" */
static void
print_first_lines(const int32_t *date, const double *utc0, uint32_t n)
{
	for (uint32_t k = 0; k < n; k++) {
		char at[64];
		utc_text(at, date[k], utc0[k]);
		printf("%s %sZ", k ? "," : "", at);
	}
}

/* the six lines of the world file of a latitude / longitude grid */
static void
latlon_world_file(char text[160], uint32_t sx, double sy, double lat_top, double lon_left)
{
	snprintf(text, 160, "%.17g\n0\n0\n%.17g\n%.17g\n%.17g\n", 1.0 / sx, -1.0 / sy, lon_left + 0.5 / sx, lat_top - 0.5 / sy);
}

/* one pass of the mosaic or of the polar layer (their structs are field for field alike) from the pictures kept of one file */
#define PASS_OF(p, res, req, auto_date) do { \
	(p)->tle_text = (req)->tle_text; (p)->norad = (req)->norad; \
	(p)->date = (req)->date_given ? (req)->map_date : (auto_date); \
	for (int k_ = 0; k_ < 3; k_++) { (p)->image[k_] = (res)->image[k_]; (p)->filled[k_] = (res)->filled[k_]; } \
	(p)->rows = (res)->summary.rows; (p)->place = (res)->place; (p)->sinfo = (res)->sinfo; (p)->n_desc = (res)->n_packets; \
} while (0)

/* What --overlay / --graticule do alike on every grid: a copy of the picture, draw(lines, copy) on it (the library's code comes
 * back), <stem>_overlay.ppm / .pgm, and beside it text[t] as <stem>_overlay.<ext[t]> for t < n_text (`tail` as write_text takes
 * it).  0, or the exit status; the line on stdout is the caller's. */
static int
overlay_tail(const char *stem, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t planes, const struct vcdu_req *req, int (*draw)(void *lines, uint8_t *copy), void *lines,
             const char *const *ext, const char *const *text, int n_text, const char *tail)
{
	const size_t bytes = (size_t)height * width * planes, len = strlen(stem) + 32;
	uint8_t *copy = malloc(bytes ? bytes : 1);
	char *name = malloc(len);
	int code = 0;
	if (!copy || !name) { fprintf(stderr, "--overlay: out of memory\n"); code = 2; }
	else {
		memcpy(copy, pixels, bytes);
		const int rc = draw(lines, copy);
		if (rc != MDEMOD_OK) { fprintf(stderr, "--overlay: %s\n", why_of(rc)); code = rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	}
	if (!code) {
		snprintf(name, len, "%s_overlay.%s", stem, planes == 3 ? "ppm" : "pgm");
		code = write_picture("--overlay", name, copy, width, height, planes, req);
	}
	for (int t = 0; t < n_text && !code; t++) {
		snprintf(name, len, "%s_overlay.%s", stem, ext[t]);
		code = write_text("--overlay", name, text[t], tail);
	}
	free(copy);
	free(name);
	return code;
}

/* the lines of --overlay / --graticule on a latitude / longitude grid, as mdemod_overlay_draw_host takes them, and its report */
struct latlon_lines {
	mdemod_overlay_geo geo;
	mdemod_overlay_layer layers[OVERLAY_FILES + 1];
	uint32_t n, planes;
	const mdemod_overlay_style *style;
	const uint8_t *valid;
	mdemod_overlay_report rep;
	int device;
};

static int
latlon_draw(void *lines, uint8_t *copy)
{
	struct latlon_lines *l = lines;
	return mdemod_overlay_draw_host(&l->geo, l->layers, l->n, l->style, 2, l->planes, copy, l->valid, NULL, 0, &l->rep, l->device);
}

/* --overlay / --graticule: a copy of a picture on the grid given with the lines on it: <stem>_overlay.ppm / .pgm, a world file of
 * the picture's six lines and one line on stdout.  0, or the exit status. */
static int
overlay_file(const char *stem, uint32_t width, uint32_t height, uint32_t planes, uint32_t sx, double sy, double lat_top, double lon_left,
             const uint8_t *pixels, const uint8_t *valid, const struct vcdu_req *req)
{
	struct latlon_lines l;
	mdemod_overlay_vectors grat;
	char wld[160];
	const char *ext[1] = { "wld" }, *text[1] = { wld };
	memset(&l, 0, sizeof l);
	memset(&grat, 0, sizeof grat);
	l.geo = (mdemod_overlay_geo){ width, height, sx, 0, sy, lat_top, lon_left };
	l.planes = planes; l.style = req->overlay->style; l.valid = valid; l.device = req->device;
	if (req->overlay->graticule) {
		/* (the order of the layers decides no byte: style 0 meets a pixel before style 1) */
		if (mdemod_overlay_graticule(&l.geo, req->overlay->step, &grat) != MDEMOD_OK) { fprintf(stderr, "--graticule: %s\n", mdemod_last_error()); return 1; }
		l.layers[l.n].vectors = &grat; l.layers[l.n++].style = 1;
	}
	for (uint32_t k = 0; k < req->overlay->n_files; k++) { l.layers[l.n].vectors = &req->overlay->coast[k]; l.layers[l.n++].style = 0; }
	latlon_world_file(wld, sx, sy, lat_top, lon_left);
	const int code = overlay_tail(stem, pixels, width, height, planes, req, latlon_draw, &l, ext, text, 1, ": the world file is incomplete");
	if (!code)
		printf("%s_overlay: %llu pieces kept, %llu tiles touched; lines: %llu pieces, %llu pixels; graticule: %llu pieces, %llu pixels\n", stem,
		       (unsigned long long)(l.rep.pieces[0] + l.rep.pieces[1]), (unsigned long long)l.rep.tiles, (unsigned long long)l.rep.pieces[0],
		       (unsigned long long)l.rep.pixels[0], (unsigned long long)l.rep.pieces[1], (unsigned long long)l.rep.pixels[1]);
	mdemod_overlay_vectors_free(&grat);
	return code;
}

/* one map of the given slots: <tag>_map.ppm / .pgm, its world file and its line.  0, or the exit status. */
static int
map_file(const char *s_name, const mdemod_image_result *res, const struct vcdu_req *req, const uint32_t *select, uint32_t planes, const char *tag)
{
	const uint8_t *image[3] = { res->image[0], res->image[1], res->image[2] }, *filled[3] = { res->filled[0], res->filled[1], res->filled[2] };
	mdemod_map_opts mo;
	mdemod_map_result map;
	map_options(req, &mo);
	const int rc = mdemod_map_compose_host(&mo, &req->tle, image, filled, res->summary.rows, res->place, res->sinfo, res->n_packets, select, planes, &map, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--map: %s: %s\n", s_name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	int code = 0;
	char ext[48], wld[160], at[64];
	snprintf(ext, sizeof ext, "_%s_map.%s", tag, planes == 3 ? "ppm" : "pgm");
	char *name = beside(s_name, ext), *base = beside(s_name, "");
	if (!name) { fprintf(stderr, "--map: could not open the picture\n"); code = 1; }
	else if (!(code = equalise_picture(name, map.pixels, map.valid, map.width, map.height, planes, 1, req)))
		code = write_picture("--map", name, map.pixels, map.width, map.height, planes, req);
	free(name);
	snprintf(ext, sizeof ext, "_%s_map.wld", tag);
	name = code ? NULL : beside(s_name, ext);
	latlon_world_file(wld, map.sx, map.sy, map.lat_top, map.lon_left);
	if (!code && !name) { fprintf(stderr, "--map: could not open the world file\n"); code = 1; }
	else if (!code) code = write_text("--map", name, wld, ": the world file is incomplete");
	free(name);
	if (!code) {
		utc_text(at, map.timing.date, map.utc0);
		printf("%s: map %s: %u x %u at %u x %g px/deg; lat %.4f .. %.4f, lon %.4f .. %.4f; row period %.6f s over %u rows; first line %sZ; "
		       "%.1f %% of pixels valid\n", base ? base : s_name, tag, map.width, map.height, map.sx, map.sy, map.lat_top - map.height / map.sy, map.lat_top,
		       map.lon_left, map.lon_left + (double)map.width / map.sx, map.timing.row_period, map.timing.rows_fit, at,
		       100.0 * (double)map.valid_pixels / ((double)map.width * map.height));
	}
	free(base);
	if (!code && req->overlay) {
		snprintf(ext, sizeof ext, "_%s_map", tag);
		char *stem = beside(s_name, ext);
		if (!stem) { fprintf(stderr, "--overlay: out of memory\n"); code = 2; }
		else code = overlay_file(stem, map.width, map.height, planes, map.sx, map.sy, map.lat_top, map.lon_left, map.pixels, map.valid, req);
		free(stem);
	}
	mdemod_map_free(&map);
	return code;
}

/* --map: the composite (--composite) or every channel that received a strip on the grid.  0, or the exit status. */
static int
map_files(const char *s_name, const mdemod_image_result *res, const struct vcdu_req *req)
{
	int got[3] = { 0, 0, 0 }, code = 0, slot = 0;
	uint32_t select[3], planes;
	char tag[16];
	slots_received(res, got);
	/* (where --composite auto finds nothing the composite's own line has said so) */
	while (!code && next_choice(req, got, &slot, select, &planes, tag) > 0) code = map_file(s_name, res, req, select, planes, tag);
	return code;
}

/* --mosaic: one mosaic of the given slots of the kept passes: <base>_<tag>_mosaic.ppm / .pgm, its world file and its line.  0, or
 * the exit status. */
static int
mosaic_file(const char *base, const mdemod_mosaic_pass *passes, uint32_t n, const struct vcdu_req *req, const uint32_t *select, uint32_t planes, const char *tag)
{
	mdemod_mosaic_opts mo;
	mdemod_mosaic_result mos;
	mdemod_mosaic_default_opts(&mo);
	if (req->scan_deg != 0.0) mo.scan_deg = req->scan_deg;
	if (req->map_scale != 0.0) mo.px_per_deg = req->map_scale;
	if (req->offset_given) mo.time_offset = req->time_offset;
	if (req->side) mo.side = req->side;
	mo.blend = req->mosaic_blend;
	const int rc = mdemod_mosaic_compose_host(&mo, passes, n, select, planes, &mos, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--mosaic: %s\n", why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	int code = 0;
	const size_t len = strlen(base) + strlen(tag) + 32;
	char *name = malloc(len);
	if (name) snprintf(name, len, "%s_%s_mosaic.%s", base, tag, planes == 3 ? "ppm" : "pgm");
	if (!name) { fprintf(stderr, "--mosaic: could not open the picture\n"); code = 1; }
	else if (!(code = equalise_picture(name, mos.pixels, mos.valid, mos.width, mos.height, planes, 1, req)))
		code = write_picture("--mosaic", name, mos.pixels, mos.width, mos.height, planes, req);
	if (!code) {
		char wld[160];
		snprintf(name, len, "%s_%s_mosaic.wld", base, tag);
		latlon_world_file(wld, mos.sx, mos.sy, mos.lat_top, mos.lon_left);
		code = write_text("--mosaic", name, wld, ": the world file is incomplete");
	}
	if (!code) {
		const double area = (double)mos.width * mos.height;
		int32_t date[MDEMOD_MOSAIC_MAX_PASSES];
		for (uint32_t k = 0; k < mos.n; k++) date[k] = mos.timing[k].date;
		printf("%s: mosaic %s (%s): %u x %u at %u x %g px/deg; lat %.4f .. %.4f, lon %.4f .. %.4f; %u passes; first lines", base, tag,
		       mos.blend == MDEMOD_MOSAIC_BEST ? "best" : "feather", mos.width, mos.height, mos.sx, mos.sy, mos.lat_top - mos.height / mos.sy, mos.lat_top, mos.lon_left,
		       mos.lon_left + (double)mos.width / mos.sx, mos.n);
		print_first_lines(date, mos.utc0, mos.n);
		printf("; %.1f %% of pixels valid; %.1f %% seen by two or more passes\n", 100.0 * (double)mos.valid_pixels / area, 100.0 * (double)mos.overlap_pixels / area);
	}
	if (!code && req->overlay) {
		snprintf(name, len, "%s_%s_mosaic", base, tag);
		code = overlay_file(name, mos.width, mos.height, planes, mos.sx, mos.sy, mos.lat_top, mos.lon_left, mos.pixels, mos.valid, req);
	}
	free(name);
	mdemod_mosaic_free(&mos);
	return code;
}

/* --mosaic: the kept pictures of all files on one grid: the composite (--composite; auto on what the passes received together) or
 * every channel that received a strip in any pass.  Frees what was kept.  0, or the exit status. */
static int
mosaic_files(const char *base, mdemod_image_result *kept, const struct stream_io *io, int n_files, const struct vcdu_req *req)
{
	mdemod_mosaic_pass passes[MDEMOD_MOSAIC_MAX_PASSES];
	uint32_t n = 0, select[3], planes;
	int got[3] = { 0, 0, 0 }, code = 0, slot = 0, more = 0;
	char tag[16];
	memset(passes, 0, sizeof passes);
	for (int i = 0; i < n_files; i++) {
		if (!slots_received(&kept[i], got)) { fprintf(stderr, "--mosaic: %s gave no picture: left out\n", io[i].in_name); continue; }
		PASS_OF(&passes[n], &kept[i], req, MDEMOD_MOSAIC_DATE_AUTO);
		n++;
	}
	if (!n) { fprintf(stderr, "--mosaic: no pass gave a picture\n"); code = 1; }
	while (n && !code && (more = next_choice(req, got, &slot, select, &planes, tag)) > 0) code = mosaic_file(base, passes, n, req, select, planes, tag);
	if (more < 0) printf("%s: no mosaic (--composite auto wants strips in all three channels, or in the first two)\n", base);
	for (int i = 0; i < n_files; i++) mdemod_image_free(&kept[i]);
	return code;
}

/* the lines of --overlay / --graticule on a polar picture, as mdemod_polar_draw_host takes them, and its report */
struct polar_lines {
	const mdemod_polar_points *layers[OVERLAY_FILES + 1];
	uint32_t style_of[OVERLAY_FILES + 1], n;
	mdemod_polar_style styles[2];
	const mdemod_polar_result *pic;
	mdemod_polar_drawn rep;
	int device;
};

static int
polar_draw(void *lines, uint8_t *copy)
{
	struct polar_lines *l = lines;
	const mdemod_polar_frame *f = &l->pic->frame;
	return mdemod_polar_draw_host(l->layers, l->style_of, l->n, l->styles, 2, f->width, f->height, l->pic->planes, copy, l->pic->valid, &l->rep, l->device);
}

/* --map-proj stereo with --overlay / --graticule: a copy of a polar picture with the lines on it, <stem>_overlay.ppm / .pgm with the
 * picture's world file and .prj, and one line.  The lines go through the polar layer's vertices and the overlay layer's kernel. */
static int
polar_overlay_file(const char *stem, const mdemod_polar_result *pic, const char *wld, const char *prj, const struct vcdu_req *req)
{
	const mdemod_polar_frame *f = &pic->frame;
	struct polar_lines l;
	mdemod_polar_lines grat;
	mdemod_polar_points pts[OVERLAY_FILES + 1];
	const char *ext[2] = { "wld", "prj" }, *text[2] = { wld, prj };
	int code = 0;
	memset(&l, 0, sizeof l);
	memset(&grat, 0, sizeof grat);
	memset(pts, 0, sizeof pts);
	l.pic = pic; l.device = req->device;
	for (int s = 0; s < 2; s++) {
		l.styles[s].half_width = req->overlay->style[s].half_width; l.styles[s].opacity = req->overlay->style[s].opacity; l.styles[s].inside_only = req->overlay->style[s].inside_only;
		memcpy(l.styles[s].colour, req->overlay->style[s].colour, 3);
	}
	if (req->overlay->graticule) {
		if (mdemod_polar_graticule(f, req->overlay->step, &grat) != MDEMOD_OK || mdemod_polar_vertices(f, grat.lon, grat.lat, grat.first, grat.n_lines, &pts[l.n]) != MDEMOD_OK) {
			fprintf(stderr, "--graticule: %s\n", mdemod_last_error());
			code = 1;
		} else { l.layers[l.n] = &pts[l.n]; l.style_of[l.n++] = 1; }
	}
	for (uint32_t k = 0; k < req->overlay->n_files && !code; k++) {
		if (mdemod_polar_vertices(f, req->overlay->coast[k].lon, req->overlay->coast[k].lat, req->overlay->coast[k].first, req->overlay->coast[k].n_lines, &pts[l.n]) != MDEMOD_OK) {
			fprintf(stderr, "--overlay: %s\n", mdemod_last_error());
			code = 1;
		} else { l.layers[l.n] = &pts[l.n]; l.style_of[l.n++] = 0; }
	}
	if (!code) code = overlay_tail(stem, pic->pixels, f->width, f->height, pic->planes, req, polar_draw, &l, ext, text, 2, "");
	if (!code)
		printf("%s_overlay: %llu pieces kept, %llu tiles touched; lines: %llu pieces; graticule: %llu pieces every %g degrees\n", stem,
		       (unsigned long long)(l.rep.pieces[0] + l.rep.pieces[1]), (unsigned long long)l.rep.tiles, (unsigned long long)l.rep.pieces[0],
		       (unsigned long long)l.rep.pieces[1], grat.step_deg);
	for (uint32_t k = 0; k < OVERLAY_FILES + 1; k++) mdemod_polar_points_free(&pts[k]);
	mdemod_polar_lines_free(&grat);
	return code;
}

/* --map-proj stereo: one picture of the given slots of n passes: <stem>_<tag>_polar.ppm / .pgm, its world file, its .prj and its
 * line.  0, or the exit status. */
static int
polar_file(const char *stem, const mdemod_polar_pass *passes, uint32_t n, const struct vcdu_req *req, const uint32_t *select, uint32_t planes, const char *tag)
{
	mdemod_polar_opts po;
	mdemod_polar_result pic;
	mdemod_polar_default_opts(&po);
	if (req->scan_deg != 0.0) po.scan_deg = req->scan_deg;
	if (req->offset_given) po.time_offset = req->time_offset;
	if (req->side) po.side = req->side;
	if (req->polar_res != 0.0) po.metres_per_pixel = req->polar_res;
	if (req->polar_lat_ts != 0.0) po.lat_ts_deg = req->polar_lat_ts;
	if (req->lon0_given) po.lon0_deg = req->polar_lon0;
	po.blend = req->mosaic_blend;
	const int rc = mdemod_polar_compose_host(&po, passes, n, select, planes, &pic, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--map-proj stereo: %s: %s\n", stem, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	int code = 0;
	char wld[256], prj[1024];
	if (mdemod_polar_world_file(&pic.frame, wld, sizeof wld) != MDEMOD_OK || mdemod_polar_prj(&pic.frame, prj, sizeof prj) != MDEMOD_OK) {
		fprintf(stderr, "--map-proj stereo: %s\n", mdemod_last_error());
		code = 2;
	}
	const size_t len = strlen(stem) + strlen(tag) + 32;
	char *name = malloc(len);
	if (!code && !name) { fprintf(stderr, "--map-proj stereo: out of memory\n"); code = 2; }
	if (!code) {
		snprintf(name, len, "%s_%s_polar.%s", stem, tag, planes == 3 ? "ppm" : "pgm");
		if (!(code = equalise_picture(name, pic.pixels, pic.valid, pic.frame.width, pic.frame.height, planes, 1, req)))
			code = write_picture("--map-proj stereo", name, pic.pixels, pic.frame.width, pic.frame.height, planes, req);
	}
	for (int t = 0; t < 2 && !code; t++) {
		snprintf(name, len, "%s_%s_polar.%s", stem, tag, t ? "prj" : "wld");
		code = write_text("--map-proj stereo", name, t ? prj : wld, "");
	}
	if (!code) {
		const double area = (double)pic.frame.width * pic.frame.height;
		int32_t date[MDEMOD_POLAR_MAX_PASSES];
		for (uint32_t k = 0; k < pic.n; k++) date[k] = pic.timing[k].date;
		printf("%s: polar %s (%s): %u x %u at %g m; %s pole, central meridian %g, true scale at %g; E %.0f .. %.0f, N %.0f .. %.0f; %u pass%s; first lines", stem, tag,
		       pic.blend == MDEMOD_POLAR_BEST ? "best" : "feather", pic.frame.width, pic.frame.height, pic.frame.res, pic.frame.pole > 0 ? "north" : "south",
		       pic.frame.lon0_deg, pic.frame.lat_ts_deg, pic.frame.e_left, pic.frame.e_left + pic.frame.width * pic.frame.res,
		       pic.frame.n_top - pic.frame.height * pic.frame.res, pic.frame.n_top, pic.n, pic.n == 1 ? "" : "es");
		print_first_lines(date, pic.utc0, pic.n);
		printf("; %.1f %% of pixels valid; %.1f %% seen by two or more passes\n", 100.0 * (double)pic.valid_pixels / area, 100.0 * (double)pic.overlap_pixels / area);
	}
	if (!code && req->overlay) {
		snprintf(name, len, "%s_%s_polar", stem, tag);
		code = polar_overlay_file(name, &pic, wld, prj, req);
	}
	free(name);
	mdemod_polar_free(&pic);
	return code;
}

/* --map-proj stereo: the composite (--composite; auto on what the passes received together) or every channel that received a strip
 * in any pass, of the n passes that gave a picture.  0, or the exit status. */
static int
polar_files(const char *stem, const mdemod_image_result *const *results, int n_results, const struct vcdu_req *req)
{
	mdemod_polar_pass passes[MDEMOD_POLAR_MAX_PASSES];
	uint32_t n = 0, select[3], planes;
	int got[3] = { 0, 0, 0 }, code = 0, slot = 0;
	char tag[16];
	memset(passes, 0, sizeof passes);
	for (int i = 0; i < n_results && n < MDEMOD_POLAR_MAX_PASSES; i++) {
		if (!slots_received(results[i], got)) continue;
		PASS_OF(&passes[n], results[i], req, MDEMOD_POLAR_DATE_AUTO);
		n++;
	}
	/* (no picture: the image layer's line has said so; nothing for --composite auto: the composite's has) */
	while (n && !code && next_choice(req, got, &slot, select, &planes, tag) > 0) code = polar_file(stem, passes, n, req, select, planes, tag);
	return code;
}

/* --sun: the reflective channels of one file's pictures in place, with the options of --map, and the file's line on stdout.  Nothing
 * without the option or without a picture.  0, or the exit status. */
static int
sun_pictures(const char *s_name, mdemod_image_result *res, const struct vcdu_req *req)
{
	if (!req->sun.on || !res->summary.rows) return 0;
	mdemod_sun_opts so;
	mdemod_sun_summary ss;
	mdemod_map_opts mo;
	mdemod_sun_default_opts(&so);
	if (req->sun.ref_given) so.ref_deg = req->sun.ref_deg;
	if (req->sun.limit_given) so.limit_deg = req->sun.limit_deg;
	map_options(req, &mo);
	/* (the sun layer's header repeats the map layer's options and element set field for field) */
	mdemod_sun_pass_opts po;
	mdemod_sun_orbit orbit;
	_Static_assert(sizeof po == sizeof mo && sizeof orbit == sizeof req->tle, "the sun layer's pass is the map layer's");
	memcpy(&po, &mo, sizeof po);
	memcpy(&orbit, &req->tle, sizeof orbit);
	uint8_t *image[3] = { res->image[0], res->image[1], res->image[2] };
	const int rc = mdemod_sun_correct_host(&so, &po, &orbit, image, req->apids, res->summary.rows, res->place, res->sinfo, res->n_packets, &ss, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--sun: %s: %s\n", s_name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	char *base = beside(s_name, "");
	char slots[32] = "";
	unsigned long long sat = 0, pixels = 0;
	for (int k = 0; k < 3; k++) {
		if (!(ss.slot_mask >> k & 1u)) continue;
		snprintf(slots + strlen(slots), sizeof slots - strlen(slots), "%s%u", *slots ? ", " : "", (unsigned)req->apids[k]);
		sat += ss.saturated[k];
		pixels += (unsigned long long)res->summary.rows * 8 * MDEMOD_IMAGE_WIDTH;
	}
	printf("%s: sun: zenith %.2f .. %.2f deg, reference %g, limit %g (%u of %u nodes beyond it, %u missing); corrected: %s; %.3f %% of pixels saturated\n",
	       base ? base : s_name, ss.zenith_min, ss.zenith_max, so.ref_deg, so.limit_deg, ss.at_limit, ss.nodes, ss.missing, *slots ? slots : "none",
	       pixels ? 100.0 * (double)sat / (double)pixels : 0.0);
	free(base);
	return 0;
}

/* --image: n VCDUs through the image layer, one PGM per active channel that received a strip beside the output file, one line.
 * 0, or the exit status. */
static int
image_files(const char *s_name, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, const struct vcdu_req *req)
{
	const uint32_t *apids = req->apids;
	mdemod_image_opts io;
	mdemod_image_result res;
	mdemod_image_default_opts(&io);
	for (int k = 0; k < 3; k++) io.apids[k] = apids[k];
	const int rc = mdemod_image_decode_host(&io, vcdu, info, n, &res, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--image: %s: %s\n", s_name, why_of(rc)); return 2; }
	int code = 0;
	const uint32_t rows = res.summary.rows;
	int got[3] = { 0, 0, 0 };
	slots_received(&res, got);
	for (int k = 0; k < 3 && !code; k++) {
		if (!got[k]) continue;
		char ext[32];
		snprintf(ext, sizeof ext, "_%u.pgm", (unsigned)apids[k]);
		char *name = beside(s_name, ext);
		if (!name) { fprintf(stderr, "--image: could not open the picture\n"); code = 1; break; }
		code = write_picture("--image", name, res.image[k], MDEMOD_IMAGE_WIDTH, rows * 8, 1, req);
		free(name);
	}
	if (!code) {
		char *base = beside(s_name, "");
		printf("%s: %llu packets; image packets", base ? base : s_name, (unsigned long long)res.summary.packets);
		for (int k = 0; k < 3; k++) printf("%s apid %u: %llu", k ? "," : "", (unsigned)apids[k], (unsigned long long)res.summary.per_apid[apids[k] - 64]);
		printf("; %llu strips truncated; %u lines; %.1f %% of cells filled\n", (unsigned long long)res.summary.truncated, rows * 8,
		       rows ? 100.0 * (double)res.summary.cells_filled / (3.0 * rows * MDEMOD_IMAGE_CELLS) : 0.0);
		free(base);
	}
	if (!code) code = sun_pictures(s_name, &res, req);                  /* (--sun: everything below comes from the corrected buffers) */
	if (!code && (req->rectify || req->composite)) code = picture_files(s_name, &res, req);
	if (!code && req->map && req->polar) {
		const mdemod_image_result *one[1] = { &res };
		char *stem = beside(s_name, "");
		if (!stem) { fprintf(stderr, "--map-proj stereo: out of memory\n"); code = 2; }
		else code = polar_files(stem, one, 1, req);
		free(stem);
	} else if (!code && req->map) code = map_files(s_name, &res, req);
	if (!code && req->keep) *req->keep = res;                                  /* (the mosaic frees it) */
	else mdemod_image_free(&res);
	return code;
}

/* --vcdu / --image: n CADUs through the transfer-frame layer; the VCDUs beside the output file and one line (--vcdu), the pictures
 * (--image).  0, or the exit status. */
static int
vcdu_file(const char *s_name, const uint8_t *cadu, uint64_t n, const struct vcdu_req *req)
{
	uint8_t *vcdu = malloc(n ? (size_t)n * MDEMOD_RS_VCDU_BYTES : 1);
	mdemod_rs_info *info = calloc(n ? (size_t)n : 1, sizeof(*info));
	char *out_name = beside(s_name, ".vcdu");
	int code = 1;
	if (!vcdu || !info || !out_name) { fprintf(stderr, "--vcdu: out of memory for the frames of %s\n", s_name); goto done; }
	mdemod_rs_opts ro;
	mdemod_rs_default_opts(&ro);
	const int rc = mdemod_rs_decode_host(&ro, cadu, n, vcdu, info, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--vcdu: %s: %s\n", s_name, why_of(rc)); code = 2; goto done; }
	if (!req->write_vcdu) { code = image_files(s_name, vcdu, info, n, req); goto done; }
	FILE *o = fopen(out_name, "wb");
	if (!o) { fprintf(stderr, "--vcdu: could not open %s\n", out_name); goto done; }
	const int short_write = fwrite(vcdu, MDEMOD_RS_VCDU_BYTES, (size_t)n, o) != (size_t)n;
	if ((fclose(o) != 0) | short_write) { fprintf(stderr, "--vcdu: writing %s failed: the output is incomplete\n", out_name); goto done; }
	/* per VCID, over the frames without an uncorrectable codeword: frames, and places where the counter does not follow */
	uint64_t lost = 0, fixed = 0, per[64] = { 0 }, gaps[64] = { 0 };
	uint32_t last[64];
	int seen[64] = { 0 };
	for (uint64_t i = 0; i < n; i++) {
		for (int c = 0; c < 4; c++)
			if (info[i].corrected[c] != MDEMOD_RS_FAILED) fixed += info[i].corrected[c];
		if (info[i].flags & MDEMOD_RS_UNCORRECTABLE) { lost++; continue; }
		mdemod_rs_header h;
		mdemod_rs_vcdu_header(vcdu + i * MDEMOD_RS_VCDU_BYTES, &h);
		const uint32_t v = h.vcid & 63u;
		per[v]++;
		if (seen[v] && h.counter != ((last[v] + 1) & 0xFFFFFFu)) gaps[v]++;
		seen[v] = 1;
		last[v] = h.counter;
	}
	printf("%s: %llu frames, %llu uncorrectable, %llu bytes corrected;", out_name, (unsigned long long)n, (unsigned long long)lost, (unsigned long long)fixed);
	int any = 0;
	for (int v = 0; v < 64; v++)
		if (seen[v]) { printf("%s vcid %d: %llu frames, %llu counter gaps", any ? "," : "", v, (unsigned long long)per[v], (unsigned long long)gaps[v]); any = 1; }
	printf("%s\n", any ? "" : " no VCID");
	code = req->image ? image_files(s_name, vcdu, info, n, req) : 0;
done:
	free(out_name); free(info); free(vcdu);
	return code;
}

/* --cadu / --vcdu: the soft symbols of one finished output file through the frame layer, the CADUs (and the VCDUs) beside it.  0, or
 * the exit status. */
static int
cadu_file(const char *s_name, const struct vcdu_req *req)
{
	FILE *f = fopen(s_name, "rb");
	if (!f) { fprintf(stderr, "--cadu: %s: %s\n", s_name, strerror(errno)); return 1; }
	long len = -1;
	if (!fseek(f, 0, SEEK_END)) len = ftell(f);
	if (len < 0 || fseek(f, 0, SEEK_SET)) { fprintf(stderr, "--cadu: cannot read %s\n", s_name); fclose(f); return 1; }
	uint64_t m = (uint64_t)len / 2;
	const uint64_t cap = m / MDEMOD_FRAME_SYMBOLS;
	const uint32_t il_delay = req->il_delay;
	const int diff = req->diff, skew = req->skew;                                /* (never a skew with --int: the sync word resolves it) */
	/* --int: the deinterleaved stream (never longer than this) and the segments (never more than the windows) */
	const uint64_t il_room = il_delay ? mdemod_il_max_output_symbols(m) : 0, il_cap = il_delay ? mdemod_il_windows(m) : 0;
	int8_t *deint = il_delay ? malloc((size_t)il_room * 2) : NULL;
	mdemod_il_segment *segs = il_delay ? calloc(il_cap ? (size_t)il_cap : 1, sizeof(*segs)) : NULL;
	int8_t *soft = malloc(len ? (size_t)len : 1);
	uint8_t *cadu = malloc(cap ? (size_t)cap * MDEMOD_FRAME_BYTES : 1);
	mdemod_frame_info *frames = calloc(cap ? (size_t)cap : 1, sizeof(*frames));
	char *out_name = beside(s_name, ".cadu");
	int code = 1;
	if (!soft || !cadu || !frames || !out_name || (il_delay && (!deint || !segs))) { fprintf(stderr, "--cadu: out of memory reading %s\n", s_name); goto done; }
	if (fread(soft, 1, (size_t)len, f) != (size_t)len) { fprintf(stderr, "--cadu: cannot read %s\n", s_name); goto done; }
	const int8_t *sym = soft;                                                    /* what the frame pass reads */
	if (il_delay) {
		mdemod_il_opts io;
		mdemod_il_default_opts(&io);
		io.branch_delay = il_delay;
		uint64_t n_segs = 0, periods = 0;
		int32_t mean = 0;
		const int irc = mdemod_il_decode_host(&io, soft, m, deint, il_room, segs, il_cap, &n_segs, &periods, &mean, req->device);
		if (irc != MDEMOD_OK) { fprintf(stderr, "--int: %s: %s\n", s_name, why_of(irc)); code = 2; goto done; }
		printf("%s: interleaver: %llu segments, %llu periods, mean sync score %d / 24576\n", s_name, (unsigned long long)n_segs,
		       (unsigned long long)periods, (int)mean);
		const uint64_t written = periods < il_room / MDEMOD_IL_BRANCHES ? periods : il_room / MDEMOD_IL_BRANCHES;
		sym = deint;
		m = written * MDEMOD_IL_BRANCHES;
	}
	mdemod_frames_opts fo;
	mdemod_frames_default_opts(&fo);
	uint64_t n = 0;
	mdemod_frames_link link = { (uint32_t)diff, (uint32_t)skew, { 0, 0 } };
	const int rc = diff || skew ? mdemod_frames_link_decode_host(&link, &fo, sym, m, cadu, frames, cap, &n, req->device)
	                            : mdemod_frames_decode_host(&fo, sym, m, cadu, frames, cap, &n, req->device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--cadu: %s: %s\n", s_name, why_of(rc)); code = 2; goto done; }
	if (n > cap) n = cap;
	if (!req->write_cadu) { code = vcdu_file(s_name, cadu, n, req); goto done; }
	FILE *o = fopen(out_name, "wb");
	if (!o) { fprintf(stderr, "--cadu: could not open %s\n", out_name); goto done; }
	const int short_write = fwrite(cadu, MDEMOD_FRAME_BYTES, (size_t)n, o) != (size_t)n;
	if ((fclose(o) != 0) | short_write) { fprintf(stderr, "--cadu: writing %s failed: the output is incomplete\n", out_name); goto done; }
	uint64_t fly = 0, errors = 0;
	uint32_t runs = 0, last_run = 0;
	for (uint64_t i = 0; i < n; i++) {
		fly += frames[i].flags & MDEMOD_FRAME_FLYWHEEL ? 1 : 0;
		errors += frames[i].channel_errors;
		if (i == 0 || frames[i].run > last_run) { runs++; last_run = frames[i].run; }     /* (run numbers ascend with the position where runs do not interleave; a run seen again is not counted twice) */
	}
	printf("%s: %llu frames (%llu flywheel) in %u runs, mean channel errors %.1f / %d\n", out_name, (unsigned long long)n, (unsigned long long)fly, runs,
	       n ? (double)errors / (double)n : 0.0, MDEMOD_FRAME_DECISIONS);
	code = req->write_vcdu || req->image ? vcdu_file(s_name, cadu, n, req) : 0;
done:
	free(out_name); free(frames); free(cadu); free(soft); free(segs); free(deint);
	fclose(f);
	return code;
}
