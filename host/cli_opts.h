/*
 * cli_opts.h - what the command line of meteor_demod_amd says: the option table, the value every option goes into (struct cli_opts),
 * the one function that fills it (parse_options) and the one that refuses what does not go together (check_options).  Part of
 * host/meteor_demod_amd.c, which includes it; not a translation unit of its own.
 */
/* the front end's entries: weak, so that the program links (and runs without --offset / --decimate) against a library that has none */
#pragma weak mdemod_fe_design
#pragma weak mdemod_fe_create
#pragma weak mdemod_fe_destroy
#pragma weak mdemod_fe_demodulator
#pragma weak mdemod_fe_process_host
#pragma weak mdemod_fe_demodulate_recording_host
static int
have_frontend(void)
{
	return mdemod_fe_design && mdemod_fe_create && mdemod_fe_destroy && mdemod_fe_demodulator && mdemod_fe_process_host &&
	       mdemod_fe_demodulate_recording_host;
}

/* the survey's entries (include/meteor_demod_amd_survey.h: --offset auto, --decimate auto, --scan): weak as well */
#pragma weak mdemod_survey_default_opts
#pragma weak mdemod_survey_plan
#pragma weak mdemod_survey_host
static int
have_survey(void)
{
	return mdemod_survey_default_opts && mdemod_survey_plan && mdemod_survey_host;
}

/* the frame layer's entries (include/meteor_demod_amd_frames.h: --cadu): weak as well */
#pragma weak mdemod_frames_default_opts
#pragma weak mdemod_frames_decode_host
static int
have_frames(void)
{
	return mdemod_frames_default_opts && mdemod_frames_decode_host;
}

/* the frame layer's link variant (include/meteor_demod_amd_frames_link.h: --diff, --skew): weak as well */
#pragma weak mdemod_frames_link_decode_host
static int
have_frames_link(void)
{
	return mdemod_frames_link_decode_host != NULL;
}

/* the 80 k interleaved mode (include/meteor_demod_amd_interleave.h: --int): weak as well */
#pragma weak mdemod_il_default_opts
#pragma weak mdemod_il_windows
#pragma weak mdemod_il_max_output_symbols
#pragma weak mdemod_il_decode_host
static int
have_interleave(void)
{
	return mdemod_il_default_opts && mdemod_il_windows && mdemod_il_max_output_symbols && mdemod_il_decode_host;
}

/* the transfer-frame layer's entries (include/meteor_demod_amd_rs.h: --vcdu): weak as well */
#pragma weak mdemod_rs_default_opts
#pragma weak mdemod_rs_decode_host
#pragma weak mdemod_rs_vcdu_header
static int
have_rs(void)
{
	return mdemod_rs_default_opts && mdemod_rs_decode_host && mdemod_rs_vcdu_header;
}

/* the image layer's entries (include/meteor_demod_amd_image.h: --image): weak as well */
#pragma weak mdemod_image_default_opts
#pragma weak mdemod_image_decode_host
#pragma weak mdemod_image_free
static int
have_image(void)
{
	return mdemod_image_default_opts && mdemod_image_decode_host && mdemod_image_free;
}

/* the picture layer's entries (include/meteor_demod_amd_picture.h: --rectify, --composite): weak as well */
#pragma weak mdemod_picture_default_opts
#pragma weak mdemod_picture_column_map
#pragma weak mdemod_picture_compose_host
#pragma weak mdemod_picture_free
static int
have_picture(void)
{
	return mdemod_picture_default_opts && mdemod_picture_compose_host && mdemod_picture_free;
}

/* the map layer's entries (include/meteor_demod_amd_map.h: --map): weak as well */
#pragma weak mdemod_map_default_opts
#pragma weak mdemod_map_parse_tle
#pragma weak mdemod_map_fit_time
#pragma weak mdemod_map_compose_host
#pragma weak mdemod_map_free
static int
have_map(void)
{
	return mdemod_map_default_opts && mdemod_map_parse_tle && mdemod_map_fit_time && mdemod_map_compose_host && mdemod_map_free;
}

/* the mosaic layer's entries (include/meteor_demod_amd_mosaic.h: --mosaic): weak as well */
#pragma weak mdemod_mosaic_default_opts
#pragma weak mdemod_mosaic_compose_host
#pragma weak mdemod_mosaic_free
static int
have_mosaic(void)
{
	return mdemod_mosaic_default_opts && mdemod_mosaic_compose_host && mdemod_mosaic_free;
}

/* the polar layer's entries (include/meteor_demod_amd_polar.h: --map-proj stereo): weak as well */
#pragma weak mdemod_polar_default_opts
#pragma weak mdemod_polar_compose_host
#pragma weak mdemod_polar_free
#pragma weak mdemod_polar_graticule
#pragma weak mdemod_polar_lines_free
#pragma weak mdemod_polar_vertices
#pragma weak mdemod_polar_points_free
#pragma weak mdemod_polar_draw_host
#pragma weak mdemod_polar_world_file
#pragma weak mdemod_polar_prj
static int
have_polar(void)
{
	return mdemod_polar_default_opts && mdemod_polar_compose_host && mdemod_polar_free && mdemod_polar_graticule && mdemod_polar_lines_free && mdemod_polar_vertices &&
	       mdemod_polar_points_free && mdemod_polar_draw_host && mdemod_polar_world_file && mdemod_polar_prj;
}

/* the overlay layer's entries (include/meteor_demod_amd_overlay.h: --overlay, --graticule): weak as well */
#pragma weak mdemod_overlay_read
#pragma weak mdemod_overlay_graticule
#pragma weak mdemod_overlay_vectors_free
#pragma weak mdemod_overlay_draw_host
static int
have_overlay(void)
{
	return mdemod_overlay_read && mdemod_overlay_graticule && mdemod_overlay_vectors_free && mdemod_overlay_draw_host;
}

/* the JPEG encoder's entries (include/meteor_demod_amd_jpeg.h: --jpeg): weak as well */
#pragma weak mdemod_jpeg_encode_host
#pragma weak mdemod_jpeg_free
static int
have_jpeg(void)
{
	return mdemod_jpeg_encode_host && mdemod_jpeg_free;
}

/* the equalise layer's entries (include/meteor_demod_amd_equalise.h: --equalise): weak as well */
#pragma weak mdemod_equalise_default_opts
#pragma weak mdemod_equalise_host
static int
have_equalise(void)
{
	return mdemod_equalise_default_opts && mdemod_equalise_host;
}

/* the sun layer's entries (include/meteor_demod_amd_sun.h: --sun): weak as well */
#pragma weak mdemod_sun_default_opts
#pragma weak mdemod_sun_correct_host
static int
have_sun(void)
{
	return mdemod_sun_default_opts && mdemod_sun_correct_host;
}

#define MAX_DEVICES 64
#define OVERLAY_FILES 3

/* what --overlay / --graticule ask of every map and mosaic */
struct overlay_req {
	mdemod_overlay_vectors coast[OVERLAY_FILES];   /* the files of --overlay, read by check_options before anything is demodulated */
	uint32_t n_files;
	int      graticule;                  /* --graticule given */
	double   step;                       /* 0: auto */
	mdemod_overlay_style style[2];       /* 0: the files' lines, 1: the graticule */
};

/* --jpeg: what went through the encoder.  The pictures are written by one thread, after the workers have joined. */
struct jpeg_totals { unsigned long long files, bytes_in, bytes_out; };

/* what --cadu / --vcdu / --image and the options behind them ask of one finished output file: the options as parse_options left
 * them, what check_options read for them, and per file the GPU and the place of its pictures */
struct vcdu_req {
	int      write_cadu, write_vcdu;     /* the .cadu / the .vcdu and their lines */
	int      diff, skew;                 /* --diff, --skew: the link variant of the frame pass */
	uint32_t il_delay;                   /* --int: the branch delay (0: no interleaver) */
	int      image;                      /* the pictures and their line */
	uint32_t apids[3];
	int      rectify;                    /* --rectify: one _rect.pgm per channel; the composite is rectified too */
	int      composite;                  /* 0: none, 1: the slots of comp[], 2: auto */
	uint32_t comp[3];                    /* slots (0 .. 2) of R, G, B */
	double   altitude_km, scan_deg;      /* 0: the library's default */
	int      map;                        /* --map: the pictures on a latitude / longitude grid */
	mdemod_map_tle tle;                  /* the element set of --map (and --norad) */
	double   map_scale, time_offset;     /* --map-scale (0: the default); --time-offset when offset_given */
	int      offset_given, date_given;
	int32_t  map_date;                   /* --date: days since 1970-01-01 */
	int      side;                       /* --scan-side: 0 for the default */
	const char *tle_text;                /* the text of the file of --map, and the catalogue number of --norad (the mosaic takes these) */
	uint32_t norad;
	uint32_t mosaic_blend;               /* --mosaic-blend */
	mdemod_image_result *keep;           /* --mosaic: where this file's pictures go instead of being freed (rows = 0: nothing kept) */
	const struct overlay_req *overlay;   /* --overlay / --graticule: NULL without them */
	int      polar;                      /* --map-proj stereo: _polar.* on a polar stereographic grid instead of _map.* / _mosaic.* */
	double   polar_res, polar_lat_ts;    /* --map-res, --map-lat-ts (0: the defaults) */
	double   polar_lon0;                 /* --map-lon0 when lon0_given (otherwise the pass's own) */
	int      lon0_given;
	unsigned jpeg_quality;               /* --jpeg (0: not given) */
	struct jpeg_totals *jpeg;            /* and where its files are counted */
	struct { unsigned clip_percent, tile, amount; int tile_given, amount_given; } equalise;   /* --equalise: the clip in percent (0: not given), the tile, the amount (0 .. 256) */
	struct { int on; double ref_deg, limit_deg; int ref_given, limit_given; } sun;            /* --sun: given, and the two angles */
	int      device;                     /* the GPU of this file */
};

/* Everything getopt_long produces.  parse_options fills it; nothing writes to it afterwards. */
struct cli_opts {
	const char *prog;
	char *const *files;                  /* the input files: what follows the options */
	int      n_files;
	float    pll_bw, symrate, freq_max_delta;
	int      rrc_order, interp, oqpsk, bps, samplerate;
	int      quiet, batch, stdout_mode, update_interval, force_tui;
	const char *output_fname;
	int      device, devs[MAX_DEVICES], n_dev, plan;
	int      tiled, tile_samples, pilot_margin, carrier_seed, jobs;
	int      use_fe, decimation, auto_offset, auto_decimate, decimate_given, scan;
	double   offset_hz;
	int      want_int;
	long     int_delay;
	struct vcdu_req req;                 /* the options of the product chain (nothing read, no GPU, no place to keep yet) */
	struct overlay_req overlay;          /* the options of --overlay / --graticule (no file read yet) */
	const char *map_fname, *mosaic_base, *overlay_fname[OVERLAY_FILES];
	uint32_t map_norad;
	int      n_overlay;
	int      apids_given, geometry_given, altitude_given, map_opts_given, mosaic_blend_given, polar_opts_given, overlay_opts_given;
};

/* What the checks leave for the product chain: the request every file gets a copy of, the vector files and the element set read,
 * and the run's JPEG count. */
struct products {
	struct vcdu_req req;
	struct overlay_req overlay;
	struct jpeg_totals jpeg;
	char tle_text[65536];
};

/* the long options without a letter */
enum {
	OPT_STDOUT = 256,
	OPT_DEVICE, OPT_TILED, OPT_TILE_SAMPLES, OPT_PILOT_MARGIN, OPT_CARRIER_SEED, OPT_DEVICES, OPT_PLAN, OPT_TUI_SELFTEST,
	OPT_TUI, OPT_JOBS, OPT_OFFSET, OPT_DECIMATE, OPT_SCAN, OPT_CADU, OPT_VCDU, OPT_DIFF, OPT_SKEW, OPT_INT, OPT_INT_DELAY,
	OPT_IMAGE, OPT_APIDS, OPT_RECTIFY, OPT_COMPOSITE, OPT_ALTITUDE, OPT_SCAN_ANGLE, OPT_MAP, OPT_NORAD, OPT_MAP_SCALE,
	OPT_DATE, OPT_TIME_OFFSET, OPT_SCAN_SIDE, OPT_MOSAIC, OPT_MOSAIC_BLEND, OPT_OVERLAY, OPT_GRATICULE, OPT_OVERLAY_COLOUR,
	OPT_OVERLAY_WIDTH, OPT_JPEG, OPT_MAP_PROJ, OPT_MAP_RES, OPT_MAP_LON0, OPT_MAP_LAT_TS, OPT_EQUALISE, OPT_EQUALISE_TILE,
	OPT_EQUALISE_AMOUNT, OPT_SUN, OPT_SUN_REF, OPT_SUN_LIMIT
};

static const struct option longopts[] = {
	{ "batch", 0, NULL, 'B' },      { "pll-bw", 1, NULL, 'b' },   { "freq-delta", 1, NULL, 'd' },
	{ "fir-order", 1, NULL, 'f' },  { "help", 0, NULL, 'h' },     { "mode", 1, NULL, 'm' },
	{ "output", 1, NULL, 'o' },     { "oversamp", 1, NULL, 'O' }, { "quiet", 0, NULL, 'q' },
	{ "refresh-rate", 1, NULL, 'R' }, { "symrate", 1, NULL, 'r' }, { "stdout", 0, NULL, OPT_STDOUT },
	{ "samplerate", 1, NULL, 's' }, { "bps", 1, NULL, 'S' },      { "version", 0, NULL, 'v' },
	{ "device", 1, NULL, OPT_DEVICE },    { "tiled", 0, NULL, OPT_TILED },   { "tile-samples", 1, NULL, OPT_TILE_SAMPLES },
	{ "pilot-margin", 1, NULL, OPT_PILOT_MARGIN }, { "carrier-seed", 1, NULL, OPT_CARRIER_SEED }, { "devices", 1, NULL, OPT_DEVICES }, { "plan", 0, NULL, OPT_PLAN },
	{ "tui-selftest", 0, NULL, OPT_TUI_SELFTEST }, { "tui", 0, NULL, OPT_TUI }, { "jobs", 1, NULL, OPT_JOBS },
	{ "offset", 1, NULL, OPT_OFFSET },    { "decimate", 1, NULL, OPT_DECIMATE }, { "scan", 0, NULL, OPT_SCAN },
	{ "cadu", 0, NULL, OPT_CADU },      { "vcdu", 0, NULL, OPT_VCDU },    { "diff", 0, NULL, OPT_DIFF },    { "skew", 0, NULL, OPT_SKEW },
	{ "int", 0, NULL, OPT_INT },       { "int-delay", 1, NULL, OPT_INT_DELAY }, { "image", 0, NULL, OPT_IMAGE },   { "apids", 1, NULL, OPT_APIDS },
	{ "rectify", 0, NULL, OPT_RECTIFY },   { "composite", 1, NULL, OPT_COMPOSITE }, { "altitude", 1, NULL, OPT_ALTITUDE }, { "scan-angle", 1, NULL, OPT_SCAN_ANGLE },
	{ "map", 1, NULL, OPT_MAP },       { "norad", 1, NULL, OPT_NORAD },   { "map-scale", 1, NULL, OPT_MAP_SCALE }, { "date", 1, NULL, OPT_DATE },
	{ "time-offset", 1, NULL, OPT_TIME_OFFSET }, { "scan-side", 1, NULL, OPT_SCAN_SIDE }, { "mosaic", 1, NULL, OPT_MOSAIC },   { "mosaic-blend", 1, NULL, OPT_MOSAIC_BLEND },
	{ "overlay", 1, NULL, OPT_OVERLAY },   { "graticule", 1, NULL, OPT_GRATICULE }, { "overlay-colour", 1, NULL, OPT_OVERLAY_COLOUR }, { "overlay-width", 1, NULL, OPT_OVERLAY_WIDTH },
	{ "jpeg", 1, NULL, OPT_JPEG },      { "map-proj", 1, NULL, OPT_MAP_PROJ },  { "map-res", 1, NULL, OPT_MAP_RES },   { "map-lon0", 1, NULL, OPT_MAP_LON0 },
	{ "map-lat-ts", 1, NULL, OPT_MAP_LAT_TS }, { "equalise", 1, NULL, OPT_EQUALISE }, { "equalise-tile", 1, NULL, OPT_EQUALISE_TILE }, { "equalise-amount", 1, NULL, OPT_EQUALISE_AMOUNT },
	{ "sun", 0, NULL, OPT_SUN },       { "sun-ref", 1, NULL, OPT_SUN_REF },   { "sun-limit", 1, NULL, OPT_SUN_LIMIT },
	{ NULL, 0, NULL, 0 }
};

/* --offset: a signed number of Hz with an optional k / M suffix (fractions kept); 1 on a malformed one */
static int
parse_hz(const char *s, double *out)
{
	char *end;
	double v = strtod(s, &end);
	if (end == s) return 1;
	if (*end == 'k' || *end == 'K') { v *= 1e3; end++; }
	else if (*end == 'M') { v *= 1e6; end++; }
	if (*end) return 1;
	*out = v;
	return 0;
}

/* utils.c:60-86: number with optional k/M suffix, truncated to int, returned as float */
static float
human_number(const char *s)
{
	const float v = (float)atof(s);
	const char *p = s;
	int out;
	while ((*p >= '0' && *p <= '9') || *p == '.') p++;
	if (*p == 'k' || *p == 'K') out = (int)(v * 1000);
	else if (*p == 'M') out = (int)(v * 1000000);
	else out = (int)v;
	return (float)out;
}

/* "0,2,3" -> device ordinals; returns the count (0 on a malformed list) */
static int
parse_devices(const char *s, int *out, int cap)
{
	int n = 0;
	while (*s && n < cap) {
		char *end;
		const long v = strtol(s, &end, 10);
		if (end == s || v < 0) return 0;
		out[n++] = (int)v;
		if (*end == ',') end++;
		else if (*end) return 0;
		s = end;
	}
	return n;
}

/* the whole of `s` as a number into *out; 0 where it is not one (the message is the caller's) */
static int
whole_double(const char *s, double *out)
{
	char *end;
	*out = strtod(s, &end);
	return end != s && !*end;
}

/* the same within lo .. hi */
static int
double_within(const char *s, double lo, double hi, double *out)
{
	return whole_double(s, out) && *out >= lo && *out <= hi;
}

static int
long_within(const char *s, long lo, long hi, long *out)
{
	char *end;
	*out = strtol(s, &end, 10);
	return end != s && !*end && *out >= lo && *out <= hi;
}

static int
refused(const char *message)
{
	fputs(message, stderr);
	return 1;
}

static void
usage(const char *prog)
{
	fprintf(stderr,
	        "Usage: %s [options] file_in [file_in ...]\n"
	        "   -B, --batch             No full-screen display, status lines one below the other\n"
	        "       --tui               Full-screen display even when stdin / stdout are not a terminal\n"
	        "   -b, --pll-bw <bw>       PLL bandwidth (default: 1)\n"
	        "   -d, --freq-delta <hz>   Max carrier deviation in Hz (default: +-3.5 kHz at 72 ksym/s)\n"
	        "   -f, --fir-order <ord>   RRC filter order (default: 32)\n"
	        "   -m, --mode <mode>       qpsk (default) or oqpsk\n"
	        "   -o, --output <file>     Output file (single input only; default LRPT_<date>.s)\n"
	        "   -O, --oversamp <mult>   Interpolation factor (default: 5)\n"
	        "   -q, --quiet             No status output\n"
	        "   -r, --symrate <rate>    Symbol rate (default: 72000)\n"
	        "   -s, --samplerate <rate> Sample rate of raw input\n"
	        "       --bps <bits>        Bits per sample of raw input (8, 16, 32)\n"
	        "       --stdout            Write soft symbols to stdout (implies -B -q)\n"
	        "       --device <n>        HIP device ordinal (one GPU)\n"
	        "       --devices <a,b,..>  GPUs to spread the input files over, file i on GPU i mod G (default: all\n"
	        "                           GPUs of the node when several files are given); --plan prints the assignment\n"
	        "       --tiled             Each file on many lanes as overlapped tiles (fast, not bit-exact\n"
	        "                           after the head); --tile-samples <n>, --pilot-margin <symbols>,\n"
	        "                           --carrier-seed spectrum|pilot (default spectrum: tiles follow Doppler);\n"
	        "                           --jobs <n>: files of one GPU in flight at once (default 4: their serial heads\n"
	        "                           and file reads overlap)\n"
	        "       --offset <hz>       The signal sits <hz> from the recording's centre (k/M suffixes, may be negative):\n"
	        "                           a front end on the GPU moves it to 0 Hz before the demodulator\n"
	        "       --decimate <n>      The front end low-pass filters and keeps every n-th sample (1..128; the sample\n"
	        "                           rate must be a multiple of n, and rate / n at least 2.4 x the symbol rate); the\n"
	        "                           demodulator runs at rate / n.  Either option turns the front end on\n"
	        "       --offset auto       Survey each input file first (spectrum of the whole file on the GPU, candidates\n"
	        "                           confirmed by their symbol-rate line) and use the offset of the first confirmed\n"
	        "                           signal; exit 1, without an output file, when none is confirmed.  Not on stdin\n"
	        "       --decimate auto     The largest n the front end accepts for this sample and symbol rate (implied by\n"
	        "                           --offset auto when --decimate is absent)\n"
	        "       --scan              Survey only: one line per candidate of each file on stdout,\n"
	        "                           offset_hz psd_snr_db clock_quality carrier_quality confirmed\n"
	        "                           (confirmed ones first, then by psd_snr_db), and exit 0 without demodulating\n"
	        "       --cadu              Frames as well: after an output file is complete, find and decode its CCSDS frames\n"
	        "                           on the GPU (sync search, Viterbi) and write them, 1024 bytes each, beside it as\n"
	        "                           <output>.cadu (.s replaced); one line per file on stdout: frames, flywheel frames,\n"
	        "                           runs, mean channel errors / 16372.  Not with --stdout\n"
	        "       --vcdu              Transfer frames as well: the frames of --cadu derandomised and Reed-Solomon corrected\n"
	        "                           on the GPU, written 892 bytes each as <output>.vcdu (uncorrectable frames included:\n"
	        "                           frame i of the .vcdu is frame i of the .cadu); one more line on stdout: frames,\n"
	        "                           uncorrectable frames, bytes corrected, frames and counter gaps per VCID.  The .cadu\n"
	        "                           is written only with --cadu.  Not with --stdout\n"
	        "       --image             Pictures as well: the packet zone of the transfer frames demultiplexed into CCSDS packets\n"
	        "                           and the MSU-MR image packets decoded on the GPU; every active channel that received a\n"
	        "                           strip is written as <output>_<apid>.pgm (binary P5, 1568 wide, 8 bit); one more line on\n"
	        "                           stdout: packets, image packets per APID, strips truncated, lines, share of cells\n"
	        "                           filled.  Implies the --vcdu pass; the .vcdu / .cadu are written only with --vcdu /\n"
	        "                           --cadu.  Not with --stdout\n"
	        "       --apids <a,b,c>     With --image: the three active channels, each 64 .. 69 (default: 64,65,66)\n"
	        "       --rectify           With --image: every channel that received a strip also as <output>_<apid>_rect.pgm,\n"
	        "                           resampled on the GPU to equal ground distance (the Earth's curvature taken out; wider\n"
	        "                           than 1568) and contrast-stretched between the 0.5 %% and 99.5 %% points of its pixels\n"
	        "       --composite <abc>   With --image: a colour picture <output>_<abc>.ppm (binary P6); a, b, c are the channels\n"
	        "                           of red, green and blue, each 1 .. 3, counted in --apids order (e.g. 321); stretched,\n"
	        "                           and rectified when --rectify is given; one more line on stdout: width, lines, the\n"
	        "                           stretch limits per plane, the share of valid pixels.  --composite auto: 321 when all\n"
	        "                           three channels received a strip, 221 when only the first two did, otherwise none\n"
	        "       --altitude <km>     With --rectify: the orbit's altitude (300 .. 2000, default: 820)\n"
	        "       --scan-angle <deg>  With --rectify: the scanner's full scan angle (1 .. 130, default: 110)\n"
	        "       --map <tle file>    With --image: the pictures on a north-up latitude / longitude grid (EPSG:4326), from the\n"
	        "                           packets' onboard time stamps and the two-line element set of the file (a circular orbit\n"
	        "                           with the secular J2 terms, not SGP4): with --composite <output>_<abc>_map.ppm, without\n"
	        "                           it one <output>_<apid>_map.pgm per channel that received a strip; beside each a world\n"
	        "                           file ending in .wld; one more line on stdout: size, scale, corners, the fitted row\n"
	        "                           period, the UTC of the first line, the share of valid pixels.  --scan-angle applies\n"
	        "       --norad <id>        With --map: the catalogue number of the set to take (default: the file's first)\n"
	        "       --map-scale <n>     With --map: pixels per degree of latitude (1 .. 1000, default: 100)\n"
	        "       --date <yyyy-mm-dd> With --map: the date of the first line's onboard time (default: the one nearest the epoch)\n"
	        "       --time-offset <s>   With --map: onboard clock minus UTC in seconds (default: 10800, Moscow time)\n"
	        "       --scan-side <1|-1>  With --map: which way the mirror turns (default: 1)\n"
	        "       --map-proj <p>      With --map: latlon (default) or stereo: a polar stereographic grid on WGS-84 in metres, for\n"
	        "                           passes over a pole, which the latitude / longitude grid refuses beyond 85 degrees.  The\n"
	        "                           pictures are <output>_<tag>_polar.ppm / .pgm instead of _map.*, each with a world file\n"
	        "                           (.wld) and the projection as WKT (.prj); with --mosaic also <base>_<tag>_polar.* of all\n"
	        "                           passes; --overlay and --graticule draw onto _polar_overlay.*; one line on stdout each\n"
	        "       --map-res <metres>  With --map-proj stereo: metres per pixel (100 .. 100000, default: 1000)\n"
	        "       --map-lon0 <deg|auto>  With --map-proj stereo: the meridian that points down (north) or up (south) in the\n"
	        "                           picture (default: auto, the longitude of the pass's middle rounded to a degree)\n"
	        "       --map-lat-ts <deg>  With --map-proj stereo: the latitude of true scale, a magnitude (default: 70)\n"
	        "       --mosaic <base>     With --map: the input files (1 .. 8) are passes of one satellite; besides each file's own\n"
	        "                           maps all passes are blended onto one common grid on the first GPU, where several saw the\n"
	        "                           same ground weighted by the distance from the edge of the swath: <base>_<abc>_mosaic.ppm\n"
	        "                           with --composite (auto: on what the passes received together), without it one\n"
	        "                           <base>_<apid>_mosaic.pgm per channel; beside each a world file ending in .wld; one more\n"
	        "                           line on stdout: size, scale, corners, the passes with the UTC of their first lines, the\n"
	        "                           share of valid pixels and of pixels seen by two or more passes.  The options of --map\n"
	        "                           apply to every pass; a file without a picture is left out\n"
	        "       --mosaic-blend <m>  With --mosaic: feather (default: the weighted mean) or best (the pass nearest its nadir)\n"
	        "       --overlay <file>    With --map: beside every map and mosaic a second picture, <...>_map_overlay.ppm / .pgm or\n"
        "                           <...>_mosaic_overlay.*, with the polylines of the file drawn on it on the GPU, and its own\n"
        "                           world file; the plain pictures stay as they are.  The file is a shapefile's main file\n"
        "                           (.shp; lines and polygons) or text, one \"lon lat\" per line, an empty line or one that\n"
        "                           begins with > between polylines.  Up to three times.  One more line on stdout: pieces\n"
        "                           kept, tiles touched and pixels drawn per style\n"
        "       --graticule <deg>   With --map: meridians and parallels every <deg> degrees on the overlay picture (auto: from\n"
        "                           the scale)\n"
        "       --overlay-colour <rrggbb>  The colour of the lines of --overlay (default: ffff00)\n"
        "       --overlay-width <px>       Their width in pixels (0 .. 16, default: 1)\n"
        "       --jpeg <quality>    With --image: every picture (the channels, _rect, the composite, _map, _mosaic, _overlay) as a\n"
        "                           baseline JPEG <same name>.jpg of that quality (1 .. 100), encoded on the GPU, instead of the\n"
        "                           .pgm / .ppm; world files keep their names.  One line on stdout per file, and one at the end:\n"
        "                           files, bytes of pictures in, bytes of JPEG out\n"
        "       --equalise <clip>   With --image and --rectify, --composite or --map: local contrast (CLAHE) on the GPU for every\n"
        "                           derived picture (_rect, the composite, _map, _mosaic, _polar) in place, after it is composed\n"
        "                           and before lines are drawn on it or it is written: per tile a histogram of the valid pixels\n"
        "                           clipped at <clip> times a flat one (1 .. 256; 3 is usual), tables blended between tile\n"
        "                           centres; colour pictures through their luminance.  The channel pictures stay as decoded and\n"
        "                           no file changes its name.  One line on stdout per picture: tile, clip, tiles, empty tiles\n"
        "       --equalise-tile <pixels>   With --equalise: the tile, a multiple of 8, 16 .. 512 (default: 128)\n"
        "       --equalise-amount <percent>  With --equalise: how much of the equalised picture is taken, 0 .. 100 (default: 100)\n"
        "       --sun               With --image and --map: take the cosine of the sun's zenith angle out of the reflective channels\n"
        "                           (APIDs 64 .. 66) on the GPU before any derived picture or the mosaic is made; the channel\n"
        "                           pictures stay as decoded\n"
        "       --sun-ref <deg>     With --sun: the zenith angle whose counts stay as they are, 0 .. 80 (default: 45)\n"
        "       --sun-limit <deg>   With --sun: the zenith angle beyond which the gain grows no further, 60 .. 89 (default: 85)\n"
        "       --diff              With --cadu / --vcdu: the sender codes differentially (NRZ-M); the frame pass searches\n"
	        "                           the differential marker and undoes the coding after the Viterbi decoder\n"
	        "       --skew              With --cadu / --vcdu: the rails may stand one symbol apart, as after -m oqpsk when\n"
	        "                           the carrier loop settles a quarter turn off; the frame pass tries both skews as well.\n"
	        "                           Meteor-M N2-3 / N2-4 (72k OQPSK) want: -m oqpsk --skew --diff\n"
	        "       --int               With --cadu / --vcdu: the 80k interleaved mode; the interleaver's sync word is found,\n"
	        "                           followed across slips and stripped, and the stream deinterleaved on the GPU before\n"
	        "                           the frame pass; one more line on stdout: segments, periods, mean sync score.\n"
	        "                           --skew beside it is ignored (the sync word resolves the skew); --diff still applies\n"
	        "       --int-delay <M>     The interleaver's branch delay (default: 2048)\n"
	        "   -h, --help   -v, --version\n", prog);
}

/* days since 1970-01-01 to a civil date */
static void
civil_from_days(int64_t z, int *y, unsigned *m, unsigned *d)
{
	z += 719468;
	const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
	const unsigned doe = (unsigned)(z - era * 146097), yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
	const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100), mp = (5 * doy + 2) / 153;
	*d = doy - (153 * mp + 2) / 5 + 1;
	*m = mp < 10 ? mp + 3 : mp - 9;
	*y = (int)((int64_t)yoe + era * 400 + (*m <= 2));
}

static int64_t
days_from_civil(int64_t y, unsigned m, unsigned d)
{
	y -= m <= 2;
	const int64_t era = (y >= 0 ? y : y - 399) / 400;
	const unsigned yoe = (unsigned)(y - era * 400), doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1, doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
	return era * 146097 + (int64_t)doe - 719468;
}

/* the options of --map as the layer takes them */
static void
map_options(const struct vcdu_req *req, mdemod_map_opts *mo)
{
	mdemod_map_default_opts(mo);
	if (req->scan_deg != 0.0) mo->scan_deg = req->scan_deg;
	if (req->map_scale != 0.0) mo->px_per_deg = req->map_scale;
	if (req->offset_given) mo->time_offset = req->time_offset;
	if (req->date_given) mo->date = req->map_date;
	if (req->side) mo->side = req->side;
}

#define GO_ON (-1)                      /* what a stage of main returns when the run goes on: anything else is the exit status */

/* One option of --map and of what goes on from it (--mosaic, --overlay, --map-proj stereo) into *o, or none of the program's: the
 * usage text.  GO_ON, or the exit status. */
static int
set_map_option(struct cli_opts *o, int c, const char *arg)
{
	struct vcdu_req *q = &o->req;
	double v;
	long n;
	switch (c) {
	case OPT_MAP: o->map_fname = arg; break;
	case OPT_NORAD:
		if (!long_within(arg, 1, 999999999, &n)) return refused("--norad: a catalogue number\n");
		o->map_norad = (uint32_t)n; o->map_opts_given = 1; break;
	case OPT_MAP_SCALE:
		if (!whole_double(arg, &v)) return refused("--map-scale: a number\n");
		q->map_scale = v == 0.0 ? -1.0 : v;                                      /* (0 stands for the default inside: let the layer refuse it) */
		o->map_opts_given = 1; break;
	case OPT_TIME_OFFSET:
		if (!whole_double(arg, &v)) return refused("--time-offset: a number\n");
		q->time_offset = v; q->offset_given = o->map_opts_given = 1; break;
	case OPT_DATE: {
		int y;
		unsigned m, d;
		char tail;
		if (sscanf(arg, "%d-%u-%u%c", &y, &m, &d, &tail) != 3 || y < 1957 || y > 2200 || m < 1 || m > 12 || d < 1 || d > 31) return refused("--date: yyyy-mm-dd\n");
		q->map_date = (int32_t)days_from_civil(y, m, d); q->date_given = o->map_opts_given = 1; break;
	}
	case OPT_SCAN_SIDE:
		if (strcmp(arg, "1") && strcmp(arg, "-1")) return refused("--scan-side: 1 or -1\n");
		q->side = atoi(arg); o->map_opts_given = 1; break;
	case OPT_MOSAIC: o->mosaic_base = arg; break;
	case OPT_MOSAIC_BLEND:
		if (!strcmp(arg, "feather")) q->mosaic_blend = MDEMOD_MOSAIC_FEATHER;
		else if (!strcmp(arg, "best")) q->mosaic_blend = MDEMOD_MOSAIC_BEST;
		else return refused("--mosaic-blend: feather or best\n");
		o->mosaic_blend_given = 1; break;
	case OPT_OVERLAY:
		if (o->n_overlay == OVERLAY_FILES) { fprintf(stderr, "--overlay: at most %d files\n", OVERLAY_FILES); return 1; }
		o->overlay_fname[o->n_overlay++] = arg; break;
	case OPT_GRATICULE:
		o->overlay.graticule = 1;
		o->overlay.step = 0.0;
		if (strcmp(arg, "auto") && !double_within(arg, 0.01, 90.0, &o->overlay.step)) return refused("--graticule: a number of degrees (0.01 .. 90) or auto\n");
		break;
	case OPT_OVERLAY_COLOUR: {
		unsigned r, g, b;
		char tail;
		if (strlen(arg) != 6 || sscanf(arg, "%2x%2x%2x%c", &r, &g, &b, &tail) != 3) return refused("--overlay-colour: six hexadecimal digits, rrggbb\n");
		o->overlay.style[0].colour[0] = (uint8_t)r; o->overlay.style[0].colour[1] = (uint8_t)g; o->overlay.style[0].colour[2] = (uint8_t)b;
		o->overlay_opts_given = 1; break;
	}
	case OPT_OVERLAY_WIDTH:
		if (!double_within(arg, 0.0, 16.0, &v)) return refused("--overlay-width: a number of pixels, 0 .. 16\n");
		o->overlay.style[0].half_width = (uint32_t)(128.0 * v + 0.5); o->overlay_opts_given = 1; break;
	case OPT_MAP_PROJ:
		if (!strcmp(arg, "stereo")) q->polar = 1;
		else if (!strcmp(arg, "latlon")) q->polar = 0;
		else return refused("--map-proj: latlon or stereo\n");
		o->map_opts_given = 1; break;
	case OPT_MAP_RES:
		if (!whole_double(arg, &v)) return refused("--map-res: a number\n");
		if (!(v >= MDEMOD_POLAR_MIN_RES && v <= MDEMOD_POLAR_MAX_RES)) return refused("--map-res: metres per pixel, 100 .. 100000\n");
		q->polar_res = v; o->polar_opts_given = o->map_opts_given = 1; break;
	case OPT_MAP_LON0:
		q->lon0_given = strcmp(arg, "auto") != 0;
		if (q->lon0_given && !whole_double(arg, &q->polar_lon0)) return refused("--map-lon0: a number\n");
		if (q->lon0_given && !(q->polar_lon0 >= -360.0 && q->polar_lon0 <= 360.0)) return refused("--map-lon0: degrees, -360 .. 360, or auto\n");
		o->polar_opts_given = o->map_opts_given = 1; break;
	case OPT_MAP_LAT_TS:
		if (!whole_double(arg, &v)) return refused("--map-lat-ts: a number\n");
		if (!(v > 0.0 && v <= 90.0)) return refused("--map-lat-ts: the magnitude of the standard parallel in degrees, 0 < .. <= 90\n");
		q->polar_lat_ts = v; o->polar_opts_given = o->map_opts_given = 1; break;
	default: usage(o->prog); return 1;
	}
	return GO_ON;
}

/* One option of --image and of what is made of its pictures into *o (the maps: above).  GO_ON, or the exit status. */
static int
set_picture_option(struct cli_opts *o, int c, const char *arg)
{
	struct vcdu_req *q = &o->req;
	double v;
	long n;
	switch (c) {
	case OPT_IMAGE: q->image = 1; break;
	case OPT_APIDS: {
		unsigned a[3];
		char tail;
		if (sscanf(arg, "%u,%u,%u%c", &a[0], &a[1], &a[2], &tail) != 3) return refused("--apids: three numbers, e.g. 64,65,66\n");
		for (int k = 0; k < 3; k++) {
			if (a[k] < 64 || a[k] > 69 || (k && a[k] == a[0]) || (k == 2 && a[2] == a[1])) return refused("--apids: three different channels, each 64 .. 69\n");
			q->apids[k] = a[k];
		}
		o->apids_given = 1; break;
	}
	case OPT_RECTIFY: q->rectify = 1; break;
	case OPT_COMPOSITE:
		if (!strcmp(arg, "auto")) { q->composite = 2; break; }
		if (strlen(arg) != 3 || strspn(arg, "123") != 3)
			return refused("--composite: three digits, each 1 .. 3 (the channels of red, green, blue in --apids order, e.g. 321), or auto\n");
		for (int k = 0; k < 3; k++) q->comp[k] = (uint32_t)(arg[k] - '1');
		q->composite = 1; break;
	case OPT_ALTITUDE:
		if (!whole_double(arg, &v) || !(v > 0.0)) return refused("--altitude: a positive number\n");
		q->altitude_km = v; o->altitude_given = o->geometry_given = 1; break;
	case OPT_SCAN_ANGLE:
		if (!whole_double(arg, &v) || !(v > 0.0)) return refused("--scan-angle: a positive number\n");
		q->scan_deg = v; o->geometry_given = 1; break;
	case OPT_JPEG:
		if (!long_within(arg, 1, 100, &n)) return refused("--jpeg: a quality, 1 .. 100\n");
		q->jpeg_quality = (unsigned)n; break;
	case OPT_EQUALISE:
		if (!double_within(arg, 1.0, 256.0, &v)) return refused("--equalise: a clip limit, 1 .. 256 (times a flat histogram; 3 is usual)\n");
		q->equalise.clip_percent = (unsigned)(100.0 * v + 0.5); break;
	case OPT_EQUALISE_TILE:
		if (!long_within(arg, MDEMOD_EQUALISE_MIN_TILE, MDEMOD_EQUALISE_MAX_TILE, &n) || n % 8) return refused("--equalise-tile: pixels, a multiple of 8, 16 .. 512\n");
		q->equalise.tile = (unsigned)n; q->equalise.tile_given = 1; break;
	case OPT_EQUALISE_AMOUNT:
		if (!double_within(arg, 0.0, 100.0, &v)) return refused("--equalise-amount: percent, 0 .. 100\n");
		q->equalise.amount = (unsigned)(2.56 * v + 0.5); q->equalise.amount_given = 1; break;
	case OPT_SUN: q->sun.on = 1; break;
	case OPT_SUN_REF:
		if (!double_within(arg, 0.0, MDEMOD_SUN_MAX_REF, &q->sun.ref_deg)) return refused("--sun-ref: degrees of zenith angle, 0 .. 80\n");
		q->sun.ref_given = 1; break;
	case OPT_SUN_LIMIT:
		if (!double_within(arg, MDEMOD_SUN_MIN_LIMIT, MDEMOD_SUN_MAX_LIMIT, &q->sun.limit_deg)) return refused("--sun-limit: degrees of zenith angle, 60 .. 89\n");
		q->sun.limit_given = 1; break;
	default: return set_map_option(o, c, arg);
	}
	return GO_ON;
}

/* One option into *o: the demodulator's, the GPUs', the front end's and the frame pass's here, the rest above.  GO_ON, or the exit
 * status (--help, --version and --tui-selftest end the run as well). */
static int
set_option(struct cli_opts *o, int c, const char *arg)
{
	long n;
	switch (c) {
	case OPT_STDOUT: o->stdout_mode = 1; break;
	case OPT_DEVICE: o->device = atoi(arg); o->devs[0] = o->device; o->n_dev = 1; break;
	case OPT_DEVICES:
		o->n_dev = parse_devices(arg, o->devs, MAX_DEVICES);
		if (!o->n_dev) return refused("--devices: a comma separated list of GPU ordinals\n");
		break;
	case OPT_PLAN: o->plan = 1; break;
	case OPT_TUI: o->force_tui = 1; break;               /* (in a build without the display: accepted, nothing to draw) */
	case OPT_JOBS: o->jobs = atoi(arg); if (o->jobs < 1) return refused("--jobs: a positive number\n"); break;
	case OPT_SCAN: o->scan = 1; break;
	case OPT_CADU: o->req.write_cadu = 1; break;
	case OPT_VCDU: o->req.write_vcdu = 1; break;
	case OPT_DIFF: o->req.diff = 1; break;
	case OPT_SKEW: o->req.skew = 1; break;
	case OPT_INT: o->want_int = 1; break;
	case OPT_INT_DELAY: o->int_delay = atol(arg); break;
	case OPT_OFFSET:
		o->use_fe = 1;
		o->auto_offset = !strcmp(arg, "auto");
		if (!o->auto_offset && parse_hz(arg, &o->offset_hz)) return refused("--offset: a number of Hz (k/M suffixes), e.g. 300k or -1.2M\n");
		break;
	case OPT_DECIMATE:
		o->use_fe = 1;
		o->auto_decimate = !strcmp(arg, "auto");
		o->decimate_given = !o->auto_decimate;
		if (o->auto_decimate) break;
		if (!long_within(arg, 1, 1 << 20, &n)) return refused("--decimate: a positive integer, or auto\n");
		o->decimation = (int)n; break;
	case OPT_TUI_SELFTEST:
#ifdef MDEMOD_TUI
		return tui_selftest(o->force_tui);
#else
		return refused("built without ncurses\n");
#endif
	case OPT_TILED: o->tiled = 1; break;
	case OPT_TILE_SAMPLES: o->tile_samples = (int)human_number(arg); break;
	case OPT_PILOT_MARGIN: o->pilot_margin = (int)human_number(arg); break;
	case OPT_CARRIER_SEED:
		if (!strcmp(arg, "spectrum")) o->carrier_seed = 1;
		else if (!strcmp(arg, "pilot")) o->carrier_seed = 0;
		else return refused("--carrier-seed: spectrum or pilot\n");
		break;
	case 'b': o->pll_bw = human_number(arg); break;
	case 'B': o->batch = 1; break;
	case 'd': o->freq_max_delta = human_number(arg); break;
	case 'f': o->rrc_order = atoi(arg); break;
	case 'h': usage(o->prog); return 0;
	case 'm': if (!strcmp(arg, "oqpsk")) o->oqpsk = 1; break;     /* unknown modes stay QPSK, main.c:104 */
	case 'o': o->output_fname = arg; break;
	case 'O': o->interp = atoi(arg); break;
	case 'q': o->quiet = 1; break;
	case 'R': o->update_interval = atoi(arg); break;              /* main.c:116 */
	case 'r': o->symrate = human_number(arg); break;
	case 's': o->samplerate = (int)human_number(arg); break;
	case 'S': o->bps = atoi(arg); break;
	case 'v': printf("meteor_demod_amd (MI355X) ABI %u\n", mdemod_abi_version()); return 0;
	default: return set_picture_option(o, c, arg);
	}
	return GO_ON;
}

/* The command line into *o: the defaults, every option, and what the reference derives from them at once.  GO_ON, or the exit status. */
static int
parse_options(int argc, char **argv, struct cli_opts *o)
{
	memset(o, 0, sizeof *o);
	o->prog = argv[0];
	o->pll_bw = MDEMOD_DEFAULT_PLL_BW; o->symrate = MDEMOD_DEFAULT_SYM_RATE; o->freq_max_delta = -1;
	o->rrc_order = MDEMOD_DEFAULT_RRC_ORDER; o->interp = MDEMOD_DEFAULT_INTERP;
	o->samplerate = -1; o->pilot_margin = -1; o->carrier_seed = -1; o->update_interval = -1;
	o->jobs = 4; o->decimation = 1; o->int_delay = MDEMOD_IL_DEFAULT_BRANCH_DELAY;
	o->req.apids[0] = 64; o->req.apids[1] = 65; o->req.apids[2] = 66; o->req.comp[0] = 2; o->req.comp[1] = 1;
	o->req.equalise.tile = 128; o->req.equalise.amount = 256;
	/* --overlay: yellow, one pixel, opaque; --graticule: grey, one pixel, opacity 160 */
	o->overlay.style[0] = (mdemod_overlay_style){ 128, 256, { 255, 255, 0 }, 0 };
	o->overlay.style[1] = (mdemod_overlay_style){ 128, 160, { 128, 128, 128 }, 0 };
	int c;
	while ((c = getopt_long(argc, argv, "a:Bb:d:f:hm:o:O:qR:r:s:S:v", longopts, NULL)) != -1) {
		const int code = set_option(o, c, optarg);
		if (code != GO_ON) return code;
	}
	o->freq_max_delta = (float)(o->freq_max_delta * (2 * M_PI) / o->symrate);       /* main.c:136 */
	if (argc - optind < 1) { usage(argv[0]); return 1; }
	o->files = argv + optind; o->n_files = argc - optind;
	if (o->update_interval < 0) o->update_interval = o->batch ? 2000 : 50;             /* main.c:144 (before batch is forced below) */
	if (o->stdout_mode) { o->batch = 1; o->quiet = 1; }
	for (int i = 0; i < o->n_files; i++) if (!strcmp(o->files[i], "-")) o->batch = 1;  /* stdin forces batch: main.c:157 */
	return GO_ON;
}

/* The rules about which options go together and which layers the library has, in the order in which they are refused: the first
 * broken one speaks.  Nothing is read and the library is not asked anything yet.  GO_ON, or 1. */
static int
check_combinations(const struct cli_opts *o)
{
	const struct vcdu_req *q = &o->req;
	const int overlays = o->n_overlay || o->overlay.graticule;
	if (o->n_files > 1 && (o->output_fname || o->stdout_mode)) return refused("-o/--stdout need a single input file\n");
	if (o->use_fe && !have_frontend()) return refused("--offset / --decimate: this library has no front end (built without include/meteor_demod_amd_frontend.h's entries)\n");
	if ((o->auto_offset || o->auto_decimate || o->scan) && !have_survey()) return refused("--offset auto / --decimate auto / --scan: this library has no survey (built without include/meteor_demod_amd_survey.h's entries)\n");
	if (q->write_cadu && o->stdout_mode) return refused("--cadu: not with --stdout (the frames are decoded from the finished output file)\n");
	if (q->write_cadu && !have_frames()) return refused("--cadu: this library has no frame layer (built without include/meteor_demod_amd_frames.h's entries)\n");
	if (q->write_vcdu && o->stdout_mode) return refused("--vcdu: not with --stdout (the frames are decoded from the finished output file)\n");
	if (q->write_vcdu && !(have_frames() && have_rs())) {
		fprintf(stderr, "--vcdu: this library has no %s (built without include/%s's entries)\n", have_frames() ? "transfer-frame layer" : "frame layer",
		        have_frames() ? "meteor_demod_amd_rs.h" : "meteor_demod_amd_frames.h");
		return 1;
	}
	if (q->polar && !(have_polar() && have_map() && have_picture())) return refused("--map-proj stereo: this library has no polar layer (built without include/meteor_demod_amd_polar.h's entries)\n");
	if (o->polar_opts_given && !q->polar) return refused("--map-res / --map-lon0 / --map-lat-ts: only with --map-proj stereo (they are its options)\n");
	if (q->polar && q->map_scale != 0.0) return refused("--map-scale: not with --map-proj stereo (pixels per degree belong to the latitude / longitude grid: --map-res)\n");
	if (o->mosaic_base && !(have_mosaic() && have_map() && have_picture())) return refused("--mosaic: this library has no mosaic layer (built without include/meteor_demod_amd_mosaic.h's entries)\n");
	if ((overlays || o->overlay_opts_given) && !have_overlay()) return refused("--overlay / --graticule: this library has no overlay layer (built without include/meteor_demod_amd_overlay.h's entries)\n");
	if (o->map_fname && !(have_map() && have_picture())) return refused("--map: this library has no map layer (built without include/meteor_demod_amd_map.h's entries)\n");
	if (o->apids_given && !q->image) return refused("--apids: only with --image (it chooses the channels of the pictures)\n");
	if (q->image && o->stdout_mode) return refused("--image: not with --stdout (the frames are decoded from the finished output file)\n");
	if (q->image && !(have_frames() && have_rs() && have_image())) {
		fprintf(stderr, "--image: this library has no %s (built without include/%s's entries)\n",
		        !have_frames() ? "frame layer" : !have_rs() ? "transfer-frame layer" : "image layer",
		        !have_frames() ? "meteor_demod_amd_frames.h" : !have_rs() ? "meteor_demod_amd_rs.h" : "meteor_demod_amd_image.h");
		return 1;
	}
	if ((q->rectify || q->composite) && !q->image) return refused("--rectify / --composite: only with --image (they work on its pictures)\n");
	if ((o->map_fname || o->map_opts_given) && !q->image) return refused("--map: only with --image (it works on its pictures and their time stamps)\n");
	if (o->map_opts_given && !o->map_fname) return refused("--norad / --map-scale / --date / --time-offset / --scan-side / --map-proj: only with --map (they are its options)\n");
	if (o->mosaic_base && !(o->map_fname && q->image)) return refused("--mosaic: only with --map (and --image: it blends the maps of the input files)\n");
	if (o->mosaic_blend_given && !o->mosaic_base) return refused("--mosaic-blend: only with --mosaic (it is its option)\n");
	if (overlays && !(o->map_fname && q->image)) return refused("--overlay / --graticule: only with --map (they draw on its pictures)\n");
	if (o->overlay_opts_given && !o->n_overlay) return refused("--overlay-colour / --overlay-width: only with --overlay (they are its options)\n");
	if ((q->equalise.tile_given || q->equalise.amount_given) && !q->equalise.clip_percent) return refused("--equalise-tile / --equalise-amount: only with --equalise (they are its options)\n");
	if (q->equalise.clip_percent && !q->image) return refused("--equalise: only with --image (it works on its pictures)\n");
	if (q->equalise.clip_percent && !(q->rectify || q->composite || o->map_fname)) return refused("--equalise: only with --rectify, --composite or --map (it works on the derived pictures; the channel pictures stay as decoded)\n");
	if ((q->sun.ref_given || q->sun.limit_given) && !q->sun.on) return refused("--sun-ref / --sun-limit: only with --sun (they are its options)\n");
	if (q->sun.on && !q->image) return refused("--sun: only with --image (it works on its pictures)\n");
	if (q->sun.on && !o->map_fname) return refused("--sun: only with --map <tle file> (the sun's angle needs the orbit and the line times; the channel pictures stay as decoded)\n");
	if (q->sun.on && !have_sun()) return refused("--sun: this build of libmeteor_demod_amd has no sun layer\n");
	if (q->equalise.clip_percent && !have_equalise()) return refused("--equalise: this build of libmeteor_demod_amd has no equalise layer\n");
	if (q->jpeg_quality && !q->image) return refused("--jpeg: only with --image (it is the format of its pictures)\n");
	if (q->jpeg_quality && !have_jpeg()) return refused("--jpeg: this build of libmeteor_demod_amd has no JPEG encoder\n");
	if (o->mosaic_base && o->n_files > MDEMOD_MOSAIC_MAX_PASSES) {
		fprintf(stderr, "--mosaic: %d input files are more than a mosaic takes (1 .. 8 passes)\n", o->n_files);
		return 1;
	}
	return GO_ON;
}

/* Every refusal between the option loop and the first input file, in the order the program has always had: the rules above, then
 * what is read and tried before anything is demodulated - the element set of --map with a fit of no packets (options out of range
 * are refused with their own text first), the vector files of --overlay, the geometry of --rectify - then the rules of the frame
 * pass.  What the product chain needs of it goes into *pr.  GO_ON, or 1. */
static int
check_options(const struct cli_opts *o, struct products *pr)
{
	struct vcdu_req *q = &pr->req;
	const int frames = o->req.write_cadu || o->req.write_vcdu || o->req.image;
	pr->req = o->req;
	memset(&pr->jpeg, 0, sizeof pr->jpeg);
	pr->req.jpeg = &pr->jpeg;
	pr->overlay = o->overlay;
	if (check_combinations(o) != GO_ON) return 1;
	if (o->map_fname) {
		FILE *tf = fopen(o->map_fname, "rb");
		const size_t got = tf ? fread(pr->tle_text, 1, sizeof pr->tle_text - 1, tf) : 0;
		if (!tf || ferror(tf)) { fprintf(stderr, "--map: could not read %s\n", o->map_fname); if (tf) fclose(tf); return 1; }
		fclose(tf);
		pr->tle_text[got] = 0;
		for (size_t k = 0; k < got; k++) if (!pr->tle_text[k]) pr->tle_text[k] = ' ';
		if (mdemod_map_parse_tle(pr->tle_text, o->map_norad, &q->tle) != MDEMOD_OK) { fprintf(stderr, "--map: %s: %s\n", o->map_fname, mdemod_last_error()); return 1; }
		mdemod_map_opts mo;
		mdemod_map_timing none;
		map_options(q, &mo);
		if (mdemod_map_fit_time(NULL, NULL, 0, &mo, &none) != MDEMOD_OK && strncmp(mdemod_last_error(), "map: no placed packet", 21)) {
			fprintf(stderr, "--map: %s\n", mdemod_last_error());
			return 1;
		}
		q->map = 1;
		q->tle_text = pr->tle_text;
		q->norad = o->map_norad;
	}
	for (int k = 0; k < o->n_overlay; k++) {
		if (mdemod_overlay_read(o->overlay_fname[k], &pr->overlay.coast[k]) != MDEMOD_OK) { fprintf(stderr, "--overlay: %s: %s\n", o->overlay_fname[k], mdemod_last_error()); return 1; }
		pr->overlay.n_files++;
	}
	if (o->n_overlay || o->overlay.graticule) q->overlay = &pr->overlay;
	if (o->geometry_given && !q->rectify && (o->altitude_given || !o->map_fname)) return refused("--altitude / --scan-angle: only with --rectify (they are the geometry it takes out)\n");
	if ((q->rectify || q->composite) && !have_picture()) return refused("--rectify / --composite: this library has no picture layer (built without include/meteor_demod_amd_picture.h's entries)\n");
	if (q->rectify) {
		mdemod_picture_opts po;
		mdemod_picture_default_opts(&po);
		if (q->altitude_km != 0.0) po.altitude_km = q->altitude_km;
		if (q->scan_deg != 0.0) po.scan_deg = q->scan_deg;
		uint32_t w = 0;
		if (!mdemod_picture_column_map || mdemod_picture_column_map(&po, NULL, 0, &w) != MDEMOD_OK) {
			fprintf(stderr, "--rectify: %s\n", mdemod_picture_column_map ? mdemod_last_error() : "this library has no column map");
			return 1;
		}
	}
	if ((q->diff || q->skew) && !frames) return refused("--diff / --skew: only with --cadu or --vcdu (they change how the frames are found and decoded, not the soft symbols)\n");
	if (o->want_int && o->stdout_mode) return refused("--int: not with --stdout (the frames are decoded from the finished output file)\n");
	if (o->want_int && !frames) return refused("--int: only with --cadu or --vcdu (it changes how the frames are found and decoded, not the soft symbols)\n");
	if (o->want_int && !have_interleave()) return refused("--int: this library has no interleaved mode (built without include/meteor_demod_amd_interleave.h's entries)\n");
	if (o->want_int && (o->int_delay < 1 || o->int_delay > 0x7FFFFFFFL)) return refused("--int-delay: the branch delay is a number of bits, 1 or more\n");
	if (o->want_int) q->il_delay = (uint32_t)o->int_delay;
	if (o->want_int && q->skew) {
		fprintf(stderr, "--skew: ignored with --int (the interleaver's sync word resolves the skew)\n");
		q->skew = 0;
	}
	if ((q->diff || q->skew) && !have_frames_link()) return refused("--diff / --skew: this library has no link variant of the frame layer (built without include/meteor_demod_amd_frames_link.h's entries)\n");
	if (o->auto_offset || o->scan)
		for (int i = 0; i < o->n_files; i++)
			if (!strcmp(o->files[i], "-"))
				return refused("--offset auto / --scan: not on stdin (there is nothing to look ahead in): give the offset with --offset <hz>\n");
	return GO_ON;
}
