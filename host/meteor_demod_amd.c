/*
 * meteor_demod_amd — C host for the MI355X LRPT demodulator.
 *
 * Same command line as the reference's CLI for the path this repository replaces
 * (main.c:19,35-51,82-152): -b -d -f -m -o -O -q -B -R -r -s -S/--bps --stdout -h -v,
 * same defaults (demod.h:8-15), k/M suffixes (utils.c:60-86), WAV header overriding
 * -s/--bps with raw fallback (main.c:164-166, wavfile.c:34-48), and the same file-level
 * behaviour: input consumed in whole 32768-byte reads (wavfile.c:6,55), 1024-byte
 * chunks written only once the PLL has locked (main.c:308-315), final flush of
 * 2*ring_idx bytes (main.c:321).
 *
 * All demodulation happens on the GPU through the C-ABI (include/meteor_demod_amd.h);
 * there is no CPU demodulator in this program.  Extensions: several input files are
 * demodulated as one batch, one stream per file (outputs <input>.s); --tiled demodulates
 * ONE file on many GPU lanes as overlapped tiles (mdemod_demodulate_recording_host: the head
 * up to PLL lock + settling is the reference's own serial run, the rest agrees with it
 * statistically, NOTEBOOK.md 3.1).  --devices a,b,... (default: every GPU of the node when there is more than one file) starts
 * one worker thread and one library context per GPU: file i goes to GPU i mod G, each worker demodulates its files as its own
 * batch (exact mode) or one after the other (--tiled) and writes its own outputs - no data crosses GPUs.
 *
 * Status line: the reference's "(%5.1f%%) Carrier: ... Symbol rate: ... Locked: ..." (main.c:249-261) from the status
 * snapshot of stream 0, at most once per -R milliseconds (default 2000 with -B, 50 without: main.c:144), "\n" separated
 * with -B and redrawn in place otherwise.  On a terminal, without -B / -q / --tiled, the full-screen display of the reference
 * (tui.c; main.c:197,224-245) is drawn instead: host/tui.c, built in when ncurses is there (as the reference's ENABLE_TUI).
 * Unlike the reference it is not started when stdin or stdout is not a terminal, unless --tui asks for it.
 * --offset <Hz> / --decimate <N> put the front end of include/meteor_demod_amd_frontend.h in front of the demodulator: the signal
 * is moved from <Hz> off the recording's centre to 0 Hz, filtered and decimated on the GPU, and demodulated at fs / N.  -s / --bps
 * (or the WAV header) describe the recording as always.  Its entries are weak references: this program still links against a
 * library without them (and says so when asked for the front end).
 * --offset auto surveys each input file first (include/meteor_demod_amd_survey.h: spectrum of the whole file, candidates
 * confirmed by their symbol-rate line) and uses the first confirmed signal's offset - each file of a batch its own; no confirmed
 * signal is exit 1 before any output file exists.  --decimate auto takes the largest N the front end accepts; --scan prints the
 * candidates and exits.  Weak references as well.
 * --cadu runs the frame layer (include/meteor_demod_amd_frames.h) over every output file once it is complete and closed: sync
 * search and Viterbi decoding on the GPU, the CADUs (1024 bytes each) into <output without .s>.cadu, one line about them on stdout.
 * Weak references again; refused with --stdout.
 * --vcdu goes on from there (include/meteor_demod_amd_rs.h): the CADUs derandomised and Reed-Solomon corrected on the GPU, the VCDUs
 * (892 bytes each, uncorrectable frames included) into <output without .s>.vcdu, one more line on stdout.  It implies the frame
 * pass; the .cadu is written only when --cadu is given too.  Weak references; refused with --stdout.
 * --diff and --skew choose the link variant of the frame pass (include/meteor_demod_amd_frames_link.h: NRZ-M coding, a one-symbol
 * skew between the rails): what Meteor-M N2-3 / N2-4 need with -m oqpsk.  Only with --cadu / --vcdu.  Weak references.
 * --int puts the 80 k interleaved mode (include/meteor_demod_amd_interleave.h) in front of the frame pass: the interleaver's sync
 * word found, followed and stripped and the 36 branches undone on the GPU (branch delay --int-delay, 2048 by default), one more
 * line on stdout.  Independent of --diff; --skew is accepted and ignored beside it, because the sync word resolves the skew.  Only
 * with --cadu / --vcdu.  Weak references.
 * --image goes on from the VCDUs (include/meteor_demod_amd_image.h): the packet zone demultiplexed and the MSU-MR image packets
 * decoded on the GPU, one <output without .s>_<apid>.pgm (binary P5, 1568 wide) per active channel that received a strip, one more
 * line on stdout.  It implies the --vcdu pass; the .vcdu and the .cadu are written only when asked for.  --apids a,b,c chooses the
 * active channels.  Weak references; refused with --stdout.
 * --rectify and --composite go on from the pictures (include/meteor_demod_amd_picture.h): every channel's picture resampled to equal
 * ground distance and contrast-stretched as <output without .s>_<apid>_rect.pgm, and three channels as one colour picture
 * <output without .s>_<abc>.ppm (binary P6) with one more line on stdout.  --altitude and --scan-angle set the geometry of
 * --rectify.  Only with --image.  Weak references.
 * --map puts the pictures on a latitude / longitude grid (include/meteor_demod_amd_map.h): the packets' onboard time stamps and a
 * two-line element set geolocate every line, and the GPU resamples the channels north-up.  With --composite one
 * <output without .s>_<abc>_map.ppm, without it one <output without .s>_<apid>_map.pgm per channel that received a strip; beside
 * each a world file of the same name ending in .wld, and one more line on stdout.  --norad, --map-scale, --date, --time-offset and
 * --scan-side set its options; --scan-angle applies, --altitude is not consulted (the orbit's radius comes from the element set).
 * Only with --image.  Weak references.
 * --mosaic <base> goes on from there (include/meteor_demod_amd_mosaic.h): the pictures of all input files (1 .. 8 passes of one
 * satellite) are kept after their own maps are written, and once every file is done they are blended onto one common grid on the
 * first GPU: <base>_<tag>_mosaic.ppm / .pgm, its world file and one more line.  --mosaic-blend feather|best.  Only with --map.
 * Weak references.
 * --overlay <file> (up to three times) and --graticule <deg|auto> go on from --map as well (include/meteor_demod_amd_overlay.h):
 * beside every map and mosaic a second picture, <...>_map_overlay.* / <...>_mosaic_overlay.*, with the polylines of the files (a
 * shapefile's .shp or text lines "lon lat") and the graticule drawn on it on the GPU, its own world file and one more line.  The
 * plain pictures stay as they are.  --overlay-colour <rrggbb>, --overlay-width <pixels>.  Weak references.
 * --map-proj stereo puts the pictures of --map (and of --mosaic, --overlay, --graticule) on a polar stereographic grid instead
 * (include/meteor_demod_amd_polar.h), for passes over a pole: <...>_polar.* with a world file and a .prj, <...>_polar_overlay.*;
 * --map-res <metres>, --map-lon0 <deg|auto>, --map-lat-ts <deg>.  Without it nothing changes.  Weak references.
 * --jpeg <quality> changes the format of every picture above (include/meteor_demod_amd_jpeg.h): a baseline JPEG encoded on the GPU,
 * <same name>.jpg instead of .pgm / .ppm, one line per file and one at the end.  Only with --image.  Weak references.
 * --equalise <clip> gives every derived picture (_rect, the composite, _map, _mosaic, _polar) local contrast on the GPU
 * (include/meteor_demod_amd_equalise.h: CLAHE under the picture's own mask) in place, after it is composed and before lines are drawn on
 * its copy or it is written; --equalise-tile <pixels>, --equalise-amount <percent>; one line per picture.  The channel pictures stay as
 * decoded.  Only with --image and --rectify, --composite or --map.  Weak references.
 * --sun takes the cosine of the sun's zenith angle out of the reflective channels (APIDs 64 .. 66) of the swath pictures on the GPU
 * (include/meteor_demod_amd_sun.h), after the channel pictures are written - they stay as decoded - and before any derived picture or
 * the mosaic is made of them; --sun-ref <deg>, --sun-limit <deg>; one line per file.  Only with --image and --map <tle file>: the orbit
 * comes from the element set.  Weak references.
 * Known deviation: if the final flush would read past the 1024-byte ring (ring_idx >
 * 512, where the reference reads out of bounds) only the bytes inside the ring are
 * written.
 */
#include <getopt.h>
#include <math.h>
#include <errno.h>
#include <stdint.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "meteor_demod_amd.h"
#include "meteor_demod_amd_frontend.h"
#include "meteor_demod_amd_survey.h"
#include "meteor_demod_amd_frames.h"
#include "meteor_demod_amd_frames_link.h"
#include "meteor_demod_amd_rs.h"
#include "meteor_demod_amd_interleave.h"
#include "meteor_demod_amd_image.h"
#include "meteor_demod_amd_picture.h"
#include "meteor_demod_amd_map.h"
#include "meteor_demod_amd_mosaic.h"
#include "meteor_demod_amd_polar.h"
#include "meteor_demod_amd_overlay.h"
#include "meteor_demod_amd_jpeg.h"
#include "meteor_demod_amd_equalise.h"
#include "meteor_demod_amd_sun.h"
#ifdef MDEMOD_TUI
#include "tui.h"
#endif

#define FILE_BUFFER_SIZE 32768          /* wavfile.c:6 */
#define RINGSIZE 512                    /* main.c:20   */
#define BLOCK_BUFFERS 128               /* 4 MiB of input per stream per GPU call (files) */
#define PIPE_BUFFERS  8                 /* 256 KiB when reading a pipe: ~0.3 s of a live 230 kS/s s16 stream */
#define MAX_JOBS 16                     /* --tiled: files of one GPU in flight at once, at most */

struct stream_io {
	const char *in_name;
	char       *out_name;
	FILE       *in, *out;
	int8_t      ring[2 * RINGSIZE];      /* main.c:34 (static => zero initialised) */
	unsigned    ring_idx;
	uint64_t    symbols;                 /* symbols emitted so far */
	unsigned long bytes_out;
	unsigned long file_len;              /* 0 = unknown (pipe): main.c:192 */
	int         eof;
};

static const struct option longopts[] = {
	{ "batch", 0, NULL, 'B' },      { "pll-bw", 1, NULL, 'b' },   { "freq-delta", 1, NULL, 'd' },
	{ "fir-order", 1, NULL, 'f' },  { "help", 0, NULL, 'h' },     { "mode", 1, NULL, 'm' },
	{ "output", 1, NULL, 'o' },     { "oversamp", 1, NULL, 'O' }, { "quiet", 0, NULL, 'q' },
	{ "refresh-rate", 1, NULL, 'R' }, { "symrate", 1, NULL, 'r' }, { "stdout", 0, NULL, 0x00 },
	{ "samplerate", 1, NULL, 's' }, { "bps", 1, NULL, 'S' },      { "version", 0, NULL, 'v' },
	{ "device", 1, NULL, 0x01 },    { "tiled", 0, NULL, 0x02 },   { "tile-samples", 1, NULL, 0x03 },
	{ "pilot-margin", 1, NULL, 0x04 }, { "carrier-seed", 1, NULL, 0x05 }, { "devices", 1, NULL, 0x06 }, { "plan", 0, NULL, 0x07 },
	{ "tui-selftest", 0, NULL, 0x08 }, { "tui", 0, NULL, 0x09 }, { "jobs", 1, NULL, 0x0a },
	{ "offset", 1, NULL, 0x0b },    { "decimate", 1, NULL, 0x0c }, { "scan", 0, NULL, 0x0d },
	{ "cadu", 0, NULL, 0x0e },      { "vcdu", 0, NULL, 0x0f },    { "diff", 0, NULL, 0x10 },    { "skew", 0, NULL, 0x11 },
	{ "int", 0, NULL, 0x12 },       { "int-delay", 1, NULL, 0x13 }, { "image", 0, NULL, 0x14 },   { "apids", 1, NULL, 0x15 },
	{ "rectify", 0, NULL, 0x16 },   { "composite", 1, NULL, 0x17 }, { "altitude", 1, NULL, 0x18 }, { "scan-angle", 1, NULL, 0x19 },
	{ "map", 1, NULL, 0x1a },       { "norad", 1, NULL, 0x1b },   { "map-scale", 1, NULL, 0x1c }, { "date", 1, NULL, 0x1d },
	{ "time-offset", 1, NULL, 0x1e }, { "scan-side", 1, NULL, 0x1f }, { "mosaic", 1, NULL, 0x20 },   { "mosaic-blend", 1, NULL, 0x21 },
	{ "overlay", 1, NULL, 0x22 },   { "graticule", 1, NULL, 0x23 }, { "overlay-colour", 1, NULL, 0x24 }, { "overlay-width", 1, NULL, 0x25 },
	{ "jpeg", 1, NULL, 0x26 },      { "map-proj", 1, NULL, 0x27 },  { "map-res", 1, NULL, 0x28 },   { "map-lon0", 1, NULL, 0x29 },
	{ "map-lat-ts", 1, NULL, 0x2a }, { "equalise", 1, NULL, 0x2b }, { "equalise-tile", 1, NULL, 0x2c }, { "equalise-amount", 1, NULL, 0x2d },
	{ "sun", 0, NULL, 0x2e },       { "sun-ref", 1, NULL, 0x2f },   { "sun-limit", 1, NULL, 0x30 },
	{ NULL, 0, NULL, 0 }
};

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

/* what --overlay / --graticule ask of every map and mosaic */
#define OVERLAY_FILES 3
struct overlay_req {
	mdemod_overlay_vectors coast[OVERLAY_FILES];   /* the files of --overlay, read before anything is demodulated */
	uint32_t n_files;
	int      graticule;                  /* --graticule given */
	double   step;                       /* 0: auto */
	mdemod_overlay_style style[2];       /* 0: the files' lines, 1: the graticule */
};

/* what --vcdu / --image ask of the transfer frames of one file */
struct vcdu_req {
	int      write_vcdu;                 /* the .vcdu and its line */
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
	        "                           than 1568) and contrast-stretched between the 0.5 % and 99.5 % points of its pixels\n"
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

/* wavfile.c:16-48: canonical 44-byte header, two channels */
static int
parse_wav(FILE *f, int *samplerate, int *bps)
{
	unsigned char h[44];
	if (fread(h, sizeof(h), 1, f) != 1) return 1;
	if (memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) return 1;
	const unsigned channels = h[22] | (h[23] << 8);
	const unsigned bits = h[34] | (h[35] << 8);
	if (channels != 2) return 1;
	*bps = (int)bits;                    /* wavfile.c:44: assigned before the zero test, so a 0 here overrides --bps */
	if (!bits) return 1;
	*samplerate = (int)(h[24] | (h[25] << 8) | (h[26] << 16) | ((unsigned)h[27] << 24));
	return 0;
}

/* main.c:305-315: ring of 512 symbols, a chunk is written when it completes iff the PLL has
 * locked at least once by then, i.e. first_lock <= index of the chunk's last symbol. */
static void
write_gated(struct stream_io *io, const int8_t *soft, uint32_t n, int64_t first_lock)
{
	for (uint32_t k = 0; k < n; k++) {
		/* whole chunks with the gate open (it never closes again): straight from the caller's buffer */
		if (io->ring_idx == 0 && n - k >= RINGSIZE && first_lock >= 0 && (uint64_t)first_lock <= io->symbols + RINGSIZE - 1) {
			const uint32_t chunks = (n - k) / RINGSIZE;
			fwrite(soft + 2 * (size_t)k, 2 * RINGSIZE, chunks, io->out);
			io->symbols += (uint64_t)chunks * RINGSIZE;
			io->bytes_out += 2ull * RINGSIZE * chunks;
			k += chunks * RINGSIZE;
			memcpy(io->ring, soft + 2 * (size_t)(k - RINGSIZE), 2 * RINGSIZE);     /* the ring holds the last chunk: the final flush writes stale bytes of it (main.c:321) */
			if (k >= n) break;
		}
		io->ring[io->ring_idx++] = soft[2 * k];
		io->ring[io->ring_idx++] = soft[2 * k + 1];
		io->symbols++;
		if (io->ring_idx >= 2 * RINGSIZE) {
			io->ring_idx = 0;
			if (first_lock >= 0 && (uint64_t)first_lock <= io->symbols - 1) {
				fwrite(io->ring, RINGSIZE, 2, io->out);
				io->bytes_out += 2 * RINGSIZE;
			}
		}
	}
}

/* The reference never looks at what fwrite / fclose return (main.c:314,321,274): a full disk ends in a short file and exit status 0.
 * The status stays the reference's; the loss is said, once per file, on stderr. */
static void
close_output(struct stream_io *o)
{
	if (!o->out) return;
	int failed = ferror(o->out);
	errno = 0;
	if (o->out == stdout) failed |= fflush(stdout) != 0;
	else failed |= fclose(o->out) != 0;
	const int why = errno;                                       /* (of the flush / close; an earlier fwrite's is long overwritten) */
	if (failed) fprintf(stderr, "%s: writing the soft symbols failed (%s): the output is incomplete\n", o->out_name ? o->out_name : "(stdout)",
	                    why ? strerror(why) : "a write was refused");
	o->out = NULL;
}

/* error exits: whatever was written so far is flushed and closed */
static void
close_all(struct stream_io *io, int n)
{
	for (int i = 0; i < n; i++) {
		close_output(&io[i]);
		if (io[i].in && io[i].in != stdin) fclose(io[i].in);
		io[i].in = NULL;
	}
}

static void *
init_device_thread(void *arg)        /* the HIP runtime comes up (0.1-0.2 s) while --tiled reads its file */
{
	(void)mdemod_init_device(*(int *)arg);
	return NULL;
}

static double
now_ms(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}


/* main.c:150: messages go to stdout, or into the display's log pane while that is up */
static int (*say)(const char *, ...) = printf;

#ifdef MDEMOD_TUI
/* --tui-selftest: the display's formatting helpers as text, and - on a terminal - one frame of made-up values (no GPU call) */
static int
tui_selftest(int force)
{
	int8_t sym[2 * RINGSIZE];
	unsigned lcg = 12345;
	for (int k = 0; k < RINGSIZE; k++) {
		lcg = lcg * 1664525u + 1013904223u;
		sym[2 * k] = (int8_t)(((lcg >> 8) & 1 ? 90 : -90) + (int)((lcg >> 16) % 21) - 10);
		sym[2 * k + 1] = (int8_t)(((lcg >> 9) & 1 ? 90 : -90) + (int)((lcg >> 24) % 21) - 10);
	}
	if ((force || (isatty(STDIN_FILENO) && isatty(STDOUT_FILENO))) && tui_open(50) == 0) {
		const struct tui_frame f = { 1234.5, 72000.1, 0.031, 1, 60ul << 20, 110ul << 20, 920000, 23456789ul, sym, RINGSIZE };
		tui_log("Input: %s, output: %s\n", "selftest.wav", "selftest.s");
		tui_log("Demodulator initialized\n");
		tui_draw(&f);
		tui_log("Demodulation complete\n");
		tui_log("Press any key to exit...\n");
		tui_wait_key();
		tui_close();
	}
	const unsigned long sizes[] = { 0, 999, 1000, 1001, 12345, 123456, 23456789ul, 4000000000ul };
	for (unsigned i = 0; i < sizeof(sizes) / sizeof(sizes[0]); i++) { char b[16]; tui_fmt_size(sizes[i], b); printf("size %lu -> [%sB]\n", sizes[i], b); }
	const unsigned long secs[] = { 0, 59, 3725, 356400, 360000 };
	for (unsigned i = 0; i < sizeof(secs) / sizeof(secs[0]); i++) { char b[16]; tui_fmt_clock(secs[i], b); printf("clock %lu -> %s\n", secs[i], b); }
	unsigned char hits[9 * 19];
	tui_constellation(sym, RINGSIZE, 9, 19, hits);
	for (int r = 0; r < 9; r++) { printf("plot |"); for (int c = 0; c < 19; c++) putchar(tui_glyph(hits[r * 19 + c])); printf("|\n"); }
	return 0;
}
#endif

/* What one worker (= one GPU) needs: its files and a copy of the options. */
struct worker {
	pthread_t   thr;
	int         index;                   /* worker 0 prints the status line (stream 0 of ITS batch, as the reference prints its one stream) */
	int         n_files;
	struct stream_io *io;                /* this worker's files (a contiguous copy; the originals are not touched again) */
	mdemod_params p;                     /* p.device, p.n_streams are this worker's */
	int         tiled, quiet, batch, update_interval, tile_samples, pilot_margin, carrier_seed;
	int         tui;                     /* worker 0 only: the full-screen display is up */
	int         jobs;                    /* --tiled: files of this worker in flight at once */
	int         use_fe;                  /* --offset / --decimate: the front end ahead of the demodulator */
	mdemod_fe_params fe;
	double     *fe_offsets;              /* --offset auto: one offset per file of this worker (NULL: fe.offset_hz for all) */
	int         rc;                      /* exit code of this worker: 0 ok, 1 host error, 2 library error */
};

/* the code in words plus what the library has to add (mdemod_last_error: it prints nothing itself), taken at once - the text belongs
 * to the failing call and the next call into the library may replace it */
static const char *
why_of(int rc)
{
	static __thread char buf[640];
	const char *more = mdemod_last_error();
	if (more && *more) snprintf(buf, sizeof buf, "%s: %s", mdemod_strerror(rc), more);
	else snprintf(buf, sizeof buf, "%s", mdemod_strerror(rc));
	return buf;
}

/* ---- --tiled: each file on many lanes: read it whole (32768-byte buffers only, wavfile.c:55), one library call per file.  The
 * serial head of a recording keeps one wavefront busy for ~0.1 s and its file takes as long to read: up to `jobs` files of a worker
 * are in flight at once, each on a host thread of its own (the library calls are independent: own contexts, own streams).
 * Measured on page-cached files (tools/cli_jobs_time.py, 8 x 2^25 samples, 0.45 s of it process and runtime start): 1.66 s with one
 * job, 1.25 with two, 1.13 with four (the default), 1.15 with eight - the heads and the file reads overlap, the tile phases (each
 * fills the GPU) do not. ---- */
struct tiled_pool {
	struct worker  *w;
	pthread_mutex_t lock;
	int             next;                /* next file of the worker nobody has taken */
	int             rc;                  /* worst exit code so far */
};

static int
tiled_one_file(struct worker *w, int f)
{
	struct stream_io *io = w->io;
	const int quiet = w->quiet, bps = w->p.bps, samplerate = w->p.samplerate;
	const float symrate = (float)w->p.symrate;
	const int tile_samples = w->tile_samples, pilot_margin = w->pilot_margin, carrier_seed = w->carrier_seed;
	mdemod_params p = w->p;
	mdemod_fe_params fe_one = w->fe;
	if (w->fe_offsets) { fe_one.offset_hz = w->fe_offsets[f]; fe_one.offsets_hz = NULL; }
	const int timing = getenv("MDEMOD_CLI_TIMING") != NULL;       /* where the wall time of a --tiled run goes (stderr) */
	const double t_begin = now_ms();
	size_t cap_bytes = 1u << 26, len = 0;
	if (io[f].file_len + 2 * FILE_BUFFER_SIZE > cap_bytes) cap_bytes = io[f].file_len + 2 * FILE_BUFFER_SIZE;   /* a regular file: one allocation, no copies */
	unsigned char *data = malloc(cap_bytes);
	for (;;) {
		if (len + FILE_BUFFER_SIZE > cap_bytes) {
			unsigned char *grown = realloc(data, cap_bytes * 2);
			if (!grown) { free(data); data = NULL; break; }
			data = grown; cap_bytes *= 2;
		}
		if (!data) break;
		if (fread(data + len, FILE_BUFFER_SIZE, 1, io[f].in) != 1) break;
		len += FILE_BUFFER_SIZE;
	}
	if (!data) { fprintf(stderr, "out of memory reading %s\n", io[f].in_name); return 1; }
	const uint64_t n_samples = len / (2 * (size_t)bps / 8);
	/* (rates the library will refuse anyway must not size an allocation: a WAV header may say 0 Hz) */
	const double nominal = samplerate > 0 && symrate > 0 ? (double)n_samples * symrate / samplerate * 1.02 : -1.0;
	if (!(nominal >= 0.0 && nominal < 1e15)) {
		fprintf(stderr, "mdemod_demodulate_recording_host: %s\n", mdemod_strerror(MDEMOD_ERR_PARAM));
		free(data);
		return 2;
	}
	const uint64_t cap_sym = (uint64_t)nominal + 4096;
	int8_t *soft_all = malloc(cap_sym * 2);
	if (!soft_all) { free(data); return 1; }
	mdemod_recording_opts ro;
	mdemod_recording_default_opts(&ro);
	if (getenv("MDEMOD_RECORDING_DEBUG")) ro.debug = atoi(getenv("MDEMOD_RECORDING_DEBUG")) > 0 ? atoi(getenv("MDEMOD_RECORDING_DEBUG")) : 1;     /* the library reads no environment: the CLI does */
	if (tile_samples > 0) ro.tile_samples = (uint32_t)tile_samples;
	if (pilot_margin >= 0) ro.pilot_margin_symbols = (uint32_t)pilot_margin;
	if (carrier_seed >= 0) ro.carrier_seed = (uint32_t)carrier_seed;
	mdemod_recording_report rr;
	const double t_read = now_ms();
	int rc2 = w->use_fe ? mdemod_fe_demodulate_recording_host(&p, &fe_one, &ro, data, n_samples, soft_all, cap_sym, &rr)
	                    : mdemod_demodulate_recording_host(&p, &ro, data, n_samples, soft_all, cap_sym, &rr);
	const double t_lib = now_ms();
	if (rc2 != MDEMOD_OK) {
		fprintf(stderr, "%s: %s\n", w->use_fe ? "mdemod_fe_demodulate_recording_host" : "mdemod_demodulate_recording_host", why_of(rc2));
		free(data); free(soft_all);
		return 2;
	}
	if (rr.pilot_locked == 2)
		fprintf(stderr, "%s: note: the reference's PLL reports lock far from this signal's carrier (a false lock, common with "
		        "-m oqpsk): the exact mode would write what it produces from there on; --tiled demodulates the signal\n", io[f].in_name);
	if (!quiet)
		fprintf(stderr, "%s: %llu samples: %llu serial (pilot) + %u tiles, %llu symbols, first lock at symbol %lld, %u seam fixes, "
		        "%u weak seams, %u rotation jumps, %u tiles without a carrier line, %.2f s\n", io[f].in_name, (unsigned long long)n_samples,
		        (unsigned long long)rr.pilot_samples, rr.n_tiles, (unsigned long long)rr.n_symbols, (long long)rr.first_lock_symbol,
		        rr.seam_fixes, rr.weak_seams, rr.rotation_jumps, rr.weak_carrier_tiles, rr.pilot_seconds + rr.tiles_seconds);
	for (uint64_t k = 0; k < rr.n_symbols; k += 1u << 20)
		write_gated(&io[f], soft_all + 2 * k, (uint32_t)((rr.n_symbols - k < (1u << 20)) ? rr.n_symbols - k : (1u << 20)), rr.first_lock_symbol);
	size_t tail = 2 * (size_t)io[f].ring_idx;                       /* main.c:321 */
	if (tail > sizeof(io[f].ring)) tail = sizeof(io[f].ring);
	fwrite(io[f].ring, 1, tail, io[f].out);
	close_output(&io[f]);
	if (io[f].in != stdin) fclose(io[f].in);
	io[f].in = NULL;
	free(data); free(soft_all);
	if (timing)
		fprintf(stderr, "%s: read %.0f ms, library call %.0f ms (pilot %.0f + tiles %.0f on the device), write %.0f ms\n", io[f].in_name,
		        t_read - t_begin, t_lib - t_read, rr.pilot_seconds * 1e3, rr.tiles_seconds * 1e3, now_ms() - t_lib);
	return 0;
}

static void *
tiled_job(void *arg)
{
	struct tiled_pool *pool = arg;
	for (;;) {
		pthread_mutex_lock(&pool->lock);
		const int f = pool->next < pool->w->n_files && pool->rc == 0 ? pool->next++ : -1;
		pthread_mutex_unlock(&pool->lock);
		if (f < 0) return NULL;
		const int rc = tiled_one_file(pool->w, f);
		if (rc) {
			pthread_mutex_lock(&pool->lock);
			if (rc > pool->rc) pool->rc = rc;
			pthread_mutex_unlock(&pool->lock);
		}
	}
}

static int
run_tiled(struct worker *w)
{
	int device = w->p.device;
	/* the HIP runtime comes up (0.1-0.2 s) on a thread of its own while the first file is read */
	pthread_t init_thr;
	const int init_started = pthread_create(&init_thr, NULL, init_device_thread, &device) == 0;
	struct tiled_pool pool = { w, PTHREAD_MUTEX_INITIALIZER, 0, 0 };
	int jobs = w->jobs < 1 ? 1 : w->jobs;
	if (jobs > w->n_files) jobs = w->n_files;
	if (jobs > MAX_JOBS) jobs = MAX_JOBS;
	for (int i = 0; i < w->n_files; i++) if (w->io[i].in == stdin || w->io[i].out == stdout) jobs = 1;
	if (jobs == 1) {
		tiled_job(&pool);
		if (init_started) pthread_join(init_thr, NULL);
	} else {
		pthread_t thr[MAX_JOBS];
		int started = 0;
		for (; started < jobs; started++) if (pthread_create(&thr[started], NULL, tiled_job, &pool)) break;
		if (!started) tiled_job(&pool);
		for (int i = 0; i < started; i++) pthread_join(thr[i], NULL);
		if (init_started) pthread_join(init_thr, NULL);
	}
	if (pool.rc) close_all(w->io, w->n_files);
	return pool.rc;
}

/* an error path of run_exact: the full-screen display comes down first (the reference's main.c:241-244 tears it down on every exit),
 * so that the message lands on a sane terminal */
static int
exact_failed(struct worker *w, int code, const char *what, const char *why)
{
#ifdef MDEMOD_TUI
	if (w->tui) { tui_close(); say = printf; }
#endif
	fprintf(stderr, "%s: %s\n", what, why);
	close_all(w->io, w->n_files);
	return code;
}

/* ---- exact mode: this worker's files as ONE batch, one stream per file, block by block (main.c:303-316) ---- */
static int
run_exact(struct worker *w)
{
	struct stream_io *io = w->io;
	const int n_files = w->n_files, quiet = w->quiet || w->index != 0, batch = w->batch, update_interval = w->update_interval;
	const int bps = w->p.bps, samplerate = w->p.samplerate, interp = w->p.interp_factor, oqpsk = w->p.oqpsk;
	const float symrate = (float)w->p.symrate;
	mdemod_params p = w->p;
	mdemod_ctx *ctx = NULL;
	mdemod_fe *fe = NULL;
	const int D = w->use_fe ? w->fe.decimation : 1;
	int rc = w->use_fe ? mdemod_fe_create(&p, &w->fe, &fe) : mdemod_create(&p, &ctx);
	if (rc != MDEMOD_OK) return exact_failed(w, 2, w->use_fe ? "mdemod_fe_create" : "mdemod_create", why_of(rc));
	if (fe) ctx = mdemod_fe_demodulator(fe);
	/* (the context goes with its front end when there is one) */
#define DESTROY_CTX() do { if (fe) mdemod_fe_destroy(fe); else mdemod_destroy(ctx); } while (0)
	if (!quiet) say("Demodulator initialized\n");                                    /* main.c:219 */
	if (!quiet && !w->tui && n_files < 64 && io[0].file_len > (64ul << 20))
		fprintf(stderr, "note: %d file%s demodulated exactly = %d serial stream%s, one GPU wavefront each (about 3.6 MS/s: slower than the "
		        "reference on one host core); --tiled puts a long recording on many lanes (50x faster, same symbols, soft values within "
		        "+-1 LSB of these on 99.6-99.9 %%), and a batch of many files fills the GPU in exact mode\n",
		        n_files, n_files == 1 ? "" : "s", n_files, n_files == 1 ? "" : "s");

	size_t block_buffers = BLOCK_BUFFERS;
	for (int i = 0; i < n_files; i++) if (io[i].in == stdin) block_buffers = PIPE_BUFFERS;     /* live input: short blocks */
	const size_t block_bytes = block_buffers * FILE_BUFFER_SIZE;
	const uint32_t block_samples = (uint32_t)(block_bytes / (2 * (size_t)bps / 8));
	const uint32_t cap = (uint32_t)mdemod_max_symbols(ctx, (block_samples + (uint32_t)D - 1) / (uint32_t)D);
	unsigned char *in_buf = malloc(block_bytes * (size_t)n_files);
	int8_t *soft = malloc((size_t)cap * 2 * (size_t)n_files);
	const void **iq = malloc(sizeof(*iq) * (size_t)n_files);
	int8_t **outp = malloc(sizeof(*outp) * (size_t)n_files);
	uint32_t *n_in = malloc(sizeof(uint32_t) * (size_t)n_files), *caps = malloc(sizeof(uint32_t) * (size_t)n_files);
	uint32_t *n_out = malloc(sizeof(uint32_t) * (size_t)n_files);
	mdemod_status *st = malloc(sizeof(*st) * (size_t)n_files);
#define FREE_BLOCKS() do { free(in_buf); free(soft); free(iq); free(outp); free(n_in); free(caps); free(n_out); free(st); } while (0)
	if (!in_buf || !soft || !iq || !outp || !n_in || !caps || !n_out || !st) { DESTROY_CTX(); FREE_BLOCKS(); return exact_failed(w, 1, "meteor_demod_amd", "out of memory"); }

	/* the read buffer is the same for every block: pinned once, the batch then goes to the GPU from where fread put it
	   (a batch of files; one file is a few MiB per call either way.  A refusal - no memory to pin - only means the library stages the
	   blocks itself.  The context is destroyed, which unpins, BEFORE the buffer is freed on every way out.) */
	if (!fe && n_files >= 2 && block_buffers == BLOCK_BUFFERS) (void)mdemod_pin_host_buffer(ctx, in_buf, block_bytes * (size_t)n_files);

	double last_status = -1e18;
#ifdef MDEMOD_TUI
	int8_t shown[2 * RINGSIZE];                 /* the latest symbols of stream 0 for the constellation (main.c:238 shows its ring) */
	unsigned n_shown = 0;
#endif
	for (;;) {
		int active = 0;
		for (int i = 0; i < n_files; i++) {
			iq[i] = in_buf + block_bytes * (size_t)i;
			outp[i] = soft + (size_t)cap * 2 * (size_t)i;
			caps[i] = cap;
			n_in[i] = 0;
			if (io[i].eof) continue;
			/* whole 32768-byte buffers only: a short trailing read ends the stream (wavfile.c:55) */
			const size_t got = fread(in_buf + block_bytes * (size_t)i, FILE_BUFFER_SIZE, block_buffers, io[i].in);
			if (got < block_buffers) io[i].eof = 1;
			n_in[i] = (uint32_t)(got * FILE_BUFFER_SIZE / (2 * (size_t)bps / 8));
			if (got) active = 1;
		}
		if (!active) break;
		rc = fe ? mdemod_fe_process_host(fe, iq, n_in, outp, caps, n_out)
		        : mdemod_process_host(ctx, iq, n_in, outp, caps, n_out);          /* demod(&sample) x n: main.c:304 */
		if (rc != MDEMOD_OK) { const char *why = why_of(rc); DESTROY_CTX(); FREE_BLOCKS(); return exact_failed(w, 2, fe ? "mdemod_fe_process_host" : "mdemod_process_host", why); }
		rc = mdemod_get_status(ctx, 0, (uint32_t)n_files, st, NULL);
		if (rc != MDEMOD_OK) { const char *why = why_of(rc); DESTROY_CTX(); FREE_BLOCKS(); return exact_failed(w, 2, "mdemod_get_status", why); }
		for (int i = 0; i < n_files; i++)
			write_gated(&io[i], outp[i], n_out[i], st[i].first_lock_symbol);
#ifdef MDEMOD_TUI
		if (w->tui && n_out[0]) {
			n_shown = n_out[0] < RINGSIZE ? n_out[0] : RINGSIZE;
			memcpy(shown, outp[0] + 2 * (size_t)(n_out[0] - n_shown), 2 * (size_t)n_shown);
		}
#endif
		if (!quiet && now_ms() - last_status >= update_interval) {
			/* main.c:249-261: status line from the snapshot of stream 0, at most once per refresh period */
			last_status = now_ms();
			/* with the front end: the carrier from the recording's centre (offset + the PLL's estimate), the clock at fs / D */
			const double freq_hz = st[0].pll_freq * symrate / (2 * M_PI) * (oqpsk ? 2 : 1) + (fe ? (w->fe_offsets ? w->fe_offsets[0] : w->fe.offset_hz) : 0.0);
			const double rate_hz = st[0].omega * ((double)(samplerate / D) * interp) / (2 * M_PI);
			const long pos = io[0].in != stdin ? ftell(io[0].in) : 0;
#ifdef MDEMOD_TUI
			if (w->tui) {
				/* main.c:224-239: the display instead of the line; q ends the run after this block (the reference's `done = 1`) */
				const struct tui_frame f = { freq_hz, rate_hz, st[0].gain, st[0].locked, pos > 0 ? (unsigned long)pos : 0, io[0].file_len,
				                             (unsigned)(2 * (size_t)samplerate * (size_t)bps / 8), io[0].bytes_out, shown, n_shown };
				if (tui_draw(&f)) for (int i = 0; i < n_files; i++) io[i].eof = 1;
				continue;
			}
#endif
			printf(batch ? "\n" : "\033[1K\r");
			printf("(%5.1f%%) Carrier: %+7.1f Hz, Symbol rate: %.1f Hz, Locked: %s",
			       io[0].file_len && pos > 0 ? 100.0 * (double)pos / (double)io[0].file_len : 0.0, freq_hz, rate_hz, st[0].locked ? "Yes" : "No");
			fflush(stdout);
		}
	}
	if (!quiet && !w->tui) printf("\n");

	for (int i = 0; i < n_files; i++) {
		/* main.c:321: fwrite(ring, ring_idx, 2, f) */
		size_t tail = 2 * (size_t)io[i].ring_idx;
		if (tail > sizeof(io[i].ring)) tail = sizeof(io[i].ring);
		fwrite(io[i].ring, 1, tail, io[i].out);
		io[i].bytes_out += io[i].ring_idx;
		close_output(&io[i]);
		if (io[i].in != stdin) fclose(io[i].in);
		io[i].in = NULL;
	}
	DESTROY_CTX();                                                                /* demod_deinit: main.c:273 */
	FREE_BLOCKS();
#undef FREE_BLOCKS
#undef DESTROY_CTX
#ifdef MDEMOD_TUI
	if (w->tui) {                                                                 /* main.c:241-244 */
		say("Demodulation complete\n");
		say("Press any key to exit...\n");
		tui_wait_key();
		tui_close();
		say = printf;
	}
#endif
	return 0;
}

static void *
worker_main(void *arg)
{
	struct worker *w = arg;
	w->rc = w->tiled ? run_tiled(w) : run_exact(w);
	return NULL;
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

#define MAX_DEVICES 64

/* the offset as --scan prints it (0.1 Hz): --offset auto uses the same number, so --offset <what --scan printed> is the same run */
static double
round_offset(double hz)
{
	char buf[64];
	snprintf(buf, sizeof buf, "%.1f", hz);
	return strtod(buf, NULL);
}

/* The survey of one input file: its samples from where the header ended to the end of the file, read whole, and the file put back
 * where it was.  0, 1 (a host error, already reported) or the library's code (< 0). */
static int
survey_file(const mdemod_params *in, const mdemod_survey_opts *so, struct stream_io *io, mdemod_survey_hit *hits, uint32_t *n_hits)
{
	const long here = ftell(io->in);
	if (here < 0 || fseek(io->in, 0, SEEK_END)) { fprintf(stderr, "%s: cannot look ahead in this input (not a regular file)\n", io->in_name); return 1; }
	const long end = ftell(io->in);
	if (end < here || fseek(io->in, here, SEEK_SET)) { fprintf(stderr, "%s: cannot look ahead in this input\n", io->in_name); return 1; }
	const size_t len = (size_t)(end - here), sb = 2 * (size_t)in->bps / 8;
	unsigned char *data = malloc(len ? len : 1);
	if (!data) { fprintf(stderr, "out of memory reading %s\n", io->in_name); return 1; }
	const size_t got = fread(data, 1, len, io->in);
	int rc = 1;
	if (fseek(io->in, here, SEEK_SET)) fprintf(stderr, "%s: cannot look ahead in this input\n", io->in_name);
	else rc = mdemod_survey_host(in, so, data, got / sb, hits, MDEMOD_SURVEY_MAX_CANDIDATES, n_hits);
	free(data);
	if (*n_hits > MDEMOD_SURVEY_MAX_CANDIDATES) *n_hits = MDEMOD_SURVEY_MAX_CANDIDATES;
	return rc;
}

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

/* --jpeg: the quality (0: not given) and what went through the encoder.  The pictures are written by one thread, after the workers
 * have joined. */
static struct { unsigned quality; unsigned long long files, bytes_in, bytes_out; } jpeg_req;

/* --equalise: the clip in percent (0: not given), the tile and the amount (0 .. 256) */
static struct { unsigned clip_percent, tile, amount; int tile_given, amount_given; } equalise_req = { 0, 128, 256, 0, 0 };

/* --equalise: a derived picture in place under its own mask (valid_step lines of the picture per line of the mask), before lines are
 * drawn on a copy of it and before it is written, and its line on stdout.  Nothing without the option.  0, or the exit status. */
static int
equalise_picture(const char *name, uint8_t *pixels, const uint8_t *valid, uint32_t width, uint32_t height, uint32_t planes, uint32_t valid_step, int device)
{
	if (!equalise_req.clip_percent || !height || !width) return 0;
	mdemod_equalise_opts eo;
	mdemod_equalise_summary es;
	mdemod_equalise_default_opts(&eo);
	eo.tile = equalise_req.tile; eo.clip_percent = equalise_req.clip_percent; eo.amount = equalise_req.amount; eo.valid_step = valid_step;
	const int rc = mdemod_equalise_host(&eo, pixels, valid, width, height, planes, &es, device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--equalise: %s: %s\n", name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	printf("%s: equalised: tile %u, clip %g, %u x %u tiles, %u empty\n", name, eo.tile, eo.clip_percent / 100.0, es.nx, es.ny, es.empty_tiles);
	return 0;
}

/* One picture of the program, pixels[height][width][planes], into `name`, which ends in ".pgm" or ".ppm": as that binary P5 / P6
 * file, or with --jpeg encoded on the GPU into the same name ending in ".jpg" (`name` is changed), with one line on stdout that names
 * the file.  `what` is the option the messages begin with.  0, or the exit status. */
static int
write_picture(const char *what, char *name, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t planes, int device)
{
	const size_t bytes = (size_t)height * width * planes;
	uint8_t *file = NULL;
	uint64_t file_bytes = 0;
	if (jpeg_req.quality) {
		const int rc = mdemod_jpeg_encode_host(pixels, width, height, planes, jpeg_req.quality, 0, &file, &file_bytes, device);
		if (rc != MDEMOD_OK) { fprintf(stderr, "--jpeg: %s: %s\n", name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
		memcpy(name + strlen(name) - 3, "jpg", 3);
	}
	FILE *o = fopen(name, "wb");
	if (!o) { fprintf(stderr, "%s: could not open %s\n", what, name); if (file) mdemod_jpeg_free(file); return 1; }
	int short_write;
	if (jpeg_req.quality) short_write = fwrite(file, 1, file_bytes, o) != file_bytes;
	else short_write = fprintf(o, "P%d\n%u %u\n255\n", planes == 3 ? 6 : 5, width, height) < 0 || (bytes && fwrite(pixels, 1, bytes, o) != bytes);
	if (jpeg_req.quality) mdemod_jpeg_free(file);
	if ((fclose(o) != 0) | short_write) { fprintf(stderr, "%s: writing %s failed: the picture is incomplete\n", what, name); return 1; }
	if (jpeg_req.quality) {
		printf("%s: JPEG quality %u: %u x %u x %u, %llu bytes of %llu\n", name, jpeg_req.quality, width, height, planes, (unsigned long long)file_bytes,
		       (unsigned long long)bytes);
		jpeg_req.files++; jpeg_req.bytes_in += bytes; jpeg_req.bytes_out += file_bytes;
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
picture_files(const char *s_name, const mdemod_image_result *res, const struct vcdu_req *req, int device)
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
		const int rc = mdemod_picture_compose_host(&po, image, filled, rows, select, 1, &pic, device);
		if (rc != MDEMOD_OK) { fprintf(stderr, "--rectify: %s: %s\n", s_name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
		char ext[32];
		snprintf(ext, sizeof ext, "_%u_rect.pgm", (unsigned)req->apids[k]);
		char *name = beside(s_name, ext);
		if (!name) { fprintf(stderr, "--rectify: could not open the picture\n"); code = 1; }
		else if (!(code = equalise_picture(name, pic.pixels, pic.valid, pic.width, pic.lines, 1, 8, device)))
			code = write_picture("--rectify", name, pic.pixels, pic.width, pic.lines, 1, device);
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
	const int rc = mdemod_picture_compose_host(&po, image, filled, rows, select, 3, &pic, device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--composite: %s: %s\n", s_name, why_of(rc)); free(base); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	char ext[32];
	snprintf(ext, sizeof ext, "_%s.ppm", tag);
	char *name = beside(s_name, ext);
	if (!name) { fprintf(stderr, "--composite: could not open the picture\n"); code = 1; }
	else if (!(code = equalise_picture(name, pic.pixels, pic.valid, pic.width, pic.lines, 3, 8, device)))
		code = write_picture("--composite", name, pic.pixels, pic.width, pic.lines, 3, device);
	if (!code)
		printf("%s: composite %s: %u x %u%s; stretch R %u .. %u, G %u .. %u, B %u .. %u; %.1f %% of pixels valid\n", base ? base : s_name,
		       tag, pic.width, pic.lines, req->rectify ? " rectified" : "",
		       pic.lo[0], pic.hi[0], pic.lo[1], pic.hi[1], pic.lo[2], pic.hi[2],
		       rows ? 100.0 * (double)pic.valid_cells / ((double)rows * pic.width) : 0.0);
	free(name); free(base);
	mdemod_picture_free(&pic);
	return code;
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
overlay_tail(const char *stem, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t planes, int device, int (*draw)(void *lines, uint8_t *copy), void *lines,
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
		code = write_picture("--overlay", name, copy, width, height, planes, device);
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
overlay_file(const char *stem, const struct overlay_req *ov, uint32_t width, uint32_t height, uint32_t planes, uint32_t sx, double sy, double lat_top, double lon_left,
             const uint8_t *pixels, const uint8_t *valid, int device)
{
	struct latlon_lines l;
	mdemod_overlay_vectors grat;
	char wld[160];
	const char *ext[1] = { "wld" }, *text[1] = { wld };
	memset(&l, 0, sizeof l);
	memset(&grat, 0, sizeof grat);
	l.geo = (mdemod_overlay_geo){ width, height, sx, 0, sy, lat_top, lon_left };
	l.planes = planes; l.style = ov->style; l.valid = valid; l.device = device;
	if (ov->graticule) {
		/* (the order of the layers decides no byte: style 0 meets a pixel before style 1) */
		if (mdemod_overlay_graticule(&l.geo, ov->step, &grat) != MDEMOD_OK) { fprintf(stderr, "--graticule: %s\n", mdemod_last_error()); return 1; }
		l.layers[l.n].vectors = &grat; l.layers[l.n++].style = 1;
	}
	for (uint32_t k = 0; k < ov->n_files; k++) { l.layers[l.n].vectors = &ov->coast[k]; l.layers[l.n++].style = 0; }
	latlon_world_file(wld, sx, sy, lat_top, lon_left);
	const int code = overlay_tail(stem, pixels, width, height, planes, device, latlon_draw, &l, ext, text, 1, ": the world file is incomplete");
	if (!code)
		printf("%s_overlay: %llu pieces kept, %llu tiles touched; lines: %llu pieces, %llu pixels; graticule: %llu pieces, %llu pixels\n", stem,
		       (unsigned long long)(l.rep.pieces[0] + l.rep.pieces[1]), (unsigned long long)l.rep.tiles, (unsigned long long)l.rep.pieces[0],
		       (unsigned long long)l.rep.pixels[0], (unsigned long long)l.rep.pieces[1], (unsigned long long)l.rep.pixels[1]);
	mdemod_overlay_vectors_free(&grat);
	return code;
}

/* one map of the given slots: <tag>_map.ppm / .pgm, its world file and its line.  0, or the exit status. */
static int
map_file(const char *s_name, const mdemod_image_result *res, const struct vcdu_req *req, const uint32_t *select, uint32_t planes, const char *tag, int device)
{
	const uint8_t *image[3] = { res->image[0], res->image[1], res->image[2] }, *filled[3] = { res->filled[0], res->filled[1], res->filled[2] };
	mdemod_map_opts mo;
	mdemod_map_result map;
	map_options(req, &mo);
	const int rc = mdemod_map_compose_host(&mo, &req->tle, image, filled, res->summary.rows, res->place, res->sinfo, res->n_packets, select, planes, &map, device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--map: %s: %s\n", s_name, why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	int code = 0;
	char ext[48], wld[160], at[64];
	snprintf(ext, sizeof ext, "_%s_map.%s", tag, planes == 3 ? "ppm" : "pgm");
	char *name = beside(s_name, ext), *base = beside(s_name, "");
	if (!name) { fprintf(stderr, "--map: could not open the picture\n"); code = 1; }
	else if (!(code = equalise_picture(name, map.pixels, map.valid, map.width, map.height, planes, 1, device)))
		code = write_picture("--map", name, map.pixels, map.width, map.height, planes, device);
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
		else code = overlay_file(stem, req->overlay, map.width, map.height, planes, map.sx, map.sy, map.lat_top, map.lon_left, map.pixels, map.valid, device);
		free(stem);
	}
	mdemod_map_free(&map);
	return code;
}

/* --map: the composite (--composite) or every channel that received a strip on the grid.  0, or the exit status. */
static int
map_files(const char *s_name, const mdemod_image_result *res, const struct vcdu_req *req, int device)
{
	int got[3] = { 0, 0, 0 }, code = 0, slot = 0;
	uint32_t select[3], planes;
	char tag[16];
	slots_received(res, got);
	/* (where --composite auto finds nothing the composite's own line has said so) */
	while (!code && next_choice(req, got, &slot, select, &planes, tag) > 0) code = map_file(s_name, res, req, select, planes, tag, device);
	return code;
}

/* --mosaic: one mosaic of the given slots of the kept passes: <base>_<tag>_mosaic.ppm / .pgm, its world file and its line.  0, or
 * the exit status. */
static int
mosaic_file(const char *base, const mdemod_mosaic_pass *passes, uint32_t n, const struct vcdu_req *req, const uint32_t *select, uint32_t planes, const char *tag,
            int device)
{
	mdemod_mosaic_opts mo;
	mdemod_mosaic_result mos;
	mdemod_mosaic_default_opts(&mo);
	if (req->scan_deg != 0.0) mo.scan_deg = req->scan_deg;
	if (req->map_scale != 0.0) mo.px_per_deg = req->map_scale;
	if (req->offset_given) mo.time_offset = req->time_offset;
	if (req->side) mo.side = req->side;
	mo.blend = req->mosaic_blend;
	const int rc = mdemod_mosaic_compose_host(&mo, passes, n, select, planes, &mos, device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--mosaic: %s\n", why_of(rc)); return rc == MDEMOD_ERR_PARAM ? 1 : 2; }
	int code = 0;
	const size_t len = strlen(base) + strlen(tag) + 32;
	char *name = malloc(len);
	if (name) snprintf(name, len, "%s_%s_mosaic.%s", base, tag, planes == 3 ? "ppm" : "pgm");
	if (!name) { fprintf(stderr, "--mosaic: could not open the picture\n"); code = 1; }
	else if (!(code = equalise_picture(name, mos.pixels, mos.valid, mos.width, mos.height, planes, 1, device)))
		code = write_picture("--mosaic", name, mos.pixels, mos.width, mos.height, planes, device);
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
		code = overlay_file(name, req->overlay, mos.width, mos.height, planes, mos.sx, mos.sy, mos.lat_top, mos.lon_left, mos.pixels, mos.valid, device);
	}
	free(name);
	mdemod_mosaic_free(&mos);
	return code;
}

/* --mosaic: the kept pictures of all files on one grid: the composite (--composite; auto on what the passes received together) or
 * every channel that received a strip in any pass.  Frees what was kept.  0, or the exit status. */
static int
mosaic_files(const char *base, mdemod_image_result *kept, const struct stream_io *io, int n_files, const struct vcdu_req *req, int device)
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
	while (n && !code && (more = next_choice(req, got, &slot, select, &planes, tag)) > 0) code = mosaic_file(base, passes, n, req, select, planes, tag, device);
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
polar_overlay_file(const char *stem, const struct overlay_req *ov, const mdemod_polar_result *pic, const char *wld, const char *prj, int device)
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
	l.pic = pic; l.device = device;
	for (int s = 0; s < 2; s++) {
		l.styles[s].half_width = ov->style[s].half_width; l.styles[s].opacity = ov->style[s].opacity; l.styles[s].inside_only = ov->style[s].inside_only;
		memcpy(l.styles[s].colour, ov->style[s].colour, 3);
	}
	if (ov->graticule) {
		if (mdemod_polar_graticule(f, ov->step, &grat) != MDEMOD_OK || mdemod_polar_vertices(f, grat.lon, grat.lat, grat.first, grat.n_lines, &pts[l.n]) != MDEMOD_OK) {
			fprintf(stderr, "--graticule: %s\n", mdemod_last_error());
			code = 1;
		} else { l.layers[l.n] = &pts[l.n]; l.style_of[l.n++] = 1; }
	}
	for (uint32_t k = 0; k < ov->n_files && !code; k++) {
		if (mdemod_polar_vertices(f, ov->coast[k].lon, ov->coast[k].lat, ov->coast[k].first, ov->coast[k].n_lines, &pts[l.n]) != MDEMOD_OK) {
			fprintf(stderr, "--overlay: %s\n", mdemod_last_error());
			code = 1;
		} else { l.layers[l.n] = &pts[l.n]; l.style_of[l.n++] = 0; }
	}
	if (!code) code = overlay_tail(stem, pic->pixels, f->width, f->height, pic->planes, device, polar_draw, &l, ext, text, 2, "");
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
polar_file(const char *stem, const mdemod_polar_pass *passes, uint32_t n, const struct vcdu_req *req, const uint32_t *select, uint32_t planes, const char *tag, int device)
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
	const int rc = mdemod_polar_compose_host(&po, passes, n, select, planes, &pic, device);
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
		if (!(code = equalise_picture(name, pic.pixels, pic.valid, pic.frame.width, pic.frame.height, planes, 1, device)))
			code = write_picture("--map-proj stereo", name, pic.pixels, pic.frame.width, pic.frame.height, planes, device);
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
		code = polar_overlay_file(name, req->overlay, &pic, wld, prj, device);
	}
	free(name);
	mdemod_polar_free(&pic);
	return code;
}

/* --map-proj stereo: the composite (--composite; auto on what the passes received together) or every channel that received a strip
 * in any pass, of the n passes that gave a picture.  0, or the exit status. */
static int
polar_files(const char *stem, const mdemod_image_result *const *results, int n_results, const struct vcdu_req *req, int device)
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
	while (n && !code && next_choice(req, got, &slot, select, &planes, tag) > 0) code = polar_file(stem, passes, n, req, select, planes, tag, device);
	return code;
}

/* --sun: given, and the two angles (0: the library's default) */
static struct { int on; double ref_deg, limit_deg; int ref_given, limit_given; } sun_req;

/* --sun: the reflective channels of one file's pictures in place, with the options of --map, and the file's line on stdout.  Nothing
 * without the option or without a picture.  0, or the exit status. */
static int
sun_pictures(const char *s_name, mdemod_image_result *res, const struct vcdu_req *req, int device)
{
	if (!sun_req.on || !res->summary.rows) return 0;
	mdemod_sun_opts so;
	mdemod_sun_summary ss;
	mdemod_map_opts mo;
	mdemod_sun_default_opts(&so);
	if (sun_req.ref_given) so.ref_deg = sun_req.ref_deg;
	if (sun_req.limit_given) so.limit_deg = sun_req.limit_deg;
	map_options(req, &mo);
	/* (the sun layer's header repeats the map layer's options and element set field for field) */
	mdemod_sun_pass_opts po;
	mdemod_sun_orbit orbit;
	_Static_assert(sizeof po == sizeof mo && sizeof orbit == sizeof req->tle, "the sun layer's pass is the map layer's");
	memcpy(&po, &mo, sizeof po);
	memcpy(&orbit, &req->tle, sizeof orbit);
	uint8_t *image[3] = { res->image[0], res->image[1], res->image[2] };
	const int rc = mdemod_sun_correct_host(&so, &po, &orbit, image, req->apids, res->summary.rows, res->place, res->sinfo, res->n_packets, &ss, device);
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
image_files(const char *s_name, const uint8_t *vcdu, const mdemod_rs_info *info, uint64_t n, int device, const struct vcdu_req *req)
{
	const uint32_t *apids = req->apids;
	mdemod_image_opts io;
	mdemod_image_result res;
	mdemod_image_default_opts(&io);
	for (int k = 0; k < 3; k++) io.apids[k] = apids[k];
	const int rc = mdemod_image_decode_host(&io, vcdu, info, n, &res, device);
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
		code = write_picture("--image", name, res.image[k], MDEMOD_IMAGE_WIDTH, rows * 8, 1, device);
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
	if (!code) code = sun_pictures(s_name, &res, req, device);                  /* (--sun: everything below comes from the corrected buffers) */
	if (!code && (req->rectify || req->composite)) code = picture_files(s_name, &res, req, device);
	if (!code && req->map && req->polar) {
		const mdemod_image_result *one[1] = { &res };
		char *stem = beside(s_name, "");
		if (!stem) { fprintf(stderr, "--map-proj stereo: out of memory\n"); code = 2; }
		else code = polar_files(stem, one, 1, req, device);
		free(stem);
	} else if (!code && req->map) code = map_files(s_name, &res, req, device);
	if (!code && req->keep) *req->keep = res;                                  /* (the mosaic frees it) */
	else mdemod_image_free(&res);
	return code;
}

/* --vcdu / --image: n CADUs through the transfer-frame layer; the VCDUs beside the output file and one line (--vcdu), the pictures
 * (--image).  0, or the exit status. */
static int
vcdu_file(const char *s_name, const uint8_t *cadu, uint64_t n, int device, const struct vcdu_req *req)
{
	uint8_t *vcdu = malloc(n ? (size_t)n * MDEMOD_RS_VCDU_BYTES : 1);
	mdemod_rs_info *info = calloc(n ? (size_t)n : 1, sizeof(*info));
	char *out_name = beside(s_name, ".vcdu");
	int code = 1;
	if (!vcdu || !info || !out_name) { fprintf(stderr, "--vcdu: out of memory for the frames of %s\n", s_name); goto done; }
	mdemod_rs_opts ro;
	mdemod_rs_default_opts(&ro);
	const int rc = mdemod_rs_decode_host(&ro, cadu, n, vcdu, info, device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--vcdu: %s: %s\n", s_name, why_of(rc)); code = 2; goto done; }
	if (!req->write_vcdu) { code = image_files(s_name, vcdu, info, n, device, req); goto done; }
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
	code = req->image ? image_files(s_name, vcdu, info, n, device, req) : 0;
done:
	free(out_name); free(info); free(vcdu);
	return code;
}

/* --cadu / --vcdu: the soft symbols of one finished output file through the frame layer, the CADUs (and the VCDUs) beside it.  0, or
 * the exit status. */
static int
cadu_file(const char *s_name, int device, int write_cadu, const struct vcdu_req *req, int diff, int skew, uint32_t il_delay)
{
	FILE *f = fopen(s_name, "rb");
	if (!f) { fprintf(stderr, "--cadu: %s: %s\n", s_name, strerror(errno)); return 1; }
	long len = -1;
	if (!fseek(f, 0, SEEK_END)) len = ftell(f);
	if (len < 0 || fseek(f, 0, SEEK_SET)) { fprintf(stderr, "--cadu: cannot read %s\n", s_name); fclose(f); return 1; }
	uint64_t m = (uint64_t)len / 2;
	const uint64_t cap = m / MDEMOD_FRAME_SYMBOLS;
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
		const int irc = mdemod_il_decode_host(&io, soft, m, deint, il_room, segs, il_cap, &n_segs, &periods, &mean, device);
		if (irc != MDEMOD_OK) { fprintf(stderr, "--int: %s: %s\n", s_name, why_of(irc)); code = 2; goto done; }
		printf("%s: interleaver: %llu segments, %llu periods, mean sync score %d / 24576\n", s_name, (unsigned long long)n_segs,
		       (unsigned long long)periods, (int)mean);
		const uint64_t written = periods < il_room / MDEMOD_IL_BRANCHES ? periods : il_room / MDEMOD_IL_BRANCHES;
		sym = deint;
		m = written * MDEMOD_IL_BRANCHES;
		skew = 0;                                                                /* (resolved by the sync word) */
	}
	mdemod_frames_opts fo;
	mdemod_frames_default_opts(&fo);
	uint64_t n = 0;
	mdemod_frames_link link = { (uint32_t)diff, (uint32_t)skew, { 0, 0 } };
	const int rc = diff || skew ? mdemod_frames_link_decode_host(&link, &fo, sym, m, cadu, frames, cap, &n, device)
	                            : mdemod_frames_decode_host(&fo, sym, m, cadu, frames, cap, &n, device);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--cadu: %s: %s\n", s_name, why_of(rc)); code = 2; goto done; }
	if (n > cap) n = cap;
	if (!write_cadu) { code = vcdu_file(s_name, cadu, n, device, req); goto done; }
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
	code = req->write_vcdu || req->image ? vcdu_file(s_name, cadu, n, device, req) : 0;
done:
	free(out_name); free(frames); free(cadu); free(soft); free(segs); free(deint);
	fclose(f);
	return code;
}

int
main(int argc, char **argv)
{
	float pll_bw = MDEMOD_DEFAULT_PLL_BW, symrate = MDEMOD_DEFAULT_SYM_RATE, freq_max_delta = -1;
	int rrc_order = MDEMOD_DEFAULT_RRC_ORDER, interp = MDEMOD_DEFAULT_INTERP;
	int quiet = 0, batch = 0, oqpsk = 0, bps = 0, samplerate = -1, stdout_mode = 0, device = 0, tiled = 0;
	int tile_samples = 0, pilot_margin = -1, carrier_seed = -1, update_interval = -1;
	const char *output_fname = NULL;
	int devs[MAX_DEVICES], n_dev = 0, plan = 0, jobs = 4;
	int use_fe = 0, decimation = 1;
	double offset_hz = 0.0;
	int auto_offset = 0, auto_decimate = 0, decimate_given = 0, scan = 0, want_cadu = 0, want_vcdu = 0, want_diff = 0, want_skew = 0, want_int = 0, want_image = 0, apids_given = 0, geometry_given = 0, altitude_given = 0, map_opts_given = 0;
	const char *map_fname = NULL, *mosaic_base = NULL;
	uint32_t map_norad = 0;
	int mosaic_blend_given = 0, polar_opts_given = 0;
	struct vcdu_req vreq = { 0, 0, { 64, 65, 66 }, 0, 0, { 2, 1, 0 }, 0.0, 0.0 };
	/* --overlay: yellow, one pixel, opaque; --graticule: grey, one pixel, opacity 160 */
	static struct overlay_req oreq = { .style = { { 128, 256, { 255, 255, 0 }, 0 }, { 128, 160, { 128, 128, 128 }, 0 } } };
	const char *overlay_fname[OVERLAY_FILES] = { NULL, NULL, NULL };
	int n_overlay = 0, overlay_opts_given = 0;
	long int_delay = MDEMOD_IL_DEFAULT_BRANCH_DELAY;
	double *auto_offsets = NULL;               /* --offset auto: the offset chosen for each file */
#ifdef MDEMOD_TUI
	int force_tui = 0;
#endif
	int c;

	while ((c = getopt_long(argc, argv, "a:Bb:d:f:hm:o:O:qR:r:s:S:v", longopts, NULL)) != -1) {
		switch (c) {
		case 0x00: stdout_mode = 1; break;
		case 0x01: device = atoi(optarg); devs[0] = device; n_dev = 1; break;
		case 0x06:
			n_dev = parse_devices(optarg, devs, MAX_DEVICES);
			if (!n_dev) { fprintf(stderr, "--devices: a comma separated list of GPU ordinals\n"); return 1; }
			break;
		case 0x07: plan = 1; break;
#ifdef MDEMOD_TUI
		case 0x09: force_tui = 1; break;
#else
		case 0x09: break;                             /* --tui in a build without the display: accepted, nothing to draw */
#endif
		case 0x0a: jobs = atoi(optarg); if (jobs < 1) { fprintf(stderr, "--jobs: a positive number\n"); return 1; } break;
		case 0x0d: scan = 1; break;
		case 0x0e: want_cadu = 1; break;
		case 0x0f: want_vcdu = 1; break;
		case 0x10: want_diff = 1; break;
		case 0x11: want_skew = 1; break;
		case 0x12: want_int = 1; break;
		case 0x13: int_delay = atol(optarg); break;
		case 0x14: want_image = 1; break;
		case 0x15: {
			unsigned a[3];
			char tail;
			if (sscanf(optarg, "%u,%u,%u%c", &a[0], &a[1], &a[2], &tail) != 3) { fprintf(stderr, "--apids: three numbers, e.g. 64,65,66\n"); return 1; }
			for (int k = 0; k < 3; k++) {
				if (a[k] < 64 || a[k] > 69 || (k && a[k] == a[0]) || (k == 2 && a[2] == a[1])) {
					fprintf(stderr, "--apids: three different channels, each 64 .. 69\n");
					return 1;
				}
				vreq.apids[k] = a[k];
			}
			apids_given = 1;
			break;
		}
		case 0x16: vreq.rectify = 1; break;
		case 0x17:
			if (!strcmp(optarg, "auto")) { vreq.composite = 2; break; }
			if (strlen(optarg) != 3 || strspn(optarg, "123") != 3) {
				fprintf(stderr, "--composite: three digits, each 1 .. 3 (the channels of red, green, blue in --apids order, e.g. 321), or auto\n");
				return 1;
			}
			for (int k = 0; k < 3; k++) vreq.comp[k] = (uint32_t)(optarg[k] - '1');
			vreq.composite = 1;
			break;
		case 0x18:
		case 0x19: {
			char *end;
			const double v = strtod(optarg, &end);
			if (end == optarg || *end || !(v > 0.0)) { fprintf(stderr, "%s: a positive number\n", c == 0x18 ? "--altitude" : "--scan-angle"); return 1; }
			if (c == 0x18) { vreq.altitude_km = v; altitude_given = 1; } else vreq.scan_deg = v;
			geometry_given = 1;
			break;
		}
		case 0x1a: map_fname = optarg; break;
		case 0x1b: {
			char *end;
			const long v = strtol(optarg, &end, 10);
			if (end == optarg || *end || v < 1 || v > 999999999) { fprintf(stderr, "--norad: a catalogue number\n"); return 1; }
			map_norad = (uint32_t)v;
			map_opts_given = 1;
			break;
		}
		case 0x1c:
		case 0x1e: {
			char *end;
			const double v = strtod(optarg, &end);
			if (end == optarg || *end) { fprintf(stderr, "%s: a number\n", c == 0x1c ? "--map-scale" : "--time-offset"); return 1; }
			if (c == 0x1c) vreq.map_scale = v; else { vreq.time_offset = v; vreq.offset_given = 1; }
			if (c == 0x1c && v == 0.0) vreq.map_scale = -1.0;                        /* (0 stands for the default inside: let the layer refuse it) */
			map_opts_given = 1;
			break;
		}
		case 0x1d: {
			int y;
			unsigned m, d;
			char tail;
			if (sscanf(optarg, "%d-%u-%u%c", &y, &m, &d, &tail) != 3 || y < 1957 || y > 2200 || m < 1 || m > 12 || d < 1 || d > 31) {
				fprintf(stderr, "--date: yyyy-mm-dd\n");
				return 1;
			}
			vreq.map_date = (int32_t)days_from_civil(y, m, d);
			vreq.date_given = 1;
			map_opts_given = 1;
			break;
		}
		case 0x1f:
			if (strcmp(optarg, "1") && strcmp(optarg, "-1")) { fprintf(stderr, "--scan-side: 1 or -1\n"); return 1; }
			vreq.side = atoi(optarg);
			map_opts_given = 1;
			break;
		case 0x20: mosaic_base = optarg; break;
		case 0x22:
			if (n_overlay == OVERLAY_FILES) { fprintf(stderr, "--overlay: at most %d files\n", OVERLAY_FILES); return 1; }
			overlay_fname[n_overlay++] = optarg;
			break;
		case 0x23: {
			char *end = optarg;
			const int automatic = !strcmp(optarg, "auto");
			oreq.graticule = 1;
			oreq.step = automatic ? 0.0 : strtod(optarg, &end);
			if (!automatic && (end == optarg || *end || !(oreq.step >= 0.01 && oreq.step <= 90.0))) {
				fprintf(stderr, "--graticule: a number of degrees (0.01 .. 90) or auto\n");
				return 1;
			}
			break;
		}
		case 0x24: {
			unsigned r, g, b;
			char tail;
			if (strlen(optarg) != 6 || sscanf(optarg, "%2x%2x%2x%c", &r, &g, &b, &tail) != 3) { fprintf(stderr, "--overlay-colour: six hexadecimal digits, rrggbb\n"); return 1; }
			oreq.style[0].colour[0] = (uint8_t)r; oreq.style[0].colour[1] = (uint8_t)g; oreq.style[0].colour[2] = (uint8_t)b;
			overlay_opts_given = 1;
			break;
		}
		case 0x25: {
			char *end;
			const double w = strtod(optarg, &end);
			if (end == optarg || *end || !(w >= 0.0 && w <= 16.0)) { fprintf(stderr, "--overlay-width: a number of pixels, 0 .. 16\n"); return 1; }
			oreq.style[0].half_width = (uint32_t)(128.0 * w + 0.5);
			overlay_opts_given = 1;
			break;
		}
		case 0x26: {
			char *end;
			const long q = strtol(optarg, &end, 10);
			if (end == optarg || *end || q < 1 || q > 100) { fprintf(stderr, "--jpeg: a quality, 1 .. 100\n"); return 1; }
			jpeg_req.quality = (unsigned)q;
			break;
		}
		case 0x2b: {
			char *end;
			const double v = strtod(optarg, &end);
			if (end == optarg || *end || !(v >= 1.0 && v <= 256.0)) { fprintf(stderr, "--equalise: a clip limit, 1 .. 256 (times a flat histogram; 3 is usual)\n"); return 1; }
			equalise_req.clip_percent = (unsigned)(100.0 * v + 0.5);
			break;
		}
		case 0x2c: {
			char *end;
			const long v = strtol(optarg, &end, 10);
			if (end == optarg || *end || v < MDEMOD_EQUALISE_MIN_TILE || v > MDEMOD_EQUALISE_MAX_TILE || v % 8) {
				fprintf(stderr, "--equalise-tile: pixels, a multiple of 8, 16 .. 512\n");
				return 1;
			}
			equalise_req.tile = (unsigned)v;
			equalise_req.tile_given = 1;
			break;
		}
		case 0x2d: {
			char *end;
			const double v = strtod(optarg, &end);
			if (end == optarg || *end || !(v >= 0.0 && v <= 100.0)) { fprintf(stderr, "--equalise-amount: percent, 0 .. 100\n"); return 1; }
			equalise_req.amount = (unsigned)(2.56 * v + 0.5);
			equalise_req.amount_given = 1;
			break;
		}
		case 0x2e:
			sun_req.on = 1;
			break;
		case 0x2f: {
			char *end;
			const double v = strtod(optarg, &end);
			if (end == optarg || *end || !(v >= 0.0 && v <= MDEMOD_SUN_MAX_REF)) { fprintf(stderr, "--sun-ref: degrees of zenith angle, 0 .. 80\n"); return 1; }
			sun_req.ref_deg = v;
			sun_req.ref_given = 1;
			break;
		}
		case 0x30: {
			char *end;
			const double v = strtod(optarg, &end);
			if (end == optarg || *end || !(v >= MDEMOD_SUN_MIN_LIMIT && v <= MDEMOD_SUN_MAX_LIMIT)) { fprintf(stderr, "--sun-limit: degrees of zenith angle, 60 .. 89\n"); return 1; }
			sun_req.limit_deg = v;
			sun_req.limit_given = 1;
			break;
		}
		case 0x27:
			if (!strcmp(optarg, "stereo")) vreq.polar = 1;
			else if (!strcmp(optarg, "latlon")) vreq.polar = 0;
			else { fprintf(stderr, "--map-proj: latlon or stereo\n"); return 1; }
			map_opts_given = 1;
			break;
		case 0x28:
		case 0x29:
		case 0x2a: {
			char *end = optarg;
			const int automatic = c == 0x29 && !strcmp(optarg, "auto");
			const double v = automatic ? 0.0 : strtod(optarg, &end);
			if (!automatic && (end == optarg || *end)) { fprintf(stderr, "%s: a number\n", c == 0x28 ? "--map-res" : c == 0x29 ? "--map-lon0" : "--map-lat-ts"); return 1; }
			if (c == 0x28 && !(v >= MDEMOD_POLAR_MIN_RES && v <= MDEMOD_POLAR_MAX_RES)) { fprintf(stderr, "--map-res: metres per pixel, 100 .. 100000\n"); return 1; }
			if (c == 0x29 && !automatic && !(v >= -360.0 && v <= 360.0)) { fprintf(stderr, "--map-lon0: degrees, -360 .. 360, or auto\n"); return 1; }
			if (c == 0x2a && !(v > 0.0 && v <= 90.0)) { fprintf(stderr, "--map-lat-ts: the magnitude of the standard parallel in degrees, 0 < .. <= 90\n"); return 1; }
			if (c == 0x28) vreq.polar_res = v;
			else if (c == 0x2a) vreq.polar_lat_ts = v;
			else { vreq.polar_lon0 = v; vreq.lon0_given = !automatic; }
			polar_opts_given = 1;
			map_opts_given = 1;
			break;
		}
		case 0x21:
			if (!strcmp(optarg, "feather")) vreq.mosaic_blend = MDEMOD_MOSAIC_FEATHER;
			else if (!strcmp(optarg, "best")) vreq.mosaic_blend = MDEMOD_MOSAIC_BEST;
			else { fprintf(stderr, "--mosaic-blend: feather or best\n"); return 1; }
			mosaic_blend_given = 1;
			break;
		case 0x0b:
			if (!strcmp(optarg, "auto")) { auto_offset = 1; use_fe = 1; break; }
			auto_offset = 0;
			if (parse_hz(optarg, &offset_hz)) { fprintf(stderr, "--offset: a number of Hz (k/M suffixes), e.g. 300k or -1.2M\n"); return 1; }
			use_fe = 1;
			break;
		case 0x0c: {
			char *end;
			if (!strcmp(optarg, "auto")) { auto_decimate = 1; decimate_given = 0; use_fe = 1; break; }
			const long v = strtol(optarg, &end, 10);
			if (end == optarg || *end || v < 1 || v > 1 << 20) { fprintf(stderr, "--decimate: a positive integer, or auto\n"); return 1; }
			decimation = (int)v;
			auto_decimate = 0; decimate_given = 1;
			use_fe = 1;
			break;
		}
		case 0x08:
#ifdef MDEMOD_TUI
			return tui_selftest(force_tui);
#else
			fprintf(stderr, "built without ncurses\n"); return 1;
#endif
		case 0x02: tiled = 1; break;
		case 0x03: tile_samples = (int)human_number(optarg); break;
		case 0x04: pilot_margin = (int)human_number(optarg); break;
		case 0x05:
			if (!strcmp(optarg, "spectrum")) carrier_seed = 1;
			else if (!strcmp(optarg, "pilot")) carrier_seed = 0;
			else { fprintf(stderr, "--carrier-seed: spectrum or pilot\n"); return 1; }
			break;
		case 'b': pll_bw = human_number(optarg); break;
		case 'B': batch = 1; break;
		case 'd': freq_max_delta = human_number(optarg); break;
		case 'f': rrc_order = atoi(optarg); break;
		case 'h': usage(argv[0]); return 0;
		case 'm': if (!strcmp(optarg, "oqpsk")) oqpsk = 1; break;     /* unknown modes stay QPSK, main.c:104 */
		case 'o': output_fname = optarg; break;
		case 'O': interp = atoi(optarg); break;
		case 'q': quiet = 1; break;
		case 'R': update_interval = atoi(optarg); break;              /* main.c:116 */
		case 'r': symrate = human_number(optarg); break;
		case 's': samplerate = (int)human_number(optarg); break;
		case 'S': bps = atoi(optarg); break;
		case 'v': printf("meteor_demod_amd (MI355X) ABI %u\n", mdemod_abi_version()); return 0;
		default: usage(argv[0]); return 1;
		}
	}
	freq_max_delta = (float)(freq_max_delta * (2 * M_PI) / symrate);       /* main.c:136 */
	if (argc - optind < 1) { usage(argv[0]); return 1; }
	if (update_interval < 0) update_interval = batch ? 2000 : 50;                 /* main.c:144 (before batch is forced below) */
	if (stdout_mode) { batch = 1; quiet = 1; }
	for (int i = optind; i < argc; i++) if (!strcmp(argv[i], "-")) batch = 1;     /* stdin forces batch: main.c:157 */

	const int n_files = argc - optind;
	if (n_files > 1 && (output_fname || stdout_mode)) {
		fprintf(stderr, "-o/--stdout need a single input file\n");
		return 1;
	}
	if (use_fe && !have_frontend()) {
		fprintf(stderr, "--offset / --decimate: this library has no front end (built without include/meteor_demod_amd_frontend.h's entries)\n");
		return 1;
	}
	if ((auto_offset || auto_decimate || scan) && !have_survey()) {
		fprintf(stderr, "--offset auto / --decimate auto / --scan: this library has no survey (built without include/meteor_demod_amd_survey.h's entries)\n");
		return 1;
	}
	if (want_cadu && stdout_mode) {
		fprintf(stderr, "--cadu: not with --stdout (the frames are decoded from the finished output file)\n");
		return 1;
	}
	if (want_cadu && !have_frames()) {
		fprintf(stderr, "--cadu: this library has no frame layer (built without include/meteor_demod_amd_frames.h's entries)\n");
		return 1;
	}
	if (want_vcdu && stdout_mode) {
		fprintf(stderr, "--vcdu: not with --stdout (the frames are decoded from the finished output file)\n");
		return 1;
	}
	if (want_vcdu && !(have_frames() && have_rs())) {
		fprintf(stderr, "--vcdu: this library has no %s (built without include/%s's entries)\n", have_frames() ? "transfer-frame layer" : "frame layer",
		        have_frames() ? "meteor_demod_amd_rs.h" : "meteor_demod_amd_frames.h");
		return 1;
	}
	if (vreq.polar && !(have_polar() && have_map() && have_picture())) {
		fprintf(stderr, "--map-proj stereo: this library has no polar layer (built without include/meteor_demod_amd_polar.h's entries)\n");
		return 1;
	}
	if (polar_opts_given && !vreq.polar) {
		fprintf(stderr, "--map-res / --map-lon0 / --map-lat-ts: only with --map-proj stereo (they are its options)\n");
		return 1;
	}
	if (vreq.polar && vreq.map_scale != 0.0) {
		fprintf(stderr, "--map-scale: not with --map-proj stereo (pixels per degree belong to the latitude / longitude grid: --map-res)\n");
		return 1;
	}
	if (mosaic_base && !(have_mosaic() && have_map() && have_picture())) {
		fprintf(stderr, "--mosaic: this library has no mosaic layer (built without include/meteor_demod_amd_mosaic.h's entries)\n");
		return 1;
	}
	if ((n_overlay || oreq.graticule || overlay_opts_given) && !have_overlay()) {
		fprintf(stderr, "--overlay / --graticule: this library has no overlay layer (built without include/meteor_demod_amd_overlay.h's entries)\n");
		return 1;
	}
	if (map_fname && !(have_map() && have_picture())) {
		fprintf(stderr, "--map: this library has no map layer (built without include/meteor_demod_amd_map.h's entries)\n");
		return 1;
	}
	if (apids_given && !want_image) {
		fprintf(stderr, "--apids: only with --image (it chooses the channels of the pictures)\n");
		return 1;
	}
	if (want_image && stdout_mode) {
		fprintf(stderr, "--image: not with --stdout (the frames are decoded from the finished output file)\n");
		return 1;
	}
	if (want_image && !(have_frames() && have_rs() && have_image())) {
		fprintf(stderr, "--image: this library has no %s (built without include/%s's entries)\n",
		        !have_frames() ? "frame layer" : !have_rs() ? "transfer-frame layer" : "image layer",
		        !have_frames() ? "meteor_demod_amd_frames.h" : !have_rs() ? "meteor_demod_amd_rs.h" : "meteor_demod_amd_image.h");
		return 1;
	}
	if ((vreq.rectify || vreq.composite) && !want_image) {
		fprintf(stderr, "--rectify / --composite: only with --image (they work on its pictures)\n");
		return 1;
	}
	if ((map_fname || map_opts_given) && !want_image) {
		fprintf(stderr, "--map: only with --image (it works on its pictures and their time stamps)\n");
		return 1;
	}
	if (map_opts_given && !map_fname) {
		fprintf(stderr, "--norad / --map-scale / --date / --time-offset / --scan-side / --map-proj: only with --map (they are its options)\n");
		return 1;
	}
	if (mosaic_base && !(map_fname && want_image)) {
		fprintf(stderr, "--mosaic: only with --map (and --image: it blends the maps of the input files)\n");
		return 1;
	}
	if (mosaic_blend_given && !mosaic_base) {
		fprintf(stderr, "--mosaic-blend: only with --mosaic (it is its option)\n");
		return 1;
	}
	if ((n_overlay || oreq.graticule) && !(map_fname && want_image)) {
		fprintf(stderr, "--overlay / --graticule: only with --map (they draw on its pictures)\n");
		return 1;
	}
	if (overlay_opts_given && !n_overlay) {
		fprintf(stderr, "--overlay-colour / --overlay-width: only with --overlay (they are its options)\n");
		return 1;
	}
	if ((equalise_req.tile_given || equalise_req.amount_given) && !equalise_req.clip_percent) {
		fprintf(stderr, "--equalise-tile / --equalise-amount: only with --equalise (they are its options)\n");
		return 1;
	}
	if (equalise_req.clip_percent && !want_image) {
		fprintf(stderr, "--equalise: only with --image (it works on its pictures)\n");
		return 1;
	}
	if (equalise_req.clip_percent && !(vreq.rectify || vreq.composite || map_fname)) {
		fprintf(stderr, "--equalise: only with --rectify, --composite or --map (it works on the derived pictures; the channel pictures stay as decoded)\n");
		return 1;
	}
	if ((sun_req.ref_given || sun_req.limit_given) && !sun_req.on) {
		fprintf(stderr, "--sun-ref / --sun-limit: only with --sun (they are its options)\n");
		return 1;
	}
	if (sun_req.on && !want_image) {
		fprintf(stderr, "--sun: only with --image (it works on its pictures)\n");
		return 1;
	}
	if (sun_req.on && !map_fname) {
		fprintf(stderr, "--sun: only with --map <tle file> (the sun's angle needs the orbit and the line times; the channel pictures stay as decoded)\n");
		return 1;
	}
	if (sun_req.on && !have_sun()) {
		fprintf(stderr, "--sun: this build of libmeteor_demod_amd has no sun layer\n");
		return 1;
	}
	if (equalise_req.clip_percent && !have_equalise()) {
		fprintf(stderr, "--equalise: this build of libmeteor_demod_amd has no equalise layer\n");
		return 1;
	}
	if (jpeg_req.quality && !want_image) {
		fprintf(stderr, "--jpeg: only with --image (it is the format of its pictures)\n");
		return 1;
	}
	if (jpeg_req.quality && !have_jpeg()) {
		fprintf(stderr, "--jpeg: this build of libmeteor_demod_amd has no JPEG encoder\n");
		return 1;
	}
	if (mosaic_base && n_files > MDEMOD_MOSAIC_MAX_PASSES) {
		fprintf(stderr, "--mosaic: %d input files are more than a mosaic takes (1 .. 8 passes)\n", n_files);
		return 1;
	}
	if (map_fname) {
		/* the element set and the options are refused before anything is demodulated */
		FILE *tf = fopen(map_fname, "rb");
		static char text[65536];
		const size_t got = tf ? fread(text, 1, sizeof text - 1, tf) : 0;
		if (!tf || ferror(tf)) { fprintf(stderr, "--map: could not read %s\n", map_fname); if (tf) fclose(tf); return 1; }
		fclose(tf);
		text[got] = 0;
		for (size_t k = 0; k < got; k++) if (!text[k]) text[k] = ' ';
		if (mdemod_map_parse_tle(text, map_norad, &vreq.tle) != MDEMOD_OK) { fprintf(stderr, "--map: %s: %s\n", map_fname, mdemod_last_error()); return 1; }
		mdemod_map_opts mo;
		mdemod_map_timing none;
		map_options(&vreq, &mo);
		/* (a fit of no packets: options out of range are refused with their own text first) */
		if (mdemod_map_fit_time(NULL, NULL, 0, &mo, &none) != MDEMOD_OK && strncmp(mdemod_last_error(), "map: no placed packet", 21)) {
			fprintf(stderr, "--map: %s\n", mdemod_last_error());
			return 1;
		}
		vreq.map = 1;
		vreq.tle_text = text;
		vreq.norad = map_norad;
	}
	/* the vector files are read, and refused, before anything is demodulated */
	for (int k = 0; k < n_overlay; k++) {
		if (mdemod_overlay_read(overlay_fname[k], &oreq.coast[k]) != MDEMOD_OK) { fprintf(stderr, "--overlay: %s: %s\n", overlay_fname[k], mdemod_last_error()); return 1; }
		oreq.n_files++;
	}
	if (n_overlay || oreq.graticule) vreq.overlay = &oreq;
	if (geometry_given && !vreq.rectify && (altitude_given || !map_fname)) {
		fprintf(stderr, "--altitude / --scan-angle: only with --rectify (they are the geometry it takes out)\n");
		return 1;
	}
	if ((vreq.rectify || vreq.composite) && !have_picture()) {
		fprintf(stderr, "--rectify / --composite: this library has no picture layer (built without include/meteor_demod_amd_picture.h's entries)\n");
		return 1;
	}
	if (vreq.rectify) {
		/* the geometry is refused before anything is demodulated */
		mdemod_picture_opts po;
		mdemod_picture_default_opts(&po);
		if (vreq.altitude_km != 0.0) po.altitude_km = vreq.altitude_km;
		if (vreq.scan_deg != 0.0) po.scan_deg = vreq.scan_deg;
		uint32_t w = 0;
		if (!mdemod_picture_column_map || mdemod_picture_column_map(&po, NULL, 0, &w) != MDEMOD_OK) {
			fprintf(stderr, "--rectify: %s\n", mdemod_picture_column_map ? mdemod_last_error() : "this library has no column map");
			return 1;
		}
	}
	vreq.write_vcdu = want_vcdu;
	vreq.image = want_image;
	if ((want_diff || want_skew) && !(want_cadu || want_vcdu || want_image)) {
		fprintf(stderr, "--diff / --skew: only with --cadu or --vcdu (they change how the frames are found and decoded, not the soft symbols)\n");
		return 1;
	}
	if (want_int && stdout_mode) {
		fprintf(stderr, "--int: not with --stdout (the frames are decoded from the finished output file)\n");
		return 1;
	}
	if (want_int && !(want_cadu || want_vcdu || want_image)) {
		fprintf(stderr, "--int: only with --cadu or --vcdu (it changes how the frames are found and decoded, not the soft symbols)\n");
		return 1;
	}
	if (want_int && !have_interleave()) {
		fprintf(stderr, "--int: this library has no interleaved mode (built without include/meteor_demod_amd_interleave.h's entries)\n");
		return 1;
	}
	if (want_int && (int_delay < 1 || int_delay > 0x7FFFFFFFL)) {
		fprintf(stderr, "--int-delay: the branch delay is a number of bits, 1 or more\n");
		return 1;
	}
	if (want_int && want_skew) {
		fprintf(stderr, "--skew: ignored with --int (the interleaver's sync word resolves the skew)\n");
		want_skew = 0;
	}
	if ((want_diff || want_skew) && !have_frames_link()) {
		fprintf(stderr, "--diff / --skew: this library has no link variant of the frame layer (built without include/meteor_demod_amd_frames_link.h's entries)\n");
		return 1;
	}
	if (auto_offset || scan)
		for (int i = optind; i < argc; i++)
			if (!strcmp(argv[i], "-")) { fprintf(stderr, "--offset auto / --scan: not on stdin (there is nothing to look ahead in): give the offset with --offset <hz>\n"); return 1; }
	if (plan) {
		/* the sharding arithmetic, without touching files or GPUs: file i on the (i mod G)-th device of the list */
		if (!n_dev) { fprintf(stderr, "--plan needs --devices\n"); return 1; }
		const int g = n_dev > n_files ? n_files : n_dev;
		for (int d = 0; d < g; d++) {
			printf("device %d:", devs[d]);
			for (int i = d; i < n_files; i += g) printf(" %s", argv[optind + i]);
			printf("\n");
		}
		return 0;
	}
	struct stream_io *io = calloc((size_t)n_files, sizeof(*io));
	if (!io) return 1;
	struct worker *ws = NULL;
	int n_workers = 0;
	/* every way out from here on: files closed, nothing left allocated (the sanitizer builds of tests/test_sanitize.py look) */
#define LEAVE(code) do { \
		close_all(io, n_files); \
		for (int d_ = 0; d_ < n_workers; d_++) { free(ws[d_].io); free(ws[d_].fe_offsets); } \
		free(ws); \
		free(auto_offsets); \
		for (int i_ = 0; i_ < n_files; i_++) { free(io[i_].out_name); } \
		free(io); \
		return (code); \
	} while (0)

	for (int i = 0; i < n_files; i++) {
		io[i].in_name = argv[optind + i];
		io[i].in = !strcmp(io[i].in_name, "-") ? stdin : fopen(io[i].in_name, "rb");
		if (!io[i].in) { fprintf(stderr, "Could not open input file\n"); LEAVE(1); }
		int sr = samplerate, b = bps;
		if (parse_wav(io[i].in, &sr, &b)) fseek(io[i].in, 0, SEEK_SET);    /* raw: main.c:164-166 */
		if (i == 0) { samplerate = sr; bps = b; }
		else if (sr != samplerate || b != bps) { fprintf(stderr, "all inputs of a batch must share rate and format\n"); LEAVE(1); }
	}
	if (samplerate < 0) {
		fprintf(stderr, "Could not auto-detect sample rate. Please specify it with -s <samplerate>\n");
		usage(argv[0]);                                                                /* main.c:170 */
		LEAVE(1);
	}
	if (!bps) { fprintf(stderr, "Could not auto-detect bits per sample, assuming 16\n"); bps = 16; }
	/* any other sample size: the reference's reader returns 0 on the first sample (wavfile.c:71-73) and it writes an empty
	 * output file; same here, without touching the GPU */
	const int bps_ok = (bps == 8 || bps == 16 || bps == 32);
	if (!bps_ok) fprintf(stderr, "%d bits per sample: nothing to demodulate (8, 16 or 32 expected)\n", bps);
	mdemod_fe_params fep;
	memset(&fep, 0, sizeof(fep));
	fep.offset_hz = offset_hz; fep.decimation = decimation; fep.taps_per_phase = 0;
	if ((auto_offset || auto_decimate || scan) && bps_ok) {
		/* the survey: before any output file exists, so that a file without a signal leaves nothing behind */
		mdemod_params in;
		memset(&in, 0, sizeof(in));
		in.pll_bw = pll_bw; in.sym_bw = MDEMOD_DEFAULT_SYM_BW; in.samplerate = samplerate; in.symrate = (int)symrate;
		in.interp_factor = interp; in.rrc_order = rrc_order; in.oqpsk = oqpsk; in.freq_max = freq_max_delta;
		in.bps = bps; in.device = n_dev ? devs[0] : device; in.n_streams = 1;
		if (auto_decimate || (!decimate_given && (auto_offset || scan))) {
			const int rc = mdemod_survey_plan(&in, NULL, &decimation);
			if (rc != MDEMOD_OK) { fprintf(stderr, "--decimate auto: %s\n", why_of(rc)); LEAVE(1); }
			fep.decimation = decimation;
		}
		if (auto_offset || scan) {
			mdemod_survey_opts so;
			mdemod_survey_default_opts(&so);
			so.decimation = decimation;
			auto_offsets = calloc((size_t)n_files, sizeof(*auto_offsets));
			if (!auto_offsets) LEAVE(1);
			for (int i = 0; i < n_files; i++) {
				mdemod_survey_hit hits[MDEMOD_SURVEY_MAX_CANDIDATES];
				uint32_t n_hits = 0;
				const int rc = survey_file(&in, &so, &io[i], hits, &n_hits);
				if (rc == 1) LEAVE(1);
				if (rc) { fprintf(stderr, "%s: survey: %s\n", io[i].in_name, why_of(rc)); LEAVE(2); }
				if (scan) {
					if (n_files > 1) printf("# %s\n", io[i].in_name);
					for (uint32_t k = 0; k < n_hits; k++)
						printf("%.1f %.2f %.2f %.2f %d\n", round_offset(hits[k].offset_hz), hits[k].psd_snr_db, hits[k].clock_quality,
						       hits[k].carrier_quality, hits[k].confirmed);
					continue;
				}
				if (!n_hits || !hits[0].confirmed) {             /* (confirmed hits come first) */
					if (n_hits)
						fprintf(stderr, "%s: no LRPT signal of %d sym/s confirmed; the best candidate, at %+.1f Hz (%.1f dB over the floor), has a "
						        "symbol-rate line of quality %.1f\n", io[i].in_name, (int)symrate, hits[0].offset_hz, hits[0].psd_snr_db, hits[0].clock_quality);
					else
						fprintf(stderr, "%s: no LRPT signal of %d sym/s found: nothing stands out of the noise floor\n", io[i].in_name, (int)symrate);
					LEAVE(1);
				}
				auto_offsets[i] = round_offset(hits[0].offset_hz);
			}
			if (scan) LEAVE(0);
			fep.offset_hz = auto_offsets[0];
		}
	}
	if (scan) LEAVE(0);
	if (use_fe && bps_ok) {
		/* the front end's settings are checked on the host, before any output file or the GPU: a refusal leaves nothing behind */
		mdemod_params in;
		memset(&in, 0, sizeof(in));
		in.samplerate = samplerate; in.symrate = (int)symrate; in.bps = bps; in.n_streams = 1;
		const int rc = mdemod_fe_design(&in, &fep, NULL, 0, NULL, NULL);
		if (rc != MDEMOD_OK) { fprintf(stderr, "--offset / --decimate: %s\n", why_of(rc)); LEAVE(1); }
	}

	for (int i = 0; i < n_files; i++) {
		if (stdout_mode) { io[i].out = stdout; continue; }
		if (n_files == 1 && output_fname) io[i].out_name = strdup(output_fname);
		else if (n_files == 1) {                                           /* utils.c:8: LRPT_%Y_%m_%d-%H_%M.s */
			char buf[64]; time_t t = time(NULL);
			strftime(buf, sizeof(buf), "LRPT_%Y_%m_%d-%H_%M.s", localtime(&t));
			io[i].out_name = strdup(buf);
		} else {
			io[i].out_name = malloc(strlen(io[i].in_name) + 3);
			sprintf(io[i].out_name, "%s.s", io[i].in_name);
		}
		io[i].out = fopen(io[i].out_name, "wb");
		if (!io[i].out) { fprintf(stderr, "Could not open output file\n"); LEAVE(1); }
	}

	int use_tui = 0;
#ifdef MDEMOD_TUI
	/* main.c:197: the display unless -B (or a mode that forces it); here also only when both ends are a terminal, or with --tui
	   (the reference draws into whatever stdout is) */
	if (!batch && !quiet && !tiled && bps_ok && (force_tui || (isatty(STDIN_FILENO) && isatty(STDOUT_FILENO))) && tui_open(update_interval) == 0) {
		use_tui = 1;
		say = tui_log;
	}
#endif
	if (!quiet)                                                                        /* main.c:200 */
		for (int i = 0; i < n_files; i++) say("Input: %s, output: %s\n", io[i].in_name, stdout_mode ? "(stdout)" : io[i].out_name);
	if (!quiet && auto_offsets)                                                        /* (the display's log when it is up: the chosen offset stays on screen) */
		for (int i = 0; i < n_files; i++) say("%s: LRPT found %+.1f Hz from the centre, front end /%d\n", io[i].in_name, auto_offsets[i], decimation);
	if (!bps_ok) {
		LEAVE(0);
	}
	/* file lengths for the progress figure of the status line (main.c:189-193) */
	for (int i = 0; i < n_files; i++) {
		if (io[i].in == stdin) continue;
		const long here = ftell(io[i].in);
		if (here < 0 || fseek(io[i].in, 0, SEEK_END)) continue;
		const long end = ftell(io[i].in);
		io[i].file_len = end > 0 ? (unsigned long)end : 0;
		fseek(io[i].in, here, SEEK_SET);
	}
	/* demod_init(pll_bw, SYM_BW, samplerate, symrate, interp, order, oqpsk, freq_max): main.c:187 */
	mdemod_params p;
	memset(&p, 0, sizeof(p));
	p.pll_bw = pll_bw; p.sym_bw = MDEMOD_DEFAULT_SYM_BW; p.samplerate = samplerate; p.symrate = (int)symrate;
	p.interp_factor = interp; p.rrc_order = rrc_order; p.oqpsk = oqpsk; p.freq_max = freq_max_delta;
	p.bps = bps; p.device = device; p.n_streams = (uint32_t)n_files;
	/* ---- one worker per GPU: file i on GPU i mod G (streams shard, nothing crosses GPUs) ---- */
	if (n_dev == 0) {
		/* (one file: one GPU, and no question to the HIP runtime before its input is being read - the runtime takes 50-100 ms to
		   come up, which --tiled hides behind the file read) */
		const int have = n_files < 2 ? 1 : mdemod_device_count();
		if (n_files < 2 || have < 2) { devs[0] = device; n_dev = 1; }
		else for (n_dev = 0; n_dev < have && n_dev < MAX_DEVICES; n_dev++) devs[n_dev] = n_dev;
	}
	if (n_dev > n_files) n_dev = n_files;
	ws = calloc((size_t)n_dev, sizeof(*ws));
	if (!ws) LEAVE(1);
	n_workers = n_dev;
	for (int d = 0; d < n_dev; d++) {
		struct worker *w = &ws[d];
		w->index = d; w->p = p; w->p.device = devs[d];
		w->tiled = tiled; w->quiet = quiet; w->batch = batch; w->update_interval = update_interval;
		w->tile_samples = tile_samples; w->pilot_margin = pilot_margin; w->carrier_seed = carrier_seed;
		w->tui = use_tui && d == 0;
		w->jobs = jobs;
		w->use_fe = use_fe; w->fe = fep;
		for (int i = d; i < n_files; i += n_dev) w->n_files++;
		w->io = calloc((size_t)w->n_files, sizeof(*w->io));
		if (!w->io) LEAVE(1);
		for (int i = d, k = 0; i < n_files; i += n_dev, k++) w->io[k] = io[i];
		if (auto_offsets && n_files > 1) {
			/* each file its own offset: the worker's share of the list, in the order of its streams */
			w->fe_offsets = calloc((size_t)w->n_files, sizeof(double));
			if (!w->fe_offsets) LEAVE(1);
			for (int i = d, k = 0; i < n_files; i += n_dev, k++) w->fe_offsets[k] = auto_offsets[i];
			w->fe.offset_hz = w->fe_offsets[0];
			w->fe.offsets_hz = w->fe_offsets;
		}
		w->p.n_streams = (uint32_t)w->n_files;
	}
	if (n_dev == 1) {
		worker_main(&ws[0]);
	} else {
		for (int d = 0; d < n_dev; d++)
			if (pthread_create(&ws[d].thr, NULL, worker_main, &ws[d])) { fprintf(stderr, "could not start the worker of device %d\n", devs[d]); for (int k = 0; k < d; k++) pthread_join(ws[k].thr, NULL); for (int i = 0; i < n_files; i++) { io[i].in = NULL; io[i].out = NULL; } LEAVE(1); }
		for (int d = 0; d < n_dev; d++) pthread_join(ws[d].thr, NULL);
	}
	int rc_all = 0;
	for (int d = 0; d < n_dev; d++) if (ws[d].rc > rc_all) rc_all = ws[d].rc;
	/* (the workers closed their files through their own copies of the stream_io entries: nothing of the originals is open any more) */
	for (int i = 0; i < n_files; i++) { io[i].in = NULL; io[i].out = NULL; }
	/* (the frames, the pictures and the maps are made here, one file after the other, after the workers have joined: what --mosaic
	   keeps of a file goes into that file's own entry, and nothing else touches it) */
	mdemod_image_result kept[MDEMOD_MOSAIC_MAX_PASSES];
	memset(kept, 0, sizeof kept);
	if ((want_cadu || want_vcdu || want_image) && rc_all == 0)
		for (int i = 0; i < n_files && rc_all == 0; i++) {
			struct vcdu_req one = vreq;
			if (mosaic_base) one.keep = &kept[i];
			rc_all = cadu_file(io[i].out_name, devs[i % n_dev], want_cadu, &one, want_diff, want_skew, want_int ? (uint32_t)int_delay : 0);
		}
	if (mosaic_base) {
		if (rc_all == 0 && vreq.polar) {
			/* (all passes on one polar grid instead of the latitude / longitude mosaic) */
			const mdemod_image_result *all[MDEMOD_POLAR_MAX_PASSES];
			for (int i = 0; i < n_files; i++) all[i] = &kept[i];
			rc_all = polar_files(mosaic_base, all, n_files, &vreq, devs[0]);
			for (int i = 0; i < n_files; i++) mdemod_image_free(&kept[i]);
		}
		else if (rc_all == 0) rc_all = mosaic_files(mosaic_base, kept, io, n_files, &vreq, devs[0]);
		else for (int i = 0; i < n_files; i++) mdemod_image_free(&kept[i]);
	}
	if (jpeg_req.quality && rc_all == 0)
		printf("--jpeg %u: %llu files, %llu bytes of pictures in, %llu bytes of JPEG out\n", jpeg_req.quality, jpeg_req.files, jpeg_req.bytes_in, jpeg_req.bytes_out);
	LEAVE(rc_all);
}
