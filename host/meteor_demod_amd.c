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

#include "cli_opts.h"
#include "cli_products.h"

/* What main's stages hand on to each other: the streams, what the inputs turned out to be, the front end, the workers. */
struct run {
	struct stream_io *io;                /* one per input file; the workers get copies */
	int         n_files;
	int         samplerate, bps, bps_ok; /* -s / --bps, or the WAV header's */
	mdemod_fe_params fep;
	double     *auto_offsets;            /* --offset auto: the offset chosen for each file */
	int         use_tui;
	struct worker *ws;
	int         n_workers, devs[MAX_DEVICES];
};

/* --plan: the sharding arithmetic, without touching files or GPUs: file i on the (i mod G)-th device of the list */
static int
print_plan(const struct cli_opts *o)
{
	if (!o->n_dev) return refused("--plan needs --devices\n");
	const int g = o->n_dev > o->n_files ? o->n_files : o->n_dev;
	for (int d = 0; d < g; d++) {
		printf("device %d:", o->devs[d]);
		for (int i = d; i < o->n_files; i += g) printf(" %s", o->files[i]);
		printf("\n");
	}
	return 0;
}

/* The input files opened and their headers read: the rate and the sample size of the run.  GO_ON, or the exit status. */
static int
open_inputs(const struct cli_opts *o, struct run *r)
{
	r->io = calloc((size_t)o->n_files, sizeof(*r->io));
	if (!r->io) return 1;
	r->n_files = o->n_files;
	r->samplerate = o->samplerate; r->bps = o->bps;
	for (int i = 0; i < r->n_files; i++) {
		struct stream_io *io = &r->io[i];
		io->in_name = o->files[i];
		io->in = !strcmp(io->in_name, "-") ? stdin : fopen(io->in_name, "rb");
		if (!io->in) return refused("Could not open input file\n");
		int sr = r->samplerate, b = r->bps;
		if (parse_wav(io->in, &sr, &b)) fseek(io->in, 0, SEEK_SET);        /* raw: main.c:164-166 */
		if (i == 0) { r->samplerate = sr; r->bps = b; }
		else if (sr != r->samplerate || b != r->bps) return refused("all inputs of a batch must share rate and format\n");
	}
	if (r->samplerate < 0) {
		fprintf(stderr, "Could not auto-detect sample rate. Please specify it with -s <samplerate>\n");
		usage(o->prog);                                                                /* main.c:170 */
		return 1;
	}
	if (!r->bps) { fprintf(stderr, "Could not auto-detect bits per sample, assuming 16\n"); r->bps = 16; }
	/* any other sample size: the reference's reader returns 0 on the first sample (wavfile.c:71-73) and it writes an empty
	 * output file; same here, without touching the GPU */
	r->bps_ok = (r->bps == 8 || r->bps == 16 || r->bps == 32);
	if (!r->bps_ok) fprintf(stderr, "%d bits per sample: nothing to demodulate (8, 16 or 32 expected)\n", r->bps);
	r->fep.offset_hz = o->offset_hz; r->fep.decimation = o->decimation; r->fep.taps_per_phase = 0;
	return GO_ON;
}

/* demod_init(pll_bw, SYM_BW, samplerate, symrate, interp, order, oqpsk, freq_max) for this run's inputs: main.c:187 */
static mdemod_params
demod_params(const struct cli_opts *o, const struct run *r, int device, int n_streams)
{
	mdemod_params p;
	memset(&p, 0, sizeof(p));
	p.pll_bw = o->pll_bw; p.sym_bw = MDEMOD_DEFAULT_SYM_BW; p.samplerate = r->samplerate; p.symrate = (int)o->symrate;
	p.interp_factor = o->interp; p.rrc_order = o->rrc_order; p.oqpsk = o->oqpsk; p.freq_max = o->freq_max_delta;
	p.bps = r->bps; p.device = device; p.n_streams = (uint32_t)n_streams;
	return p;
}

/* --offset auto / --decimate auto / --scan: the survey, before any output file exists, so that a file without a signal leaves nothing
 * behind: the decimation planned, every file's candidates printed (--scan) or its first confirmed signal's offset taken.  GO_ON, or
 * the exit status (--scan ends here). */
static int
survey(const struct cli_opts *o, struct run *r)
{
	if (!(o->auto_offset || o->auto_decimate || o->scan) || !r->bps_ok) return o->scan ? 0 : GO_ON;
	mdemod_params in = demod_params(o, r, o->n_dev ? o->devs[0] : o->device, 1);
	if (o->auto_decimate || (!o->decimate_given && (o->auto_offset || o->scan))) {
		const int rc = mdemod_survey_plan(&in, NULL, &r->fep.decimation);
		if (rc != MDEMOD_OK) { fprintf(stderr, "--decimate auto: %s\n", why_of(rc)); return 1; }
	}
	if (!o->auto_offset && !o->scan) return GO_ON;
	mdemod_survey_opts so;
	mdemod_survey_default_opts(&so);
	so.decimation = r->fep.decimation;
	r->auto_offsets = calloc((size_t)r->n_files, sizeof(*r->auto_offsets));
	if (!r->auto_offsets) return 1;
	for (int i = 0; i < r->n_files; i++) {
		mdemod_survey_hit hits[MDEMOD_SURVEY_MAX_CANDIDATES];
		uint32_t n_hits = 0;
		const char *name = r->io[i].in_name;
		const int rc = survey_file(&in, &so, &r->io[i], hits, &n_hits);
		if (rc == 1) return 1;
		if (rc) { fprintf(stderr, "%s: survey: %s\n", name, why_of(rc)); return 2; }
		if (o->scan) {
			if (r->n_files > 1) printf("# %s\n", name);
			for (uint32_t k = 0; k < n_hits; k++)
				printf("%.1f %.2f %.2f %.2f %d\n", round_offset(hits[k].offset_hz), hits[k].psd_snr_db, hits[k].clock_quality,
				       hits[k].carrier_quality, hits[k].confirmed);
			continue;
		}
		if (!n_hits || !hits[0].confirmed) {             /* (confirmed hits come first) */
			if (n_hits)
				fprintf(stderr, "%s: no LRPT signal of %d sym/s confirmed; the best candidate, at %+.1f Hz (%.1f dB over the floor), has a "
				        "symbol-rate line of quality %.1f\n", name, (int)o->symrate, hits[0].offset_hz, hits[0].psd_snr_db, hits[0].clock_quality);
			else
				fprintf(stderr, "%s: no LRPT signal of %d sym/s found: nothing stands out of the noise floor\n", name, (int)o->symrate);
			return 1;
		}
		r->auto_offsets[i] = round_offset(hits[0].offset_hz);
	}
	if (o->scan) return 0;
	r->fep.offset_hz = r->auto_offsets[0];
	return GO_ON;
}

/* The front end's settings are checked on the host, before any output file or the GPU: a refusal leaves nothing behind. */
static int
check_front_end(const struct cli_opts *o, const struct run *r)
{
	if (!o->use_fe || !r->bps_ok) return GO_ON;
	mdemod_params in;
	memset(&in, 0, sizeof(in));
	in.samplerate = r->samplerate; in.symrate = (int)o->symrate; in.bps = r->bps; in.n_streams = 1;
	const int rc = mdemod_fe_design(&in, &r->fep, NULL, 0, NULL, NULL);
	if (rc != MDEMOD_OK) { fprintf(stderr, "--offset / --decimate: %s\n", why_of(rc)); return 1; }
	return GO_ON;
}

/* The output files opened, the display brought up, the opening lines said, the inputs' lengths taken.  GO_ON, or the exit status. */
static int
open_outputs(const struct cli_opts *o, struct run *r)
{
	struct stream_io *io = r->io;
	const int n_files = r->n_files;
	for (int i = 0; i < n_files; i++) {
		if (o->stdout_mode) { io[i].out = stdout; continue; }
		if (n_files == 1 && o->output_fname) io[i].out_name = strdup(o->output_fname);
		else if (n_files == 1) {                                           /* utils.c:8: LRPT_%Y_%m_%d-%H_%M.s */
			char buf[64]; time_t t = time(NULL);
			strftime(buf, sizeof(buf), "LRPT_%Y_%m_%d-%H_%M.s", localtime(&t));
			io[i].out_name = strdup(buf);
		} else {
			io[i].out_name = malloc(strlen(io[i].in_name) + 3);
			sprintf(io[i].out_name, "%s.s", io[i].in_name);
		}
		io[i].out = fopen(io[i].out_name, "wb");
		if (!io[i].out) return refused("Could not open output file\n");
	}
#ifdef MDEMOD_TUI
	/* main.c:197: the display unless -B (or a mode that forces it); here also only when both ends are a terminal, or with --tui
	   (the reference draws into whatever stdout is) */
	if (!o->batch && !o->quiet && !o->tiled && r->bps_ok && (o->force_tui || (isatty(STDIN_FILENO) && isatty(STDOUT_FILENO))) && tui_open(o->update_interval) == 0) {
		r->use_tui = 1;
		say = tui_log;
	}
#endif
	if (!o->quiet)                                                                     /* main.c:200 */
		for (int i = 0; i < n_files; i++) say("Input: %s, output: %s\n", io[i].in_name, o->stdout_mode ? "(stdout)" : io[i].out_name);
	if (!o->quiet && r->auto_offsets)                                                  /* (the display's log when it is up: the chosen offset stays on screen) */
		for (int i = 0; i < n_files; i++) say("%s: LRPT found %+.1f Hz from the centre, front end /%d\n", io[i].in_name, r->auto_offsets[i], r->fep.decimation);
	if (!r->bps_ok) return 0;
	/* file lengths for the progress figure of the status line (main.c:189-193) */
	for (int i = 0; i < n_files; i++) {
		if (io[i].in == stdin) continue;
		const long here = ftell(io[i].in);
		if (here < 0 || fseek(io[i].in, 0, SEEK_END)) continue;
		const long end = ftell(io[i].in);
		io[i].file_len = end > 0 ? (unsigned long)end : 0;
		fseek(io[i].in, here, SEEK_SET);
	}
	return GO_ON;
}

/* One worker per GPU, file i on GPU i mod G (streams shard, nothing crosses GPUs): built, run and joined.  GO_ON when
 * every file is demodulated and closed, or the exit status. */
static int
run_workers(const struct cli_opts *o, struct run *r)
{
	const int n_files = r->n_files;
	int n_dev = o->n_dev;
	memcpy(r->devs, o->devs, sizeof r->devs);
	if (n_dev == 0) {
		/* (one file: one GPU, and no question to the HIP runtime before its input is being read - the runtime takes 50-100 ms to
		   come up, which --tiled hides behind the file read) */
		const int have = n_files < 2 ? 1 : mdemod_device_count();
		if (n_files < 2 || have < 2) { r->devs[0] = o->device; n_dev = 1; }
		else for (n_dev = 0; n_dev < have && n_dev < MAX_DEVICES; n_dev++) r->devs[n_dev] = n_dev;
	}
	if (n_dev > n_files) n_dev = n_files;
	r->ws = calloc((size_t)n_dev, sizeof(*r->ws));
	if (!r->ws) return 1;
	r->n_workers = n_dev;
	for (int d = 0; d < n_dev; d++) {
		struct worker *w = &r->ws[d];
		w->index = d;
		w->tiled = o->tiled; w->quiet = o->quiet; w->batch = o->batch; w->update_interval = o->update_interval;
		w->tile_samples = o->tile_samples; w->pilot_margin = o->pilot_margin; w->carrier_seed = o->carrier_seed;
		w->tui = r->use_tui && d == 0;
		w->jobs = o->jobs;
		w->use_fe = o->use_fe; w->fe = r->fep;
		for (int i = d; i < n_files; i += n_dev) w->n_files++;
		w->p = demod_params(o, r, r->devs[d], w->n_files);
		w->io = calloc((size_t)w->n_files, sizeof(*w->io));
		if (!w->io) return 1;
		for (int i = d, k = 0; i < n_files; i += n_dev, k++) w->io[k] = r->io[i];
		if (r->auto_offsets && n_files > 1) {
			/* each file its own offset: the worker's share of the list, in the order of its streams */
			w->fe_offsets = calloc((size_t)w->n_files, sizeof(double));
			if (!w->fe_offsets) return 1;
			for (int i = d, k = 0; i < n_files; i += n_dev, k++) w->fe_offsets[k] = r->auto_offsets[i];
			w->fe.offset_hz = w->fe_offsets[0];
			w->fe.offsets_hz = w->fe_offsets;
		}
	}
	int started = 0;
	if (n_dev == 1) worker_main(&r->ws[0]);
	else {
		for (; started < n_dev; started++) if (pthread_create(&r->ws[started].thr, NULL, worker_main, &r->ws[started])) break;
		if (started < n_dev) fprintf(stderr, "could not start the worker of device %d\n", r->devs[started]);
		for (int d = 0; d < started; d++) pthread_join(r->ws[d].thr, NULL);
	}
	/* (the workers closed their files through their own copies of the stream_io entries: nothing of the originals is open any more) */
	for (int i = 0; i < n_files; i++) { r->io[i].in = NULL; r->io[i].out = NULL; }
	if (n_dev > 1 && started < n_dev) return 1;
	int rc_all = 0;
	for (int d = 0; d < n_dev; d++) if (r->ws[d].rc > rc_all) rc_all = r->ws[d].rc;
	return rc_all ? rc_all : GO_ON;
}

/* The frames, the pictures and the maps, one file after the other, after the workers have joined (what --mosaic keeps of a file goes
 * into that file's own entry, and nothing else touches it); then the mosaic or the polar picture of all files, and the closing line
 * of --jpeg.  The exit status. */
static int
make_products(const struct cli_opts *o, struct products *pr, const struct run *r)
{
	const int n_files = r->n_files;
	int code = 0;
	mdemod_image_result kept[MDEMOD_MOSAIC_MAX_PASSES];
	memset(kept, 0, sizeof kept);
	pr->req.device = r->devs[0];                                                  /* (the mosaic is made on the first GPU) */
	if (pr->req.write_cadu || pr->req.write_vcdu || pr->req.image)
		for (int i = 0; i < n_files && code == 0; i++) {
			struct vcdu_req one = pr->req;
			one.device = r->devs[i % r->n_workers];
			if (o->mosaic_base) one.keep = &kept[i];
			code = cadu_file(r->io[i].out_name, &one);
		}
	if (o->mosaic_base && code == 0 && !pr->req.polar) code = mosaic_files(o->mosaic_base, kept, r->io, n_files, &pr->req);   /* (it frees what was kept) */
	else if (o->mosaic_base) {
		/* (all passes on one polar grid instead of the latitude / longitude mosaic) */
		const mdemod_image_result *all[MDEMOD_POLAR_MAX_PASSES];
		for (int i = 0; i < n_files; i++) all[i] = &kept[i];
		if (code == 0) code = polar_files(o->mosaic_base, all, n_files, &pr->req);
		for (int i = 0; i < n_files; i++) mdemod_image_free(&kept[i]);
	}
	if (pr->req.jpeg_quality && code == 0)
		printf("--jpeg %u: %llu files, %llu bytes of pictures in, %llu bytes of JPEG out\n", pr->req.jpeg_quality, pr->jpeg.files, pr->jpeg.bytes_in, pr->jpeg.bytes_out);
	return code;
}

/* every way out: files closed, nothing left allocated (the sanitizer builds of tests/test_sanitize.py look) */
static void
leave(struct run *r, struct products *pr)
{
	close_all(r->io, r->n_files);
	for (int d = 0; d < r->n_workers; d++) { free(r->ws[d].io); free(r->ws[d].fe_offsets); }
	free(r->ws);
	free(r->auto_offsets);
	for (int i = 0; i < r->n_files; i++) free(r->io[i].out_name);
	free(r->io);
	for (uint32_t k = 0; k < pr->overlay.n_files; k++) mdemod_overlay_vectors_free(&pr->overlay.coast[k]);
}

int
main(int argc, char **argv)
{
	struct cli_opts o;
	struct products pr;
	struct run r;
	memset(&r, 0, sizeof r);
	pr.overlay.n_files = 0;
	int code = parse_options(argc, argv, &o);
	if (code == GO_ON) code = check_options(&o, &pr);
	if (code == GO_ON && o.plan) code = print_plan(&o);
	if (code == GO_ON) code = open_inputs(&o, &r);
	if (code == GO_ON) code = survey(&o, &r);
	if (code == GO_ON) code = check_front_end(&o, &r);
	if (code == GO_ON) code = open_outputs(&o, &r);
	if (code == GO_ON) code = run_workers(&o, &r);
	if (code == GO_ON) code = make_products(&o, &pr, &r);
	leave(&r, &pr);
	return code;
}
