/*
 * vdl2hip_iqfile - minimal `dumpvdl2 --iq-file` work-alike on top of libvdl2hip.so (plain C host code).
 *
 * It reproduces the part of the reference's command line that feeds the hot path
 * (src/dumpvdl2.c:831-1099 option handling, :168-180 centre-frequency rule, :323-358 file loop):
 *   --iq-file <path|->            raw IQ file, read in FILE_BUFSIZE (320000-byte) blocks; sets oversample 10 and U8
 *   --blocks-per-feed <n>         how many of those blocks go to the GPU as one feed (default: as many as hold 64 000 decimated
 *                                 samples - 16 s16 blocks at oversample 20, 4 u8 blocks at 10; 1 = the reference's block by block).
 *                                 A block is microseconds of GPU work behind a fixed chain of launches (and, now and then, a 2 ms
 *                                 scan of the referee's): collected blocks give the same frames at 5-7x the rate
 *   --sample-format U8|S16_LE|CF32|S8  (the reference's token is S16_LE, src/dumpvdl2.c:849; CF32 - interleaved float32 I, Q, full scale 1.0,
 *                                 what GNU Radio file sinks and SoapySDR write - is this library's own, VDL2HIP_FMT_CF32; so is S8 - interleaved
 *                                 signed bytes, what hackrf_transfer writes and SigMF calls ci8, VDL2HIP_FMT_S8: a byte b counts b / 128)
 *   --sample-rate <Hz>            the rate of the file, where it is not 105000 * oversample (this library's own: the reference sets its
 *                                 radios to that rate and takes files at it).  The receiver resamples on the GPU, vdl2hip_cfg.input_rate;
 *                                 rates it does not take (vdl2hip.h) are refused
 *   --oversample <n>  --centerfreq <Hz>  --max-ppm <x>  --station-id <s>
 *   --avlc-filter                 deliver only frames that pass avlc_parse()'s first checks (length, FCS) - src/avlc.c:168-187
 *   --statsd-out <path>           at exit, write the per-channel counters in the reference's statsd names
 *                                 ("dumpvdl2[.<station-id>].<freq>.<counter>:<n>|c", src/statsd.c:34-65,153-160)
 *   --raw-frames-out <path>       write every frame in the reference's raw-frame archive format, so that a stock
 *                                 `dumpvdl2 --raw-frames-file <path>` decodes them through the full protocol stack
 *   --spectrum-out <path>         (this library's own) switch the input monitor on and, at exit, write what it saw of the file as fed: a
 *                                 "# key value" line per field of vdl2hip_spectrum_info, then "freq_hz dbfs" per bin, ascending; the
 *                                 per-channel summary lines gain " level=<x> dBFS" (vdl2hip_spectrum_channels)
 *   --spectrum-nfft <n>           bins: a power of two in 64 .. 4096 (default 1024)
 *   --spectrum-window rect|hann|bh4   (default hann)
 *   --activity-out <path>         (this library's own) switch the activity monitor on and, at exit, write what every channel carried: a
 *                                 "# key value" line per field of vdl2hip_activity_info, then per channel
 *                                 "freq_hz bins busy_bins occupancy transmissions longest_ms mean_dbfs max_dbfs p10_dbfs p50_dbfs"
 *                                 (the percentiles from the level histogram, as the centre of the 2 dB bucket); the per-channel
 *                                 summary lines gain " busy=<x>% tx=<n>"
 *   --activity-bin <samples>      bin length in decimated samples, 10 .. 10500 (default 105 = 1 ms)
 *   --activity-threshold <dBFS>   a bin above it is busy (default -40)
 *   --activity-hang <bins>        idle bins a transmission bridges, 0 .. 255 (default 0)
 *   --tx-out <path>               (this library's own) switch the transmission log on - and with it the activity monitor, which the
 *                                 --activity-* options above configure - and, at exit, write every transmission the channels carried,
 *                                 decoded or not: a "# key value" line per field of vdl2hip_txlog_info, then per transmission
 *                                 "chan freq_hz first_sample length_ms peak_dbfs mean_dbfs frames frames_ok flags", then per channel
 *                                 "# channel <chan> <freq_hz> transmissions=<n> decoded=<n> ratio=<decoded / transmissions>"
 *   --tx-search-out <path>        (this library's own) switch the preamble search on - and with it the transmission log and the activity
 *                                 monitor, as --tx-out does - and, at exit, write to a file of its own what the search found in every
 *                                 transmission: one line "# flags <f> records <n> samples_searched <n> clipped <n> kernel_ms <x>", then per
 *                                 transmission the fields of vdl2hip_tx_search in the structure's order - "chan freq first_bin search_first
 *                                 search_last best_sample first_lock best_pherr best_slope best_ppm lock_points below_thr lock_phases
 *                                 flags frames frames_ok why"
 *   --relook-out <path>           (this library's own) switch the second look on - and with it the preamble search, the transmission log
 *                                 and the activity monitor - and, at exit, write to a file of its own one line "# flags <f> threshold <x>
 *                                 max_anchors <n> records <n> anchors_found <n> attempts <n> frames <n> frames_ok <n> frames_new <n>
 *                                 dropped <n> kernel_ms <x>", then per attempt "chan freq first_bin anchor end_sample pherr slope ppm_error
 *                                 prev_phase tl_bits nsym synd_weight stop frames frames_ok frames_new fec_corrections flags"
 *   --relook-frames <path>        ... and write the NEW frames that pass the AVLC front door (frames of attempts the main path did not
 *                                 deliver) to a file of their own, in the raw-frame archive format of --output raw:binary:file.  They are
 *                                 never mixed into the main output: dumpvdl2, given the same IQ, does not deliver them
 *   --relook-threshold <x>        the anchors' threshold on the preamble metric (default 4, at most 30)
 *   --tx-capture-out <path>       (this library's own) switch the transmission capture on - and with it the transmission log and the activity
 *                                 monitor, as --tx-out does - and, at exit, write what every transmission looked like: two lines "# key value
 *                                 ..." with the fields of vdl2hip_txcap_info, then per transmission the fields of vdl2hip_tx_capture in the
 *                                 structure's order and the four figures of vdl2hip_txcap_measure() - "chan freq first_bin win_first win_last
 *                                 iq_off spec_off iq_count flags segments nfft frames frames_ok total peak_bin peak_hz centroid_hz obw_hz"
 *   --tx-iq <path>                the transmissions' IQ windows (256 samples ahead of the first busy bin, a bin behind the last) one after the
 *                                 other as cf32 at 105 kS/s; iq_off of a line is then the pair in this file its window begins at
 *   --tx-spectra <path>           their power spectra one after the other as float32, nfft values each, bin i at freq + (i - nfft / 2)
 *                                 105000 / nfft Hz; spec_off of a line is then the float in this file its spectrum begins at
 *   --tx-capture-undecoded-only   only the transmissions that produced no frame that passes the AVLC checks
 *   --tx-capture-nfft <n>         bins of a spectrum: 64, 128, 256, 512 or 1024 (default 256)
 *   --bursts-out <path>           (this library's own) switch the burst capture on and, at exit, write every burst handed to the burst decoder,
 *                                 decoded or not: a "# key value" line per field of vdl2hip_capture_info, then per burst every field of
 *                                 vdl2hip_burst in the structure's order - "chan freq burst_ord sync_sample end_sample first_symbol nsym
 *                                 tl_bits ppm_error dphi prev_phase flags iq_first iq_count iq_off frames frames_ok fec_corrections
 *                                 weak_symbols mean_power min_power max_power phase_err_rms phase_err_mean phase_err_max"
 *   --bursts-iq <path>            the bursts' IQ windows one after the other as cf32 (interleaved float32 I, Q at 105 kS/s); iq_off of a
 *                                 burst's line is then the pair in this file its window begins at (without the option: 0)
 *   --bursts-failed-only          only the bursts that produced no frame that passes the AVLC checks
 *   --bursts-pre <samples>        decimated samples kept ahead of the sync, 0 .. 4096 (default 256)
 *   --bursts-post <samples>       ... and behind the last symbol, 0 .. 1024 (default 32)
 *   --toa-out <path>              (this library's own) switch burst timing on and, at exit, write one CSV line per burst handed to the burst
 *                                 decoder, decoded or not: a "# key value" line per field of vdl2hip_toa_info, a header line, then
 *                                 "chan,freq,burst_ord,sync_sample,first_symbol,peak_sample,peak_lag,nlags,toa_frac,toa_sample,peak_power,
 *                                 energy,rho,carrier_phase,cfo_hz,dphi,resid,flags,frames,frames_ok" - toa_sample = peak_sample + toa_frac,
 *                                 the arrival of unique-word symbol 0's centre in decimated samples (105 000 a second) from the file's start
 *   --toa-max-lag <n>             lags searched on either side of the decoder's symbol clock, 1 .. 32 (default 8)
 *   freq [freq ...]               channel frequencies in Hz; default: the CSC, 136975000
 * and prints one line per AVLC frame (metadata in the reference's "[S:…] [L:…] [F:…] [#idx]" style + hex octets).
 * Everything after avlc_decoder_queue_push() (AVLC/ACARS/X.25/... decoding, formatters) is out of scope here.
 */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include "vdl2hip.h"

#define FILE_BUFSIZE 320000U        /* src/dumpvdl2.h:48 */
#define FILE_OVERSAMPLE 10          /* src/dumpvdl2.h:49 */
#define CSC_FREQ 136975000U         /* src/dumpvdl2.h:47 */
#define SYMBOL_RATE 10500

static FILE *raw_out;
static const char *station_id;
static unsigned long nframes;

/* the centre, in dBFS, of the level bucket that holds the bin of rank ceil(q bins) - bucket i spans -122 + 2 i .. -120 + 2 i dBFS */
static double hist_percentile(const vdl2hip_activity_chan *ch, double q) {
	uint64_t want = (uint64_t)ceil(q * (double)ch->bins), seen = 0;
	if(want < 1) want = 1;
	for(int i = 0; i < 64; i++) { seen += ch->hist[i]; if(seen >= want) return -121.0 + 2.0 * i; }
	return NAN;
}
static double dbfs_of(double p) { return p > 0.0 ? 10.0 * log10(p) : -INFINITY; }

/* burst capture: the records so far (written at exit, behind the totals), the IQ file as it grows */
static vdl2hip_burst *bursts;
static size_t nbursts, cap_bursts;
static FILE *bursts_iq;
static uint64_t bursts_iq_pairs;
static int take_bursts(vdl2hip_ctx *rx) {
	enum { RECS = 256, PAIRS = 1 << 18 };                                       /* (a window is shorter than 2^16 pairs) */
	static vdl2hip_burst rec[RECS];
	static float iq[2 * PAIRS];
	for(;;) {
		size_t used = 0;
		const int n = vdl2hip_capture_read(rx, rec, RECS, iq, PAIRS, &used);
		if(n <= 0) return n;
		if(nbursts + (size_t)n > cap_bursts) {
			cap_bursts = 2 * (nbursts + (size_t)n);
			bursts = realloc(bursts, cap_bursts * sizeof *bursts);
			if(!bursts) { perror("realloc"); exit(3); }
		}
		for(int i = 0; i < n; i++) {
			rec[i].iq_off = bursts_iq ? bursts_iq_pairs + rec[i].iq_off : 0;
			bursts[nbursts++] = rec[i];
		}
		if(bursts_iq) { fwrite(iq, 2 * sizeof(float), used, bursts_iq); bursts_iq_pairs += used; }
	}
}

/* burst timing: the records so far (written at exit, behind the totals); the curves are not kept */
static vdl2hip_burst_toa *toas;
static size_t ntoas, cap_toas;
static int take_toa(vdl2hip_ctx *rx) {
	enum { RECS = 256 };
	static vdl2hip_burst_toa rec[RECS];
	static float curves[RECS * 65];
	for(;;) {
		const int n = vdl2hip_toa_read(rx, rec, RECS, curves, RECS * 65, NULL);
		if(n <= 0) return n;
		if(ntoas + (size_t)n > cap_toas) {
			cap_toas = 2 * (ntoas + (size_t)n);
			toas = realloc(toas, cap_toas * sizeof *toas);
			if(!toas) { perror("realloc"); exit(3); }
		}
		for(int i = 0; i < n; i++) toas[ntoas++] = rec[i];
	}
}

/* transmission log: the records so far (written at exit, behind the totals) */
static vdl2hip_tx *txs;
static size_t ntxs, cap_txs;
static int take_tx(vdl2hip_ctx *rx) {
	enum { RECS = 256 };
	static vdl2hip_tx rec[RECS];
	for(;;) {
		const int n = vdl2hip_txlog_read(rx, rec, RECS);
		if(n <= 0) return n;
		if(ntxs + (size_t)n > cap_txs) {
			cap_txs = 2 * (ntxs + (size_t)n);
			txs = realloc(txs, cap_txs * sizeof *txs);
			if(!txs) { perror("realloc"); exit(3); }
		}
		memcpy(txs + ntxs, rec, (size_t)n * sizeof *rec);
		ntxs += (size_t)n;
	}
}

/* preamble search: the records so far (written at exit, behind the totals) */
static vdl2hip_tx_search *txss;
static size_t ntxss, cap_txss;
static int take_tx_search(vdl2hip_ctx *rx) {
	enum { RECS = 256 };
	static vdl2hip_tx_search rec[RECS];
	for(;;) {
		const int n = vdl2hip_txsearch_read(rx, rec, RECS);
		if(n <= 0) return n;
		if(ntxss + (size_t)n > cap_txss) {
			cap_txss = 2 * (ntxss + (size_t)n);
			txss = realloc(txss, cap_txss * sizeof *txss);
			if(!txss) { perror("realloc"); exit(3); }
		}
		memcpy(txss + ntxss, rec, (size_t)n * sizeof *rec);
		ntxss += (size_t)n;
	}
}
/* second look: the attempt records so far (written at exit, behind the totals); the NEW good frames go to their own archive as they come */
static vdl2hip_relook *rls;
static size_t nrls, cap_rls;
static FILE *relook_frames;
static int take_relook(vdl2hip_ctx *rx) {
	enum { RECS = 64, FRAMES = 1024, OCTETS = 1 << 20 };
	static vdl2hip_relook rec[RECS];
	static vdl2hip_packed_frame fr[FRAMES];
	static uint8_t oct[OCTETS];
	for(;;) {
		size_t used = 0;
		const int n = vdl2hip_relook_read(rx, rec, RECS, fr, FRAMES, oct, OCTETS, &used);
		if(n <= 0) return n;
		if(nrls + (size_t)n > cap_rls) {
			cap_rls = 2 * (nrls + (size_t)n);
			rls = realloc(rls, cap_rls * sizeof *rls);
			if(!rls) { perror("realloc"); exit(3); }
		}
		memcpy(rls + nrls, rec, (size_t)n * sizeof *rec);
		nrls += (size_t)n;
		for(int i = 0; relook_frames && i < n; i++) {
			if(rec[i].frames_new == 0) continue;
			/* (new_mask names the NEW good frames among an attempt's first 32; beyond that only an attempt all of whose good frames are new is taken) */
			for(uint32_t k = 0; k < rec[i].frames; k++) {
				vdl2hip_frame f = fr[rec[i].frame_first + k].frame;
				const int is_new = k < 32 ? (int)((rec[i].new_mask >> k) & 1u) : rec[i].frames_new == rec[i].frames_ok;
				if(f.avlc_status != VDL2HIP_AVLC_OK || !is_new) continue;
				f.octets = oct + fr[rec[i].frame_first + k].octets_off;
				f.nf_pwr_dbfs = f.frame_pwr_dbfs;                        /* (the archive has no way to say "unknown": SNR 0) */
				static uint8_t out[70000];
				struct timeval tv; gettimeofday(&tv, NULL);
				const int m = vdl2hip_pack_raw_frame(&f, station_id, tv.tv_sec, tv.tv_usec, out, sizeof out);
				if(m > 0) fwrite(out, 1, (size_t)m, relook_frames);
				else fprintf(stderr, "second-look frame not archived: %s\n", vdl2hip_strerror(m));
			}
		}
	}
}
/* transmission capture: the records so far with the four figures of each spectrum (written at exit, behind the totals), the IQ and
 * the spectra files as they grow - raw float32, record i's at iq_off pairs / spec_off floats */
typedef struct { vdl2hip_tx_capture r; vdl2hip_tx_shape shape; } tx_cap_row;
static tx_cap_row *txcs;
static size_t ntxcs, cap_txcs;
static FILE *txc_iq, *txc_spectra;
static uint64_t txc_iq_pairs, txc_spec_floats;
static int take_tx_capture(vdl2hip_ctx *rx) {
	enum { RECS = 256, PAIRS = 1 << 18, FLOATS = 1 << 18 };                     /* (a window is shorter than 2^16 pairs, a spectrum 1024 floats at the most) */
	static vdl2hip_tx_capture rec[RECS];
	static float iq[2 * PAIRS], sp[FLOATS];
	for(;;) {
		size_t used = 0, fused = 0;
		const int n = vdl2hip_txcap_read(rx, rec, RECS, iq, PAIRS, &used, sp, FLOATS, &fused);
		if(n <= 0) return n;
		if(ntxcs + (size_t)n > cap_txcs) {
			cap_txcs = 2 * (ntxcs + (size_t)n);
			txcs = realloc(txcs, cap_txcs * sizeof *txcs);
			if(!txcs) { perror("realloc"); exit(3); }
		}
		for(int i = 0; i < n; i++) {
			tx_cap_row *row = &txcs[ntxcs++];
			memset(row, 0, sizeof *row);
			const int has = rec[i].nfft && !(rec[i].flags & VDL2HIP_TXC_NO_SPECTRUM);
			if(has) (void)vdl2hip_txcap_measure(sp + rec[i].spec_off, rec[i].nfft, &row->shape);
			rec[i].iq_off = txc_iq ? txc_iq_pairs + rec[i].iq_off : 0;
			rec[i].spec_off = txc_spectra && has ? txc_spec_floats + rec[i].spec_off : 0;
			row->r = rec[i];
		}
		if(txc_iq) { fwrite(iq, 2 * sizeof(float), used, txc_iq); txc_iq_pairs += used; }
		if(txc_spectra) { fwrite(sp, sizeof(float), fused, txc_spectra); txc_spec_floats += fused; }
	}
}
/* ... without --tx-out the log's own records are read and let go, so that they do not pile up */
static int drop_tx(vdl2hip_ctx *rx) {
	static vdl2hip_tx rec[256];
	for(;;) { const int n = vdl2hip_txlog_read(rx, rec, 256); if(n <= 0) return n; }
}

/* --waterfall-mean / --waterfall-max: the spectrogram's lines completed since the last call, appended as raw float32, nfft values per
 * line - after every drain, so that the ring never has to hold the whole file */
static FILE *wf_mean, *wf_max;
static int64_t wf_next;
static int take_lines(vdl2hip_ctx *rx) {
	static float mean[16 * 4096], max[16 * 4096];
	vdl2hip_specgram_info gi;
	memset(&gi, 0, sizeof gi); gi.struct_size = sizeof gi;
	int n = vdl2hip_specgram_read(rx, &gi, NULL, NULL, 0, 0);
	if(n < 0) return n;
	const size_t nfft = (size_t)n, room = sizeof mean / sizeof mean[0] / nfft;
	while((uint64_t)wf_next < gi.lines) {
		n = vdl2hip_specgram_lines(rx, wf_next, wf_mean ? mean : NULL, wf_max ? max : NULL, room);
		if(n <= 0) return n < 0 ? n : VDL2HIP_E_INVAL;
		if(wf_mean) fwrite(mean, sizeof(float), (size_t)n * nfft, wf_mean);
		if(wf_max) fwrite(max, sizeof(float), (size_t)n * nfft, wf_max);
		wf_next += n;
	}
	return 0;
}

static void on_frame(const vdl2hip_frame *f, void *user) {
	(void)user;
	nframes++;
	printf("%u Hz [%.1f/%.1f dBFS] [%.1f dB] [%.1f ppm] [S:%u] [L:%u] [F:%d] [#%d] len=%u ",
			f->freq, f->frame_pwr_dbfs, f->nf_pwr_dbfs, f->frame_pwr_dbfs - f->nf_pwr_dbfs, f->ppm_error,
			f->synd_weight, f->datalen_octets, f->num_fec_corrections, f->idx, f->len);
	for(uint32_t i = 0; i < f->len; i++) printf("%02x", f->octets[i]);
	printf("\n");
	if(raw_out) {
		static uint8_t rec[70000];
		struct timeval tv; gettimeofday(&tv, NULL);
		int n = vdl2hip_pack_raw_frame(f, station_id, tv.tv_sec, tv.tv_usec, rec, sizeof rec);
		if(n > 0) fwrite(rec, 1, (size_t)n, raw_out);
		else fprintf(stderr, "frame not archived: %s\n", vdl2hip_strerror(n));
	}
}

int main(int argc, char **argv) {
	const char *infile = NULL, *rawpath = NULL, *statsd_path = NULL, *spectrum_path = NULL;
	uint32_t spectrum_nfft = 1024, spectrum_window = VDL2HIP_WIN_HANN;
	const char *waterfall_path = NULL, *wf_mean_path = NULL, *wf_max_path = NULL;
	uint32_t waterfall_segments = 0;
	const char *activity_path = NULL;
	uint32_t activity_bin = 105, activity_hang = 0; float activity_thr = -40.f;
	const char *bursts_path = NULL, *bursts_iq_path = NULL, *tx_path = NULL, *tx_search_path = NULL;
	const char *relook_path = NULL, *relook_frames_path = NULL; float relook_thr = 0.f;
	const char *tx_capture_path = NULL, *tx_iq_path = NULL, *tx_spectra_path = NULL;
	uint32_t tx_capture_flags = VDL2HIP_TXCAP_SPECTRUM, tx_capture_nfft = 0;
	uint32_t bursts_pre = 256, bursts_post = 32, bursts_flags = 0;
	const char *toa_path = NULL;
	uint32_t toa_max_lag = 0;
	int avlc_filter = 0;
	uint32_t per_feed = 0;
	uint32_t oversample = 0, centerfreq = 0, fmt = VDL2HIP_FMT_U8, freqs[1024], nfreq = 0, input_rate = 0;
	float max_ppm = 0.f;
	int fmt_set = 0;
	for(int i = 1; i < argc; i++) {
		const char *a = argv[i];
		#define NEEDARG() do { if(i + 1 >= argc) { fprintf(stderr, "%s needs an argument\n", a); return 1; } } while(0)
		if(!strcmp(a, "--iq-file")) { NEEDARG(); infile = argv[++i]; if(!oversample) oversample = FILE_OVERSAMPLE; }
		else if(!strcmp(a, "--sample-format")) {
			NEEDARG(); i++; fmt_set = 1;
			if(!strcmp(argv[i], "U8")) fmt = VDL2HIP_FMT_U8;
			else if(!strcmp(argv[i], "S16_LE")) fmt = VDL2HIP_FMT_S16LE;
			else if(!strcmp(argv[i], "CF32")) fmt = VDL2HIP_FMT_CF32;
			else if(!strcmp(argv[i], "S8")) fmt = VDL2HIP_FMT_S8;
			else { fprintf(stderr, "Unknown sample format\n"); return 1; }
		}
		else if(!strcmp(a, "--sample-rate")) { NEEDARG(); input_rate = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--oversample")) { NEEDARG(); oversample = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--centerfreq")) { NEEDARG(); centerfreq = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--max-ppm")) { NEEDARG(); max_ppm = strtof(argv[++i], NULL); }
		else if(!strcmp(a, "--station-id")) { NEEDARG(); station_id = argv[++i]; }
		else if(!strcmp(a, "--raw-frames-out")) { NEEDARG(); rawpath = argv[++i]; }
		else if(!strcmp(a, "--statsd-out")) { NEEDARG(); statsd_path = argv[++i]; }
		else if(!strcmp(a, "--avlc-filter")) avlc_filter = 1;
		else if(!strcmp(a, "--spectrum-out")) { NEEDARG(); spectrum_path = argv[++i]; }
		else if(!strcmp(a, "--spectrum-nfft")) { NEEDARG(); spectrum_nfft = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--spectrum-window")) {
			NEEDARG(); i++;
			if(!strcmp(argv[i], "rect")) spectrum_window = VDL2HIP_WIN_RECT;
			else if(!strcmp(argv[i], "hann")) spectrum_window = VDL2HIP_WIN_HANN;
			else if(!strcmp(argv[i], "bh4")) spectrum_window = VDL2HIP_WIN_BH4;
			else { fprintf(stderr, "Unknown spectrum window\n"); return 1; }
		}
		else if(!strcmp(a, "--waterfall-out")) { NEEDARG(); waterfall_path = argv[++i]; }
		else if(!strcmp(a, "--waterfall-segments")) { NEEDARG(); waterfall_segments = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--waterfall-mean")) { NEEDARG(); wf_mean_path = argv[++i]; }
		else if(!strcmp(a, "--waterfall-max")) { NEEDARG(); wf_max_path = argv[++i]; }
		else if(!strcmp(a, "--activity-out")) { NEEDARG(); activity_path = argv[++i]; }
		else if(!strcmp(a, "--activity-bin")) { NEEDARG(); activity_bin = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--activity-threshold")) { NEEDARG(); activity_thr = strtof(argv[++i], NULL); }
		else if(!strcmp(a, "--activity-hang")) { NEEDARG(); activity_hang = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--tx-out")) { NEEDARG(); tx_path = argv[++i]; }
		else if(!strcmp(a, "--tx-search-out")) { NEEDARG(); tx_search_path = argv[++i]; }
		else if(!strcmp(a, "--relook-out")) { NEEDARG(); relook_path = argv[++i]; }
		else if(!strcmp(a, "--relook-frames")) { NEEDARG(); relook_frames_path = argv[++i]; }
		else if(!strcmp(a, "--relook-threshold")) { NEEDARG(); relook_thr = (float)atof(argv[++i]); }
		else if(!strcmp(a, "--tx-capture-out")) { NEEDARG(); tx_capture_path = argv[++i]; }
		else if(!strcmp(a, "--tx-iq")) { NEEDARG(); tx_iq_path = argv[++i]; tx_capture_flags |= VDL2HIP_TXCAP_IQ; }
		else if(!strcmp(a, "--tx-spectra")) { NEEDARG(); tx_spectra_path = argv[++i]; }
		else if(!strcmp(a, "--tx-capture-undecoded-only")) tx_capture_flags |= VDL2HIP_TXCAP_UNDECODED_ONLY;
		else if(!strcmp(a, "--tx-capture-nfft")) { NEEDARG(); tx_capture_nfft = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--toa-out")) { NEEDARG(); toa_path = argv[++i]; }
		else if(!strcmp(a, "--toa-max-lag")) { NEEDARG(); toa_max_lag = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--bursts-out")) { NEEDARG(); bursts_path = argv[++i]; }
		else if(!strcmp(a, "--bursts-iq")) { NEEDARG(); bursts_iq_path = argv[++i]; }
		else if(!strcmp(a, "--bursts-failed-only")) bursts_flags |= VDL2HIP_CAPTURE_FAILED_ONLY;
		else if(!strcmp(a, "--bursts-pre")) { NEEDARG(); bursts_pre = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--bursts-post")) { NEEDARG(); bursts_post = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(!strcmp(a, "--blocks-per-feed")) { NEEDARG(); per_feed = (uint32_t)strtoul(argv[++i], NULL, 10); }
		else if(a[0] == '-' && a[1]) { fprintf(stderr, "unknown option %s\n", a); return 1; }
		else if(nfreq < 1024) freqs[nfreq++] = (uint32_t)strtoul(a, NULL, 10);
	}
	(void)fmt_set;
	if(!infile) { fprintf(stderr, "usage: %s --iq-file <file|-> [--sample-format U8|S16_LE|CF32|S8] [--sample-rate Hz] [--oversample n] [--centerfreq Hz] "
			"[--max-ppm x] [--station-id s] [--raw-frames-out file] [--avlc-filter] [--statsd-out file] [--blocks-per-feed n] "
			"[--spectrum-out file] [--spectrum-nfft n] [--spectrum-window rect|hann|bh4] "
			"[--waterfall-out file] [--waterfall-segments R] [--waterfall-mean file] [--waterfall-max file] "
			"[--activity-out file] [--activity-bin samples] [--activity-threshold dBFS] [--activity-hang bins] [--tx-out file] [--tx-search-out file] [--relook-out file] [--relook-frames file] [--relook-threshold x] "
			"[--tx-capture-out file] [--tx-iq file] [--tx-spectra file] [--tx-capture-undecoded-only] [--tx-capture-nfft n] "
			"[--bursts-out file] [--bursts-iq file] [--bursts-failed-only] [--bursts-pre samples] [--bursts-post samples] [--toa-out file] [--toa-max-lag n] [freq ...]\n", argv[0]); return 1; }
	if(nfreq == 0) {
		fprintf(stderr, "Warning: frequency not set - using VDL2 Common Signalling Channel as a default (%u Hz)\n", CSC_FREQ);
		freqs[nfreq++] = CSC_FREQ;
	}
	const uint32_t sample_rate = SYMBOL_RATE * 10u * oversample;             /* src/dumpvdl2.c:1073 */
	fprintf(stderr, "Sampling rate set to %u sps\n", sample_rate);
	if(input_rate && input_rate != sample_rate) fprintf(stderr, "Input at %u sps is resampled to that rate\n", input_rate);
	if(centerfreq == 0) {                                                      /* calc_centerfreq(), src/dumpvdl2.c:168-180 */
		uint32_t lo = freqs[0], hi = freqs[0];
		for(uint32_t i = 0; i < nfreq; i++) { if(freqs[i] < lo) lo = freqs[i]; if(freqs[i] > hi) hi = freqs[i]; }
		if(hi - lo > sample_rate - SYMBOL_RATE * 4) { fprintf(stderr, "Error: given frequencies are too far apart\n"); return 2; }
		centerfreq = lo + (hi - lo) / 2;
	}
	FILE *f = !strcmp(infile, "-") ? stdin : fopen(infile, "r");
	if(!f) { perror("Could not open input file"); return 2; }
	if(rawpath && !(raw_out = fopen(rawpath, "w"))) { perror("Could not open raw frames output"); return 2; }
	if(bursts_iq_path && !bursts_path) { fprintf(stderr, "--bursts-iq needs --bursts-out\n"); return 1; }
	if(bursts_iq_path && !(bursts_iq = fopen(bursts_iq_path, "w"))) { perror("Could not open bursts IQ output"); return 2; }
	if((tx_iq_path || tx_spectra_path) && !tx_capture_path) { fprintf(stderr, "--tx-iq and --tx-spectra need --tx-capture-out\n"); return 1; }
	if(tx_iq_path && !(txc_iq = fopen(tx_iq_path, "w"))) { perror("Could not open transmission IQ output"); return 2; }
	if(tx_spectra_path && !(txc_spectra = fopen(tx_spectra_path, "w"))) { perror("Could not open transmission spectra output"); return 2; }

	vdl2hip_cfg cfg;
	memset(&cfg, 0, sizeof cfg);
	cfg.struct_size = sizeof cfg; cfg.centerfreq = centerfreq; cfg.oversample = oversample; cfg.sample_fmt = fmt;
	if(per_feed == 0) {
		const uint32_t blk = FILE_BUFSIZE / (fmt == VDL2HIP_FMT_CF32 ? 8u : fmt == VDL2HIP_FMT_S16LE ? 4u : 2u);                   /* samples per block (U8, S8: 2 bytes) */
		const uint32_t dec = (uint32_t)((uint64_t)blk * (SYMBOL_RATE * 10u) / (input_rate ? input_rate : sample_rate));              /* decimated samples per block */
		per_feed = dec ? (64000u + dec - 1) / dec : 1;
	}
	if(per_feed > 64) per_feed = 64;
	cfg.nchan = nfreq; cfg.freqs = freqs; cfg.max_ppm = max_ppm; cfg.device = 0; cfg.max_block_bytes = (size_t)per_feed * FILE_BUFSIZE;
	cfg.input_rate = input_rate;
	vdl2hip_ctx *rx = NULL;
	int r = vdl2hip_create(&cfg, &rx);
	if(r != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_create: %s\n", vdl2hip_strerror(r)); return 3; }

	if(avlc_filter) vdl2hip_set_avlc_filter(rx, 1);
	const int waterfall = waterfall_path || wf_mean_path || wf_max_path;
	if(spectrum_path || waterfall) {                                           /* (the spectrogram sits on top of the input monitor) */
		vdl2hip_spectrum_cfg sc = { sizeof sc, spectrum_nfft, spectrum_window, 1 };
		if(spectrum_nfft == 0 || (r = vdl2hip_spectrum_enable(rx, &sc)) != VDL2HIP_OK) {
			fprintf(stderr, "vdl2hip_spectrum_enable: %s\n", vdl2hip_strerror(spectrum_nfft ? r : VDL2HIP_E_INVAL)); return 3;
		}
	}
	if(waterfall) {
		vdl2hip_specgram_cfg gc = { sizeof gc, waterfall_segments, 0, 0 };
		if((r = vdl2hip_specgram_enable(rx, &gc)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_specgram_enable: %s\n", vdl2hip_strerror(r)); return 3; }
		if(wf_mean_path && !(wf_mean = fopen(wf_mean_path, "w"))) { perror("Could not open waterfall mean output"); return 2; }
		if(wf_max_path && !(wf_max = fopen(wf_max_path, "w"))) { perror("Could not open waterfall max output"); return 2; }
	}
	const int relook = relook_path || relook_frames_path, search = tx_search_path || relook;
	if(activity_path || tx_path || search || tx_capture_path) {
		vdl2hip_activity_cfg ac = { sizeof ac, activity_bin, activity_hang, 0, activity_thr, 0 };
		if(activity_bin == 0 || (r = vdl2hip_activity_enable(rx, &ac)) != VDL2HIP_OK) {
			fprintf(stderr, "vdl2hip_activity_enable: %s\n", vdl2hip_strerror(activity_bin ? r : VDL2HIP_E_INVAL)); return 3;
		}
	}
	if(tx_path || search || tx_capture_path) {
		vdl2hip_txlog_cfg tc = { sizeof tc, 0, 0, 0 };
		if((r = vdl2hip_txlog_enable(rx, &tc)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_txlog_enable: %s\n", vdl2hip_strerror(r)); return 3; }
	}
	if(search) {
		vdl2hip_txsearch_cfg sc = { sizeof sc, 0, { 0, 0 } };
		if((r = vdl2hip_txsearch_enable(rx, &sc)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_txsearch_enable: %s\n", vdl2hip_strerror(r)); return 3; }
	}
	if(relook) {
		vdl2hip_relook_cfg lc = { sizeof lc, 0, relook_thr, 0.f, 0, 0, 0, 0 };
		if((r = vdl2hip_relook_enable(rx, &lc)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_relook_enable: %s\n", vdl2hip_strerror(r)); return 3; }
		if(relook_frames_path && !(relook_frames = fopen(relook_frames_path, "wb"))) { perror("Could not open second-look frames output"); return 2; }
	}
	if(tx_capture_path) {
		/* (post: a bin's worth behind the last busy bin, which the record's feed always holds) */
		vdl2hip_txcap_cfg xc = { sizeof xc, tx_capture_flags, 256, activity_bin, 0, tx_capture_nfft, VDL2HIP_WIN_HANN, 0, 0, 0 };
		if((r = vdl2hip_txcap_enable(rx, &xc)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_txcap_enable: %s\n", vdl2hip_strerror(r)); return 3; }
	}
	if(bursts_path) {
		vdl2hip_capture_cfg cc = { sizeof cc, bursts_pre, bursts_post, bursts_flags, 0, 0 };
		if((r = vdl2hip_capture_enable(rx, &cc)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_capture_enable: %s\n", vdl2hip_strerror(r)); return 3; }
	}
	if(toa_path) {
		vdl2hip_toa_cfg tc = { sizeof tc, toa_max_lag, 0, 0 };
		if((r = vdl2hip_toa_enable(rx, &tc)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_toa_enable: %s\n", vdl2hip_strerror(r)); return 3; }
	}

	unsigned char *buf = malloc((size_t)per_feed * FILE_BUFSIZE);
	if(!buf) { perror("malloc"); return 3; }
	size_t len, held = 0;
	if(per_feed > 1) vdl2hip_set_drain_lag(rx, 2);                              /* the frames of a feed are printed while the next two are on the GPU */
	do {                                                                        /* process_iq_file(), src/dumpvdl2.c:353-356 */
		len = fread(buf + held, 1, FILE_BUFSIZE, f);
		held += len;
		if(held + FILE_BUFSIZE <= (size_t)per_feed * FILE_BUFSIZE && len == FILE_BUFSIZE) continue;      /* room for another block, and there may be one */
		if(len != FILE_BUFSIZE) vdl2hip_set_drain_lag(rx, 0);                   /* the last feed: every frame out */
		if((r = vdl2hip_feed(rx, buf, held)) != VDL2HIP_OK) { fprintf(stderr, "vdl2hip_feed: %s\n", vdl2hip_strerror(r)); return 3; }
		if((r = vdl2hip_drain(rx, on_frame, NULL)) < 0) { fprintf(stderr, "vdl2hip_drain: %s\n", vdl2hip_strerror(r)); return 3; }
		if((wf_mean || wf_max) && (r = take_lines(rx)) < 0) { fprintf(stderr, "vdl2hip_specgram_lines: %s\n", vdl2hip_strerror(r)); return 3; }
		if(bursts_path && (r = take_bursts(rx)) < 0) { fprintf(stderr, "vdl2hip_capture_read: %s\n", vdl2hip_strerror(r)); return 3; }
		if(toa_path && (r = take_toa(rx)) < 0) { fprintf(stderr, "vdl2hip_toa_read: %s\n", vdl2hip_strerror(r)); return 3; }
		if(tx_path && (r = take_tx(rx)) < 0) { fprintf(stderr, "vdl2hip_txlog_read: %s\n", vdl2hip_strerror(r)); return 3; }
		if((search || tx_capture_path) && !tx_path && (r = drop_tx(rx)) < 0) { fprintf(stderr, "vdl2hip_txlog_read: %s\n", vdl2hip_strerror(r)); return 3; }
		if(search && (r = take_tx_search(rx)) < 0) { fprintf(stderr, "vdl2hip_txsearch_read: %s\n", vdl2hip_strerror(r)); return 3; }
		if(relook && (r = take_relook(rx)) < 0) { fprintf(stderr, "vdl2hip_relook_read: %s\n", vdl2hip_strerror(r)); return 3; }
		if(tx_capture_path && (r = take_tx_capture(rx)) < 0) { fprintf(stderr, "vdl2hip_txcap_read: %s\n", vdl2hip_strerror(r)); return 3; }
		held = 0;
	} while(len == FILE_BUFSIZE);
	free(buf);
	uint64_t cnt[VDL2HIP_NUM_COUNTERS];
	static float level[1024];
	const int have_levels = spectrum_path && vdl2hip_spectrum_channels(rx, level, 1024) == (int)nfreq;
	static float wf_peak[1024], wf_floor[1024];
	const int have_holds = waterfall && vdl2hip_specgram_channels(rx, wf_peak, wf_floor, 1024) == (int)nfreq;
	static vdl2hip_activity_chan act[1024];
	vdl2hip_activity_info ai;
	memset(&ai, 0, sizeof ai); ai.struct_size = sizeof ai;
	const int nact = activity_path ? vdl2hip_activity_read(rx, &ai, act, 1024, 0) : 0;
	for(uint32_t c = 0; c < nfreq; c++)
		if(vdl2hip_counters(rx, c, cnt) == VDL2HIP_OK) {
			fprintf(stderr, "%u Hz: sync.good=%" PRIu64 " crc.good=%" PRIu64 " blocks=%" PRIu64 "/%" PRIu64 " msg.good=%" PRIu64 " fec_bad=%" PRIu64,
					freqs[c], cnt[VDL2HIP_CNT_SYNC_GOOD], cnt[VDL2HIP_CNT_CRC_GOOD], cnt[VDL2HIP_CNT_BLOCKS_FEC_OK],
					cnt[VDL2HIP_CNT_BLOCKS_PROCESSED], cnt[VDL2HIP_CNT_MSG_GOOD], cnt[VDL2HIP_CNT_ERR_FEC_BAD]);
			if(have_levels) fprintf(stderr, " level=%.2f dBFS", (double)level[c]);
			if(have_holds) fprintf(stderr, " peak=%.2f dBFS floor=%.2f dBFS", (double)wf_peak[c], (double)wf_floor[c]);
			if(nact == (int)nfreq) fprintf(stderr, " busy=%.2f%% tx=%" PRIu64, act[c].bins ? 100.0 * (double)act[c].busy_bins / (double)act[c].bins : 0.0, act[c].transmissions);
			fprintf(stderr, "\n");
		}
	fprintf(stderr, "%lu frames\n", nframes);
	{
		vdl2hip_stats st;                                                       /* the drain calls only count buffer overflows: say so */
		if(vdl2hip_get_stats(rx, &st) == VDL2HIP_OK && st.overflow_feeds)
			fprintf(stderr, "warning: device output buffers overflowed in %llu block(s): frames were dropped\n", (unsigned long long)st.overflow_feeds);
	}
	if(spectrum_path) {
		static double power[4096];
		vdl2hip_spectrum_info si;
		memset(&si, 0, sizeof si); si.struct_size = sizeof si;
		int n = vdl2hip_spectrum_read(rx, &si, power, 4096, 0);
		FILE *so = n > 0 ? fopen(spectrum_path, "w") : NULL;
		if(so) {
			fprintf(so, "# nfft %u\n# window %u\n# stride %u\n# sample_rate %u\n# centerfreq %u\n", si.nfft, si.window, si.stride, si.sample_rate, si.centerfreq);
			fprintf(so, "# segments %" PRIu64 "\n# samples %" PRIu64 "\n# clipped %" PRIu64 "\n", si.segments, si.samples, si.clipped);
			fprintf(so, "# enbw_bins %.9g\n# mean_power %.9g\n# dc_i %.9g\n# dc_q %.9g\n# peak %.9g\n# kernel_ms %.6g\n",
					si.enbw_bins, si.mean_power, si.dc_i, si.dc_q, (double)si.peak, (double)si.kernel_ms);
			for(int i = 0; i < n; i++)                                              /* bin i: centerfreq + (i - nfft / 2) sample_rate / nfft */
				fprintf(so, "%.3f %.4f\n", (double)si.centerfreq + ((double)i - (double)(n / 2)) * (double)si.sample_rate / (double)n,
						power[i] > 0.0 ? 10.0 * log10(power[i]) : -INFINITY);
			fclose(so);
		}
		else fprintf(stderr, "spectrum not written: %s\n", n < 0 ? vdl2hip_strerror(n) : "cannot open file");
	}
	if(wf_mean) fclose(wf_mean);
	if(wf_max) fclose(wf_max);
	if(waterfall_path) {
		static float max_hold[4096], floor_hold[4096];
		vdl2hip_specgram_info gi;
		memset(&gi, 0, sizeof gi); gi.struct_size = sizeof gi;
		int n = vdl2hip_specgram_read(rx, &gi, max_hold, floor_hold, 4096, 0);
		FILE *so = n > 0 ? fopen(waterfall_path, "w") : NULL;
		if(so) {
			fprintf(so, "# nfft %u\n# window %u\n# stride %u\n# line_segments %u\n# ring_lines %u\n# sample_rate %u\n# centerfreq %u\n", gi.nfft, gi.window, gi.stride,
					gi.line_segments, gi.ring_lines, gi.sample_rate, gi.centerfreq);
			fprintf(so, "# first_segment %" PRIu64 "\n# first_sample %" PRIu64 "\n# lines %" PRIu64 "\n# hold_segments %" PRIu64 "\n# hold_lines %" PRIu64 "\n",
					gi.first_segment, gi.first_sample, gi.lines, gi.hold_segments, gi.hold_lines);
			for(int i = 0; i < n; i++)                                              /* freq_hz max_dbfs floor_dbfs */
				fprintf(so, "%.3f %.4f %.4f\n", (double)gi.centerfreq + ((double)i - (double)(n / 2)) * (double)gi.sample_rate / (double)n,
						dbfs_of((double)max_hold[i]), dbfs_of((double)floor_hold[i]));
			fclose(so);
		}
		else fprintf(stderr, "waterfall not written: %s\n", n < 0 ? vdl2hip_strerror(n) : "cannot open file");
	}
	if(activity_path) {
		FILE *so = nact == (int)nfreq ? fopen(activity_path, "w") : NULL;
		if(so) {
			fprintf(so, "# bin_samples %u\n# hang_bins %u\n# series_bins %u\n# threshold_dbfs %.9g\n# threshold_power %.9g\n", ai.bin_samples, ai.hang_bins,
					ai.series_bins, (double)ai.threshold_dbfs, (double)ai.threshold_power);
			fprintf(so, "# first_sample %" PRId64 "\n# bins %" PRIu64 "\n# kernel_ms %.6g\n", ai.first_sample, ai.bins, (double)ai.kernel_ms);
			const double bin_ms = 1000.0 * (double)ai.bin_samples / (SYMBOL_RATE * 10.0);
			for(uint32_t c = 0; c < nfreq; c++) {
				const vdl2hip_activity_chan *ch = &act[c];
				fprintf(so, "%u %" PRIu64 " %" PRIu64 " %.6f %" PRIu64 " %.3f %.2f %.2f %.1f %.1f\n", freqs[c], ch->bins, ch->busy_bins,
						ch->bins ? (double)ch->busy_bins / (double)ch->bins : 0.0, ch->transmissions, (double)ch->longest_bins * bin_ms,
						dbfs_of(ch->bins ? ch->sum_power / (double)ch->bins : 0.0), dbfs_of((double)ch->max_power), hist_percentile(ch, 0.10), hist_percentile(ch, 0.50));
			}
			fclose(so);
		}
		else fprintf(stderr, "activity not written: %s\n", nact < 0 ? vdl2hip_strerror(nact) : "cannot open file");
	}
	if(bursts_path) {
		vdl2hip_capture_info ci;
		memset(&ci, 0, sizeof ci); ci.struct_size = sizeof ci;
		r = vdl2hip_capture_info_get(rx, &ci);
		FILE *so = r == VDL2HIP_OK ? fopen(bursts_path, "w") : NULL;
		if(so) {
			fprintf(so, "# pre_samples %u\n# post_samples %u\n# flags %u\n# pool_samples %u\n", ci.pre_samples, ci.post_samples, ci.flags, ci.pool_samples);
			fprintf(so, "# bursts %" PRIu64 "\n# iq_samples %" PRIu64 "\n# iq_dropped %" PRIu64 "\n# kernel_ms %.6g\n", ci.bursts, ci.iq_samples, ci.iq_dropped, (double)ci.kernel_ms);
			for(size_t i = 0; i < nbursts; i++) {
				const vdl2hip_burst *b = &bursts[i];
				fprintf(so, "%u %u %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %u %u %.9g %.9g %.9g %u %" PRId64 " %u %" PRIu64 " %u %u %d %u %.9g %.9g %.9g %.9g %.9g %.9g\n",
						b->chan, b->freq, b->burst_ord, b->sync_sample, b->end_sample, b->first_symbol, b->nsym, b->tl_bits, (double)b->ppm_error, (double)b->dphi,
						(double)b->prev_phase, b->flags, b->iq_first, b->iq_count, b->iq_off, b->frames, b->frames_ok, b->fec_corrections, b->weak_symbols,
						(double)b->mean_power, (double)b->min_power, (double)b->max_power, (double)b->phase_err_rms, (double)b->phase_err_mean, (double)b->phase_err_max);
			}
			fclose(so);
		}
		else fprintf(stderr, "bursts not written: %s\n", r != VDL2HIP_OK ? vdl2hip_strerror(r) : "cannot open file");
		if(bursts_iq) fclose(bursts_iq);
	}
	if(toa_path) {
		vdl2hip_toa_info ti;
		memset(&ti, 0, sizeof ti); ti.struct_size = sizeof ti;
		r = vdl2hip_toa_info_get(rx, &ti);
		FILE *so = r == VDL2HIP_OK ? fopen(toa_path, "w") : NULL;
		if(so) {
			fprintf(so, "# max_lag %u\n# flags %u\n# pool_curves %u\n", ti.max_lag, ti.flags, ti.pool_curves);
			fprintf(so, "# bursts %" PRIu64 "\n# curves %" PRIu64 "\n# curves_dropped %" PRIu64 "\n# early %" PRIu64 "\n# edge %" PRIu64 "\n# kernel_ms %.6g\n",
			        ti.bursts, ti.curves, ti.curves_dropped, ti.early, ti.edge, (double)ti.kernel_ms);
			fprintf(so, "chan,freq,burst_ord,sync_sample,first_symbol,peak_sample,peak_lag,nlags,toa_frac,toa_sample,peak_power,energy,rho,carrier_phase,cfo_hz,dphi,resid,flags,frames,frames_ok\n");
			for(size_t i = 0; i < ntoas; i++) {
				const vdl2hip_burst_toa *b = &toas[i];
				fprintf(so, "%u,%u,%" PRId64 ",%" PRId64 ",%" PRId64 ",%" PRId64 ",%d,%u,%.9g,%.17g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%u,%u,%u\n",
				        b->chan, b->freq, b->burst_ord, b->sync_sample, b->first_symbol, b->peak_sample, b->peak_lag, b->nlags, (double)b->toa_frac,
				        (double)b->peak_sample + (double)b->toa_frac, (double)b->peak_power, (double)b->energy, (double)b->rho, (double)b->carrier_phase,
				        (double)b->cfo_hz, (double)b->dphi, (double)b->resid, b->flags, b->frames, b->frames_ok);
			}
			fclose(so);
		}
		else fprintf(stderr, "burst timing not written: %s\n", r != VDL2HIP_OK ? vdl2hip_strerror(r) : "cannot open file");
	}
	if(tx_path) {
		vdl2hip_txlog_info ti;
		memset(&ti, 0, sizeof ti); ti.struct_size = sizeof ti;
		r = vdl2hip_txlog_info_get(rx, &ti);
		FILE *so = r == VDL2HIP_OK ? fopen(tx_path, "w") : NULL;
		if(so) {
			fprintf(so, "# pool_records %u\n# flags %u\n# transmissions %" PRIu64 "\n# decoded %" PRIu64 "\n# dropped %" PRIu64 "\n", ti.pool_records, ti.flags,
					ti.transmissions, ti.decoded, ti.dropped);
			fprintf(so, "# frames_matched %" PRIu64 "\n# frames_unmatched %" PRIu64 "\n# kernel_ms %.6g\n", ti.frames_matched, ti.frames_unmatched, (double)ti.kernel_ms);
			static uint64_t ch_tx[1024], ch_ok[1024];
			for(size_t i = 0; i < ntxs; i++) {
				const vdl2hip_tx *t = &txs[i];
				fprintf(so, "%u %u %" PRId64 " %.3f %.2f %.2f %u %u %u\n", t->chan, t->freq, t->first_sample,
						1000.0 * (double)(t->last_sample - t->first_sample + 1) / (SYMBOL_RATE * 10.0), dbfs_of((double)t->peak_power), dbfs_of((double)t->mean_power),
						t->frames, t->frames_ok, t->flags);
				if(t->chan < 1024) { ch_tx[t->chan]++; if(t->frames_ok) ch_ok[t->chan]++; }
			}
			for(uint32_t c = 0; c < nfreq; c++)
				fprintf(so, "# channel %u %u transmissions=%" PRIu64 " decoded=%" PRIu64 " ratio=%.4f\n", c, freqs[c], ch_tx[c], ch_ok[c],
						ch_tx[c] ? (double)ch_ok[c] / (double)ch_tx[c] : 0.0);
			fclose(so);
		}
		else fprintf(stderr, "transmissions not written: %s\n", r != VDL2HIP_OK ? vdl2hip_strerror(r) : "cannot open file");
	}
	if(tx_search_path) {
		vdl2hip_txsearch_info si;
		memset(&si, 0, sizeof si); si.struct_size = sizeof si;
		r = vdl2hip_txsearch_info_get(rx, &si);
		FILE *so = r == VDL2HIP_OK ? fopen(tx_search_path, "w") : NULL;
		if(so) {
			fprintf(so, "# flags %u records %" PRIu64 " samples_searched %" PRIu64 " clipped %" PRIu64 " kernel_ms %.6g\n", si.flags, si.records, si.samples_searched,
					si.clipped, (double)si.kernel_ms);
			for(size_t i = 0; i < ntxss; i++) {
				const vdl2hip_tx_search *t = &txss[i];
				fprintf(so, "%u %u %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %.9g %.9g %.9g %u %u %u %u %u %u %u\n", t->chan, t->freq, t->first_bin,
						t->search_first, t->search_last, t->best_sample, t->first_lock, (double)t->best_pherr, (double)t->best_slope, (double)t->best_ppm,
						t->lock_points, t->below_thr, t->lock_phases, t->flags, t->frames, t->frames_ok, t->why);
			}
			fclose(so);
		}
		else fprintf(stderr, "preamble search not written: %s\n", r != VDL2HIP_OK ? vdl2hip_strerror(r) : "cannot open file");
	}
	if(relook) {
		vdl2hip_relook_info li;
		memset(&li, 0, sizeof li); li.struct_size = sizeof li;
		r = vdl2hip_relook_info_get(rx, &li);
		FILE *so = r == VDL2HIP_OK && relook_path ? fopen(relook_path, "w") : NULL;
		if(so) {
			fprintf(so, "# flags %u threshold %.9g max_anchors %u records %" PRIu64 " anchors_found %" PRIu64 " attempts %" PRIu64 " frames %" PRIu64 " frames_ok %" PRIu64
					" frames_new %" PRIu64 " dropped %" PRIu64 " kernel_ms %.6g\n", li.flags, (double)li.threshold, li.max_anchors, li.records, li.anchors_found, li.attempts,
					li.frames, li.frames_ok, li.frames_new, li.dropped, (double)li.kernel_ms);
			for(size_t i = 0; i < nrls; i++) {
				const vdl2hip_relook *t = &rls[i];
				fprintf(so, "%u %u %" PRIu64 " %" PRId64 " %" PRId64 " %.9g %.9g %.9g %.9g %u %u %u %d %u %u %u %d %u\n", t->chan, t->freq, t->first_bin, t->anchor, t->end_sample,
						(double)t->pherr, (double)t->slope, (double)t->ppm_error, (double)t->prev_phase, t->tl_bits, t->nsym, t->synd_weight, t->stop, t->frames, t->frames_ok,
						t->frames_new, t->fec_corrections, t->flags);
			}
			fclose(so);
		}
		else if(relook_path) fprintf(stderr, "second look not written: %s\n", r != VDL2HIP_OK ? vdl2hip_strerror(r) : "cannot open file");
		if(relook_frames) fclose(relook_frames);
	}
	if(tx_capture_path) {
		vdl2hip_txcap_info xi;
		memset(&xi, 0, sizeof xi); xi.struct_size = sizeof xi;
		r = vdl2hip_txcap_info_get(rx, &xi);
		FILE *so = r == VDL2HIP_OK ? fopen(tx_capture_path, "w") : NULL;
		if(so) {
			fprintf(so, "# flags %u pre_samples %u post_samples %u max_iq_samples %u nfft %u window %u pool_samples %u pool_spectra %u\n", xi.flags, xi.pre_samples,
					xi.post_samples, xi.max_iq_samples, xi.nfft, xi.window, xi.pool_samples, xi.pool_spectra);
			fprintf(so, "# records %" PRIu64 " iq_samples %" PRIu64 " iq_dropped %" PRIu64 " spectra %" PRIu64 " spectra_dropped %" PRIu64 " kernel_ms %.6g\n", xi.records,
					xi.iq_samples, xi.iq_dropped, xi.spectra, xi.spectra_dropped, (double)xi.kernel_ms);
			for(size_t i = 0; i < ntxcs; i++) {                                     /* the record's fields in their order, then total peak_bin peak_hz centroid_hz obw_hz */
				const vdl2hip_tx_capture *t = &txcs[i].r; const vdl2hip_tx_shape *m = &txcs[i].shape;
				fprintf(so, "%u %u %" PRIu64 " %" PRId64 " %" PRId64 " %" PRIu64 " %" PRIu64 " %u %u %u %u %u %u %.9g %u %.3f %.3f %.3f\n", t->chan, t->freq, t->first_bin,
						t->win_first, t->win_last, t->iq_off, t->spec_off, t->iq_count, t->flags, t->segments, t->nfft, t->frames, t->frames_ok,
						m->total, m->peak_bin, m->peak_hz, m->centroid_hz, m->obw_hz);
			}
			fclose(so);
		}
		else fprintf(stderr, "transmission capture not written: %s\n", r != VDL2HIP_OK ? vdl2hip_strerror(r) : "cannot open file");
		if(txc_iq) fclose(txc_iq);
		if(txc_spectra) fclose(txc_spectra);
	}
	if(statsd_path) {
		static char lines[1 << 20];
		char ns[300];
		if(station_id) snprintf(ns, sizeof ns, "dumpvdl2.%s", station_id); else snprintf(ns, sizeof ns, "dumpvdl2");    /* statsd.c:103-108 */
		int n = vdl2hip_statsd_lines(rx, ns, lines, sizeof lines);
		FILE *so = n >= 0 ? fopen(statsd_path, "w") : NULL;
		if(so) { fwrite(lines, 1, (size_t)n, so); fclose(so); }
		else fprintf(stderr, "statsd counters not written: %s\n", n < 0 ? vdl2hip_strerror(n) : "cannot open file");
	}
	vdl2hip_destroy(rx);
	if(raw_out) fclose(raw_out);
	if(f != stdin) fclose(f);
	return 0;
}
