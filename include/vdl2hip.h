/*
 * vdl2hip.h - C ABI of libvdl2hip.so: the MI355X-native replacement for
 * dumpvdl2's per-channel DSP + burst decoder hot path.
 *
 * Boundary it replaces (reference @ v2.6.0, paths relative to the reference root):
 *   input  : process_buf_uchar()/process_buf_short()          src/demod.c:339-365, src/dumpvdl2.h:378-380
 *   setup  : vdl2_channel_init(), input_lpf_init(),
 *            sincosf_lut_init(), demod_sync_init(), rs_init()   src/demod.c:367-392, src/demod.c:84-96, src/rs.c:27-30
 *   work   : process_samples() -> demod() -> got_sync()
 *            -> decode_vdl2_burst() -> decode_frame()            src/demod.c:105-337, src/decode.c:173-384
 *   output : avlc_decoder_queue_push(metadata, frame, flags)     src/decode.c:165-171, src/decode.h:31
 *
 * Plain C: opaque context, plain pointers and sizes, int return codes
 * (0 = ok, negative = VDL2HIP_E_*).  No HIP or torch types appear here.
 * The adapter that re-exports the reference's own symbol names on top of
 * this ABI is include/vdl2hip_dropin.h.
 */
#ifndef VDL2HIP_H
#define VDL2HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDL2HIP_ABI_VERSION 6   /* 2: vdl2hip_frame carries the AVLC verdict; vdl2hip_stats grew; avlc/statsd calls added
                                 * 3: vdl2hip_feed_pinned(); vdl2hip_stats.overflow_feeds; vdl2hip_group_*: one receiver over several
                                 *    GPUs from C (a channeliser look-back that gives up is no longer an error: it falls back)
                                 * 4: vdl2hip_group_set_exchange() / vdl2hip_group_exchange(): striped ingest + all-gather is the group's
                                 *    default exchange, broadcast stays selectable; RCCL is opt-in (VDL2HIP_USE_RCCL=1)
                                 * 5: the referee (decisions within the margin of the channeliser's distance from the reference's fp32 scan are
                                 *    taken on the reference's own samples): vdl2hip_stats grew by referee_*; vdl2hip_get_stats_sized() for callers
                                 *    built against an older vdl2hip_stats.  (Since ABI 4 chanfir_ms / chanfir_launches / chan_samples cover only
                                 *    the TIMED channeliser launches - profiling on, cold-start feeds excluded - not every launch.)
                                 * 6: vdl2hip_stats.referee_redone_next (a feed's walk no longer waits for the check of the feed before)
                                 *    VDL2HIP_FMT_CF32: one more accepted value of vdl2hip_cfg.sample_fmt - no structure, no entry point and no
                                 *    result for the other formats changed, so the version stayed
                                 *    vdl2hip_cfg.input_rate (the structure grew at its end, 56 -> 64 bytes; a struct_size of 56 is still taken and
                                 *    means input_rate 0), vdl2hip_stats.resampled_samples / resample_ms (at its end), vdl2hip_read_resampled(),
                                 *    vdl2hip_resampler_design(): nothing changed for a caller that does not set input_rate, so the version stayed
                                 *    vdl2hip_spectrum_window() / _enable() / _read() / _channels() with vdl2hip_spectrum_cfg / _info: the input monitor, off
                                 *    unless enabled - new entry points and structures only, nothing existing changed size or meaning, so the version stayed
                                 *    vdl2hip_activity_edges() / _enable() / _disable() / _read() / _series() with vdl2hip_activity_cfg / _info / _chan: the
                                 *    activity monitor, off unless enabled - again new entry points and structures only, so the version stayed
                                 *    vdl2hip_capture_enable() / _disable() / _info_get() / _read() with vdl2hip_capture_cfg / _info and vdl2hip_burst: the
                                 *    burst capture, off unless enabled - new entry points and structures only once more, so the version stayed
                                 *    VDL2HIP_FMT_S8 (4): one more accepted value of vdl2hip_cfg.sample_fmt, as VDL2HIP_FMT_CF32 was - no structure, no
                                 *    entry point and no result for the other formats changed, so the version stayed
                                 *    vdl2hip_txlog_enable() / _disable() / _info_get() / _read() with vdl2hip_txlog_cfg / _info and vdl2hip_tx: the
                                 *    transmission log, off unless enabled - new entry points and structures only, so the version stayed
                                 *    vdl2hip_stats.referee_symbol_pieces_ahead / _late (at its end, as resampled_samples was: a caller built against the
                                 *    shorter structure goes through vdl2hip_get_stats_sized() or never reads them), so the version stayed
                                 *    vdl2hip_txsearch_enable() / _disable() / _info_get() / _read() with vdl2hip_txsearch_cfg / _info and
                                 *    vdl2hip_tx_search: the preamble search, off unless enabled - new entry points and structures only, so the version stayed
                                 *    vdl2hip_specgram_enable() / _disable() / _read() / _lines() / _channels() with vdl2hip_specgram_cfg / _info: the
                                 *    spectrogram on top of the input monitor, off unless enabled - new entry points and structures only, so the version stayed
                                 *    vdl2hip_txcap_enable() / _disable() / _info_get() / _read() / _measure() with vdl2hip_txcap_cfg / _info, vdl2hip_tx_capture
                                 *    and vdl2hip_tx_shape: the transmission capture, off unless enabled - new entry points and structures only, so the version stayed
                                 *    vdl2hip_toa_template() / _enable() / _disable() / _info_get() / _read() with vdl2hip_toa_cfg / _info and vdl2hip_burst_toa:
                                 *    burst timing, off unless enabled - new entry points and structures only, so the version stayed
                                 *    vdl2hip_relook_enable() / _disable() / _info_get() / _read() with vdl2hip_relook_cfg / _info and vdl2hip_relook:
                                 *    the second look, off unless enabled - new entry points and structures only, so the version stayed */

/* enum sample_formats, src/dumpvdl2.h:319 */
#define VDL2HIP_FMT_U8     0
#define VDL2HIP_FMT_S16LE  1
/* Not in the reference's enum: complex float32 - interleaved I, Q as IEEE float32 in host byte order, 8 bytes per complex sample (GNU
 * Radio file sinks, SoapySDR's default stream format).  process_buf_uchar() / process_buf_short() do nothing but fill the float array
 * sbuf[] that every later stage reads (src/demod.c:309-310,349-365): a CF32 sample IS that sbuf[] value, taken as it is.
 *  - Full scale is 1.0.  Values are used unscaled and unclipped; beyond +-1 is legal, frame_pwr_dbfs simply goes above 0.
 *    k / 32768.0f gives exactly what the int16 k gives, (b - 127.5f) / 127.5f computed in float32 what the byte b gives.
 *  - A negative zero is read as a positive zero (x + 0.0f at the load), as the integer conversions never produce one.
 *  - Non-finite samples (NaN, infinities) are the caller's error and are not looked for: they poison that channel's filter state
 *    for good, as they would the reference's.
 *  - A feed is truncated to whole samples (8 bytes), as it is to 4 or 2 in the other formats; vdl2hip_feed_device() wants an 8-byte
 *    aligned pointer; max_block_bytes stays in bytes (default 320000 = 40000 samples). */
#define VDL2HIP_FMT_CF32   2
/* The value 3 is unassigned and refused (VDL2HIP_E_INVAL).
 * Not in the reference's enum either: signed 8-bit IQ ("CS8", SigMF's ci8 / cs8) - interleaved I, Q as two's-complement int8_t, 2 bytes
 * per complex sample: a HackRF's only format, the 8-bit wire format of USRPs and of the bladeRF 2.0.
 *  - The value of a byte b is (float)b / 128.0f, exact for all 256 bytes: -1.0 .. 127 / 128.
 *  - That is bit for bit the float process_buf_short() makes of the int16 k = 256 b ((float)(256 b) / 32768.0f == b / 128): an S8
 *    receiver IS a VDL2HIP_FMT_S16LE receiver fed b << 8 - the same frames, metadata, counters, timing and decimated stream, to the bit.
 *  - A feed is truncated to whole samples (2 bytes); vdl2hip_feed_device() wants a 2-byte aligned pointer; max_block_bytes stays in
 *    bytes (default 320000 = 160000 samples).
 *  - The drop-in adapter (vdl2hip_dropin.h) has no entry point for it: the reference has no process_buf_*() of this format to replace. */
#define VDL2HIP_FMT_S8     4

#define VDL2HIP_OK            0
#define VDL2HIP_E_INVAL      -1   /* bad argument / configuration */
#define VDL2HIP_E_NOMEM      -2
#define VDL2HIP_E_DEVICE     -3   /* HIP runtime error (no GPU, launch failure ...) */
#define VDL2HIP_E_TOOBIG     -4   /* block larger than max_block_bytes */
#define VDL2HIP_E_OVERFLOW   -5   /* device-side frame/burst buffer exhausted (frames were dropped) */

/* Per-channel counters = the reference's per-channel statsd counters on this
 * path (src/statsd.c:34-65; call sites src/demod.c:245, src/decode.c:204-373),
 * plus two that have no statsd name. */
enum {
	VDL2HIP_CNT_SYNC_GOOD = 0,          /* demod.sync.good */
	VDL2HIP_CNT_CRC_GOOD,               /* decoder.crc.good */
	VDL2HIP_CNT_CRC_BAD,                /* decoder.crc.bad */
	VDL2HIP_CNT_ERR_NO_HEADER,          /* decoder.errors.no_header */
	VDL2HIP_CNT_ERR_TOO_LONG,           /* decoder.errors.too_long */
	VDL2HIP_CNT_ERR_NO_FEC,             /* decoder.errors.no_fec */
	VDL2HIP_CNT_ERR_DATA_TRUNCATED,     /* decoder.errors.data_truncated */
	VDL2HIP_CNT_ERR_FEC_TRUNCATED,      /* decoder.errors.fec_truncated */
	VDL2HIP_CNT_ERR_DEINTERLEAVE_DATA,  /* decoder.errors.deinterleave_data */
	VDL2HIP_CNT_ERR_DEINTERLEAVE_FEC,   /* decoder.errors.deinterleave_fec */
	VDL2HIP_CNT_ERR_FEC_BAD,            /* decoder.errors.fec_bad */
	VDL2HIP_CNT_ERR_BITSTREAM,          /* decoder.errors.bitstream */
	VDL2HIP_CNT_ERR_TRUNCATED_OCTETS,   /* decoder.errors.truncated_octets */
	VDL2HIP_CNT_ERR_UNSTUFF,            /* decoder.errors.unstuff */
	VDL2HIP_CNT_BLOCKS_PROCESSED,       /* decoder.blocks.processed */
	VDL2HIP_CNT_BLOCKS_FEC_OK,          /* decoder.blocks.fec_ok */
	VDL2HIP_CNT_MSG_GOOD,               /* decoder.msg.good */
	VDL2HIP_CNT_MSG_GOOD_LOUD,          /* decoder.msg.good_loud */
	VDL2HIP_CNT_PPM_REJECT,             /* preambles dropped by max_ppm (src/demod.c:192) */
	VDL2HIP_CNT_SLICER_NEG_IDX,         /* slicer index < 0: the reference reads out of bounds there (src/demod.c:264) */
	VDL2HIP_NUM_COUNTERS
};

typedef struct vdl2hip_ctx vdl2hip_ctx;

typedef struct {
	uint32_t struct_size;       /* sizeof(vdl2hip_cfg), for ABI evolution */
	uint32_t centerfreq;        /* Hz; vdl2_channel_init() arg 1 */
	uint32_t oversample;        /* sample rate = 105000 * oversample (src/dumpvdl2.c:1073) */
	uint32_t sample_fmt;        /* VDL2HIP_FMT_* */
	uint32_t nchan;
	const uint32_t *freqs;      /* nchan channel frequencies, Hz */
	float    max_ppm;           /* Config.max_ppm; 0 disables (src/demod.c:192) */
	int32_t  device;            /* HIP device ordinal.  Every call on the context runs on this device whatever the calling thread's
	                             * current device is, and leaves the thread's current device as it found it */
	uint32_t max_block_bytes;   /* largest block a feed call may carry; 0 = 320000 (FILE_BUFSIZE) */
	uint32_t chan_first;        /* multi-GPU sharding: this context decodes channels            */
	uint32_t chan_count;        /*   [chan_first, chan_first+chan_count) of freqs[]; 0 = all     */
	uint32_t reserved0;         /* ignored (the tail padding of the 56-byte structure, which callers never initialised) */
	uint32_t input_rate;        /* Hz: the rate of the IQ the caller feeds.  0 or 105000 * oversample: nothing is resampled (the same
	                             * kernels, the same results to the bit).  Anything else: see "Resampling" below */
	uint32_t reserved1;         /* must be 0 */
} vdl2hip_cfg;
#define VDL2HIP_CFG_SIZE_V1 56u   /* sizeof(vdl2hip_cfg) before input_rate: still accepted as struct_size, by vdl2hip_create() and vdl2hip_group_create() */

/* Resampling (not in the reference, which sets its radio to 105000 * oversample itself, src/dumpvdl2.c:1073).  With
 * fout = 105000 * oversample, g = gcd(input_rate, fout), L = fout / g, M = input_rate / g the receiver converts the caller's stream
 * x[] (converted to float exactly as the formats are converted otherwise; x[i < 0] = 0) to
 *     r[n] = sum_{j=0}^{T-1} h[j L + p_n] x[b_n - j],   p_n = (n M) mod L,   b_n = floor(n M / L)
 * on the device, ahead of the channeliser, and IS a VDL2HIP_FMT_CF32 receiver at 105000 * oversample fed r[] from there on - frames,
 * counters and every channel's decimated stream are those of that receiver, to the bit (vdl2hip_read_resampled() returns r[]).
 *  - h[] is what vdl2hip_resampler_design() returns: a Kaiser-windowed sinc, L T float32 taps; with fmin = min(input_rate, fout):
 *    ripple <= 0.01 dB over |f| <= 0.40 fmin, >= 80 dB down for |f| >= 0.60 fmin (what folds back lands outside 0.40 fmin), every
 *    phase's DC gain within 3e-4 of 1.  Channels should lie within +-0.40 fmin of the centre frequency.
 *  - After N input samples exactly the outputs with b_n <= N - 1 exist: ceil(N L / M).  r[n] is computed in float32, real and imaginary
 *    part separately, always in the same order of operations: the stream depends on the input stream alone, not on how it was cut
 *    into feeds (a feed may be a single sample).  n M is kept in 64 bits: good for 2^50 samples.
 *  - The filter is causal: everything arrives (L T - 1) / (2 L) INPUT samples late - one or two decimated samples (105 kS/s) - and so
 *    do sync_sample and end_sample of every frame against the same capture at the native rate.
 *  - VDL2HIP_E_INVAL, before a device is looked for: L > 1024 (keeps the tap table small: 1024 x 29 floats), input_rate > 8 fout or
 *    4 input_rate < fout (these bound T, which grows with M / L: 29 .. 34 taps per phase near 1 : 1, 219 at 8 : 1).
 *  - max_block_bytes, vdl2hip_feed*() sizes and the alignment vdl2hip_feed_device() wants stay those of the caller's format at the
 *    caller's rate; vdl2hip_stats.input_samples counts the caller's samples, resampled_samples the samples of r[].
 *  - A large page-locked block to an idle receiver is not copied in pieces (cold_start_feeds stays 0).
 *  - In a group every member resamples the whole block itself (cheap; the exchange moves the caller's bytes). */

/* Input monitor (not in the reference, whose users look at their wideband input with a second program): an optional power spectrum
 * and level statistics of the CALLER's stream - the samples as fed, ahead of the resampler, at cfg.input_rate if that is set and at
 * 105000 * oversample otherwise - computed on the device from the block the channeliser is about to read.  Off unless enabled; with it
 * off nothing is launched and every result is what it was, to the bit.
 *  - Samples.  x[i] is the float value of input sample i as the formats are converted everywhere else (VDL2HIP_FMT_* above: u8 the
 *    correctly rounded (b - 127.5f) / 127.5f, s16 k / 32768.0f, cf32 the value itself, s8 b / 128.0f); i counts from the first sample fed after
 *    vdl2hip_spectrum_enable().
 *  - Segments.  Segment j is x[j N .. (j + 1) N), N = nfft.  It is ANALYSED iff it is complete and j % stride == 0: which segments
 *    are analysed depends on the stream alone, not on how it was cut into feeds (a feed may be one sample, a segment may span many).
 *  - Transform.  w[] is what vdl2hip_spectrum_window() returns (designed on the host in double, rounded once to float32).  For an
 *    analysed segment s:  X_s[k] = sum_n w[n] x[j N + n] exp(-2 pi i k n / N).
 *  - Accumulation.  power[i] = (1 / S) sum_s |X_s[k]|^2 / (sum_n w[n])^2,  k = (i + N / 2) mod N,  S = analysed segments so far (all
 *    zero while S = 0).  power[] is in ascending frequency: bin i is at centerfreq + (i - N / 2) sample_rate / N.  A full-scale complex
 *    tone on a bin centre reads 1.0 (0 dBFS); for a noise density divide by enbw_bins = N sum w^2 / (sum w)^2.  The transform and
 *    |X|^2 are computed in float32, the sums over segments in float64.
 *  - Windows, all periodic, t = 2 pi n / N:  VDL2HIP_WIN_RECT 1;  VDL2HIP_WIN_HANN 0.5 - 0.5 cos t;  VDL2HIP_WIN_BH4
 *    0.35875 - 0.48829 cos t + 0.14128 cos 2t - 0.01168 cos 3t (its sidelobes, 92 dB down, sit below the float32 floor).
 *  - nfft: a power of two in 64 .. 4096.  stride 0 means 1.
 *  - Levels, over the samples of the analysed segments, unwindowed: samples = S N; mean_power = mean of re^2 + im^2; dc_i, dc_q = mean
 *    I, mean Q; peak = max over samples of max(|re|, |im|); clipped = samples with a component at the rail, stated on the float value
 *    v:  u8 |v| == 1.0f (bytes 0 and 255);  s16 v == -1.0f or v == 32767 / 32768.0f;  cf32 |v| >= 1.0f (a NaN does not count);
 *    s8 v == -1.0f or v == 127 / 128.0f (bytes -128 and 127).
 *  - Determinism.  The same sequence of calls gives the same bits (no floating-point atomics anywhere).  The same stream cut
 *    differently gives segments, samples, clipped and peak exactly, and power[], mean_power, dc_* within 1e-12 relative (only the order
 *    of float64 additions moves).
 *  - With the monitor on, a large page-locked block to an idle receiver is not copied in pieces (cold_start_feeds stays 0).
 *  - Groups: there is no group call.  Every member is fed the whole block, so vdl2hip_group_ctx(g, 0) is the handle. */
#define VDL2HIP_WIN_RECT 0
#define VDL2HIP_WIN_HANN 1
#define VDL2HIP_WIN_BH4  2
typedef struct { uint32_t struct_size, nfft, window, stride; } vdl2hip_spectrum_cfg;   /* nfft 0: off; stride 0 means 1 */
typedef struct {
	uint32_t struct_size, nfft, window, stride;
	uint32_t sample_rate, centerfreq;          /* of the analysed stream */
	uint64_t segments, samples, clipped;
	double   enbw_bins, mean_power, dc_i, dc_q;
	float    peak, kernel_ms;                  /* kernel_ms: summed HIP-event time of the monitor's launches at profiling level 2, else 0
	                                            * (of the feeds collected so far: after vdl2hip_sync(), all of them) */
} vdl2hip_spectrum_info;                       /* 88 bytes */

/* Spectrogram (not in the reference): a tap on top of the input monitor that keeps what an average hides - VDL2 is bursts of a few
 * milliseconds at a duty cycle of a few percent, and a burst in a share d of the segments at a signal-to-floor ratio s lifts the
 * averaged bin by 10 log10(1 + d s) dB only (0.4 dB for a 20 dB burst at 0.1 %).  Per bin: the maximum since enable (max_hold), the
 * quietest line (floor_hold) and the last ring_lines time lines of mean and maximum (a waterfall).  Off unless enabled; with it off
 * nothing of it is launched or allocated and the monitor launches exactly the kernels it always did.  On, frames, counters, the
 * decimated stream and every other tap are exactly what they were, and the monitor's own results stay inside its determinism clause
 * (the tap's build of the kernel adds the same values in the same order; nothing but the order of float64 additions could move).
 *  - Segments.  The monitor's: N = nfft, window w, stride, the analysed segments and their transforms X_s exactly as the monitor
 *    forms them.  q_s[i] = |X_s[(i + N / 2) mod N]|^2 is the float32 value the monitor adds to its sums (re re + im im, two
 *    products and a sum in float32); i ascends in frequency like power[].  norm = 1 / (sum_n w[n])^2 in double.
 *  - Ordinals.  Analysed segments are numbered a = 0, 1, ... from vdl2hip_spectrum_enable() (a reset of vdl2hip_spectrum_read() does
 *    not restart them).  a0 = the number of them complete when vdl2hip_specgram_enable() is called; the tap sees segment a iff
 *    a >= a0 - a segment begun before the enable and completed after it counts.  Which segments it sees, and everything below,
 *    depends on the stream and on a0 alone, not on how the stream was cut into feeds.
 *  - Lines.  R = line_segments, 1 <= R <= 2^20; 0 means 16.  Line l covers the analysed segments a0 + l R .. a0 + (l + 1) R - 1 and
 *    exists once the last of them is complete.  line_mean[l][i] = (float)(sum_s q_s[i] norm / R), the sum in float64, narrowed
 *    once; line_max[l][i] = (float)((double)max_s q_s[i] norm), the maximum a float32 comparison.  A line that straddles feeds is
 *    finished from state carried on the device: a float64 partial sum and a float32 maximum per bin.  Line l begins at the monitor's
 *    sample (a0 + l R) stride N and spans R stride N samples.
 *  - Hold, since enable or the last reset:  max_hold[i] = (float)((double)max q_s[i] norm) over every segment seen, those of a line
 *    not yet complete included, so that a single segment of burst is caught; all zero while hold_segments == 0.
 *    floor_hold[i] = min over the lines completed since then of line_mean[l][i], a float32 minimum of exactly the values the ring
 *    received; all zero while hold_lines == 0.  It is the quietest line: a floor estimate that bursts cannot lift - and, being a
 *    minimum, biased low: for exponentially distributed |X|^2 some 2.8 dB under the average floor for R = 16 over 62 lines, less
 *    for a larger R.
 *  - Ring.  The device keeps the last ring_lines lines, mean and max as float32 planes: a power of two, raised to at least the
 *    lines one feed of max_block_bytes can complete, plus one; 0 means that minimum.  ring_lines nfft > 2^25 is refused
 *    (VDL2HIP_E_INVAL) before anything is allocated, as is a ring_lines that is not a power of two.
 *  - Determinism.  The same sequence of calls gives the same bytes (no floating-point atomics).  The same stream cut differently
 *    gives line_max, max_hold and all counts exactly, and line_mean - hence floor_hold - equal or adjacent float32 values: only the
 *    order of the float64 additions moves, below 1e-12 relative before the narrowing.  Within one run floor_hold equals the minimum
 *    of the delivered line_mean values bit for bit.
 *  - Accuracy against the float64 definition: per segment the monitor's bound  b_s[i] = (2 e |X[k]| ||X||_2 + e^2 ||X||_2^2 +
 *    4 2^-24 |X[k]|^2) norm,  e = log2 N 2^-24.  line_mean is within the mean of b_s over the line plus one float32 rounding of the
 *    result; line_max and max_hold within the largest b_s[i] among the segments covered plus that rounding
 *    (|max a - max b| <= max |a - b|).
 *  - Reset (of vdl2hip_specgram_read) zeroes max_hold, floor_hold, hold_segments and hold_lines after the copy.  Line numbering,
 *    the ring and the line under way are untouched.  A reset of vdl2hip_spectrum_read() does not touch the tap.
 *  - Switching.  vdl2hip_spectrum_enable() switches a running spectrogram off first, also with nfft 0.  vdl2hip_specgram_enable()
 *    with the monitor off is VDL2HIP_E_INVAL.  Enabling again restarts at the then-current a0 with zeroed state.
 *  - Groups get no group call: vdl2hip_group_ctx(g, 0) is the handle.  A resampling receiver's tap sees the caller's stream, as
 *    its monitor does.  Time spent in the tap's launches is part of vdl2hip_spectrum_info.kernel_ms. */
typedef struct { uint32_t struct_size, line_segments, ring_lines, reserved; } vdl2hip_specgram_cfg;   /* 16 bytes; 0 = 16 lines, the smallest ring; reserved must be 0 */
typedef struct {
	uint32_t struct_size, nfft, window, stride, line_segments, ring_lines;   /* as in force */
	uint32_t sample_rate, centerfreq;
	uint64_t first_segment;                    /* a0 */
	uint64_t first_sample;                     /* a0 * stride * nfft, in the monitor's sample count */
	uint64_t lines;                            /* complete so far */
	uint64_t hold_segments, hold_lines;        /* what max_hold / floor_hold cover */
} vdl2hip_specgram_info;                       /* 72 bytes */

/* Activity monitor (not in the reference, which reports what it decoded and nothing about what else was on a channel): an optional
 * power envelope of every channel's DECIMATED stream in fixed time bins, and from it the share of time a channel is occupied, the
 * transmissions it carried, a level histogram and a short series per channel - collisions, bursts too weak to synchronise and other
 * users of the channel included.  Off unless enabled; with it off nothing is launched or allocated and every result is what it was,
 * to the bit.  On, frames, counters and the decimated stream are still exactly what they were: the monitor only reads.
 *  - Samples.  y_c[k] is decimated sample k (the 105 kS/s clock of sync_sample) of channel c as the channeliser wrote it, BEFORE any
 *    stretch of it is replaced by the referee: the monitor runs on the front stream directly behind the channeliser, ahead of the sync
 *    kernels, and everything that rewrites y waits for the end of those.
 *  - Bins.  B = bin_samples, 10 <= B <= 10500; 0 means 105 (1 ms, 10.5 symbols).  k_on = the decimated samples produced before
 *    vdl2hip_activity_enable().  Bin m covers k_on + m B .. k_on + (m + 1) B - 1 and  p_c[m] = (1 / B) sum (re^2 + im^2)  over it, in
 *    float32.  A bin exists once it is complete; which bins exist depends on the stream alone, not on how it was cut into feeds (a feed
 *    may add no decimated sample, a bin may span many feeds).  A bin that straddles feeds is finished from a carried float32 partial
 *    sum per channel; the monitor never reads y behind the current feed's first sample.
 *  - Accuracy.  Against the same y summed in float64,  |p - p_ref| <= (B + 4) 2^-24 p_ref:  every term is non-negative, so any order
 *    of float32 additions stays inside (B - 1) 2^-24; the square, the add and the division take the rest.  The same sequence of calls
 *    gives the same bits (no floating-point atomics; the order of additions is fixed by the bin and by where the feeds were cut, not
 *    by the launch); the same stream cut differently gives values within twice that bound of each other.
 *  - Busy.  thr = (float)10^(threshold_dbfs / 10), computed in double and rounded once (threshold_power).  Bin m is busy iff
 *    p_c[m] > thr, a float32 comparison.  A NaN threshold is refused.
 *  - Transmissions.  H = hang_bins, 0 <= H <= 255.  A transmission is a maximal set of busy bins in which consecutive busy bins are
 *    separated by at most H idle bins; its length is last busy - first busy + 1 bins; it is counted at its first busy bin.  It is
 *    `open` after a bin iff at most H idle bins have followed its last busy bin.  The state is carried per channel across feeds.
 *  - Histogram.  64 buckets; edges E[i] = (float)10^((-120 + 2 i) / 10), i = 0 .. 62, computed in double and rounded once
 *    (vdl2hip_activity_edges());  bucket(p) = #{ i : E[i] <= p }  in 0 .. 63.
 *  - Accumulators per channel, since enable or the last reset: bins, busy_bins, transmissions, longest_bins (a transmission still
 *    open counts with what it has so far), sum_power (float64: the bins of a feed in words of 64, each word summed by a fixed tree, the
 *    words in order), max_power and min_power (float32, 0 while bins is 0), hist[64], and open.
 *  - Series.  The device keeps the last series_bins values of p_c[m] per channel: a power of two, raised to at least the bins one
 *    feed of max_block_bytes can complete; 0 means that minimum; above 2^20 is refused.
 *  - Reset zeroes the accumulators after the copy.  The bin position runs on; an open transmission stays open and is not counted a
 *    second time.
 *  - Channels are addressed by their index in cfg.freqs, like vdl2hip_counters(); one outside this context's shard: VDL2HIP_E_INVAL.
 *    Groups get no group call: vdl2hip_group_ctx(g, k) is the handle for member k's channels.
 *  - A receiver that resamples monitors the stream it decodes: nothing is special there. */
typedef struct { uint32_t struct_size, bin_samples, hang_bins, series_bins; float threshold_dbfs; uint32_t reserved; } vdl2hip_activity_cfg;   /* bin_samples 0 = 105; reserved must be 0 */
typedef struct {
	uint32_t struct_size, bin_samples, hang_bins, series_bins;    /* as in force (series_bins: what the ring holds) */
	float    threshold_dbfs, threshold_power;
	int64_t  first_sample;                     /* k_on */
	uint64_t bins;                             /* complete so far, the same for every channel */
	float    kernel_ms;                        /* summed HIP-event time of the monitor's launches at profiling level 2, else 0 (of the feeds
	                                            * collected so far: after vdl2hip_sync(), all of them) */
	uint32_t reserved;
} vdl2hip_activity_info;                       /* 48 bytes */
typedef struct {
	uint64_t bins, busy_bins, transmissions, longest_bins;
	double   sum_power;
	float    max_power, min_power;
	uint32_t open, reserved;
	uint64_t hist[64];
} vdl2hip_activity_chan;                       /* 568 bytes */

/* Burst capture (not in the reference, which reports a burst only through the frames it yields): for every burst handed to the burst
 * decoder, a window of the channel's DECIMATED stream around it, its timing, and a phase-error quality figure computed on the device
 * from the same samples - what a burst looked like on air and how good it was, whether it decoded or not.  Off unless enabled; with
 * it off nothing is launched or allocated and every result is what it was, to the bit.  On, frames, counters and the decimated stream
 * are still exactly what they were: the capture is a read-only pass behind the frame finisher of each feed.
 *  - Which bursts.  Every burst whose header decoded - the ones vdl2hip_stats.bursts counts - in the feed whose burst decoder decodes
 *    it (the feed that brings its last symbol), decoded successfully or not.  A preamble lock whose header fails (crc.bad, too_long,
 *    no_fec) never becomes a burst and is not captured.
 *  - IQ window.  pre = pre_samples <= 4096, post = post_samples <= 1024; k_end = the decimated samples that exist at the end of that
 *    feed.  iq_first = max(0, sync_sample - pre), iq_last = min(end_sample + post, k_end - 1), iq_count = iq_last - iq_first + 1.  The
 *    values are y_c[iq_first .. iq_last] as they stand when that feed's burst decoder has finished: after both of its passes and every
 *    referee scan of the feed, so stretches the referee rewrote for this feed are included.  (With the referee on, a LATER feed already
 *    under way may rewrite a stretch just ahead of its own first sample while the window is copied; a single feed, or the referee off,
 *    gives exactly what vdl2hip_read_decimated() returns after vdl2hip_sync().)  pre = 256 covers ramp-up and the 16-symbol unique
 *    word.  Only post makes the window depend on how the stream was cut into feeds; with post = 0 it does not.
 *  - Quality, over the burst's nsym symbols: t_m = first_symbol + 10 m; phi_m = the phase of y[t_m], the decoder's own double-precision
 *    atan2 narrowed to float; phi_-1 = prev_phase; u_m = exactly the number the decoder's slicer rounds - float32 (phi_m - phi_m-1)
 *    - dphi, wrapped by 2 pi in double, divided by pi / 4 in double, narrowed to float; e_m = u_m - roundf(u_m), in units of pi / 4.
 *    Sums are float64 in a fixed order (contiguous runs of symbols per lane, a fixed tree over the lanes, no atomics):
 *      phase_err_rms = (float)(sqrt(sum e^2 / nsym) pi / 4), phase_err_mean = (float)((sum e / nsym) pi / 4) - the residual carrier
 *      slope -, phase_err_max = (float)(max |e| pi / 4), weak_symbols = #{ m : |e_m| > 0.25f } - symbols nearer to a decision boundary
 *      than to a constellation point -, mean_power = (float)(sum p_m / nsym) with p_m = re^2 + im^2 of y[t_m] in float32 (two
 *      products, one addition), min_power and max_power the smallest and largest p_m.
 *  - Order.  The records of one feed are ordered by (channel, position in the channel's burst list), feeds follow one another in
 *    feed order: the same sequence of calls gives the same bytes.
 *  - Room.  Each feed in flight has an IQ pool of pool_samples pairs (0 means 2^20; above 2^24 is refused).  Offsets are the exclusive
 *    prefix sum of iq_count in record order; a burst whose window ends beyond the pool gets iq_count = 0 and VDL2HIP_BURST_NO_ROOM in
 *    flags - its quality fields are still valid - and vdl2hip_capture_info.iq_dropped counts these.  Records never run out.
 *  - Outcome, joined on the host when the feed is collected, independent of vdl2hip_set_avlc_filter(): frames = the frames the burst
 *    produced, frames_ok = those with avlc_status == VDL2HIP_AVLC_OK, fec_corrections = num_fec_corrections of its last frame, -1
 *    without one.  VDL2HIP_CAPTURE_FAILED_ONLY delivers only the records with frames_ok == 0 (filtered on the host: the device
 *    captures everything, and vdl2hip_capture_info counts everything).
 *  - chan is the index in cfg.freqs.  Groups get no group call: vdl2hip_group_ctx(g, k) is the handle for member k's channels. */
#define VDL2HIP_CAPTURE_FAILED_ONLY 1u
#define VDL2HIP_BURST_NO_ROOM       1u
typedef struct { uint32_t struct_size, pre_samples, post_samples, flags, pool_samples, reserved; } vdl2hip_capture_cfg;  /* 24 bytes; reserved must be 0 */
typedef struct {
	uint32_t chan, freq;                  /* index in cfg.freqs, Hz */
	int64_t  burst_ord, sync_sample, end_sample, first_symbol;   /* first_symbol: the sample of the first symbol after the unique word */
	uint32_t nsym, tl_bits;
	float    ppm_error, dphi, prev_phase; /* what the decoder used: the burst's ppm figure, its phase slope per symbol, the phase before symbol 0 */
	uint32_t flags;                       /* VDL2HIP_BURST_* */
	int64_t  iq_first; uint32_t iq_count, reserved; uint64_t iq_off;   /* pairs; iq_off into the caller's buffer of that vdl2hip_capture_read() */
	uint32_t frames, frames_ok; int32_t fec_corrections; uint32_t weak_symbols;
	float    mean_power, min_power, max_power, phase_err_rms, phase_err_mean, phase_err_max;
} vdl2hip_burst;                               /* 128 bytes */
typedef struct {
	uint32_t struct_size, pre_samples, post_samples, flags, pool_samples, reserved;   /* as in force */
	uint64_t bursts, iq_samples, iq_dropped;   /* captured by the device in the feeds collected so far: records, pairs, windows without room */
	float    kernel_ms;                        /* summed HIP-event time of the capture's launches at profiling level 2, else 0 */
	uint32_t reserved2;
} vdl2hip_capture_info;                        /* 56 bytes */

/* Transmission log (not in the reference): every transmission the activity monitor sees on a channel, one record each - its time,
 * length and level, and the frames it yielded - so that what was on the air can be set against what was decoded: a collision, a burst
 * too weak to synchronise, a foreign carrier are records with frames_ok == 0.  It sits on top of the activity monitor and needs it
 * enabled: it uses the monitor's bins p_c[m], its threshold_power, its hang_bins H and its transmission rule as stated above, and
 * changes none of them.  Off unless enabled; with it off nothing is launched or allocated and every result is what it was, to the
 * bit.  On, frames, counters, the decimated stream and everything the activity monitor reports are still exactly what they were: the
 * log reads the monitor's series and keeps a per-channel state of its own (initialised from the monitor's when it is enabled).
 *  - Closing.  A transmission with last busy bin l is CLOSED once bin l + H + 1 is complete.  The feed that completes that bin emits
 *    its record.  Which records exist after N samples depends on the stream alone, not on how it was cut into feeds.  A transmission
 *    still open when the stream ends is not logged; it shows in vdl2hip_activity_chan.open.
 *  - Record.  first_bin, last_bin: its first and last BUSY bin, counted from k_on like vdl2hip_activity_series(); peak_bin: the lowest
 *    bin among those with the largest p; first_sample = k_on + first_bin B, last_sample = k_on + (last_bin + 1) B - 1 (the 105 kS/s
 *    clock of sync_sample); busy_bins; peak_power = max p (float32 comparison); mean_power = (float)(S / busy_bins), S = the float64
 *    sum of p over the busy bins.
 *  - Partial records.  VDL2HIP_TX_PARTIAL marks a transmission that was already open when the log took effect.  Its first_bin is the
 *    activity monitor's; its busy_bins, peak_* and mean_power cover only bins from the log's first feed on (none of them busy:
 *    busy_bins, peak_power and mean_power are 0 and peak_bin = first_bin).
 *  - Accuracy of S.  Summed in float64 in an order fixed by the bins and by where the feeds were cut (no floating-point atomics): the
 *    same sequence of calls gives the same bytes; against any other order S is within busy_bins 2^-53 relative, every term being
 *    non-negative, so mean_power is within one float32 ulp (2^-23 relative) of any model.  Every other field is exact.
 *  - Order.  The records of one feed are ordered by (channel, first_bin); feeds follow one another in feed order.  Per channel the
 *    sequence of records is independent of the cuts.
 *  - Room.  Each feed in flight has room for pool_records records (0 means 65 536; above 2^22 is refused).  Offsets are the exclusive
 *    prefix sum of the channels' counts in record order; records beyond the room are not written and vdl2hip_txlog_info.dropped
 *    counts them.  Offsets only grow, so what survives is a prefix.
 *  - Outcome, joined on the host when the feed is collected - the feed's frames first, all of them, independent of
 *    vdl2hip_set_avlc_filter().  With close_sample = k_on + (last_bin + H + 2) B, a transmission's window is [first_sample,
 *    close_sample); the windows of consecutive transmissions on a channel are disjoint by construction.  A frame belongs to the record
 *    whose window holds its sync_sample: frames = the frames attributed, frames_ok = those with avlc_status == VDL2HIP_AVLC_OK,
 *    first_burst_ord = burst_ord of the attributed frame with the lowest sync_sample, -1 without one.  The host keeps the frames of a
 *    channel that no record has claimed yet (the newest 4 096 per channel; older ones count as unmatched).  When a record arrives,
 *    waiting frames with sync_sample < first_sample are counted in frames_unmatched and dropped: they were locked below the threshold,
 *    or arrived after their window's record had gone.  The latter happens when a burst outlasts its own transmission - a fade below
 *    the threshold for more than H bins while the decoder runs on - so that its frames come with a later feed than the record: THE
 *    ONE PLACE WHERE THE OUTCOME DEPENDS ON HOW THE STREAM WAS CUT INTO FEEDS.  Raise hang_bins where that matters.
 *  - VDL2HIP_TXLOG_UNDECODED_ONLY delivers only the records with frames_ok == 0 (filtered on the host: the device logs everything and
 *    vdl2hip_txlog_info counts everything).
 *  - vdl2hip_activity_enable() and vdl2hip_activity_disable() switch a running log off first (the feeds under way are collected, what
 *    is queued unread is dropped): its state would no longer mean anything.  vdl2hip_activity_read(..., reset) does not touch the log.
 *  - chan is the index in cfg.freqs.  Groups get no group call: vdl2hip_group_ctx(g, k) is the handle for member k's channels. */
#define VDL2HIP_TXLOG_UNDECODED_ONLY 1u
#define VDL2HIP_TX_PARTIAL           1u
typedef struct { uint32_t struct_size, pool_records, flags, reserved; } vdl2hip_txlog_cfg;      /* 16 bytes; reserved must be 0 */
typedef struct {
	uint32_t chan, freq;                  /* index in cfg.freqs, Hz */
	uint64_t first_bin, last_bin;         /* first and last BUSY bin */
	uint64_t peak_bin;
	int64_t  first_sample, last_sample;
	uint32_t busy_bins, flags;            /* VDL2HIP_TX_* */
	float    peak_power, mean_power;
	uint32_t frames, frames_ok;           /* filled in by the host, like first_burst_ord */
	int64_t  first_burst_ord;
} vdl2hip_tx;                                  /* 80 bytes: the device writes the first 64 */
typedef struct {
	uint32_t struct_size, pool_records, flags, reserved;   /* as in force */
	uint64_t transmissions, decoded, dropped;  /* of the feeds collected so far: records logged, those with frames_ok > 0, records without room */
	uint64_t frames_matched, frames_unmatched;
	float    kernel_ms;                        /* summed HIP-event time of the log's launches at profiling level 2, else 0 */
	uint32_t reserved2;
} vdl2hip_txlog_info;                          /* 64 bytes */

/* Preamble search (not in the reference): for every transmission the transmission log closes, was there a VDL2 preamble in it, and how
 * far was it from locking?  An opt-in pass on the GPU that evaluates the reference's own preamble metric - got_sync() of
 * src/demod.c:129-171, float for float - at EVERY decimated sample of the transmission, where the receiver itself evaluates it only
 * where its screening tier lets it and keeps nothing.  It sits on top of the transmission log and needs it enabled.  Off unless
 * enabled; with it off nothing is launched or allocated and every result is what it was, to the bit.  On, frames, counters, the
 * decimated stream, the activity monitor, the log and the burst capture are still exactly what they were.
 *  - Metric.  Phi(n) = the phase of y_c[n] (atan2 in float64, narrowed to float32) for n >= 0, and 0 for n < 0.  (p(n), s(n)) =
 *    the reference's phase-error sum and slope over the 16 phases Phi(n - 150 + 10 i), i = 0 .. 15: what got_sync() computes at n on
 *    a phase ring that holds the 160 most recent samples.
 *  - Samples.  y_c is taken as it stands when the burst decoder of the feed that closes the transmission has finished (the burst
 *    capture's placement and its caveat about a later feed's referee).  With the referee off, or with a single feed, it is what
 *    vdl2hip_read_decimated() returns after vdl2hip_sync().
 *  - Range.  search_last = the log record's last_sample; search_first = max(first_sample, search_last - 57 343): at most 57 344
 *    samples, more than the longest burst (56 090).  VDL2HIP_TXS_CLIPPED is set in flags if the maximum took the second term.  The
 *    range depends on the stream alone, not on how it was cut into feeds.  So that the range lies inside what the ring holds behind
 *    a feed, vdl2hip_txsearch_enable() refuses an activity monitor with (hang_bins + 1) * bin_samples > 4096.
 *  - Results, over n in [search_first, search_last]:
 *      best_pherr   the smallest p(n): a float32 <, taken in ascending n, starting from +infinity; a NaN is never the best
 *      best_sample  the lowest n that has best_pherr; -1 if none
 *      best_slope   s(best_sample): what the reference's v->dphi would be (0 if none);  best_ppm: the reference's ppm figure of it
 *      below_thr    #{ n : p(n) < 4.0f }
 *      lock points  n is one iff n - 3 >= search_first and p(n - 3) < 4.0f && p(n) > p(n - 3): the condition under which the
 *                   reference locks if its grid of every third sample evaluates at n (src/demod.c:39,173).  lock_points: their
 *                   number; first_lock: the lowest, -1 if none; lock_phases: bit r set iff some lock point has n mod 3 == r -
 *                   7: a reference in DM_INIT would have locked whatever its grid's phase, 0: none could.
 *    Every field is exact: the same y_c gives the same bytes however it is cut and however the kernel splits the range.  (What the
 *    search inherits: without the referee the channeliser's y_c itself depends, in its last bits, on how the input was cut into feeds.)
 *  - flags: VDL2HIP_TXS_CLIPPED, and VDL2HIP_TX_PARTIAL passed on from the log's record.
 *  - why, from the log's join: VDL2HIP_TXS_DECODED (frames_ok > 0), _FRAMES_BAD (frames > 0, none good), _LOCK_NO_FRAME (no frame,
 *    lock_points > 0), _NO_PREAMBLE (no frame, no lock point).  frames and frames_ok are the log record's.
 *  - Records and order.  One record per record the log wrote to its pool (a transmission the log dropped for lack of room gets none),
 *    in the log's order, feed by feed; first_bin with chan is the join key with vdl2hip_tx.
 *  - VDL2HIP_TXSEARCH_UNDECODED_ONLY delivers only the records with frames_ok == 0 (filtered on the host, like the log's).
 *  - vdl2hip_txlog_enable(), vdl2hip_txlog_disable(), vdl2hip_activity_enable() and vdl2hip_activity_disable() switch a running
 *    search off first.  Groups get no group call: vdl2hip_group_ctx(g, k) is the handle. */
#define VDL2HIP_TXSEARCH_UNDECODED_ONLY 1u
#define VDL2HIP_TXS_CLIPPED         2u         /* (bit 0 of vdl2hip_tx_search.flags is VDL2HIP_TX_PARTIAL) */
#define VDL2HIP_TXS_DECODED         0u
#define VDL2HIP_TXS_FRAMES_BAD      1u
#define VDL2HIP_TXS_LOCK_NO_FRAME   2u
#define VDL2HIP_TXS_NO_PREAMBLE     3u
typedef struct { uint32_t struct_size, flags, reserved[2]; } vdl2hip_txsearch_cfg;      /* 16 bytes; reserved must be 0 */
typedef struct {
	uint32_t chan, freq;                  /* as in vdl2hip_tx */
	uint64_t first_bin;                   /* the join key with vdl2hip_tx */
	int64_t  search_first, search_last, best_sample, first_lock;
	float    best_pherr, best_slope, best_ppm;
	uint32_t lock_points, below_thr, lock_phases, flags;   /* flags: VDL2HIP_TXS_CLIPPED | VDL2HIP_TX_PARTIAL */
	uint32_t frames, frames_ok, why;      /* filled in by the host from the log's join; why: VDL2HIP_TXS_DECODED ... _NO_PREAMBLE */
	uint32_t reserved, reserved2;
} vdl2hip_tx_search;                           /* 96 bytes */
typedef struct {
	uint32_t struct_size, flags;               /* as in force */
	uint64_t records, samples_searched, clipped;   /* of the feeds collected so far: records, the sum of their range lengths, records with VDL2HIP_TXS_CLIPPED */
	float    kernel_ms;                        /* summed HIP-event time of the search's launches at profiling level 2, else 0 */
	uint32_t reserved;
} vdl2hip_txsearch_info;                       /* 40 bytes */

/* Second look (not in the reference): for every transmission the transmission log closes, a decode attempt anchored on every preamble
 * in it, whatever state the sequential walk was in when it passed by.  The reference's per-channel FSM looks for a preamble only while
 * it is idle: from a lock to the end of the length the header announced it evaluates nothing (src/demod.c:251-284), so a burst that
 * begins while an earlier lock - a weaker burst, or a false lock with a long garbage header - is still being sliced is never seen.  The
 * second look invents no decoding rule: it runs the reference's own slicer and burst decoder from the sync state the reference would
 * have reached had it been looking, and delivers what comes out on a tap of its own.  The main path stays the reference's, to the bit.
 *  - Dependencies and placement.  It sits on top of the preamble search: vdl2hip_relook_enable() with the search off is
 *    VDL2HIP_E_INVAL, and whatever switches a running search off (vdl2hip_txsearch_enable() / _disable(), vdl2hip_txlog_enable() /
 *    _disable(), vdl2hip_activity_enable() / _disable()) switches a running second look off first.  It runs behind the search of the
 *    feed that closes the transmission and reads y_c as it stands there: the search's placement, with the same caveat about a later
 *    feed's referee.  It writes only buffers of its own.  Off unless enabled; with it off nothing is launched or allocated and every
 *    result is what it was.  On, frames, counters, the decimated stream and every other tap are still exactly what they were.
 *    Groups get no group call: vdl2hip_group_ctx(g, k) is the handle.
 *  - Metric and range.  Phi(n), p(n), s(n), search_first and search_last are exactly those of "Preamble search".  R = 160 (16 symbols
 *    of 10 samples: two preambles cannot lie closer).
 *  - Anchors.  thr = cfg.threshold; 0 means 4.0f; a value outside (0, 30] or a NaN is refused.  n in [search_first, search_last] is
 *    an anchor iff  p(n) < thr (a float32 <),  p(n) < p(m) for every m in [n - R, n) inside the range,  and  p(n) <= p(m) for every
 *    m in (n, n + R] inside the range.  A NaN is never an anchor and never beats one.  Of a transmission's anchors the max_anchors
 *    best are kept, by (p ascending, n ascending); 0 means 4, above 16 is refused.  The kept anchors are reported in ascending n;
 *    vdl2hip_relook_info.anchors_found counts all of them.  The set depends on y_c alone: not on the cuts, not on how a kernel splits
 *    the range.
 *  - Attempt at anchor a.  The reference's DM_SYNC from a channel reset with prev_phi = Phi(a), dphi = s(a) and ppm_error =
 *    ppm_of(s(a), freq).  Symbol m is taken at a + 10 (m + 1), as the walker places them behind its sync point, and sliced with the
 *    decoder's own arithmetic (src/demod.c:256-264); the bits go to decode_vdl2_burst(): header state, then data state.  The
 *    frames' frame_pwr_dbfs is that of the mean of |y|^2 over the attempt's symbols, header included (the reference's running mean of
 *    the same terms, up to rounding).  With cfg.max_ppm set (not 0) and |ppm_error| above it the attempt is not made: flag
 *    VDL2HIP_RELOOK_PPM_REJECT, every other field of the outcome 0.  The slope is taken at the dense minimum itself, where the
 *    reference takes it at its grid's minimum (v->prev_dphi, src/demod.c:184) and moves its sampling point by a parabola's vertex:
 *    the dense metric has the minimum to the sample, so no parabola is needed.
 *  - Limit.  limit = last_sample + (hang_bins + 1) * bin_samples is the last sample that exists when the log emits the record,
 *    whatever the cuts.  A header whose length needs a symbol beyond limit gives VDL2HIP_RELOOK_TRUNCATED and decodes nothing (the
 *    header's tl_bits, nsym and synd_weight are reported, the counters stay 0); an attempt whose nine header symbols themselves pass
 *    limit gives the same.  So every field depends on the stream alone.
 *  - Room.  The frames of a feed's attempts go to a pool of pool_frames records and pool_octets octets per feed in flight (0: 256
 *    records and 8192 octets per channel of the receiver, at least 4096 and 2^20; above 2^20 and 2^26: refused).  What goes to the
 *    host is what the attempts produced, whatever the pools' sizes.  An attempt claims, from its header, what it can need at the
 *    most: a frame is at least
 *    one octet behind an eight-bit flag, so with O = ceil(tl_bits / 8) it claims O / 2 + 1 records and (O + 3 (O / 2 + 1) + 3) & ~3
 *    octets (a frame's octets begin at a multiple of 4).  The claims' places are their exclusive prefix sums in record order, whether
 *    they fit or not.  An attempt whose claim does not fit gets VDL2HIP_RELOOK_NO_ROOM, keeps its header fields, decodes nothing and is
 *    counted in vdl2hip_relook_info.dropped - as are the attempts beyond 32 768 in one feed, which get no record.
 *  - Attempt record.  One vdl2hip_relook per kept anchor, in (log record order, anchor) order, feed by feed.  chan, freq, first_bin:
 *    the join key with vdl2hip_tx / vdl2hip_tx_search.  anchor, pherr = p(a), slope = s(a), ppm_error, prev_phase = Phi(a).  tl_bits,
 *    nsym (symbols behind the unique word, header included), synd_weight: of a header that decoded, else 0.  end_sample: the last
 *    symbol the attempt reads or would need (a + 90 while there is no header).  stop: the VDL2HIP_CNT_* index of the error counter
 *    that ended the attempt (crc.bad, errors.too_long, errors.no_fec, errors.fec_bad, errors.unstuff, errors.truncated_octets), -1
 *    if none did.  counters: a row private to the attempt - what the reference's counters would have gained from it, sync.good aside.
 *    frames, frames_ok (avlc_status OK), frames_new, fec_corrections (of the burst; -1 without a frame), frame_first (index of its
 *    first frame among the frames of the same vdl2hip_relook_read()).  flags: VDL2HIP_RELOOK_PPM_REJECT, _TRUNCATED, _NO_ROOM, and
 *    VDL2HIP_TX_PARTIAL passed on from the log's record.
 *  - Frames.  Delivered as vdl2hip_packed_frame plus octets by vdl2hip_relook_read(), with the frame finisher's avlc_status and
 *    addresses; sync_sample = anchor, burst_ord = -1.  nf_pwr_dbfs = NaN: the reference's figure is a state of its walk, which the
 *    attempt is not part of - the log's record (mean_power, peak_power) and the activity monitor have the levels.  Second-look
 *    frames never enter vdl2hip_drain*(), the counters or the statsd lines.
 *  - New or seen.  A host-side join, done where the log's join is done: a second-look frame is SEEN iff the log attributed to the same
 *    record a main-path frame with the same len and the same octets (compared as len plus a 64-bit FNV-1a hash taken when the feed's
 *    frames are collected); otherwise it is NEW, and frames_new counts the NEW ones with avlc_status OK; new_mask says which of the
 *    attempt's first 32 frames they are.  The join inherits the log's
 *    one stated dependence on the cuts: a frame delivered after its transmission's record was emitted is not attributed to it.
 *    VDL2HIP_RELOOK_NEW_ONLY delivers only the attempts with frames_new > 0 (filtered on the host, like its neighbours). */
#define VDL2HIP_RELOOK_NEW_ONLY     1u         /* vdl2hip_relook_cfg.flags */
#define VDL2HIP_RELOOK_PPM_REJECT   2u         /* vdl2hip_relook.flags (bit 0 is VDL2HIP_TX_PARTIAL) */
#define VDL2HIP_RELOOK_TRUNCATED    4u
#define VDL2HIP_RELOOK_NO_ROOM      8u
typedef struct {
	uint32_t struct_size, flags;               /* flags: VDL2HIP_RELOOK_NEW_ONLY */
	float    threshold, max_ppm;               /* 0: 4.0f; 0: no gate */
	uint32_t max_anchors, pool_frames, pool_octets, reserved;      /* 0: 4, and the pools' defaults ("Room"); reserved must be 0 */
} vdl2hip_relook_cfg;                          /* 32 bytes */
typedef struct {
	uint32_t chan, freq;                  /* as in vdl2hip_tx */
	uint64_t first_bin;                   /* the join key with vdl2hip_tx and vdl2hip_tx_search */
	int64_t  anchor, end_sample;
	float    pherr, slope, ppm_error, prev_phase;
	uint32_t tl_bits, nsym, synd_weight;
	int32_t  stop;
	uint32_t frames, frames_ok, frames_new;    /* frames_new: filled in by the host from the log's join */
	int32_t  fec_corrections;
	uint32_t frame_first, flags;
	uint32_t new_mask, reserved;          /* new_mask: bit k set iff frame k of the attempt (k < 32) is NEW and passes the AVLC front door; filled in by the host */
	uint64_t counters[VDL2HIP_NUM_COUNTERS];
} vdl2hip_relook;                              /* 256 bytes */
typedef struct {
	uint32_t struct_size, flags;               /* as in force */
	float    threshold, max_ppm;
	uint32_t max_anchors, pool_frames, pool_octets, reserved;
	uint64_t records, anchors_found, attempts; /* of the feeds collected so far: log records looked at, anchors, attempt records */
	uint64_t frames, frames_ok, frames_new, dropped;
	float    kernel_ms;                        /* summed HIP-event time of the second look's launches at profiling level 2, else 0 */
	uint32_t reserved2;
} vdl2hip_relook_info;                         /* 96 bytes */

/* Transmission capture (not in the reference): for every transmission the transmission log closes, the channel's decimated samples
 * around it and a compact spectral signature of the channel during it - where in the 25 kHz the energy sat and how wide it was.  The
 * burst capture shows only bursts whose header decoded; this tap is the evidence for the records with frames_ok == 0: a D8PSK burst,
 * an AM voice carrier, a stuck carrier and a neighbour's splatter look nothing alike in 400 Hz bins.  Off unless enabled; with it off
 * nothing is launched or allocated and every result is what it was, to the bit.  On, frames, counters, the decimated stream, the
 * activity monitor, the log, the search and the burst capture are still exactly what they were.
 *  - Dependencies and switching.  The tap sits on top of the transmission log: vdl2hip_txcap_enable() with the log off is
 *    VDL2HIP_E_INVAL.  It is independent of the preamble search: either, both or neither may run.  vdl2hip_txlog_enable(),
 *    vdl2hip_txlog_disable(), vdl2hip_activity_enable() and vdl2hip_activity_disable() switch a running capture off first, as they do
 *    the search.
 *  - Placement and records.  The tap runs behind the frame finisher of the feed that closes the transmission: the preamble search's
 *    placement, with the same caveat about a later feed's referee.  It reads the log's records of that feed and y, and writes buffers
 *    of its own.  One record per record the log wrote to its pool, in the log's order, feed by feed; (chan, first_bin) is the join
 *    key with vdl2hip_tx and vdl2hip_tx_search.
 *  Below, B and H are the monitor's bin_samples and hang_bins; first_sample and last_sample are the log record's.
 *  - IQ window (with VDL2HIP_TXCAP_IQ).  win_first = max(0, first_sample - pre_samples, last_sample - 57 343), win_last = last_sample
 *    + post_samples.  pre_samples <= 4096; post_samples <= (H + 1) B, a larger value is refused at enable: the samples up to
 *    last_sample + (H + 1) B exist when the record is emitted, whatever the cuts, so the window depends on the stream alone.
 *    VDL2HIP_TXC_CLIPPED is set iff last_sample - 57 343 > max(0, first_sample - pre_samples).  Nothing is read further back than the
 *    preamble search reads, and like it vdl2hip_txcap_enable() refuses a monitor with (H + 1) B > 4096.
 *    iq_count = min(win_last - win_first + 1, max_iq_samples), max_iq_samples 0 meaning no limit: the FIRST iq_count samples of the
 *    window are delivered, so the start of a transmission survives; VDL2HIP_TXC_TRUNCATED is set if the limit bit.  The values are
 *    y_c[win_first ...] as they stand at that point, bit for bit.  (win_first and win_last are stated without VDL2HIP_TXCAP_IQ too;
 *    iq_count is 0 then.)
 *  - IQ pool.  pool_samples pairs per feed in flight (0 means 2^20; above 2^24 is refused).  Offsets are the exclusive prefix sum of
 *    iq_count in record order; a window that ends beyond the pool gets iq_count = 0 and VDL2HIP_TXC_NO_ROOM, and
 *    vdl2hip_txcap_info.iq_dropped counts these.  Offsets only grow, so what survives is a prefix.  (The burst capture's rules.)
 *  - Spectrum (with VDL2HIP_TXCAP_SPECTRUM).  Extent: e_first = max(first_sample, last_sample - 57 343), e_last = last_sample - the
 *    preamble search's range, without pre or post -, len = e_last - e_first + 1.  N = nfft, one of 64, 128, 256, 512, 1024 (0 means
 *    256); the hop is N / 2;  S = len >= N ? (len - N) / (N / 2) + 1 : 0;  segment s covers e_first + s N / 2 .. + N - 1.  w[] is what
 *    vdl2hip_spectrum_window(N, window) returns.
 *      X_s[k] = sum_n w[n] y[e_first + s N / 2 + n] exp(-2 pi i k n / N)   in float32: the input monitor's transform, its twiddle table
 *      q_s[i] = |X_s[(i + N / 2) mod N]|^2                                  two products and a sum in float32
 *      power[i] = (float)((sum_s (double)q_s[i]) norm / S),  norm = 1 / (sum w)^2 in double
 *    The sum over s is float64 in an order that is a function of S and N alone (no atomics).  Bin i lies at freq + (i - N / 2)
 *    105000 / N Hz.  S = 0 sets VDL2HIP_TXC_SHORT and segments = 0; power[] is all zero.
 *  - Spectrum room.  The first pool_spectra records of a feed get a spectrum (0 means 1024; pool_spectra N > 2^24 is refused).  Later
 *    records get VDL2HIP_TXC_NO_SPECTRUM and no power[]; vdl2hip_txcap_info.spectra_dropped counts them.
 *  - Determinism.  The same sequence of calls gives the same bytes.  Every integer field - win_*, iq_count before room, segments, the
 *    flags other than the two room flags - depends on the stream alone, not on the cuts.  For the same y_c, power[] is the same bytes
 *    however the stream was cut and however the kernel splits the work.
 *  - Accuracy of power[].  Against the float64 definition on the same y, per segment the monitor's own bound holds ("Spectrogram":
 *    b_s[i] with e = log2 N 2^-24); power[i] lies within the mean of b_s[i] over the segments plus one float32 rounding.
 *  - Outcome.  frames and frames_ok are copied from the log's join on the host.  VDL2HIP_TXCAP_UNDECODED_ONLY delivers only the
 *    records with frames_ok == 0 (filtered on the host, like the log's: the device captures everything and vdl2hip_txcap_info counts
 *    everything).  A stated limit: on a busy band the pools fill with decoded transmissions; max_iq_samples, the pools and the room
 *    flags are the control.
 *  - vdl2hip_txcap_measure() turns a power[] into four figures (below).  No thresholds and no classification are in the library.
 *  - chan is the index in cfg.freqs.  Groups get no group call: vdl2hip_group_ctx(g, k) is the handle. */
#define VDL2HIP_TXCAP_IQ             1u        /* vdl2hip_txcap_cfg.flags: at least one of _IQ and _SPECTRUM */
#define VDL2HIP_TXCAP_SPECTRUM       2u
#define VDL2HIP_TXCAP_UNDECODED_ONLY 4u
#define VDL2HIP_TXC_CLIPPED          2u        /* vdl2hip_tx_capture.flags (bit 0 is VDL2HIP_TX_PARTIAL, passed on from the log's record) */
#define VDL2HIP_TXC_TRUNCATED        4u
#define VDL2HIP_TXC_NO_ROOM          8u
#define VDL2HIP_TXC_SHORT            16u
#define VDL2HIP_TXC_NO_SPECTRUM      32u
typedef struct {
	uint32_t struct_size, flags, pre_samples, post_samples, max_iq_samples, nfft, window, pool_samples, pool_spectra, reserved;
} vdl2hip_txcap_cfg;                           /* 40 bytes; reserved must be 0; window: VDL2HIP_WIN_* */
typedef struct {
	uint32_t chan, freq;                  /* as in vdl2hip_tx */
	uint64_t first_bin;                   /* the join key with vdl2hip_tx and vdl2hip_tx_search */
	int64_t  win_first, win_last;
	uint64_t iq_off, spec_off;            /* pairs / floats into the caller's buffers of that vdl2hip_txcap_read() */
	uint32_t iq_count, flags, segments, nfft;   /* flags: VDL2HIP_TXC_* | VDL2HIP_TX_PARTIAL; nfft: floats of power[], 0 without a spectrum */
	uint32_t frames, frames_ok, reserved[2];    /* frames, frames_ok: filled in by the host from the log's join */
} vdl2hip_tx_capture;                          /* 80 bytes */
typedef struct {
	uint32_t struct_size, flags, pre_samples, post_samples, max_iq_samples, nfft, window, pool_samples, pool_spectra, reserved;   /* as in force */
	uint64_t records, iq_samples, iq_dropped, spectra, spectra_dropped;   /* of the feeds collected so far: records, pairs, windows without room, spectra, records beyond pool_spectra */
	float    kernel_ms;                        /* summed HIP-event time of the tap's launches at profiling level 2, else 0 */
	uint32_t reserved2;
} vdl2hip_txcap_info;                          /* 88 bytes */
typedef struct {
	double   total, peak_hz, centroid_hz, obw_hz;
	uint32_t peak_bin, obw_lo, obw_hi, reserved;
} vdl2hip_tx_shape;                            /* 48 bytes */

/* Burst timing (not in the reference, whose sync grid evaluates every third decimated sample and rounds a parabola vertex to a whole
 * one, demod.c:173-183): for every burst handed to the burst decoder, the correlation of the channel's DECIMATED stream with the one
 * part of the burst whose waveform is known in advance - the 16-symbol unique word - at 2 W + 1 lags round the decoder's own symbol
 * clock: when symbol 0 arrived to a fraction of a sample, how far the decoder's clock and slope were from the signal's, and how well
 * the template fits.  Off unless enabled; with it off nothing is launched or allocated and every result is what it was, to the bit.
 * On, frames, counters, the decimated stream and every other tap are still exactly what they were: a read-only pass behind the frame
 * finisher of each feed, where the burst capture runs.  It is independent of the burst capture: either, both or neither may run.
 *  - Which bursts.  Exactly the burst capture's: every burst whose header decoded, in the feed whose burst decoder decodes it.
 *  - Template.  vdl2hip_toa_template() returns s[0 .. 151) as float32 (re, im) pairs, designed on the host in double and rounded once:
 *    s[n] = sum_{i = 0 .. 15} exp(j P[i]) p((n - 10 i) / 10), P[] the cumulative preamble phases of demod.c:107-124 and
 *    p(t) = sinc(t) cos(0.6 pi t) / (1 - (1.2 t)^2) the raised cosine of roll-off 0.6, untruncated (t is a multiple of 0.1, never
 *    +-1 / 1.2).  Index 0 is the centre of unique-word symbol 0, index 150 that of symbol 15: a template that reaches beyond the outer
 *    centres correlates with the constant-phase ramp-up symbols and is biased.  E_s = sum |s[n]|^2 in double from the float32 table.
 *  - Anchor and lags.  t0 = first_symbol - 160 is where the decoder's own symbol clock puts symbol 0; W = max_lag, 1 <= W <= 32, 0
 *    means 8; nlags = 2 W + 1; dphi is the burst's slope per symbol as the decoder used it.
 *  - Correlation.  For tau = -W .. W: c(tau) = sum_{n = 0 .. 150} u[n] y_c[t0 + tau + n], u[n] = conj(s[n]) (cos th_n, sin th_n),
 *    th_n = -(double)dphi n / 10, cosine and sine computed in double and narrowed to float32, the product float32 (a product and a
 *    fused multiply-add per component).  y_c[m] = 0 for m < 0, and VDL2HIP_TOA_EARLY is set if t0 - W < 0.  Products and sums are
 *    float32 fused multiply-adds from zero in an order that is a function of nothing but n: the taps l, l + 64, l + 128 in that order
 *    for l = 0 .. 63, then a tree over l that adds l + 32, then l + 16, ... l + 1.  P(tau) = re^2 + im^2 of c(tau) in float32 (a
 *    product, a fused multiply-add).  y is taken as it stands when that feed's burst decoder has finished (the burst capture's
 *    placement and its caveat about a later feed's referee).  The samples up to t0 + W + 150 < first_symbol + 32 always exist by
 *    then - a header is 9 symbols - so the record depends on the stream and y alone, not on how the stream was cut into feeds.
 *  - Peak.  peak_lag = the lowest tau among those with the largest P (a float32 >, taken in ascending tau); peak_sample = t0 +
 *    peak_lag.  With a, b, c = P(peak_lag - 1), P(peak_lag), P(peak_lag + 1) widened to double - a neighbour beyond +-W counts as 0 -
 *    den = (a - 2.0 b) + c.  VDL2HIP_TOA_EDGE if |peak_lag| == W, VDL2HIP_TOA_FLAT if den >= 0 (an all-zero window has both);
 *    toa_frac = 0 with either, else (float)(0.5 (a - c) / den).  The arrival of symbol 0's centre is peak_sample + toa_frac on the
 *    sync_sample clock - decimated samples, 105 000 a second, counted from the stream's start - and includes the channel filter's
 *    constant delay: 2.30 samples for the reference's filter at oversample 10, measured with the float64 model on synthetic bursts
 *    (tests/test_toa_definition.py), where the noise-free spread over 28 bursts is 0.014 sample WITH THE SLOPE THE BURST REALLY HAS.
 *    The unique word's waveform is not symmetric, so a slope that is off moves the peak: -0.0058 sample per Hz of dphi's error on the
 *    same run, where the decoder's own slope is up to 24 Hz off and the spread is 0.28 sample (standard deviation 0.084).  cfo_hz
 *    says how far off it was.  peak_lag + toa_frac is the error of the decoder's symbol clock.
 *  - Strength.  peak_power = P(peak_lag); energy = (float)E_y, E_y the float64 sum - per l in ascending tap order, then the same tree -
 *    of the float32 re^2 + im^2 (a product, a fused multiply-add) of the 151 samples under the template at peak_lag;
 *    rho = (float)((double)peak_power / (E_s E_y)), in 0 .. 1: 1 is the template itself; 0 if E_y == 0.
 *  - Carrier.  carrier_phase = the phase of c(peak_lag) by the decoder's double atan2, narrowed.  c_a, c_b = the same products summed
 *    over n = 0 .. 74 and 75 .. 149 (each lane's taps of that range, the same tree); resid = (float)(atan2(Im z, Re z) / 75) with
 *    z = c_b conj(c_a) in double, rad per sample: what the decoder's slope left over; cfo_hz = (float)(((double)dphi / 10 +
 *    (double)resid) 105000 / (2 pi)), of ppm_error's sign (ppm_error freq 1e-6 is the decoder's own figure for the same offset).
 *  - Curve.  The first pool_curves records of a feed (0 means 4096; pool_curves * nlags > 2^24 is refused) also deliver P(-W .. W);
 *    later ones carry VDL2HIP_TOA_NO_CURVE and curve_off 0 - their scalar fields are still valid - and vdl2hip_toa_info.curves_dropped
 *    counts them.  Records never run out.
 *  - Determinism and accuracy.  The same y gives the same bytes however the stream was cut; there are no floating-point atomics.
 *    Against float64 with the same float32 s[]: |c - c64| <= b := (151 + 16) 2^-24 sum_n |s[n]| |y[t0 + tau + n]|, and
 *    |P - P64| <= 2 |c64| b + b^2 + 2^-22 P64.  Everything from "Peak" down except the two phases is exact arithmetic on the delivered
 *    float32 P and on E_y (which is within 151 2^-53 relative of any order); carrier_phase is within asin(min(1, b / |c|)) plus a
 *    float32 ulp, resid within the sum of that for the two halves, over 75.
 *  - Outcome: frames and frames_ok are joined on the host by (chan, burst_ord) exactly as the burst capture's are;
 *    VDL2HIP_TOA_FAILED_ONLY delivers only the records with frames_ok == 0 (filtered on the host: vdl2hip_toa_info counts everything).
 *  - Order: the records of one feed are ordered by (channel, position in the channel's burst list), feeds follow one another in
 *    feed order.  chan is the index in cfg.freqs.  Groups get no group call: vdl2hip_group_ctx(g, k) is the handle for member k. */
#define VDL2HIP_TOA_FAILED_ONLY 1u        /* vdl2hip_toa_cfg.flags */
#define VDL2HIP_TOA_EARLY       1u        /* vdl2hip_burst_toa.flags */
#define VDL2HIP_TOA_EDGE        2u
#define VDL2HIP_TOA_FLAT        4u
#define VDL2HIP_TOA_NO_CURVE    8u
typedef struct { uint32_t struct_size, max_lag, flags, pool_curves; } vdl2hip_toa_cfg;   /* 16 bytes */
typedef struct {
	uint32_t chan, freq;                  /* index in cfg.freqs, Hz */
	int64_t  burst_ord, sync_sample, first_symbol, peak_sample;
	int32_t  peak_lag; uint32_t nlags;
	float    toa_frac, peak_power, energy, rho, carrier_phase, cfo_hz, dphi, resid;
	uint32_t flags, frames, frames_ok;    /* flags: VDL2HIP_TOA_*; frames, frames_ok: filled in by the host */
	uint32_t curve_off;                   /* floats into the caller's buffer of that vdl2hip_toa_read(): P(-W) is curves[curve_off] */
} vdl2hip_burst_toa;                           /* 96 bytes */
typedef struct {
	uint32_t struct_size, max_lag, flags, pool_curves;   /* as in force */
	uint64_t bursts, curves, curves_dropped, early, edge;   /* of the feeds collected so far: records, curves, records beyond pool_curves, with _EARLY, with _EDGE */
	float    kernel_ms;                        /* summed HIP-event time of k_toa at profiling level 2, else 0 */
	uint32_t reserved;
} vdl2hip_toa_info;                            /* 64 bytes */

/* One AVLC frame plus the vdl2_msg_metadata the reference attaches to it
 * (src/output-common.h:31-43).  `octets` is only valid during the callback. */
typedef struct {
	uint32_t chan;              /* index into cfg.freqs */
	uint32_t freq;              /* metadata->freq */
	int32_t  idx;               /* metadata->idx: frame number within the burst */
	uint32_t len;               /* frame length in octets (may be 0, as in the reference) */
	const uint8_t *octets;
	uint32_t synd_weight;
	uint32_t datalen_octets;
	int32_t  num_fec_corrections;
	float    frame_pwr_dbfs;
	float    nf_pwr_dbfs;
	float    ppm_error;
	int64_t  burst_ord;         /* ordinal of the burst on its channel (0,1,...) */
	int64_t  sync_sample;       /* decimated-sample index (105 kS/s clock) at which the preamble locked (a receiver that resamples -
	                             * cfg.input_rate - sees everything (L T - 1) / (2 L) input samples late: one or two of these samples) */
	int64_t  end_sample;        /* decimated-sample index at which the burst was complete */
	/* avlc_parse()'s first checks (src/avlc.c:163-199), done on the device: */
	uint32_t avlc_status;       /* VDL2HIP_AVLC_OK / _TOO_SHORT (len < 11) / _BAD_FCS (crc16_ccitt residue != 0xF0B8) */
	uint32_t dst_addr, src_addr;/* parse_dlc_addr() of octets 0-3 / 4-7: addr:24 | type:3 << 24 | status:1 << 27; 0 unless OK */
} vdl2hip_frame;

enum { VDL2HIP_AVLC_OK = 0, VDL2HIP_AVLC_TOO_SHORT = 1, VDL2HIP_AVLC_BAD_FCS = 2 };

/* Per-channel counters of the AVLC front door = the reference's statsd counters of src/decode.c:466 and
 * src/avlc.c:170-233, in this order */
enum {
	VDL2HIP_ACNT_FRAMES_PROCESSED = 0,  /* avlc.frames.processed */
	VDL2HIP_ACNT_ERR_TOO_SHORT,         /* avlc.errors.too_short */
	VDL2HIP_ACNT_FRAMES_GOOD,           /* avlc.frames.good */
	VDL2HIP_ACNT_ERR_BAD_FCS,           /* avlc.errors.bad_fcs */
	VDL2HIP_ACNT_MSG_AIR2GND, VDL2HIP_ACNT_MSG_AIR2AIR, VDL2HIP_ACNT_MSG_AIR2ALL,   /* avlc.msg.* */
	VDL2HIP_ACNT_MSG_GND2AIR, VDL2HIP_ACNT_MSG_GND2GND, VDL2HIP_ACNT_MSG_GND2ALL,
	VDL2HIP_NUM_AVLC_COUNTERS
};

typedef void (*vdl2hip_frame_cb)(const vdl2hip_frame *frame, void *user);

typedef struct {
	uint64_t feeds;             /* feed calls so far */
	uint64_t input_samples;     /* complex input samples consumed */
	uint64_t chan_samples;      /* channel-samples processed by the TIMED launches of the channeliser kernel (profiling on) */
	uint64_t chanfir_launches;  /* timed launches of the channeliser kernel: feeds with profiling on, except cold-start feeds */
	double   chanfir_ms;        /* summed HIP-event time of those launches */
	double   phase_ms, sync_ms, walk_ms, burst_ms;   /* other kernels, same convention */
	double   nf_ms;             /* noise-floor passes */
	uint64_t bursts;            /* bursts handed to the burst decoder */
	uint64_t frames;            /* frames the burst decoder produced (before the optional AVLC filter of vdl2hip_set_avlc_filter) */
	uint64_t seg_adopted;       /* segmented walk: speculative segments adopted ... */
	uint64_t seg_walked;        /* ... and segments walked sequentially because a burst straddled their start */
	uint64_t front_sync_timeouts; /* channeliser workgroups that stopped waiting for their predecessor's filter state and worked it out
	                               * themselves (one more tile of work each).  The state they compute equals the published one up to fp32
	                               * rounding (a sum instead of a scan), i.e. the first 128 decimated outputs of such a segment may differ
	                               * from a run without fall-backs in their last bit (measured with every workgroup forced to fall back:
	                               * <= 2e-7 of the signal's peak, a fiftieth of the reference's own rounding noise): NOT bit-identical, and
	                               * which workgroups fall back depends on scheduling.  0 with one process per GPU; non-zero where the GPU is time-sliced
	                               * between processes - set VDL2HIP_NO_FUSE=1 there if bit-reproducible output is required */
	uint64_t overflow_feeds;    /* feeds in which a device-side burst/frame/octet buffer ran out (bursts or frames were dropped);
	                             * vdl2hip_sync() returns VDL2HIP_E_OVERFLOW for those, the drain calls only count here */
	uint64_t cold_start_feeds;  /* large page-locked blocks fed to an idle receiver: copied and channelised in pieces (vdl2hip_feed_pinned);
	                             * their channeliser launches are not in chanfir_ms / chanfir_launches */
	/* The referee.  The channeliser's samples are what exact arithmetic gives; the reference's own fp32 scan (src/demod.c:302-329) differs
	 * from that by its rounding noise (<= 1.5e-4 of the local amplitude).  A decision of the reference that could come out differently
	 * within that distance - candidate test, parabola vertex, --max-ppm gate (src/demod.c:173-192), a symbol at a slicer boundary
	 * (:256-264) - is taken on the reference's own samples, recomputed by running its scan sequentially over the raw input: */
	uint64_t referee_scans;     /* such scans run (3.3 ms each by one wavefront, or 32 side by side by a workgroup) */
	uint64_t referee_cached;    /* requests for a stretch that had been made exact already */
	uint64_t referee_refused;   /* requests that could not be served (the raw input was no longer held): the decision stayed as it was */
	uint64_t referee_short;     /* scans whose run-up was shorter than configured (early in a stream of short blocks) */
	uint64_t referee_rewalks;   /* channels walked again because a decision taken on the channeliser's samples did not stand on the reference's */
	uint64_t referee_candidate_scans, referee_header_scans, referee_symbol_scans;   /* referee_scans by the decision that asked: a preamble candidate
	                             * (candidate test / vertex / gate), a header symbol, the symbols of a burst */
	uint64_t referee_redone_next; /* ABI 6.  A feed's walk no longer waits for the check of the feed before (it starts from that feed's unchecked end
	                             * state; referee_rewalks counts the channels walked again after a check): how often such a second walk ended in
	                             * a DIFFERENT state or counters, so that the next feed was walked once more for that channel as well */
	uint64_t referee_unmet;     /* ABI 6.  Scans (of those run side by side: all of a long feed's) whose zero-start trajectory had NOT become
	                             * bit-identical to a witness trajectory started elsewhere by the stretch's first output - the run-up (196 608
	                             * input samples; VDL2HIP_REF_WARM) was too short for it to have forgotten its start: that stretch is within the
	                             * reference's rounding noise of the reference's samples, not bit for bit them.  Counted here: those that could
	                             * NOT be run again (below).  A monitor, not a proof: a scan can meet its witness before it meets the reference's
	                             * trajectory (measured share of stretches that are not the reference's bit for bit: DESIGN 5) */
	uint64_t referee_retried;   /* ABI 6.  ... and those that were: listed and scanned again from twice as far back (VDL2HIP_REF_RETRY) */
	uint64_t resampled_samples; /* receivers with cfg.input_rate: samples of the resampled stream r[] made so far (0 otherwise) */
	double   resample_ms;       /* ... and the summed HIP-event time of the resampler's launches (profiling level 2, like the other stages) */
	uint64_t referee_symbol_pieces_ahead;   /* ABI 6 (at the structure's end).  Pieces of bursts (1 024 decimated samples each) that hold a symbol within the
	                             * margin, listed right behind the feed's walk and scanned in the same launch as the walk's noted decisions: the
	                             * burst decoder then finds them done and a feed's chain holds one round of scans, not two */
	uint64_t referee_symbol_pieces_late;    /* ... and those the burst decoder's first pass still had to list for a scan round and a second pass of its own:
	                             * bursts of a channel that the check had stitched again, what a full list left over, refused scans */
} vdl2hip_stats;

int  vdl2hip_abi_version(void);
const char *vdl2hip_strerror(int err);

/* = vdl2_channel_init() x nchan + input_lpf_init() + sincosf_lut_init() + demod_sync_init() + rs_init() */
int  vdl2hip_create(const vdl2hip_cfg *cfg, vdl2hip_ctx **out);
void vdl2hip_destroy(vdl2hip_ctx *ctx);

/* = process_buf_uchar()/process_buf_short(): one block of raw IQ from host memory (cfg.sample_fmt says what the bytes are;
 * a trailing part of a sample is dropped).
 * Returns after the block has been queued on the device (the copy out of `buf` is complete).  The copy runs on a
 * stream of its own into one of six device buffers (one per block in flight), so it overlaps the kernels of the blocks fed before. */
int  vdl2hip_feed(vdl2hip_ctx *ctx, const void *buf, size_t nbytes);
/* Same for page-locked host memory (hipHostMalloc / hipHostRegister), without waiting for the copy: the call only queues.
 * `buf` must stay unmodified until the NEXT vdl2hip_feed*() call or vdl2hip_sync() has returned - i.e. a producer
 * alternating between two pinned buffers never waits for the device.  (A block of 8 MiB or more handed to an idle receiver
 * is copied in four pieces with the channeliser following piece by piece, so that the first block of a stream does not wait
 * for its whole transfer; results do not depend on it.) */
int  vdl2hip_feed_pinned(vdl2hip_ctx *ctx, const void *buf, size_t nbytes);
/* Same, for a block that already lives in this device's memory (e.g. the
 * destination of an RCCL broadcast).  `dev_buf` must be aligned to a sample (2, 4 or 8 bytes), else VDL2HIP_E_INVAL.  The block must stay valid until it has been drained
 * (vdl2hip_sync(), or a drain that covers it - see vdl2hip_set_drain_lag). */
int  vdl2hip_feed_device(vdl2hip_ctx *ctx, const void *dev_buf, size_t nbytes);

/* Pipelining.  A feed call only queues work: the sample-rate front (K1-K3) of blocks i+1, i+2 may run while the
 * burst-rate back (K4-K5) of block i is still in flight.  By default the drain functions wait for everything (lag 0 =
 * the reference's blocking behaviour).  With lag L (1 .. VDL2HIP_MAX_DRAIN_LAG) they deliver every block except the L most recent ones,
 * so a feed/drain loop keeps L+1 blocks in flight; vdl2hip_sync() always completes everything. */
#ifndef VDL2HIP_MAX_DRAIN_LAG
#define VDL2HIP_MAX_DRAIN_LAG 5       /* feeds that may be under way undelivered: lag 0 .. 5 (ABI 6; 3 before) */
#endif
int  vdl2hip_set_drain_lag(vdl2hip_ctx *ctx, int lag);

/* Wait for all queued blocks; moves finished frames to the host-side queue. */
int  vdl2hip_sync(vdl2hip_ctx *ctx);
/* sync + deliver every queued frame, ordered by (end_sample, chan, idx); returns the number delivered (>= 0). */
int  vdl2hip_drain(vdl2hip_ctx *ctx, vdl2hip_frame_cb cb, void *user);

/* Bulk form of vdl2hip_drain for callers that want no per-frame callback: copies up to `cap_frames`
 * frame records (same order; `octets` is NULL, `octets_off` below locates the payload) and their octets,
 * concatenated, into caller memory.  Returns the number of frames copied; frames that did not fit stay queued. */
typedef struct {
	vdl2hip_frame frame;
	uint64_t octets_off;
} vdl2hip_packed_frame;
int  vdl2hip_drain_packed(vdl2hip_ctx *ctx, vdl2hip_packed_frame *frames, size_t cap_frames,
		uint8_t *octets, size_t cap_octets, size_t *octets_used);

/* Serialise one frame in the reference's raw-frame archive format, i.e. what `--output raw:binary:file:...`
 * writes and `--raw-frames-file` reads back: 2-byte big-endian record length (payload + 2) followed by the
 * proto3 message dumpvdl2.raw_avlc_frame { vdl2_msg_metadata metadata = 1; bytes data = 2; }
 * (proto/dumpvdl2.proto:24-47, src/fmtr-binary.c:28-60, src/output-file.c:176-192, reader
 * src/input-raw_frames_file.c:33-107).  `frame->octets` must be valid.  Needs no GPU.
 * Returns the number of bytes written, or VDL2HIP_E_TOOBIG if `cap` is too small / the record exceeds 65535. */
int  vdl2hip_pack_raw_frame(const vdl2hip_frame *frame, const char *station_id, int64_t tv_sec, int64_t tv_usec,
		uint8_t *out, size_t cap);

int  vdl2hip_counters(vdl2hip_ctx *ctx, uint32_t chan, uint64_t out[VDL2HIP_NUM_COUNTERS]);
int  vdl2hip_avlc_counters(vdl2hip_ctx *ctx, uint32_t chan, uint64_t out[VDL2HIP_NUM_AVLC_COUNTERS]);
/* Deliver only frames that pass the AVLC front door (avlc_parse() returns NULL for the others, src/avlc.c:171,186): with
 * `on` the drain functions skip frames whose avlc_status is not OK.  Counters are unaffected.  Default off: every frame
 * reaches the callback, as every frame reaches avlc_decoder_queue_push() in the reference. */
int  vdl2hip_set_avlc_filter(vdl2hip_ctx *ctx, int on);
/* The reference's statsd traffic (src/statsd.c:34-65,153-160) in aggregate: one "<ns>.<freq>.<counter>:<delta>|c" line per
 * counter that changed since the previous call (all counters, with :0, on the first call, like
 * statsd_initialize_counters_per_channel()).  `ns` is the namespace ("dumpvdl2" or "dumpvdl2.<station_id>").  Returns the
 * number of bytes written (excluding the terminating NUL) or VDL2HIP_E_TOOBIG if `cap` is too small (nothing is consumed). */
int  vdl2hip_statsd_lines(vdl2hip_ctx *ctx, const char *ns, char *out, size_t cap);
int  vdl2hip_set_profiling(vdl2hip_ctx *ctx, int level); /* 0 off; 1 time the channeliser kernel (start/stop events attached to
                                                          * its launch); 2 time every stage the same way (costs ~5 % throughput) */
int  vdl2hip_get_stats(vdl2hip_ctx *ctx, vdl2hip_stats *out);
int  vdl2hip_get_stats_sized(vdl2hip_ctx *ctx, vdl2hip_stats *out, size_t size);   /* writes at most `size` bytes: for a caller built against an older header */
void *vdl2hip_stream(vdl2hip_ctx *ctx);                 /* the hipStream_t all work is queued on */

/* ---- One receiver over several GPUs of this process (src/dumpvdl2.c:117-135: one worker per channel over a shared block;
 * here the workers are grouped by device).  Member k of n decodes channels [k*nchan/n, (k+1)*nchan/n) of cfg->freqs on
 * devices[k]; cfg->device, chan_first and chan_count are ignored/must be 0.  A block handed to vdl2hip_group_feed() is put on
 * every member in one of two ways (vdl2hip_group_set_exchange(), or VDL2HIP_GROUP_EXCHANGE=allgather|broadcast at create):
 *   VDL2HIP_GROUP_ALLGATHER (default)  the block is cut into n stripes; member k copies stripe k from `buf` over ITS OWN PCIe
 *                                      link, then fetches the stripes it lacks from its peers over xGMI, all links at once;
 *   VDL2HIP_GROUP_BROADCAST            the whole block crosses PCIe once, into devices[0], and is sent from there to the others
 *                                      (BASELINE's literal form; bound by that one host copy).
 * Both give every member the same bytes, hence the same frames.  Data moves with hipMemcpyPeerAsync - the path that has run on
 * hardware; a device may be listed more than once ("virtual shards", which is how the path is tested on one GPU).  RCCL
 * (ncclAllGather / ncclBroadcast, loaded at run time) is used only with VDL2HIP_USE_RCCL=1 in the environment: those calls have
 * been built and reviewed but not yet run on a multi-GPU node (tests/test_gpu_parity.py::test_group_over_two_real_gpus covers them
 * where two GPUs are visible); a failing RCCL call falls back to peer copies.  Frames are delivered merged, in vdl2hip_drain()'s
 * order.  A failure part-way through a group feed disables the group (every later call returns VDL2HIP_E_DEVICE). ---- */
typedef struct vdl2hip_group vdl2hip_group;
enum { VDL2HIP_GROUP_ALLGATHER = 0, VDL2HIP_GROUP_BROADCAST = 1 };
int  vdl2hip_group_create(const vdl2hip_cfg *cfg, const int32_t *devices, uint32_t ndev, vdl2hip_group **out);
void vdl2hip_group_destroy(vdl2hip_group *g);
int  vdl2hip_group_feed(vdl2hip_group *g, const void *buf, size_t nbytes);      /* = process_buf_*(), blocking like vdl2hip_feed() */
/* the same from page-locked memory without waiting for the copy (the rule of vdl2hip_feed_pinned(): `buf` stays untouched until the
 * next vdl2hip_group_feed*() or vdl2hip_group_sync() has returned) */
int  vdl2hip_group_feed_pinned(vdl2hip_group *g, const void *buf, size_t nbytes);
int  vdl2hip_group_sync(vdl2hip_group *g);
int  vdl2hip_group_drain(vdl2hip_group *g, vdl2hip_frame_cb cb, void *user);
int  vdl2hip_group_set_drain_lag(vdl2hip_group *g, int lag);
int  vdl2hip_group_counters(vdl2hip_group *g, uint32_t chan, uint64_t out[VDL2HIP_NUM_COUNTERS]);
int  vdl2hip_group_avlc_counters(vdl2hip_group *g, uint32_t chan, uint64_t out[VDL2HIP_NUM_AVLC_COUNTERS]);
uint32_t vdl2hip_group_size(vdl2hip_group *g);
vdl2hip_ctx *vdl2hip_group_ctx(vdl2hip_group *g, uint32_t member);            /* for the per-context calls above (stats, statsd, ...) */
int  vdl2hip_group_uses_rccl(vdl2hip_group *g);                                /* 1: RCCL loaded and in use, 0: peer copies */
int  vdl2hip_group_set_exchange(vdl2hip_group *g, int form);                   /* VDL2HIP_GROUP_ALLGATHER / _BROADCAST, for the feeds that follow */
/* what the last feed did: 0 broadcast by peer copies, 1 broadcast by RCCL, 2 all-gather by peer copies, 3 all-gather by RCCL; -1 before the first feed */
int  vdl2hip_group_exchange(vdl2hip_group *g);

/* Introspection used by the parity tests (host copies of what the kernels use) */
int  vdl2hip_get_lpf(vdl2hip_ctx *ctx, float A[3], float B[3]);      /* = static A/B of src/demod.c:55 */
int  vdl2hip_get_nco_step(vdl2hip_ctx *ctx, uint32_t chan, uint32_t *dphi); /* = v->downmix_dphi */
/* Copy up to `cap` decimated (re,im) pairs of one channel starting at decimated index `first`
 * (must still be inside the device history window); returns the count copied. */
int  vdl2hip_read_decimated(vdl2hip_ctx *ctx, uint32_t chan, int64_t first, float *dst, size_t cap);
/* Copy up to `cap` (re,im) pairs of the resampled stream r[first ...] (receivers with cfg.input_rate; VDL2HIP_E_INVAL on any other).
 * The device keeps the last six feeds' output: at least the whole most recent feed is readable.  Returns the count copied. */
int  vdl2hip_read_resampled(vdl2hip_ctx *ctx, int64_t first, float *dst, size_t cap);
/* The resampler's design for input_rate -> output_rate (= 105000 * oversample), on the host in double precision, no GPU needed: writes
 * L, M, T (taps per phase) and, if they fit in `cap` floats, the L T taps in prototype order h[j L + p].  Returns L T, VDL2HIP_E_TOOBIG
 * if `cap` is too small (L, M, T are written all the same; taps may be NULL then), VDL2HIP_E_INVAL for the ratios vdl2hip_create() refuses. */
int  vdl2hip_resampler_design(uint32_t input_rate, uint32_t output_rate, uint32_t *L, uint32_t *M, uint32_t *T, float *taps, size_t cap);

/* ---- Input monitor (see "Input monitor" above) ----
 * The window: returns nfft and writes w[0 .. nfft) if cap >= nfft, else VDL2HIP_E_TOOBIG; VDL2HIP_E_INVAL for an nfft or a window
 * that is not taken.  Host only, needs no GPU. */
int  vdl2hip_spectrum_window(uint32_t nfft, uint32_t window, float *w, size_t cap);
/* Switch the monitor on (or, with nfft 0, off: its buffers are freed).  Allowed at any time between feeds; takes effect with the next
 * feed, zeroes the accumulators and restarts the sample count i at 0.  VDL2HIP_E_INVAL for a bad struct_size, nfft or window, before
 * anything is allocated or changed. */
int  vdl2hip_spectrum_enable(vdl2hip_ctx *ctx, const vdl2hip_spectrum_cfg *cfg);
/* What the monitor has accumulated.  Waits only for the monitor's own work queued so far (an event behind its last launch), delivers
 * no frames and changes nothing in what vdl2hip_drain() or vdl2hip_sync() later return.  info->struct_size must be set; `info` or
 * `power` may be NULL; power[0 .. nfft) needs cap >= nfft, else VDL2HIP_E_TOOBIG.  `reset` zeroes the accumulators after the copy;
 * the position i runs on, so later segments stay where they were.  Monitor off: VDL2HIP_E_INVAL.  Returns nfft. */
int  vdl2hip_spectrum_read(vdl2hip_ctx *ctx, vdl2hip_spectrum_info *info, double *power, size_t cap, int reset);
/* The level of every channel c of cfg.freqs (all nchan of them, not only this shard's), host arithmetic on the same accumulators:
 * with B_c = { i : |f_i - freqs[c]| <= 12500 Hz }, or the single nearest bin if that set is empty,
 * dbfs[c] = 10 log10(sum_{B_c} power[i] / enbw_bins), -INFINITY if the sum is 0.  Returns nchan; VDL2HIP_E_TOOBIG if cap < nchan. */
int  vdl2hip_spectrum_channels(vdl2hip_ctx *ctx, float *dbfs, size_t cap);

/* ---- Spectrogram (see "Spectrogram" above) ----
 * Switch the tap on.  Allowed between feeds with the input monitor on; takes effect with the next feed.  VDL2HIP_E_INVAL for the
 * monitor off, a bad struct_size, reserved, line_segments or ring_lines, before anything is allocated or changed: a tap that was on
 * stays as it was. */
int  vdl2hip_specgram_enable(vdl2hip_ctx *ctx, const vdl2hip_specgram_cfg *cfg);
int  vdl2hip_specgram_disable(vdl2hip_ctx *ctx);
/* The holds.  Waits only for the monitor's own work queued so far (its event and read stream, as vdl2hip_spectrum_read() does) and
 * delivers no frames.  info->struct_size must be set; info, max_hold and floor_hold may each be NULL; an array given needs
 * cap >= nfft, else VDL2HIP_E_TOOBIG.  `reset`: see above.  Tap off: VDL2HIP_E_INVAL.  Returns nfft. */
int  vdl2hip_specgram_read(vdl2hip_ctx *ctx, vdl2hip_specgram_info *info, float *max_hold, float *floor_hold, size_t cap, int reset);
/* Lines first_line .. of the ring, at most cap_lines of them, row-major [line][nfft]; mean or max may be NULL.  Returns the count
 * (0 is legal for first_line == lines); VDL2HIP_E_INVAL for a line older than the ring holds or beyond `lines`. */
int  vdl2hip_specgram_lines(vdl2hip_ctx *ctx, int64_t first_line, float *mean, float *max, size_t cap_lines);
/* Host arithmetic on the hold arrays, for all nchan channels of cfg.freqs, with vdl2hip_spectrum_channels()'s bin set B_c:
 * peak_dbfs[c] = 10 log10(max over B_c of max_hold[i])                  - tone-referred: the strongest bin
 * floor_dbfs[c] = 10 log10(sum over B_c of floor_hold[i] / enbw_bins)   - the channel's floor in its bandwidth
 * -INFINITY where the argument is 0; either array may be NULL; returns nchan; VDL2HIP_E_TOOBIG if cap < nchan. */
int  vdl2hip_specgram_channels(vdl2hip_ctx *ctx, float *peak_dbfs, float *floor_dbfs, size_t cap);

/* ---- Activity monitor (see "Activity monitor" above) ----
 * The histogram's 63 edges: returns 63 and writes edges[0 .. 63) if cap >= 63, else VDL2HIP_E_TOOBIG.  Host only, needs no GPU. */
int  vdl2hip_activity_edges(float *edges, size_t cap);
/* Switch the monitor on.  Allowed between feeds; takes effect with the next feed.  Enabling again restarts at the then-current
 * decimated sample with zeroed state.  VDL2HIP_E_INVAL for a bad struct_size, bin_samples, hang_bins, series_bins, threshold or
 * reserved, before anything is allocated or changed: a monitor that was on stays as it was.  A transmission log that is running is
 * switched off first (vdl2hip_txlog_disable()). */
int  vdl2hip_activity_enable(vdl2hip_ctx *ctx, const vdl2hip_activity_cfg *cfg);
/* Switch it off: its buffers are freed, later feeds launch nothing.  A transmission log that is running is switched off first. */
int  vdl2hip_activity_disable(vdl2hip_ctx *ctx);
/* What the monitor has accumulated.  Waits only for the monitor's own work queued so far (an event behind its last launch), delivers
 * no frames and changes nothing in what vdl2hip_drain() or vdl2hip_sync() later return.  info->struct_size must be set.  chans[i] is
 * channel chan_first + i; returns the number of channels written (0 if chans is NULL), VDL2HIP_E_TOOBIG if cap_chans is smaller than
 * the shard's channel count.  `info` or `chans` may be NULL.  Monitor off: VDL2HIP_E_INVAL. */
int  vdl2hip_activity_read(vdl2hip_ctx *ctx, vdl2hip_activity_info *info, vdl2hip_activity_chan *chans, size_t cap_chans, int reset);
/* Copy up to `cap` values p[first_bin ...] of one channel (index in cfg.freqs); returns the count (0 is legal for first_bin ==
 * info.bins).  VDL2HIP_E_INVAL for a bin older than what the ring holds or beyond bins, a channel outside the shard, the monitor off. */
int  vdl2hip_activity_series(vdl2hip_ctx *ctx, uint32_t chan, int64_t first_bin, float *dst, size_t cap);

/* ---- Burst capture (see "Burst capture" above) ----
 * Switch the capture on.  Allowed between feeds; takes effect with the next feed.  Enabling again collects the feeds under way, drops
 * what is queued unread and starts afresh.  VDL2HIP_E_INVAL for a bad struct_size, pre_samples, post_samples, flags, pool_samples or
 * reserved, before anything is allocated or changed: a capture that was on stays as it was. */
int  vdl2hip_capture_enable(vdl2hip_ctx *ctx, const vdl2hip_capture_cfg *cfg);
/* Switch it off: the feeds under way are collected, its buffers and what is queued unread are freed, later feeds launch nothing. */
int  vdl2hip_capture_disable(vdl2hip_ctx *ctx);
/* The configuration in force and the totals so far; info->struct_size must be set.  Capture off: VDL2HIP_E_INVAL. */
int  vdl2hip_capture_info_get(vdl2hip_ctx *ctx, vdl2hip_capture_info *info);
/* Like vdl2hip_drain_packed(): the records of the feeds collected so far (by vdl2hip_sync() or a drain, which respects the drain lag),
 * oldest first, with their windows in iq[] as (re, im) float pairs - record i's at pair recs[i].iq_off.  What does not fit - records
 * or their IQ - stays queued for the next call; the call never waits for the device itself.  Returns the number of records written,
 * *pairs_used the pairs (pairs_used may be NULL).  Capture off: VDL2HIP_E_INVAL. */
int  vdl2hip_capture_read(vdl2hip_ctx *ctx, vdl2hip_burst *recs, size_t cap_recs, float *iq, size_t cap_pairs, size_t *pairs_used);

/* ---- Transmission log (see "Transmission log" above) ----
 * Switch the log on.  Allowed between feeds; takes effect with the next feed: its state is taken from the activity monitor's as it
 * stands behind the feeds queued so far.  Enabling again collects the feeds under way, drops what is queued unread and starts afresh.
 * VDL2HIP_E_INVAL if the activity monitor is off, or for a bad struct_size, pool_records, flags or reserved, before anything is
 * allocated or changed: a log that was on stays as it was. */
int  vdl2hip_txlog_enable(vdl2hip_ctx *ctx, const vdl2hip_txlog_cfg *cfg);
/* Switch it off: the feeds under way are collected, its buffers and what is queued unread are freed, later feeds launch nothing. */
int  vdl2hip_txlog_disable(vdl2hip_ctx *ctx);
/* The configuration in force and the totals so far; info->struct_size must be set.  Log off: VDL2HIP_E_INVAL. */
int  vdl2hip_txlog_info_get(vdl2hip_ctx *ctx, vdl2hip_txlog_info *info);
/* Like vdl2hip_capture_read(): the records of the feeds collected so far (by vdl2hip_sync() or a drain, which respects the drain
 * lag), oldest first.  What does not fit stays queued for the next call; the call never waits for the device itself.  Returns the
 * number of records written.  Log off: VDL2HIP_E_INVAL. */
int  vdl2hip_txlog_read(vdl2hip_ctx *ctx, vdl2hip_tx *recs, size_t cap_recs);

/* ---- Preamble search (see "Preamble search" above) ----
 * Switch the search on.  Allowed between feeds; takes effect with the next feed.  Enabling again collects the feeds under way, drops
 * what is queued unread and starts afresh.  VDL2HIP_E_INVAL if the transmission log is off, for a bad struct_size or flags, a reserved
 * word that is not 0, or an activity monitor with (hang_bins + 1) * bin_samples > 4096, before anything is allocated or changed: a
 * search that was on stays as it was. */
int  vdl2hip_txsearch_enable(vdl2hip_ctx *ctx, const vdl2hip_txsearch_cfg *cfg);
/* Switch it off: the feeds under way are collected, its buffers and what is queued unread are freed, later feeds launch nothing. */
int  vdl2hip_txsearch_disable(vdl2hip_ctx *ctx);
/* The configuration in force and the totals so far; info->struct_size must be set.  Search off: VDL2HIP_E_INVAL. */
int  vdl2hip_txsearch_info_get(vdl2hip_ctx *ctx, vdl2hip_txsearch_info *info);
/* Like vdl2hip_txlog_read(): the records of the feeds collected so far, oldest first.  What does not fit stays queued for the next
 * call; the call never waits for the device itself.  Returns the number of records written.  Search off: VDL2HIP_E_INVAL. */
int  vdl2hip_txsearch_read(vdl2hip_ctx *ctx, vdl2hip_tx_search *recs, size_t cap_recs);

/* ---- Second look (see "Second look" above) ----
 * Switch the second look on.  Allowed between feeds; takes effect with the next feed.  Enabling again collects the feeds under way,
 * drops what is queued unread and starts afresh.  VDL2HIP_E_INVAL if the preamble search is off, for a bad struct_size, an unknown
 * flag, a threshold that is a NaN or outside (0, 30] (0: 4.0f), a max_ppm that is negative or a NaN, max_anchors > 16, pool_frames >
 * 2^20, pool_octets > 2^26 or a reserved word that is not 0, before anything is allocated or changed: a second look that was on stays
 * as it was. */
int  vdl2hip_relook_enable(vdl2hip_ctx *ctx, const vdl2hip_relook_cfg *cfg);
/* Switch it off: the feeds under way are collected, its buffers and what is queued unread are freed, later feeds launch nothing. */
int  vdl2hip_relook_disable(vdl2hip_ctx *ctx);
/* The configuration in force and the totals so far; info->struct_size must be set.  Second look off: VDL2HIP_E_INVAL. */
int  vdl2hip_relook_info_get(vdl2hip_ctx *ctx, vdl2hip_relook_info *info);
/* The attempt records of the feeds collected so far, oldest first, with their frames: record i's recs[i].frames frames are
 * frames[recs[i].frame_first ...], in the burst's order, each frame's len octets at octets[frames[j].octets_off] (frame.octets is
 * NULL).  What does not fit - records, their frames or their octets - stays queued for the next call; the call never waits for the
 * device itself.  Returns the number of records written, *octets_used the octets (may be NULL); the frames written are the sum of
 * recs[i].frames.  Second look off: VDL2HIP_E_INVAL. */
int  vdl2hip_relook_read(vdl2hip_ctx *ctx, vdl2hip_relook *recs, size_t cap_recs, vdl2hip_packed_frame *frames, size_t cap_frames,
                         uint8_t *octets, size_t cap_octets, size_t *octets_used);

/* ---- Transmission capture (see "Transmission capture" above) ----
 * Switch the capture on.  Allowed between feeds; takes effect with the next feed.  Enabling again collects the feeds under way, drops
 * what is queued unread and starts afresh.  VDL2HIP_E_INVAL if the transmission log is off, for a bad struct_size, flags without
 * VDL2HIP_TXCAP_IQ or _SPECTRUM or with an unknown bit, pre_samples > 4096, post_samples > (hang_bins + 1) * bin_samples, an nfft
 * other than 0, 64, 128, 256, 512, 1024, an unknown window, pool_samples > 2^24, pool_spectra * nfft > 2^24, a reserved word that is
 * not 0, or an activity monitor with (hang_bins + 1) * bin_samples > 4096, before anything is allocated or changed: a capture that was
 * on stays as it was. */
int  vdl2hip_txcap_enable(vdl2hip_ctx *ctx, const vdl2hip_txcap_cfg *cfg);
/* Switch it off: the feeds under way are collected, its buffers and what is queued unread are freed, later feeds launch nothing. */
int  vdl2hip_txcap_disable(vdl2hip_ctx *ctx);
/* The configuration in force and the totals so far; info->struct_size must be set.  Capture off: VDL2HIP_E_INVAL. */
int  vdl2hip_txcap_info_get(vdl2hip_ctx *ctx, vdl2hip_txcap_info *info);
/* Like vdl2hip_capture_read(): the records of the feeds collected so far, oldest first, with their windows in iq[] as (re, im) float
 * pairs - record i's at pair recs[i].iq_off - and their spectra in spectra[] - record i's recs[i].nfft floats at recs[i].spec_off, none
 * for a record with VDL2HIP_TXC_NO_SPECTRUM or a capture without VDL2HIP_TXCAP_SPECTRUM.  What does not fit - records, their IQ or
 * their spectra - stays queued for the next call; the call never waits for the device itself.  Returns the number of records written,
 * *pairs_used the pairs and *floats_used the floats (either may be NULL).  Capture off: VDL2HIP_E_INVAL. */
int  vdl2hip_txcap_read(vdl2hip_ctx *ctx, vdl2hip_tx_capture *recs, size_t cap_recs, float *iq, size_t cap_pairs, size_t *pairs_used,
                        float *spectra, size_t cap_floats, size_t *floats_used);
/* Four figures of a power[] of nfft bins (host only, needs no GPU, needs no receiver).  All arithmetic is double, in ascending i, with
 * f_i = (i - nfft / 2) * 105000 / nfft:  total = sum power;  peak_bin = the lowest index of the maximum, peak_hz = f_peak_bin;
 * centroid_hz = sum f_i p_i / total;  obw_hz = (obw_hi - obw_lo + 1) * 105000 / nfft, obw_lo and obw_hi being the smallest i at which
 * the running sum reaches 0.005 total and 0.995 total.  Everything is 0 when total is 0.
 * VDL2HIP_E_INVAL for a NULL pointer or an nfft that is not one of the capture's. */
int  vdl2hip_txcap_measure(const float *power, uint32_t nfft, vdl2hip_tx_shape *out);

/* ---- Burst timing (see "Burst timing" above) ----
 * The template: s[0 .. 151) as (re, im) float pairs.  Host only, needs no GPU, needs no receiver.  Returns 151; VDL2HIP_E_TOOBIG if
 * cap_pairs is smaller, VDL2HIP_E_INVAL for a NULL pointer. */
int  vdl2hip_toa_template(float *s, size_t cap_pairs);
/* Switch the tap on.  Allowed between feeds; takes effect with the next feed.  Enabling again collects the feeds under way, drops
 * what is queued unread and starts afresh.  VDL2HIP_E_INVAL for a bad struct_size, max_lag > 32, an unknown flag or pool_curves *
 * nlags > 2^24, before anything is allocated or changed: a tap that was on stays as it was. */
int  vdl2hip_toa_enable(vdl2hip_ctx *ctx, const vdl2hip_toa_cfg *cfg);
/* Switch it off: the feeds under way are collected, its buffers and what is queued unread are freed, later feeds launch nothing. */
int  vdl2hip_toa_disable(vdl2hip_ctx *ctx);
/* The configuration in force and the totals so far; info->struct_size must be set.  Tap off: VDL2HIP_E_INVAL. */
int  vdl2hip_toa_info_get(vdl2hip_ctx *ctx, vdl2hip_toa_info *info);
/* Like vdl2hip_txcap_read(): the records of the feeds collected so far, oldest first, with their curves in curves[] - record i's
 * recs[i].nlags floats at recs[i].curve_off, none for a record with VDL2HIP_TOA_NO_CURVE.  What does not fit - records or their
 * curves - stays queued for the next call; the call never waits for the device itself.  Returns the number of records written,
 * *floats_used the floats (may be NULL).  Tap off: VDL2HIP_E_INVAL. */
int  vdl2hip_toa_read(vdl2hip_ctx *ctx, vdl2hip_burst_toa *recs, size_t cap_recs, float *curves, size_t cap_floats, size_t *floats_used);

#ifdef __cplusplus
}
#endif
#endif
