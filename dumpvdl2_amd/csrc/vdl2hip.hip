// vdl2hip.hip - libvdl2hip.so: context management and the C ABI of include/vdl2hip.h.
// Host code only orchestrates: every sample-rate or burst-rate computation runs in the
// kernels of kernels.h.  There is deliberately no CPU fallback: without a HIP device
// vdl2hip_create() fails with VDL2HIP_E_DEVICE.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include "../../include/vdl2hip.h"
#include "kernels.h"
#include "resample.h"
#include "resample_design.h"
#include "spectrum.h"
#include "spectrum_design.h"
#include "activity.h"
#include "txlog.h"
#include "txsearch.h"
#include "txcap.h"
#include "capture.h"
#include "toa.h"
#include "relook.h"
#include "tables.h"
#include "hostmem.h"

using namespace vdl2;
using hostmem::DevBuf; using hostmem::PinnedBuf; using hostmem::Event; using hostmem::RecordMail;

static_assert(VDL2HIP_NUM_COUNTERS == kNumCounters, "counter enum out of sync");

namespace {

// a delivered frame: its record plus the octet pool of the feed it came from (one allocation per feed, shared by its frames)
struct HostFrame {
	OutFrame f;
	std::shared_ptr<std::vector<uint8_t>> pool;
	const uint8_t *octets() const { return pool && f.pool_off + f.len <= pool->size() ? pool->data() + f.pool_off : nullptr; }
};

#ifndef VDL2_K1_RUN
#define VDL2_K1_RUN 2
#endif
constexpr int kRun = VDL2_K1_RUN;        // decimated outputs per lane in K1 (specialised builds); 2 measured best: dev/gpu_k1_variants.sh
constexpr int kRunGeneric = 2;
constexpr int kHistory = 65536;          // decimated samples kept behind the newest block (> longest burst, 56 090)
constexpr int kNumEv = 12;            // profiling: {start, stop} of K1, K2, K3, K4, K4b, K5
constexpr int kColdParts = 4;         // pieces a cold-start block is copied and channelised in
constexpr size_t kColdMinBytes = 8u << 20;
constexpr uint32_t kRetryScans = 64;       // referee: scans of one launch that may be run again from further back because they had not met their witness (more: published as they are, counted)
constexpr uint32_t kPreScans = 4096;    // referee: stretches around marked candidates one feed may list for the scan ahead of the walk (what does not fit is asked for by the walk itself)
// referee: bursts of one feed that may wait for their scans, stretches they may wait for.  What does not fit is scanned on the spot, by the
// burst's own wavefront, one stretch after the other at 4.4 ms each: with 256 / 512 (rounds 5, 6a/b) a capture full of weak bursts - config4
// WITHOUT its --max-ppm gate: the neighbours' leakage is locked on to and decoded, a symbol in a few hundred within the margin - ran over
// and a 16-block feed took 68 ms instead of 2 (profiles/r06_weak_bursts.txt).  A short feed lists a sixteenth of these.
// The lists grow with the feed: a stretch per 8 192 channel-samples of the feed (a 16 s block of 256 channels: 52 000; a rank's 32
// channels: 6 500), half as many bursts, at least kDeferScans / kDeferBursts; the grids that serve them are sized the same way - a
// workgroup that finds no request is gone within a microsecond.
constexpr uint32_t kDeferBursts = 4096, kDeferScans = 8192, kDeferScansMax = 1u << 17;
static uint32_t defer_scans_for(int64_t D, int C) {
	const uint64_t want = (uint64_t)(D > 0 ? D : 0) * (uint64_t)C / 8192u;
	const uint64_t cap = std::min<uint64_t>(kDeferScansMax, std::max<uint64_t>(kDeferScans, want));
	return (uint32_t)((cap + 63) / 64 * 64);
}
// Streams per priority class.  The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues per
// priority, round-robin in the order of their creation, and two streams on one queue run one after the other.  With a scan stream and
// a burst stream per slot (four of each), a scan stream shared its queue with the walk stream and burst streams shared theirs with the
// front and the noise-floor stream (all three of the front's priority): every fourth feed's 1.5 ms scan sat in front of the next walks
// (a rank-sized receiver: 2.64 ms per step; 1.91 with GPU_MAX_HW_QUEUES=8 - which in turn cost the 256-channel receiver 4 %:
// profiles/r06_hw_queues_ab.txt).  So: high priority = walk + 3 scan streams, the front's priority = front + noise floor + 2 burst
// streams - four each, nobody shares.  (Feed i + 3's scan, feed i + 2's burst decoder behind feed i's: done long before.)
// The streams of a receiver that is destroyed go to a pool (per device) and the next receiver takes them over: the runtime's mapping
// of streams to queues depends on every stream the process has created so far, and a receiver made after a hundred others had come
// and gone ran 30-60 % slower than the same receiver in a fresh process (bench.py's secondary workloads, round 6).
constexpr int kSidePre = 3, kSideBurst = 2;
// the streams of one receiver: not owned by it - kept when the receiver goes, taken over by the next one on the same device
struct StreamSet {
	int device = -1; hipStream_t front = nullptr, copy = nullptr, out = nullptr, back = nullptr, nf = nullptr, pre[kSidePre] = {}, burst[kSideBurst] = {};
	template<typename F> void each(F f) { for(hipStream_t *p : { &front, &copy, &out, &back, &nf }) f(*p); for(auto &x : pre) f(x); for(auto &x : burst) f(x); }
};
constexpr int kSlots = VDL2HIP_MAX_DRAIN_LAG + 1;   // feeds in flight (vdl2hip_set_drain_lag: at most kSlots - 1 undelivered).  Six: a feed's way through the device of a receiver of few channels - front 1 ms, the scans ahead of the walk 1.5, walk, the next feed's walk (the second walks are queued behind it), burst decoder and its scans 1.5-2.5 - is four to six fronts long (rank-sized receivers, walk ahead: 2.22 / 1.46 / 1.56 ms per step with four slots, 1.76 / 1.29 / 1.45 with six; with 256 channels it is three fronts and four slots were enough)

}  // namespace

// Start / stop events of the (at most two) kernels one tap launches per feed, created when profiling level 2 first asks for them;
// n: how many of the pairs the slot's last feed used.  The runtime stamps the events with the kernels' own start and stop (LAUNCH_EV).
struct KernelTimes {
	Event ev[4]; int n = 0; bool armed = false;
	// (an event that cannot be created leaves the feed untimed, not failed)
	bool arm(bool timed) { armed = timed; if(timed) for(auto &x : ev) if(x.ensure() != hipSuccess) armed = false; return armed; }
	hipEvent_t e(int i) const { return armed ? (hipEvent_t)ev[i] : (hipEvent_t) nullptr; }
	void launched(int pairs) { n = armed ? pairs : 0; }
	// the feed is done (collect_slot): its kernels' durations are added to `ms`
	void collect(double &ms) {
		for(int i = 0; i < n; i++) { float t = 0.f; if(hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) == hipSuccess) ms += t; else (void)hipGetLastError(); }
		n = 0;
	}
};

// Reading a tap's device state behind its last launch: on a stream of the tap's own, behind the event of that launch, so that the
// read waits for nothing else - not for the feeds in flight, not for what the process has on the default stream.  The event, the
// stream and the page-locked landing place stay with the context when the tap is disabled, and go with it.
struct TapRead {
	Event last; bool queued = false; hipStream_t rd = nullptr; PinnedBuf land;
	~TapRead() { if(rd) (void)hipStreamDestroy(rd); }
	hipError_t mark(hipStream_t front) { const hipError_t e = hipEventRecord(last, front); if(e == hipSuccess) queued = true; return e; }
	hipError_t fetch(void *dst_host, const void *src_dev, size_t bytes) {
		hipError_t e = hipStreamWaitEvent(rd, last, 0);
		if(e == hipSuccess) e = hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, rd);
		return e == hipSuccess ? hipStreamSynchronize(rd) : e;
	}
};

// A record tap's share of a slot: whether the slot's feed carries the tap's launches, what they took (profiling level 2), and the
// tap's per-feed buffers B, whose first records come to the host through a RecordMail (hostmem.h).  reset(): the tap is switched off -
// the buffers go as one, the timing events stay with the slot ("Ownership").
template<typename B>
struct TapSlot : B {
	bool on = false; KernelTimes times;
	void reset() { static_cast<B &>(*this) = B{}; on = false; times.n = 0; }
};

struct OutSlot {
	DevBuf<Burst> d_bursts; DevBuf<uint32_t> d_nbchan;
	DevBuf<OutFrame> d_frames; DevBuf<uint8_t> d_pool;
	DevBuf<OutMail> d_mail; OutCtl *d_ctl = nullptr;   // control block + the first few delivered frames, contiguous (d_ctl = &d_mail->ctl, not owned): one small copy brings both
	DevBuf<OutFrame> d_frames_out; DevBuf<uint8_t> d_pool_out;    // what k_frame_finish delivers (no tombstones, no holes): what the host copies
	DevBuf<EvalChunk> d_log; DevBuf<uint32_t> d_nlog;   // the walker's evaluation log of this feed (read by K4b)
	DevBuf<uint32_t> d_dq; DevBuf<ScanReq> d_sq;      // referee, long feeds: the bursts that wait for a scan, the stretches they wait for (counts: d_rqn[1], d_rqn[2])
	DevBuf<ScanReq> d_mq;               // referee: the pieces k_burst_mark lists behind the walk for the check's scan launch (count: d_rqn[7])
	DevBuf<RefReq> d_rq; DevBuf<uint32_t> d_rqn, d_rqflag; DevBuf<RefBad> d_rqbad;
	DevBuf<ScanReq> d_retry;            // [3][kRetryScans]: the unmet scans of the scans ahead of the walk / of the check / of the burst decoder (counts: d_rqn[4..6])
	DevBuf<ScanReq> d_pq; Event ev_pre;      // referee: the stretches around marked candidates, made exact between the front and the walk (count: d_rqn[3])
	PinnedBuf h_mail;                      // an OutMail
	Event done, ev_front, ev_walk, ev_nf, ev[kNumEv];
	bool pending = false, ev_valid = false, fused = false; int ev_level = 0;
	uint64_t seq = 0;
	int64_t back_D = 0, back_k0 = 0;        // the burst-rate back end of this feed (launch_back, launch_rest): its decimated samples, the first one's number
	bool k1_timed = false;                 // the channeliser launch of this feed carries start/stop events (not on a cold-start feed: its pieces wait for copies in between)
	bool prescan = false;                  // referee: the stretches around this feed's marked candidates are scanned ahead of its walk
	// launch_back() / launch_rest(): the walk and check of this feed are queued, what follows them is not yet (rest_pending); what the
	// second walks need of the first: its arguments, segmentation and speculative walks (d_spec_of: one of the context's two sets, not owned);
	// has_chk: the walk noted decisions to a list that is checked
	bool rest_pending = false, has_chk = false; int nseg = 1; int64_t seglen = 0; K4Args k4{}; SpecOut *d_spec_of = nullptr;
	Event ev_stitch, ev_chk; DevBuf<uint32_t> d_rqflag2;
	// profiling level 2: this feed's k_resample (resampling receivers) / k_spectrum and k_spectrum_reduce (input monitor; with the
	// spectrogram on k_spectrum_lines, and k_specgram_combine inside the second pair) /
	// k_activity_power and k_activity_scan (activity monitor)
	KernelTimes rs_t, mon_t, act_t;
	// burst capture (capture.h): the feed's records, windows and totals, the IQ pool.  on: this feed's back end is followed by the
	// capture's launches; times: k_capture_plan and k_capture_copy
	struct CapBufs { RecordMail<CapHdr, CapRec> mail; DevBuf<CapPlan> d_plan; DevBuf<uint64_t> d_tot; DevBuf<cf32> d_pool; };
	TapSlot<CapBufs> cap;
	// transmission log (txlog.h): the feed's records.  on: this feed completed bins and the log's launches followed its scan; times:
	// k_txlog_plan and k_txlog_emit
	struct TxlBufs { RecordMail<TxHdr, TxRec> mail; };
	TapSlot<TxlBufs> txl;
	// preamble search (txsearch.h): the feed's records, their piece offsets, the pieces' partial results.  on: the search's launches
	// followed this feed's frame finisher; times: k_txsearch_plan .. k_txsearch_reduce (one pair round the three)
	struct TxsBufs { RecordMail<TxsHdr, TxsRec> mail; DevBuf<uint32_t> d_off; DevBuf<TxsPart> d_part; };
	TapSlot<TxsBufs> txs;
	// second look (relook.h): the feed's attempt records, the pieces' anchors, the attempts' plans, the frame pool of the attempts and
	// the frame finisher's counters nobody reads.  on: its launches followed this feed's search; times: k_relook_anchors .. k_relook_decode
	// (one pair round the three)
	struct RlBufs { RecordMail<RlHdr, RlRec> mail; DevBuf<RlPiece> d_piece; DevBuf<RlPlan> d_plan; DevBuf<OutFrame> d_frames, d_frames_out; DevBuf<uint8_t> d_pool, d_pool_out; DevBuf<unsigned long long> d_acnt; };
	TapSlot<RlBufs> rl;
	// transmission capture (txcap.h): the feed's records, their piece offsets, the pieces' float64 rows, the IQ pool, the spectra.  on:
	// the capture's launches followed this feed's frame finisher; times: k_txcap_plan + k_txcap_copy, k_txcap_spectrum + k_txcap_reduce
	struct TxcBufs { RecordMail<TxcHdr, TxcRec> mail; DevBuf<uint32_t> d_poff; DevBuf<double> d_part; DevBuf<cf32> d_pool; DevBuf<float> d_spec; };
	TapSlot<TxcBufs> txc;
	// burst timing (toa.h): the feed's records and the curves of the first pool_curves of them.  on: this feed's back end is followed by
	// k_toa; times: k_toa
	struct ToaBufs { RecordMail<ToaHdr, ToaRec> mail; DevBuf<float> d_curve; };
	TapSlot<ToaBufs> toa;
	unsigned k5_waves = 0; bool small = false;   // wavefronts of this feed's burst decoder; short feed: its whole back end runs on the front stream
};

struct vdl2hip_ctx {
	vdl2hip_cfg cfg{};
	int C = 0, chan_first = 0, os = 0, fmt = 0, run = kRun, cr = 1;
	// fmt: what the channeliser and the referee read; in_fmt: what the caller feeds.  They differ only for a receiver that resamples
	// (cfg.input_rate): its blocks go through k_resample into a buffer of the feed's slot, and the rest of the receiver is a
	// VDL2HIP_FMT_CF32 receiver fed that buffer.
	int in_fmt = 0;
	struct {
		bool on = false; uint32_t L = 0, M = 0, T = 0, span_cap = 0; size_t lds = 0; bool taps_lds = false;
		DevBuf<float> d_taps; DevBuf<float2> d_tail[2]; int tail_sel = 0;
		DevBuf<float2> d_out[kSlots]; uint64_t cap = 0;                 // per slot: a feed's resampled block (samples)
		uint64_t first[kSlots] = {}, count[kSlots] = {};              // ... and which part of r[] it holds
		uint64_t n_in = 0, n_out = 0;                                 // samples taken / made so far
	} rs;
	// Input monitor (spectrum.h, vdl2hip_spectrum_*): off unless enabled.  pos: samples fed since it was enabled; carry: the
	// samples of the incomplete segment the stream stands in, where that segment will be analysed (two buffers, alternating).
	// buf: what an enabled monitor holds on the device, given back as one (monitor_free); tap: the read behind the last launch (kept)
	struct {
		bool on = false; uint32_t nfft = 0, window = 0, stride = 1, log2n = 0, threads = 0; size_t lds = 0;
		double sum_w = 0.0, enbw = 0.0; uint64_t pos = 0, segments = 0; uint32_t ncarry = 0; int carry_sel = 0;
		struct { DevBuf<float> d_w; DevBuf<float2> d_tw, d_carry[2]; DevBuf<double> d_rows, d_acc; } buf;
		TapRead tap; double kernel_ms = 0.0;
		uint64_t ordinal = 0;                                         // analysed segments since enable (segments restarts with a read's reset)
	} mon;
	// Spectrogram (spectrum.h, specgram_plan.h, vdl2hip_specgram_*): off unless enabled, and only on top of the input monitor, whose
	// launches, event, read stream and landing place it shares.  a0: the monitor's ordinal when it was enabled; seen: segments since;
	// hold_*: what the holds cover; rows: workgroups the piece buffers have room for.  buf: given back as one (specgram_free)
	struct {
		bool on = false; uint32_t R = 0, ring = 0, rows = 0; uint64_t a0 = 0, seen = 0, hold_segments = 0, hold_lines = 0;
		struct { DevBuf<double> d_piece_sum, d_carry_sum; DevBuf<float> d_piece_max, d_run_max, d_run_floor, d_ring_mean, d_ring_max, d_carry_max, d_hold; } buf;
	} spg;
	// Activity monitor (activity.h, vdl2hip_activity_*): off unless enabled.  k_on: the decimated samples made before it was enabled;
	// bins: complete so far; carry: per channel the float32 sum of what the stream holds of the incomplete bin it stands in (two
	// buffers, alternating); acc / st: the scan's accumulators and the transmission under way, per channel.
	// buf: what an enabled monitor holds on the device, given back as one (activity_free); tap: the read behind the last launch (kept)
	struct {
		bool on = false; uint32_t B = 0, H = 0, S = 0; float thr_dbfs = 0.f, thr = 0.f; int64_t k_on = 0; uint64_t bins = 0;
		struct { DevBuf<float> d_series, d_carry[2], d_edges; DevBuf<ActChan> d_acc; DevBuf<ActState> d_st; } buf;
		int carry_sel = 0; TapRead tap; double kernel_ms = 0.0;
	} act;
	// Burst capture (capture.h, vdl2hip_capture_*): off unless enabled.  queue: the records of the collected feeds, oldest first, each
	// with the IQ of its feed (one allocation per feed, shared by its records; iq_off: where the record's window begins in it).
	// stage (here and in the two taps below): the page-locked staging buffer of a feed with more records than come with the header -
	// the capture's takes the feed's IQ too - grown on demand and kept, whatever the tap does, until the receiver goes
	struct CapItem { vdl2hip_burst r; std::shared_ptr<std::vector<float>> iq; };
	struct {
		bool on = false; uint32_t pre = 0, post = 0, flags = 0, pool = 0;
		uint64_t bursts = 0, iq_samples = 0, iq_dropped = 0; double kernel_ms = 0.0;
		PinnedBuf stage; std::deque<CapItem> queue;
	} capt;
	// Transmission log (txlog.h, vdl2hip_txlog_*): off unless enabled, and only beside the activity monitor.  buf: its per-channel state
	// and counts, given back as one (txlog_free).  queue: the records of the collected feeds, oldest first; wait: per channel the frames
	// no record has claimed yet (txlog_collect)
	struct TxFrame { int64_t sync_sample, burst_ord; bool ok; uint32_t len; uint64_t hash; };      // len, hash: of its octets, for the second look's join
	struct {
		bool on = false; uint32_t pool = 0, flags = 0;
		uint64_t transmissions = 0, decoded = 0, dropped = 0, matched = 0, unmatched = 0; double kernel_ms = 0.0;
		struct { DevBuf<TxState> d_st; DevBuf<uint32_t> d_cnt; } buf;
		PinnedBuf stage; std::deque<vdl2hip_tx> queue; std::vector<std::deque<TxFrame>> wait;
	} txl;
	// Preamble search (txsearch.h, vdl2hip_txsearch_*): off unless enabled, and only beside the transmission log.  piece_cap: the
	// pieces a feed's records can have at the most (txsearch_piece_cap); queue: the records of the collected feeds, oldest first
	struct {
		bool on = false; uint32_t flags = 0, piece_cap = 0;
		uint64_t records = 0, samples = 0, clipped = 0; double kernel_ms = 0.0;
		PinnedBuf stage; std::deque<vdl2hip_tx_search> queue;
	} txs;
	// Second look (relook.h, vdl2hip_relook_*): off unless enabled, and only on top of the preamble search.  k: the configuration in
	// force; rec_cap: the attempts one feed can have at the most; queue: the attempt records of the collected feeds, oldest first, each
	// with the frame records and the octets of its feed (one allocation each per feed, shared by its records)
	struct RlItem { vdl2hip_relook r; std::shared_ptr<std::vector<OutFrame>> fr; std::shared_ptr<std::vector<uint8_t>> pool; };
	struct {
		bool on = false; uint32_t flags = 0, max_anchors = 0, pool_frames = 0, pool_octets = 0, rec_cap = 0; float thr = 0.f, max_ppm = 0.f;
		uint64_t records = 0, anchors_found = 0, attempts = 0, frames = 0, frames_ok = 0, frames_new = 0, dropped = 0; double kernel_ms = 0.0;
		PinnedBuf stage; std::deque<RlItem> queue;
	} rl;
	// Transmission capture (txcap.h, vdl2hip_txcap_*): off unless enabled, and only beside the transmission log.  k: the configuration
	// in force as the kernels take it; buf: the window and the twiddles of its transform, given back as one (txcap_free); queue: the
	// records of the collected feeds, oldest first, each with the IQ and the spectra of its feed (one allocation each per feed, shared by
	// its records; iq_off, spec_off: where the record's begin in them)
	struct TxcItem { vdl2hip_tx_capture r; std::shared_ptr<std::vector<float>> iq, spec; };
	struct {
		bool on = false; TxcCfg k{}; uint32_t window = 0, log2n = 0, piece_cap = 0; double norm = 0.0; size_t lds = 0;
		uint64_t records = 0, iq_samples = 0, iq_dropped = 0, spectra = 0, spectra_dropped = 0; double kernel_ms = 0.0;
		struct { DevBuf<float> d_w; DevBuf<float2> d_tw; } buf;
		PinnedBuf stage; std::deque<TxcItem> queue;
	} txc;
	// Burst timing (toa.h, vdl2hip_toa_*): off unless enabled.  W, pool_curves: the configuration in force; e_s: the template's energy;
	// d_s: the template on the device; queue: the records of the collected feeds, oldest first, each with the curves of its feed (one
	// allocation per feed, shared by its records; curve_off: where the record's begins in it)
	struct ToaItem { vdl2hip_burst_toa r; std::shared_ptr<std::vector<float>> curves; };
	struct {
		bool on = false; uint32_t W = 0, flags = 0, pool_curves = 0; double e_s = 0.0;
		uint64_t bursts = 0, curves = 0, curves_dropped = 0, early = 0, edge = 0; double kernel_ms = 0.0;
		DevBuf<cf32> d_s;
		PinnedBuf stage; std::deque<ToaItem> queue;
	} toa;
	uint64_t dmax = 0;                     // decimated samples one feed can make at the most
	bool specialised = false;
	std::vector<uint32_t> freqs, dphi, all_freqs;
	LpfCoeffs lpf{};
	BlockForm bf{};
	// Streams (kSidePre: which, of what priority, and why they come from a pool and go back to it: the one thing here the context
	// does not own).  front: channeliser and sync kernels; copy / out: H2D of host-fed blocks, D2H of results; back: the walk; nf: the
	// noise floor; pre: referee, VDL2HIP_REF_PRESCAN=1: the scans ahead of the walk, a stream per feed in flight (one stream would put
	// them in a row: 4.4 ms each); burst: a burst stream per feed in flight (a burst decoder that waits for the referee - a scan over a
	// whole burst takes milliseconds - does not hold up the next feed's)
	StreamSet streams;
	// device memory
	DevBuf<BlockForm> d_bf; DevBuf<Lut4> d_lut; DevBuf<Tables> d_tab;
	DevBuf<uint32_t> d_dphi, d_freq; DevBuf<float> d_ppmthr;
	// host-fed input: one device buffer + "copy done" event per slot, filled on a copy stream of its own so that the H2D of
	// block i+1 runs beside the channeliser of block i (process_buf_*() hands over host memory: src/demod.c:356-365)
	DevBuf<uint8_t> d_in[kSlots]; Event ev_copied[kSlots]; size_t in_cap = 0;
	hipEvent_t pinned_pending = nullptr;   // (one of ev_copied[], not owned) copy event of the last vdl2hip_feed_pinned() whose source buffer the caller may not touch yet
	// cold start (nothing in flight) of a large page-locked block: the copy goes in kColdParts pieces and the channeliser is launched
	// piece by piece behind them, so that the first block of a stream does not wait for its whole H2D (feed_host)
	struct { int n = 0; uint64_t samples[kColdParts] = {}; Event ev[kColdParts]; } cold;
	PinnedBuf stage;                       // page-locked D2H staging for frame records + octets, grown on demand
	DevBuf<uint8_t> d_carry[2]; int carry_sel = 0; uint32_t ncarry = 0;
	DevBuf<cf32> d_y, d_pf; DevBuf<uint64_t> d_cand, d_flag;
	uint32_t cap = 0;
	DevBuf<float4> d_segend; uint32_t nseg_cap = 0;
	DevBuf<float4> d_qpow;
	DevBuf<float4> d_tcarry[2]; int tcarry_sel = 0;
	DevBuf<unsigned long long> d_segpub; DevBuf<uint32_t> d_synctmo; bool fuse_k2 = true;   // K2 fused into K1 (one-step look-back between segments)
	DevBuf<WalkState> d_ws; DevBuf<unsigned long long> d_cnt, d_acnt;
	// The reference's per-channel counters live in TWO rows per channel, one per writer: d_cnt is the burst decoder's (atomic adds from
	// k_burst on the burst streams), d_wcnt = d_cnt + C * kNumCounters the walker's (sync.good, the header outcomes, ppm_reject: plain
	// read-modify-writes on the walk stream, and the only row the walk-again snapshot saves and restores).  A reader adds the two.  With one
	// row, a channel walked again wiped whatever the previous feed's burst decoder had added since the snapshot (round 5's red test).
	unsigned long long *d_wcnt = nullptr;   // (the second half of d_cnt, not owned)
	DevBuf<NfState> d_nf; DevBuf<int64_t> d_scfirst, d_sccum;
	DevBuf<float> d_nfring, d_lpbuf; DevBuf<NfFeed> d_nffeed; uint32_t cap_log = 0, cap_comb = 0, cap_hist = 0, nf_ring = 0;
	uint32_t cap_bursts_chan = 0;
	DevBuf<SpecOut> d_spec[2]; DevBuf<uint32_t> d_segstats; int seg_max = 1; int64_t seg_min = 16384;   // segmented walk
	OutSlot slot[kSlots];                  // per-feed output buffers: the fronts of feeds i+1, i+2 run while feed i's back still fills slot i%kSlots
	uint64_t feed_no = 0; int drain_lag = 0;
	OutCtl ctl_template{};                 // the capacities of a feed's output buffers (the counters are reset on the device: reset_out_ctl)
	bool pooled = false;                   // its streams are complete and of the product's priorities: they go to the pool when the receiver is destroyed
	bool avlc_filter = false, failed = false; int debug_force_timeout = 0, debug_force_again = 0, debug_exact_tier = 1, debug_screen_all = 0;
	// Referee (kernels.h): decisions within the margin of the channeliser's distance from the reference's fp32 scan are taken on the
	// reference's own samples, recomputed from the raw input.  The input of a feed stays where it is (d_in / the caller's device
	// buffer) while its back end runs; what lies before it - up to ref_T samples: the run-up of the scan + the longest burst - is kept
	// in a ring (ref_hist), appended to by every feed (its last min(n, ref_T) samples).  ref_pieces: what of the stream the ring holds,
	// contiguously, newest last: {first absolute sample, count, ring position of the first}.
	bool referee = true; bool ref_prescan = false;   /* VDL2HIP_REF_PRESCAN=1: the stretches around marked candidates are made exact ahead of the walk - a rank-sized shard 4.05 -> 2.88 ms per step, 256 channels 7.2 -> 7.85: for receivers of few channels */ int64_t ref_warm = 3 << 16 /* 196 608: kernels.h */, ref_T = 0; DevBuf<uint8_t> d_refhist; uint64_t ref_cap = 0, ref_wp = 0;
	struct HistPiece { int64_t s0, n; uint64_t pos; }; std::vector<HistPiece> ref_pieces;
	DevBuf<WalkState> d_ws_snap[2], d_ws_tmp; DevBuf<unsigned long long> d_cnt_snap[2], d_cnt_tmp; uint32_t rq_cap = 8192; uint32_t sq_alloc = 8192;
	int walk_ahead = 1; bool walk_ahead_auto = true; double walk_ahead_below = 1.1e8; int debug_force_mismatch = 0; uint32_t debug_mark_cap = 0;   // launch_back(): the walk of the next feed does not (1) / does (0) wait for this feed's check
	int ref_retry_mul = 2;                 // a scan that has not met its witness is run again from this many times further back (0: not at all; VDL2HIP_REF_RETRY)
	DevBuf<RefChan> d_ref[kSlots]; DevBuf<unsigned long long> d_refdone; DevBuf<uint32_t> d_refdonen, d_refstats; DevBuf<uint8_t> d_mix;
	std::vector<uint64_t> statsd_prev;
	std::vector<HostFrame> queue;
	int64_t k_total = 0; uint64_t n_total = 0;
	// profiling
	int profiling = 0;                     // 0 off, 1 channeliser only, 2 every stage
	vdl2hip_stats stats{};
};

#define HIPCHK(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) { \
	fprintf(stderr, "vdl2hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return VDL2HIP_E_DEVICE; } } while(0)

// The format inside the library is a small code (rawfmt.h); this is the one place that maps a public value to it (the public 3 is
// unassigned and refused); -1: not a format.
static int fmt_code(uint32_t sample_fmt) {
	switch(sample_fmt) {
		case VDL2HIP_FMT_U8: return kFmtU8;
		case VDL2HIP_FMT_S16LE: return kFmtS16;
		case VDL2HIP_FMT_CF32: return kFmtCF32;
		case VDL2HIP_FMT_S8: return kFmtS8;
		default: return -1;
	}
}

// Every entry point works on the context's own device whatever the calling thread's current device is (a process may hold
// receivers on several GPUs), and leaves the thread's device as it found it.
struct OnDevice {
	int prev = -1; bool switched = false;
	explicit OnDevice(const vdl2hip_ctx *c) { if(c && hipGetDevice(&prev) == hipSuccess && prev != c->cfg.device) switched = hipSetDevice(c->cfg.device) == hipSuccess; }
	~OnDevice() { if(switched) (void)hipSetDevice(prev); }
};

// Launch with the kernel's own start/stop stamped into two events (null: plain launch).  Used instead of hipEventRecord
// pairs, which are separate queue entries and cost a few microseconds of stream time each.
#define LAUNCH_EV(kernel, grid, block, stream, e0, e1, ...) hipExtLaunchKernelGGL(kernel, grid, block, 0u, stream, e0, e1, 0, __VA_ARGS__)
#define EV(i) (prof_all ? (hipEvent_t)ev[i] : (hipEvent_t) nullptr)

template<int OS, int R>
static void launch_chanfir(vdl2hip_ctx *c, const K1Args &a, int cr, size_t lds, hipEvent_t e0, hipEvent_t e1) {
	const int groups = (c->C + cr - 1) / cr;
	K1Args b = a;
	b.gy = (groups + 3) / 4;
	const int nseg8 = (a.seg1 - a.seg0 + 7) / 8 * 8;
	dim3 grid((unsigned)(nseg8 * b.gy)), block(256);
	// e0/e1 (profiling only, else null): the runtime stamps them with the kernel's own start and stop, so the roofline figure is
	// the kernel's duration and not the time the launch spent queued behind other streams' work
	// a format that has no build of its own for this shape goes to the shape's S16 build (kernels.h: has_fast_build)
	with_fmt(c->fmt, [&](auto F) {
		auto go = [&](auto CR) {
			constexpr int B = has_fast_build(F(), OS, R, CR()) ? F() : kFmtS16;
			hipExtLaunchKernelGGL((k_chanfir<OS, R, CR(), B>), grid, block, (uint32_t)lds, c->streams.front, e0, e1, 0, b);
		};
		switch(cr) {
			case 4: go(std::integral_constant<int, 4>{}); break;
			case 2: go(std::integral_constant<int, 2>{}); break;
			default: go(std::integral_constant<int, 1>{}); break;
		}
	});
}

// The front's picks among the builds of its kernel templates (channeliser, exact sync tier, resampler).  The compiler emits the
// builds of kernel templates in the order the host code first names them; with the launchers here, ahead of taps.inc, the input
// monitor's k_spectrum comes out behind the front's kernels as it always did.  Within k_chanfir the order is with_fmt's order of
// formats, which is not that of builds before rawfmt.h: the device assembly is compared with an earlier build's kernel by kernel,
// sorted by symbol (profiles/rawfmt_ab.txt).  Nothing else depends on the three launchers.
static void launch_k1(vdl2hip_ctx *c, const K1Args &a, size_t lds, hipEvent_t e0, hipEvent_t e1) {
	if(c->specialised && c->os == 20) launch_chanfir<20, kRun>(c, a, c->cr, lds, e0, e1);
	else if(c->specialised && c->os == 13) launch_chanfir<13, kRun>(c, a, c->cr, lds, e0, e1);
	else if(c->specialised) launch_chanfir<10, kRun>(c, a, c->cr, lds, e0, e1);
	else launch_chanfir<0, kRunGeneric>(c, a, c->cr, lds, e0, e1);
}
// (the exact sync tier, its stop event the feed's ev_front: feed_common)
static void launch_k3b(vdl2hip_ctx *c, const K3Args &k3, dim3 grid, hipEvent_t ev_front) {
	const bool pre = c->referee && c->ref_prescan;
	if(c->debug_exact_tier) { if(pre) LAUNCH_EV(k_sync_dense<true>, grid, dim3(256), c->streams.front, (hipEvent_t) nullptr, ev_front, k3); else LAUNCH_EV(k_sync_dense<false>, grid, dim3(256), c->streams.front, (hipEvent_t) nullptr, ev_front, k3); }
	else { if(pre) LAUNCH_EV(k_sync_exact4<true>, grid, dim3(256), c->streams.front, (hipEvent_t) nullptr, ev_front, k3); else LAUNCH_EV(k_sync_exact4<false>, grid, dim3(256), c->streams.front, (hipEvent_t) nullptr, ev_front, k3); }
}
template<int FMT>
static void launch_resample(vdl2hip_ctx *c, const K0Args &a, unsigned grid, hipEvent_t e0, hipEvent_t e1) {
	if(c->rs.taps_lds) hipExtLaunchKernelGGL((k_resample<FMT, true>), dim3(grid), dim3(kResTile), (uint32_t)c->rs.lds, c->streams.front, e0, e1, 0, a);
	else hipExtLaunchKernelGGL((k_resample<FMT, false>), dim3(grid), dim3(kResTile), (uint32_t)c->rs.lds, c->streams.front, e0, e1, 0, a);
}
static void launch_k0(vdl2hip_ctx *c, const K0Args &a, unsigned grid, hipEvent_t e0, hipEvent_t e1) {
	with_fmt(c->in_fmt, [&](auto F) { launch_resample<F()>(c, a, grid, e0, e1); });
}

static int launch_back(vdl2hip_ctx *c, OutSlot &sl);
static int launch_rest(vdl2hip_ctx *c, OutSlot &sl, struct OutSlot *succ);
static int flush_rest(vdl2hip_ctx *c, const OutSlot *upto);
// A short feed (fewer than two walk segments' worth of samples; the reference's own 320 000-byte blocks are 4 000): launch_back()
static bool feed_is_small(const vdl2hip_ctx *c, int64_t D);
static int collect_slot(vdl2hip_ctx *c, OutSlot &sl);
static int collect_pending(vdl2hip_ctx *c, int keep = 0);
// what is in flight is collected, as a tap's enable and disable need it before they touch its buffers: an output buffer that ran over
// on the way is the drain's to report, not theirs
static int collect_all(vdl2hip_ctx *c) { const int r = collect_pending(c); return r == VDL2HIP_E_OVERFLOW ? VDL2HIP_OK : r; }
static void fill_frame(const vdl2hip_ctx *c, const HostFrame &h, vdl2hip_frame &f);

#include "taps.inc"   // the taps, each in one place: its share of a feed, its collect, its vdl2hip_<tap>_* entry points

static int collect_slot(vdl2hip_ctx *c, OutSlot &sl) {
	if(!sl.pending) return VDL2HIP_OK;
	if(sl.rest_pending) { int r = flush_rest(c, &sl); if(r != VDL2HIP_OK) return r; }   // nothing followed this feed: no walk that its second walks could have been queued behind (it and what is older, oldest first)
	HIPCHK(hipEventSynchronize(sl.done));
	sl.pending = false;
	sl.rs_t.collect(c->stats.resample_ms);
	sl.mon_t.collect(c->mon.kernel_ms);
	sl.act_t.collect(c->act.kernel_ms);
	sl.cap.times.collect(c->capt.kernel_ms);
	sl.txl.times.collect(c->txl.kernel_ms);
	sl.txs.times.collect(c->txs.kernel_ms);
	sl.rl.times.collect(c->rl.kernel_ms);
	sl.txc.times.collect(c->txc.kernel_ms);
	sl.toa.times.collect(c->toa.kernel_ms);
	if(c->profiling && sl.ev_valid) {
		const Event *ev = sl.ev;
		float ms = 0.f;
		if(sl.k1_timed && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) { c->stats.chanfir_ms += ms; c->stats.chanfir_launches++; }
		if(sl.ev_level >= 2) {
		if(!sl.fused && hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) c->stats.phase_ms += ms;
		if(hipEventElapsedTime(&ms, ev[4], sl.ev_front) == hipSuccess) c->stats.sync_ms += ms;
		if(hipEventElapsedTime(&ms, ev[6], ev[7]) == hipSuccess) c->stats.walk_ms += ms;
		if(sl.small) {        // noise floor and burst decoder were one launch (k_nf_burst): booked under the burst decoder
			if(hipEventElapsedTime(&ms, ev[8], ev[11]) == hipSuccess) c->stats.burst_ms += ms;
		} else {
			if(hipEventElapsedTime(&ms, ev[8], ev[9]) == hipSuccess) c->stats.nf_ms += ms;
			if(hipEventElapsedTime(&ms, ev[10], ev[11]) == hipSuccess) c->stats.burst_ms += ms;
		}
		}
	}
	if(sl.ev_valid) (void)hipGetLastError();   // (an event query that failed above is not a device error of the next feed)
	sl.ev_valid = false;
	const OutMail *mail = sl.h_mail.as<OutMail>();
	const OutCtl ctl = mail->ctl;
	if(ctl.overflow) c->stats.overflow_feeds++;
	c->stats.bursts += std::min(ctl.nbursts, ctl.cap_bursts);
	const uint32_t nf = std::min(ctl.nvalid, ctl.cap_frames);
	const OutFrame *fr = nullptr;
	const uint8_t *po = nullptr; uint32_t pool_n = 0;
	if(nf) {
		pool_n = std::min(ctl.pool_out_used, ctl.cap_pool);
		if(nf <= (uint32_t)kMailFrames && pool_n <= (uint32_t)kMailPool) {
			// a handful of frames (the usual case for a block of a live receiver): they have come with the control block
			fr = mail->frames; po = mail->pool;
		} else {
			// one pinned staging buffer, two asynchronous copies on a stream of their own (the burst stream may already hold the
			// next feeds' kernels), one wait
			const size_t fr_bytes = sizeof(OutFrame) * (size_t)nf, need = fr_bytes + pool_n;
			HIPCHK(c->stage.reserve(need));
			HIPCHK(hipMemcpyAsync(c->stage, sl.d_frames_out, fr_bytes, hipMemcpyDeviceToHost, c->streams.out));
			if(pool_n) HIPCHK(hipMemcpyAsync(c->stage + fr_bytes, sl.d_pool_out, pool_n, hipMemcpyDeviceToHost, c->streams.out));
			HIPCHK(hipStreamSynchronize(c->streams.out));
			fr = c->stage.as<OutFrame>(); po = c->stage + fr_bytes;
		}
		auto pool = std::make_shared<std::vector<uint8_t>>(po, po + pool_n);
		// frames of one feed are sorted when they are drained, so that feeds can be appended to the queue in order
		c->queue.reserve(c->queue.size() + nf);
		for(uint32_t i = 0; i < nf; i++) {
			if(fr[i].chan < 0 || fr[i].chan >= c->C) continue;
			c->stats.frames++;                                           // frames the decoder produced (before the optional AVLC filter)
			if(!c->avlc_filter || fr[i].avlc_status == AVLC_OK) c->queue.push_back(HostFrame{ fr[i], pool });
		}
	}
	if(sl.cap.on) { sl.cap.on = false; int r = capture_collect(c, sl, fr, nf); if(r != VDL2HIP_OK) return r; }
	if(sl.toa.on) { sl.toa.on = false; int r = toa_collect(c, sl, fr, nf); if(r != VDL2HIP_OK) return r; }
	if(c->txl.on) { int r = txlog_collect(c, sl, fr, nf, po, pool_n); if(r != VDL2HIP_OK) return r; }
	return ctl.overflow ? VDL2HIP_E_OVERFLOW : VDL2HIP_OK;
}

// collect every feed except the `keep` most recent ones, oldest first
static int collect_pending(vdl2hip_ctx *c, int keep) {
	int rc = VDL2HIP_OK;
	for(int pass = 0; pass < kSlots; pass++) {
		OutSlot *oldest = nullptr;
		int npend = 0;
		for(auto &sl : c->slot) if(sl.pending) { npend++; if(!oldest || sl.seq < oldest->seq) oldest = &sl; }
		if(!oldest || npend <= keep) break;
		int r = collect_slot(c, *oldest);
		if(r != VDL2HIP_OK) rc = r;
		if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	}
	return rc;
}

static int feed_common(vdl2hip_ctx *c, const void *dev_in, size_t nbytes, bool in_parts = false) {
	const size_t sb = raw_bytes(c->fmt);
	const uint64_t nnew = nbytes / sb;
	const uint64_t nlogical = c->ncarry + nnew;
	const int64_t D = (int64_t)(nlogical / (uint64_t)c->os);
	const uint32_t nrem = (uint32_t)(nlogical - (uint64_t)D * c->os);
	const int seglen = 64 * c->run;
	if(c->failed) return VDL2HIP_E_DEVICE;
	OutSlot &sl = c->slot[c->feed_no % kSlots];
	{ int r = collect_slot(c, sl); if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r; }   // its buffers are about to be reused
	hipStream_t st = c->streams.front;
	const Event *ev = sl.ev;
	const bool prof = c->profiling != 0, prof_all = c->profiling >= 2;

	K1Args a{};
	a.in = dev_in; a.carry = c->d_carry[c->carry_sel]; a.ncarry = c->ncarry; a.nlogical = nlogical;
	a.n0 = c->n_total - c->ncarry; a.k0 = c->k_total; a.D = D;
	a.fmt = c->fmt; a.nchan = c->C; a.os = c->os; a.nseg = 0; a.gy = 1;
	a.dphi = c->d_dphi; a.lut = c->d_lut; a.bf = make_k1_consts(c->bf); a.y = c->d_y; a.seg_end = c->d_segend;
	a.qpow = c->d_qpow; a.cap = c->cap; a.mask = c->cap - 1; a.nseg_cap = c->nseg_cap;
	a.fuse = c->fuse_k2 && 64 * c->run == kFixW; a.carry_in = c->d_tcarry[c->tcarry_sel]; a.carry_out = c->d_tcarry[c->tcarry_sel ^ 1];
	a.bfd = c->d_bf; a.seg_pub = c->d_segpub; a.epoch = (uint32_t)(c->feed_no + 1); a.sync_timeouts = c->d_synctmo;
	a.pub_epoch = a.epoch; a.spin_limit = 4096;         // polls of ~1 us before a consumer helps itself: several workgroup lifetimes
	if(c->debug_force_timeout) { a.pub_epoch = a.epoch ^ 0x40000000u; a.spin_limit = 16; }   // tests only: every look-back gives up and takes the fall-back
	{
		// tiles per workgroup segment: long segments save K2 work, but the grid should still offer several thousand
		// workgroups (measured: dev/gpu_k1_tiles.sh - 2 is best at 8 channels, 8 at 256)
		const int64_t ntile = (D + seglen - 1) / seglen;
		const int groups = (c->C + c->cr - 1) / c->cr, gy = (groups + 3) / 4;
		int64_t tiles = ntile * gy / 6144; if(tiles < 1) tiles = 1; if(tiles > 8) tiles = 8;
		a.tiles = (int)tiles;
		a.nseg = (int)((ntile + tiles - 1) / tiles);
	}

	sl.ev_valid = false;
	sl.cap.on = c->capt.on && D > 0;                                // (the capture takes effect with the feed that follows its enabling)
	sl.toa.on = c->toa.on && D > 0;                                 // (... and so does burst timing)
	sl.txl.on = false;                                              // (set by activity_feed if the log's kernels follow this feed's scan)
	sl.txs.on = false;                                              // (set by launch_rest if the search's kernels follow this feed's frame finisher)
	sl.rl.on = false;                                               // (... and the second look's, behind them)
	sl.txc.on = false;                                              // (... and the transmission capture's)
	if(D > 0) {
		const size_t lds = (size_t)c->run * c->os * 65 * sizeof(float2);   // the tile; the tables are static LDS
		// (a cold-start feed launches the channeliser in pieces that wait for the pieces of the copy: not a kernel duration, not timed)
		const bool cold = in_parts && c->cold.n > 1;
		if(cold) c->stats.cold_start_feeds++;
		sl.k1_timed = prof && !cold;
		hipEvent_t e0 = sl.k1_timed ? (hipEvent_t)ev[0] : nullptr, e1 = sl.k1_timed ? (hipEvent_t)ev[1] : nullptr;
		auto launch = [&](int seg0, int seg1, hipEvent_t s_ev, hipEvent_t p_ev) { a.seg0 = seg0; a.seg1 = seg1; launch_k1(c, a, lds, s_ev, p_ev); };
		if(!in_parts || c->cold.n <= 1) launch(0, a.nseg, e0, e1);
		else {
			// cold start: piece p of the block is on the device when cold.ev[p] fires; the workgroup segments whose input lies in the
			// pieces that have arrived (whole multiples of 8, the XCD mapping) are launched behind it.  A segment reads nothing beyond its
			// own input (its tiles, the next tile's prefetch inside the segment, the look-back to the segment before), so the results are
			// those of one launch.
			const uint64_t seg_in = (uint64_t)a.tiles * (uint64_t)seglen * (uint64_t)c->os;     // logical input samples per segment
			int done = 0;
			for(int p = 0; p < c->cold.n; p++) {
				HIPCHK(hipStreamWaitEvent(st, c->cold.ev[p], 0));
				int ready = a.nseg;
				if(p < c->cold.n - 1) { const uint64_t r = (c->ncarry + c->cold.samples[p]) / seg_in; ready = r >= (uint64_t)a.nseg ? a.nseg : (int)(r & ~7ull); }
				if(ready > done) { launch(done, ready, done == 0 ? e0 : (hipEvent_t) nullptr, ready == a.nseg ? e1 : (hipEvent_t) nullptr); done = ready; }
			}
		}
		if(!a.fuse) {
			K2Args k2{ c->d_y, c->d_segend, c->d_tcarry[c->tcarry_sel], c->d_tcarry[c->tcarry_sel ^ 1], c->d_bf,
			           c->k_total, D, c->cap, c->cap - 1, c->nseg_cap, seglen * a.tiles };
			LAUNCH_EV(k_fixup, dim3((unsigned)((D + 255) / 256), (unsigned)c->C), dim3(256), st, EV(2), EV(3), k2);
		}
		c->tcarry_sel ^= 1;
		// this feed's y is complete on the front stream: the activity monitor reads it here, ahead of the sync kernels (activity_feed)
		if(c->act.on) { int r = activity_feed(c, sl, c->k_total, D); if(r != VDL2HIP_OK) return r; }
	}
	if(nrem) hipLaunchKernelGGL(k_carry, dim3(1), dim3(64), 0, st, a, (void *)c->d_carry[c->carry_sel ^ 1], nrem);
	c->carry_sel ^= 1; c->ncarry = nrem;
	// Referee: this feed's hook - the raw input it may read (what the history ring holds of the stream before this block, then the
	// block where it lies) - and the block's tail appended to the ring for the feeds that follow.
	RefChan refv{}; RefChan *ref_dst = nullptr;
	if(c->d_refhist) {
		ref_dst = c->d_ref[c->feed_no % kSlots];
		refv.y = c->d_y; refv.cap = c->cap; refv.mask = c->cap - 1; refv.dphi = c->d_dphi; refv.mix = c->d_mix; refv.lut = c->d_lut;
		refv.A0 = c->lpf.A[0]; refv.A1 = c->lpf.A[1]; refv.A2 = c->lpf.A[2]; refv.B1 = c->lpf.B[1]; refv.B2 = c->lpf.B[2];
		refv.os = c->os; refv.fmt = c->fmt; refv.warm = c->ref_warm;
		refv.done = c->d_refdone; refv.done_n = c->d_refdonen; refv.stats = c->d_refstats;
		int np = 0;
		const int64_t blk_s0 = (int64_t)c->n_total, want0 = blk_s0 - c->ref_T;
		// (at most the two newest pieces matter - an older one ends more than ref_T samples back - and each may wrap once)
		for(size_t i = c->ref_pieces.size() > 2 ? c->ref_pieces.size() - 2 : 0; i < c->ref_pieces.size(); i++) {
			vdl2hip_ctx::HistPiece hp = c->ref_pieces[i];
			if(hp.s0 + hp.n <= want0) continue;
			if(hp.s0 < want0) { hp.pos = (hp.pos + (uint64_t)(want0 - hp.s0)) % c->ref_cap; hp.n -= want0 - hp.s0; hp.s0 = want0; }
			const uint64_t first = std::min<uint64_t>((uint64_t)hp.n, c->ref_cap - hp.pos);
			refv.piece[np++] = RefPiece{ c->d_refhist + hp.pos * sb, hp.s0, (int64_t)first };
			if(first < (uint64_t)hp.n) refv.piece[np++] = RefPiece{ c->d_refhist, hp.s0 + (int64_t)first, hp.n - (int64_t)first };
		}
		refv.piece[np++] = RefPiece{ dev_in, blk_s0, (int64_t)nnew };
		refv.npiece = np;
		// the pieces must be contiguous (a gap = a block longer than ref_T whose head was not kept): drop what lies before the last gap
		int firstp = 0;
		for(int i = 1; i < np; i++) if(refv.piece[i - 1].s0 + refv.piece[i - 1].n != refv.piece[i].s0) firstp = i;
		if(firstp) { for(int i = firstp; i < np; i++) refv.piece[i - firstp] = refv.piece[i]; refv.npiece = np - firstp; }
		if(nnew) {
			const uint64_t w = std::min<uint64_t>(nnew, (uint64_t)c->ref_T);
			hipLaunchKernelGGL(k_ref_hist, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, st, (const uint8_t *)dev_in + (nnew - w) * sb, w, c->d_refhist, c->ref_wp, c->ref_cap, (int)sb);
			if(w < nnew) c->ref_pieces.clear();                          // the head of this block is not kept: nothing before it can be reached any more
			if(!c->ref_pieces.empty() && c->ref_pieces.back().s0 + c->ref_pieces.back().n == blk_s0 + (int64_t)(nnew - w)) c->ref_pieces.back().n += (int64_t)w;
			else c->ref_pieces.push_back(vdl2hip_ctx::HistPiece{ blk_s0 + (int64_t)(nnew - w), (int64_t)w, c->ref_wp });
			c->ref_wp = (c->ref_wp + w) % c->ref_cap;
			// forget what the ring has overwritten (a piece never needs to be longer than the ring is)
			auto &bp = c->ref_pieces.back();
			if((uint64_t)bp.n > c->ref_cap / 2) { const int64_t cut = bp.n - (int64_t)(c->ref_cap / 2); bp.s0 += cut; bp.pos = (bp.pos + (uint64_t)cut) % c->ref_cap; bp.n -= cut; }
			while(c->ref_pieces.size() > 2) c->ref_pieces.erase(c->ref_pieces.begin());
		}
	}
	if(D > 0) {
		const int64_t k1 = c->k_total + D, nbase = c->k_total & ~63ll;
		// wavefronts of this feed's burst decoder: each owns kResSlots frame records of the output from the start, so a short block gets few
		sl.k5_waves = (unsigned)std::min<int64_t>(2048, std::max<int64_t>(16, (D * (int64_t)c->C) >> 14));
		sl.k5_waves = (sl.k5_waves + kBurstWaves - 1) / kBurstWaves * kBurstWaves;
		// (a short feed - launch_back: `small` - has no scans ahead of its walk: its one walk notes, the noted stretches are scanned side by side and checked on the front stream)
		sl.prescan = c->referee && c->ref_prescan && !feed_is_small(c, D);
		K3Args k3{ c->d_y, c->d_pf, c->d_cand, c->d_flag, c->d_tab, nbase, k1, c->cap, c->cap - 1, 1, c->debug_screen_all, sl.d_ctl, sl.k5_waves, ref_dst, refv, c->cfg.max_ppm, c->d_ppmthr, c->referee ? 1 : 0, sl.d_rqn, sl.d_rqflag, sl.d_rqbad, sl.prescan ? sl.d_pq : nullptr, kPreScans, sl.d_rqflag2 };
		// The exact tier's stop event doubles as "front of this feed done" (what the walk stream waits for): one queue entry less
		// on the front stream than a separate hipEventRecord.
		LAUNCH_EV(k_sync_screen, dim3((unsigned)((k1 - nbase + kK3Tile - 1) / kK3Tile), (unsigned)c->C), dim3(kK3Threads), st, EV(4), (hipEvent_t) nullptr, k3);
		const int64_t nwords = ((k1 + 63) >> 6) - (nbase >> 6);
		// words per lane of the exact tier: as many as keep >= 8 workgroups per CU (a wavefront with more words amortises its scan,
		// but the kernel is latency-bound: at 32 channels 1 word per lane - 3 296 workgroups - beat 4 - 832 - by 0.02 ms of a 0.85 ms step,
		// at 256 channels 4 is as good as any; profiles/r03_k3b_forms.txt)
		for(int wpl = kK3bWordsPerLane; wpl >= 1; wpl >>= 1) { k3.wpl = wpl; if(((nwords + 256 * wpl - 1) / (256 * wpl)) * c->C >= 2048 || wpl == 1) break; }
		// (the dense form: a workgroup's evaluations should fill its wavefronts - a word in a hundred has work, seven evaluations each -
		// so it takes as many passes of 256 words as leave the chip kK3dMinGroups workgroups)
		if(c->debug_exact_tier) {
			for(int wpl = kK3dRounds; wpl >= 1; wpl >>= 1) { k3.wpl = wpl; if(((nwords + 256 * wpl - 1) / (256 * wpl)) * c->C >= kK3dMinGroups || wpl == 1) break; }
		}
		const int64_t wpb = 256 * k3.wpl;                                      // words per block
		// (receivers that scan ahead of the walk work out the windows with one or two unwrap decisions within the margin: sync_metric_ref)
		// (debug_exact_tier 0: the word-at-a-time form the dense one replaced, kept as its yardstick - same grid, same arguments)
		const dim3 k3b_grid((unsigned)((nwords + wpb - 1) / wpb), (unsigned)c->C);
		launch_k3b(c, k3, k3b_grid, sl.ev_front);
	}
	if(D <= 0) HIPCHK(hipEventRecord(sl.ev_front, st));
	if(D > 0) { sl.ev_valid = prof; sl.ev_level = c->profiling; sl.fused = a.fuse != 0; if(sl.k1_timed) c->stats.chan_samples += (uint64_t)D * c->os * c->C; } else sl.k1_timed = false;
	sl.back_D = D; sl.back_k0 = c->k_total;
	sl.pending = true; sl.seq = c->feed_no++;
	c->k_total += D; c->n_total += nnew;
	c->stats.feeds++; c->stats.input_samples += nnew;
	// this feed's back end is queued right away: it then runs beside the NEXT feed's channeliser
	{ int r = launch_back(c, sl); if(r != VDL2HIP_OK) return r; }
	HIPCHK(hipGetLastError());
	return VDL2HIP_OK;
}

// One block of the caller's IQ, in device memory and ordered ahead of the front stream's next work.  A receiver that resamples
// (cfg.input_rate) turns it into this feed's block of r[] first - K0, k_resample, on the front stream into the buffer of the feed's
// slot, which stays as it is until the slot comes round again: the referee reads it as it reads any block - and is a CF32 receiver
// fed that block from there on.
static int feed_block(vdl2hip_ctx *c, const void *dev_in, size_t nbytes, bool in_parts = false) {
	// (the monitor sees a block once nothing can refuse it any more, and ahead of everything else that reads it)
	if(c->failed) return VDL2HIP_E_DEVICE;
	if(!c->rs.on) {
		if(c->mon.on) { int r = monitor_block(c, dev_in, nbytes); if(r != VDL2HIP_OK) return r; }
		return feed_common(c, dev_in, nbytes, in_parts);
	}
	auto &rs = c->rs;
	const int k = (int)(c->feed_no % kSlots);
	OutSlot &sl = c->slot[k];
	{ int r = collect_slot(c, sl); if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r; }   // the slot's block of r[] is about to be overwritten
	const uint64_t nin = nbytes / raw_bytes(c->in_fmt);
	// outputs n with b_n = floor(n M / L) <= N - 1 exist after N input samples: ceil(N L / M) of them (64 bits: 2^50 samples)
	const uint64_t N0 = rs.n_in, N1 = N0 + nin, n0 = rs.n_out, n1 = (N1 * rs.L + rs.M - 1) / rs.M, nout = n1 - n0;
	if(nout > rs.cap) return VDL2HIP_E_TOOBIG;
	if(c->mon.on) { int r = monitor_block(c, dev_in, nbytes); if(r != VDL2HIP_OK) return r; }
	K0Args a{};
	a.in = dev_in; a.tail_in = rs.d_tail[rs.tail_sel]; a.tail_out = rs.d_tail[rs.tail_sel ^ 1]; a.taps = rs.d_taps; a.out = rs.d_out[k];
	a.q0 = n0 % rs.L; a.t0 = n0 * rs.M - N0 * rs.L;                  // b_{n0} >= N0: output n0 is the first that needed a sample of this block
	a.nin = (uint32_t)nin; a.nout = (uint32_t)nout; a.L = rs.L; a.M = rs.M; a.T = rs.T; a.span_cap = rs.span_cap;
	const uint64_t per = (uint64_t)kResTile * kResTiles;
	const unsigned grid = (unsigned)std::max<uint64_t>(1, (nout + per - 1) / per);       // (no output: workgroup 0 still moves the tail on)
	KernelTimes &t = sl.rs_t;
	t.arm(c->profiling >= 2);
	launch_k0(c, a, grid, t.e(0), t.e(1));
	HIPCHK(hipGetLastError());
	t.launched(1);
	rs.tail_sel ^= 1; rs.first[k] = n0; rs.count[k] = nout; rs.n_in = N1; rs.n_out = n1;
	int r = feed_common(c, rs.d_out[k], (size_t)nout * sizeof(float2));
	c->stats.input_samples += nin - nout;                           // (feed_common counted the block it saw) the caller's samples
	c->stats.resampled_samples += nout;
	return r;
}

// The burst-rate back end of one feed (K4 walk, K4b noise floor, K5 burst decoder, frame finish), on three streams of its own so
// that consecutive feeds overlap stage by stage:
//   stream_back   K4   walk(i) -> walk(i+1) -> ...             (each needs the previous one's FSM state)
//   stream_nf     K4b  noise floor of feed i, after walk(i)    (each needs the previous one's NfState)
//   stream_burst  K5   bursts of feed i, after walk(i); the frames get their noise-floor figure when K4b(i) is done
// (the kernel is compiled per sample format)
static bool feed_is_small(const vdl2hip_ctx *c, int64_t D) {
	const int nseg = (int)std::min<int64_t>(c->seg_max, D / c->seg_min);
	return D > 0 && D < 2 * c->seg_min && nseg < 2;
}
// (the kernel is compiled per sample format and for the oversampling factors 20 and 10; 0: any)
#define LAUNCH_SCAN_MULTI(how, ...) with_fmt(c->fmt, [&](auto F) { \
	if(c->os == 20) how((k_ref_scan_multi<F(), 20>), __VA_ARGS__); else if(c->os == 10) how((k_ref_scan_multi<F(), 10>), __VA_ARGS__); else how((k_ref_scan_multi<F(), 0>), __VA_ARGS__); })
// Referee: the listed stretches (`sq`, or the decisions `rq` whose stretches they are; *n of them, at most cap) are made the reference's own,
// many side by side, and those of them that had not met their witness - a few in ten thousand - are listed in `retry` and scanned again
// from ref_retry_mul times further back (no list, or ref_retry_mul 0: they are published as they are, counted).  e0 / e1: the first
// kernel's start and the last one's stop (the test hook's timing).
static void launch_scans(vdl2hip_ctx *c, hipStream_t st, RefChan *ref, uint32_t launch, const ScanReq *sq, const RefReq *rq, const uint32_t *n, uint32_t cap, int64_t k_end,
                         ScanReq *retry, uint32_t *retry_n, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const ScanReq *sq2 = nullptr, const uint32_t *n2 = nullptr, uint32_t cap2 = 0) {
	const int rty = retry ? c->ref_retry_mul : 0;
	// (sq2: a second list - *n2 of them, at most cap2 - served by the same launch, behind the first; the grid covers both)
	LAUNCH_SCAN_MULTI(hipExtLaunchKernelGGL, dim3((cap + (sq2 ? cap2 : 0u) + kScanLanes - 1) / kScanLanes), dim3(64 * kScanWaves), 0, st, e0, rty ? (hipEvent_t) nullptr : e1, 0, ref, launch,
	                  sq, rq, n, cap, k_end, rty ? retry : (ScanReq *) nullptr, retry_n, kRetryScans, 1, sq2, n2, sq2 ? cap2 : 0u);
	if(rty) LAUNCH_SCAN_MULTI(hipExtLaunchKernelGGL, dim3(kRetryScans / kScanLanes), dim3(64 * kScanWaves), 0, st, (hipEvent_t) nullptr, e1, 0, ref, launch,
	                  (const ScanReq *)retry, (const RefReq *) nullptr, (const uint32_t *)retry_n, kRetryScans, k_end, (ScanReq *) nullptr, (uint32_t *) nullptr, 0u, rty, (const ScanReq *) nullptr, (const uint32_t *) nullptr, 0u);
}
// The walk of feed i + 1 does not wait for the check of feed i ("walk ahead").  walk(i + 1) needs the state walk(i) leaves, and that
// state is final only when the decisions walk(i) noted have been checked - behind a scan of 1.5 ms that no hardware shortens; with a
// front of 1 ms (a rank's 32 channels) that chain was the step.  But the check confirms the walk all but always.  So:
//   walk stream:    ... stitch(i)   again(i-1) redo(i)   stitch(i+1)   again(i) redo(i+1)   stitch(i+2) ...
//   check(i) = scans + verify on the scan stream of its slot, between stitch(i) and again(i), i.e. beside stitch(i+1);
//   again(i): the channels whose decisions did not stand (or that flagged themselves) are walked again from feed i's snapshot, into a
//     scratch row; their end state and counters are compared with what stitch(i+1) started from (feed i+1's snapshot).  The same:
//     stitch(i+1) stands.  Different (a few per thousand second walks): the snapshot of feed i+1 is corrected and the channel flagged;
//   redo(i+1): the flagged channels are stitched once more over feed i+1 from the corrected snapshot, into the live rows.
// stitch(i+2) follows on the same stream: it starts from a state in which feeds <= i are checked - the check of feed i overlaps one
// walk and one front.  launch_back() queues the walk and the check; launch_rest() - called when the NEXT feed's walk has been queued,
// or, if nothing follows (a drain, a short feed, the old schedule: walk_ahead_of() 0), at once with `succ` = nullptr: again(i)
// then works on the live rows as it always did - queues the second walks and everything behind them: noise floor, burst decoder,
// frame finish, the copy of the control block.
static int launch_rest(vdl2hip_ctx *c, OutSlot &sl, OutSlot *succ);
// k_walk_stitch over a feed's segments and speculative walks (`again`: the kernel's modes), a channel per wavefront
static void launch_stitch(vdl2hip_ctx *c, hipStream_t st, const OutSlot &sl, const K4Args &k4, int again, hipEvent_t e1 = nullptr) {
	K4sArgs k4s{ k4, sl.d_spec_of, (uint32_t)(3 * (c->seg_max - 1)), sl.nseg, sl.back_k0, sl.seglen, c->d_segstats, again };
	hipExtLaunchKernelGGL(k_walk_stitch, dim3((unsigned)((c->C + kStitchWaves - 1) / kStitchWaves)), dim3(64 * kStitchWaves), (unsigned)(sizeof(StitchLds) * kStitchWaves), st, (hipEvent_t) nullptr, e1, 0, k4s);
}

// Does the walk of the feed after this one go ahead of this feed's check?  It pays when a feed's front is shorter than a check (a scan:
// 2.3 ms) - a front is 6.2 ms for 1.68 M decimated samples of 256 channels, 1.45e-8 ms per channel-sample: receivers of 16-64 channels
// on the bench's 16 s blocks (rounds 6a/b), and ANY receiver of >= 16 channels on feeds of a second or so - the drop-in adapter's
// sixteen collected 320 000-byte blocks at 256 channels: 0.155 -> 0.10 ms per block (profiles/r06_block_batch.txt).  With fewer than
// 16 channels the walk itself is longer than the front and the second walks' extra launches cost more than they save (1.22 against
// 1.11 ms at 8).  The debug option "walk_ahead" fixes the choice for every feed.
static int walk_ahead_of(const vdl2hip_ctx *c, int64_t D) {
	if(!c->walk_ahead_auto) return c->walk_ahead;
	return c->C >= 16 && (double)D * (double)c->C < c->walk_ahead_below ? 1 : 0;
}

static int launch_back(vdl2hip_ctx *c, OutSlot &sl) {
	const int64_t D = sl.back_D, k0 = sl.back_k0;
	const int wa = walk_ahead_of(c, D);
	// long feeds: the walk runs in speculative segments (vdl2_core.h), one wavefront per (channel, segment, grid phase)
	int nseg = (int)std::min<int64_t>(c->seg_max, D / c->seg_min);
	// A short feed (fewer than two walk segments' worth of samples; the reference's own 320 000-byte blocks are 4 000) is a chain of kernels that each run for
	// microseconds: its whole back end goes onto the FRONT stream, behind its own sync kernels - no event hand-offs between streams -
	// with the three noise-floor passes as one kernel.  Whoever follows on the front stream is then behind it anyway.
	const bool small = feed_is_small(c, D);
	hipStream_t sb_ = small ? c->streams.front : c->streams.back;
	const Event *ev = sl.ev;
	const bool prof_all = sl.ev_valid && sl.ev_level >= 2;
	sl.small = small; sl.has_chk = false; sl.nseg = 1; sl.seglen = D;
	OutSlot &pv = c->slot[(sl.seq + kSlots - 1) % kSlots];
	// (short feeds too, since round 6: a block with a decision within the margin - one in three of the reference's own 320 000-byte
	// blocks at 256 channels - used to wait for a scan by the walker's own wavefront, 3.1 ms; noted, scanned side by side (1.5 ms for all
	// of them) and checked, on the front stream like the rest of a short feed's back end, it is 1.34 -> 0.8 ms per block on average)
	const bool opt = c->referee && D > 0;
	const uint32_t rq_cap = small ? std::min<uint32_t>(c->rq_cap, 16u * kScanLanes) : c->rq_cap;      // (a short feed: few requests, small grids - it queues these kernels whether or not it notes anything)
	// does this feed's walk go ahead of the check of the feed before?  (long feeds with a check, segmented walks)  If not, what is
	// still waiting for a successor's walk is queued now, oldest first
	const bool ahead = wa && opt && nseg >= 2 && sl.seq > 0 && pv.pending && pv.rest_pending && pv.has_chk && pv.nseg >= 2;
	if(!ahead) { int r = flush_rest(c, nullptr); if(r != VDL2HIP_OK) return r; }
	if(small) {
		// the walker, the noise floor and the burst list carry state from feed to feed: wait for a predecessor whose back end is on the other streams
		if(sl.seq > 0 && pv.pending && !pv.small) HIPCHK(hipStreamWaitEvent(sb_, pv.done, 0));
	} else {
		HIPCHK(hipStreamWaitEvent(sb_, sl.ev_front, 0));
	}
	if(D <= 0) hipLaunchKernelGGL(k_reset_ctl, dim3(1), dim3(1), 0, sb_, sl.d_ctl, 0u);     // (a feed with a front has had it reset by its last sync kernel)
	hipStream_t sp_ = small ? c->streams.front : c->streams.pre[sl.seq % kSidePre];
	if(D > 0 && sl.prescan) {
		// Referee: the stretches the exact sync tier has listed (around its marked candidates) are made the reference's own NOW, beside
		// the next feed's front and off the walk stream - the walk of this feed waits for them, the walk of the next one does not
		// (a scan on the walk stream is 1.5 ms that every following feed's walk queues behind: with 8 channels that was the step time)
		// (on a stream of its own: behind this feed's noise floor - which waits for the walk - the next feed's scans would wait for this
		// feed's whole walk chain)
		if(!small) HIPCHK(hipStreamWaitEvent(sp_, sl.ev_front, 0));
		launch_scans(c, sp_, c->d_ref[sl.seq % kSlots], (uint32_t)(16 * sl.seq + 8), sl.d_pq, nullptr, sl.d_rqn + 3, kPreScans, k0 + D, sl.d_retry, sl.d_rqn + 4);
		if(!small) { HIPCHK(hipEventRecord(sl.ev_pre, sp_)); HIPCHK(hipStreamWaitEvent(sb_, sl.ev_pre, 0)); }
	}
	if(D > 0) {
		const int64_t k1 = k0 + D;
		// Two sets of snapshots and speculative walks.  With the next feed's walk at most ONE feed ahead the walk stream runs
		// ... S(i+1) again(i) redo(i+1) S(i+2) again(i+1) redo(i+2) ... (S is queued below, then the feed before is flushed): S(i+2) is the
		// first writer of set i mod 2 after S(i), and the last reader of that set, again(i), is ahead of it on the same stream; check(i) on
		// the scan stream reads neither snapshots nor speculative walks (k_ref_verify -> ref_verify() is handed none).
		const int par = (int)(sl.seq % 2);
		sl.k4 = K4Args{ c->d_y, c->d_pf, c->d_cand, c->d_tab, c->d_ws, c->d_wcnt, sl.d_bursts, sl.d_nbchan, c->cap_bursts_chan, sl.d_ctl, c->d_freq,
		           sl.d_log, sl.d_nlog, c->cap_log, k1, c->cfg.max_ppm, c->cap, c->cap - 1, c->chan_first, c->C, c->d_ppmthr, c->referee ? c->d_ref[sl.seq % kSlots] : nullptr, (uint32_t)(16 * sl.seq + 1),
		           opt ? sl.d_rq : nullptr, sl.d_rqn, rq_cap, sl.d_rqflag, c->d_ws_snap[par], c->d_cnt_snap[par], sl.d_rqbad, sl.prescan ? 1 : 0, c->debug_force_again,
		           c->d_ws_tmp, c->d_cnt_tmp, nullptr, nullptr, sl.d_rqflag2, nullptr, c->debug_force_mismatch };   // (a short feed's walk notes and is checked like a long one's since round 6a: `opt`)
		const K4Args &k4 = sl.k4;
		sl.d_spec_of = c->d_spec[par];
		if(nseg >= 2) {
			sl.seglen = (D + nseg - 1) / nseg;
			nseg = (int)((D + sl.seglen - 1) / sl.seglen);
			sl.nseg = nseg;
			K4sArgs k4s{ k4, sl.d_spec_of, (uint32_t)(3 * (c->seg_max - 1)), nseg, k0, sl.seglen, c->d_segstats, 0 };
			LAUNCH_EV(k_walk_spec, dim3((unsigned)((1 + 3 * (nseg - 1) + kWalkWaves - 1) / kWalkWaves), (unsigned)c->C), dim3(64 * kWalkWaves), sb_, EV(6), (hipEvent_t) nullptr, k4s);
			launch_stitch(c, sb_, sl, k4, 0, EV(7));
		} else {
			LAUNCH_EV(k_walk, dim3((unsigned)c->C), dim3(64), sb_, EV(6), EV(7), k4);
		}
		if(k4.rq) {
			// referee, optimistic mode (long feeds): the decisions within the margin that the walk took are checked, all at once - the
			// stretches first, many side by side (k_ref_scan_multi), then the decisions on them, a wavefront each - on the scan stream of
			// the feed's slot (idle since the scans ahead of the walk): the walk stream goes on with the next feed meanwhile
			// (in the old schedule - receivers of many channels: the front hides the chain - the check stays on the walk stream: on a stream
			// of its own it cost the 256-channel receiver 0.6 ms per step, profiles/r06_walk_ahead_ab.txt)
			sl.has_chk = true;
			hipStream_t sc_ = wa ? sp_ : sb_;
			// ... and with them, in the same launch, the pieces the burst decoder will want exact: which they are depends on the burst
			// descriptors this walk has written and on y, on nothing the check decides - k_burst_mark lists them here, right behind the
			// walk, and the burst decoder's first pass finds them done (a channel stitched again, a list that ran over, a refused scan:
			// the decoder's own list and second pass, as before).  One scan round in a feed's chain instead of two.
			uint32_t mq_cap = small ? kDeferScans / 16 : std::min(c->sq_alloc, defer_scans_for(D, c->C));
			if(c->debug_mark_cap) mq_cap = std::min(mq_cap, c->debug_mark_cap);
			// (on the walk stream, ahead of the hand-over to the check's stream: the kernels that rewrite this feed's burst rows later - the
			// second stitch, the feed once more after a corrected start - follow on this stream, so it reads the rows the first walk wrote)
			{
				K5mArgs k5m{ c->d_y, sl.d_bursts, sl.d_nbchan, c->cap_bursts_chan, c->C, c->cap, c->cap - 1, k4.ref, k4.ref_launch - 1u, sl.d_mq, sl.d_rqn + 7, mq_cap };
				const unsigned k5_lds = (unsigned)((sizeof(BurstShared) + 4 * (kK5MaxChan + 1)) * kBurstWaves);
				hipLaunchKernelGGL(k_burst_mark, dim3(sl.k5_waves / kBurstWaves), dim3(64 * kBurstWaves), k5_lds, sb_, k5m);
			}
			if(sc_ != sb_) { HIPCHK(hipEventRecord(sl.ev_stitch, sb_)); HIPCHK(hipStreamWaitEvent(sc_, sl.ev_stitch, 0)); }
			launch_scans(c, sc_, k4.ref, k4.ref_launch - 1u, nullptr, k4.rq, k4.rq_n, rq_cap, k1, sl.d_retry + kRetryScans, sl.d_rqn + 5, nullptr, nullptr, sl.d_mq, sl.d_rqn + 7, mq_cap);
			hipLaunchKernelGGL(k_ref_verify, dim3(small ? 64 : 1024), dim3(64), 0, sc_, k4);
			HIPCHK(hipEventRecord(sl.ev_chk, sc_));
		}
	}
	sl.rest_pending = true;
	// the feeds whose second walks have now waited for the one successor's walk that they may (walk ahead), or for none ...
	for(;;) {
		OutSlot *old = nullptr;
		for(auto &x : c->slot) if(x.pending && x.rest_pending && (!old || x.seq < old->seq)) old = &x;
		if(!old || old == &sl || sl.seq - old->seq < (uint64_t)wa) break;
		int r = flush_rest(c, old); if(r != VDL2HIP_OK) return r;
	}
	// does the NEXT feed's walk get the chance to go ahead of this feed's check?  Not if there is nothing to check, nor in the old schedule
	if(!(wa && sl.has_chk && sl.nseg >= 2)) return flush_rest(c, nullptr);
	HIPCHK(hipGetLastError());
	return VDL2HIP_OK;
}

// The feeds whose walk and check are queued and the rest is not (rest_pending), oldest first, up to and including `upto` (nullptr: all
// of them): each with the feed behind it, if that one's walk is queued, as its successor (its walk went ahead of this feed's check).
static int flush_rest(vdl2hip_ctx *c, const OutSlot *upto) {
	for(;;) {
		OutSlot *old = nullptr;
		for(auto &x : c->slot) if(x.pending && x.rest_pending && (!old || x.seq < old->seq)) old = &x;
		if(!old || (upto && old->seq > upto->seq)) return VDL2HIP_OK;
		OutSlot *s1 = &c->slot[(old->seq + 1) % kSlots];
		if(!(s1->pending && s1->rest_pending && s1->seq == old->seq + 1)) s1 = nullptr;
		int r = launch_rest(c, *old, s1); if(r != VDL2HIP_OK) return r;
	}
}

static int launch_rest(vdl2hip_ctx *c, OutSlot &sl, OutSlot *succ) {
	const int64_t D = sl.back_D, k0 = sl.back_k0;
	const bool small = sl.small;
	hipStream_t sb_ = small ? c->streams.front : c->streams.back, sn_ = small ? c->streams.front : c->streams.nf, s5_ = small ? c->streams.front : c->streams.burst[sl.seq % kSideBurst];

	const Event *ev = sl.ev;
	const bool prof_all = sl.ev_valid && sl.ev_level >= 2;
	sl.rest_pending = false;
	if(D > 0 && sl.has_chk) {
		// the (rare) channel one of whose decisions did not stand is stitched again
		HIPCHK(hipStreamWaitEvent(sb_, sl.ev_chk, 0));
		K4Args k4 = sl.k4;
		if(succ) { k4.ws_snap_next = succ->k4.ws_snap; k4.cnt_snap_next = succ->k4.cnt_snap; k4.rq_flag2_next = succ->d_rqflag2; }
		if(sl.nseg >= 2) launch_stitch(c, sb_, sl, k4, succ ? 2 : 1);
		else hipLaunchKernelGGL(k_walk_again, dim3((unsigned)c->C), dim3(64), 0, sb_, k4);      // (never with a successor: launch_back)
	}
	if(!small) {
		HIPCHK(hipEventRecord(sl.ev_walk, sb_));
		HIPCHK(hipStreamWaitEvent(sn_, sl.ev_walk, 0));
		HIPCHK(hipStreamWaitEvent(s5_, sl.ev_walk, 0));
	}
	// ... and the next feed once more for the channels whose start state that has corrected (none, all but always: the kernel looks at the flags and ends)
	if(succ) launch_stitch(c, sb_, *succ, succ->k4, 3);
	if(D > 0) {
		K4bArgs k4b{ c->d_y, c->d_nf, sl.d_log, sl.d_nlog, c->d_scfirst, c->d_sccum, c->d_nffeed, c->d_lpbuf, c->d_nfring, c->nf_ring - 1,
		             c->cap, c->cap - 1, c->cap_log, c->cap_comb, c->cap_hist, c->C };
		const unsigned nf_lds = (unsigned)(sizeof(NfShared) * kNfWaves), nf_grid = (unsigned)((c->C + kNfWaves - 1) / kNfWaves);
		if(small) {
			// (queued below, together with the burst decoder: k_nf_burst)
		} else {
			hipExtLaunchKernelGGL(k_nf_prepare, dim3(nf_grid), dim3(64 * kNfWaves), nf_lds, sn_, EV(8), (hipEvent_t) nullptr, 0, k4b);
			const unsigned ngrp = (unsigned)std::min<uint64_t>(64, (c->cap_hist + kNfGroup * kNfWaves - 1) / (kNfGroup * kNfWaves));   // workgroups per channel
			hipLaunchKernelGGL(k_nf_replay, dim3(ngrp, (unsigned)c->C), dim3(64 * kNfWaves), nf_lds, sn_, k4b);
			hipExtLaunchKernelGGL(k_nf_finish, dim3(nf_grid), dim3(64 * kNfWaves), nf_lds, sn_, (hipEvent_t) nullptr, EV(9), 0, k4b);
			HIPCHK(hipEventRecord(sl.ev_nf, sn_));
		}
		K5Args k5{ c->d_y, c->d_tab, c->d_cnt, sl.d_bursts, sl.d_nbchan, c->cap_bursts_chan, c->C,
		           sl.d_frames, sl.d_pool, sl.d_ctl, c->d_freq, c->cap, c->cap - 1, c->referee ? c->d_ref[sl.seq % kSlots] : nullptr, (uint32_t)(16 * sl.seq + 5), BurstDefer{} };
		// referee: a burst that needs a scan is listed by the first pass, the scans run side by side, a second pass decodes the listed bursts.
		// (Short feeds too, since round 6c: their burst wavefronts used to scan on the spot - a weak burst with ten marked symbols held its
		// block for 22 ms, profiles/r06_weak_bursts.txt; their lists and the grids that serve them are a sixteenth of a long feed's.)
		const bool defer5 = c->referee;
		const uint32_t sq_cap = small ? kDeferScans / 16 : std::min(c->sq_alloc, defer_scans_for(D, c->C)), dq_cap = sq_cap / 2;
		if(defer5) k5.df = BurstDefer{ sl.d_dq, sl.d_rqn + 1, dq_cap, sl.d_sq, sl.d_rqn + 2, sq_cap, 1, c->d_refstats + 12 };
		const unsigned k5_lds = (unsigned)((sizeof(BurstShared) + 4 * (kK5MaxChan + 1)) * kBurstWaves);
		hipEvent_t ev_last5 = defer5 ? (hipEvent_t) nullptr : EV(11);
		if(small) hipExtLaunchKernelGGL(k_nf_burst, dim3(nf_grid + sl.k5_waves / kBurstWaves), dim3(64 * kNfWaves), std::max(nf_lds, k5_lds), s5_, EV(8), ev_last5, 0, k4b, k5, (uint32_t)nf_grid);
		else hipExtLaunchKernelGGL(k_burst, dim3(sl.k5_waves / kBurstWaves), dim3(64 * kBurstWaves), k5_lds, s5_, EV(10), ev_last5, 0, k5);
		if(defer5) {
			launch_scans(c, s5_, k5.ref, (uint32_t)(16 * sl.seq + 6), sl.d_sq, nullptr, sl.d_rqn + 2, sq_cap, k0 + D, sl.d_retry + 2 * kRetryScans, sl.d_rqn + 6);
			K5Args k5b = k5; k5b.df.pass = 2; k5b.ref_launch = (uint32_t)(16 * sl.seq + 7);
			hipExtLaunchKernelGGL(k_burst, dim3(std::max(1u, dq_cap / kBurstWaves / 4)), dim3(64 * kBurstWaves), k5_lds, s5_, (hipEvent_t) nullptr, EV(11), 0, k5b);
		}
		if(!small) HIPCHK(hipStreamWaitEvent(s5_, sl.ev_nf, 0));
		// record chunks of kFrameChunk: enough workgroups for the records the burst decoder's wavefronts own, at most 256
		const unsigned ff_grid = std::min(256u, (sl.k5_waves * (unsigned)kResSlots * 2 / kFrameChunk + kFrameWaves - 1) / kFrameWaves);
		hipLaunchKernelGGL(k_frame_finish, dim3(ff_grid), dim3(64 * kFrameWaves), 0, s5_, sl.d_frames, (const uint8_t *)sl.d_pool, sl.d_mail, (const Tables *)c->d_tab,
		                   c->d_acnt, (const float *)c->d_nfring, c->nf_ring - 1, sl.d_frames_out, sl.d_pool_out);
		// the burst capture reads this feed's burst lists and y here: both passes of the burst decoder and its scans are done
		if(sl.cap.on) { int r = capture_launch(c, sl, s5_); if(r != VDL2HIP_OK) return r; }
		// ... and so does burst timing
		if(sl.toa.on) { int r = toa_launch(c, sl, s5_); if(r != VDL2HIP_OK) return r; }
		// the transmission log's header and first records of this feed (written on the front stream ahead of the sync kernels: long done)
		if(sl.txl.on) HIPCHK(sl.txl.mail.post(s5_));
		// the preamble search reads the log's records of this feed (the same ordering) and y here, like the capture
		if(sl.txl.on && c->txs.on) { int r = txsearch_launch(c, sl, s5_); if(r != VDL2HIP_OK) return r; }
		// the second look reads the search's plan of this feed, the log's records and y behind it
		if(sl.txs.on && c->rl.on) { int r = relook_launch(c, sl, s5_); if(r != VDL2HIP_OK) return r; }
		// ... and so does the transmission capture
		if(sl.txl.on && c->txc.on) { int r = txcap_launch(c, sl, s5_); if(r != VDL2HIP_OK) return r; }
	}
	// the control block and the first few delivered frames in one copy (collect_slot)
	HIPCHK(hipMemcpyAsync(sl.h_mail, sl.d_mail, sizeof(OutMail), hipMemcpyDeviceToHost, s5_));
	HIPCHK(hipEventRecord(sl.done, s5_));
	HIPCHK(hipGetLastError());
	return VDL2HIP_OK;
}

static void sort_queue(vdl2hip_ctx *c) {
	std::stable_sort(c->queue.begin(), c->queue.end(), [](const HostFrame &a, const HostFrame &b) {
		if(a.f.end_sample != b.f.end_sample) return a.f.end_sample < b.f.end_sample;
		if(a.f.chan != b.f.chan) return a.f.chan < b.f.chan;
		return a.f.idx < b.f.idx;
	});
}

static void fill_frame(const vdl2hip_ctx *c, const HostFrame &h, vdl2hip_frame &f) {
	f.chan = (uint32_t)(h.f.chan + c->chan_first); f.freq = c->freqs[h.f.chan]; f.idx = h.f.idx;
	f.len = h.f.len; f.octets = h.octets();
	f.synd_weight = h.f.synd_weight; f.datalen_octets = h.f.datalen_octets; f.num_fec_corrections = h.f.num_fec_corrections;
	f.frame_pwr_dbfs = h.f.frame_pwr_dbfs; f.nf_pwr_dbfs = h.f.nf_pwr_dbfs; f.ppm_error = h.f.ppm_error;
	f.burst_ord = h.f.burst_ord; f.sync_sample = h.f.sync_sample; f.end_sample = h.f.end_sample;
	f.avlc_status = h.f.avlc_status; f.dst_addr = h.f.dst_addr; f.src_addr = h.f.src_addr;
}

namespace {
std::mutex g_pool_mutex;
std::vector<StreamSet> g_pool;
}  // namespace

extern "C" {

int vdl2hip_abi_version(void) { return VDL2HIP_ABI_VERSION; }

const char *vdl2hip_strerror(int err) {
	switch(err) {
		case VDL2HIP_OK: return "ok";
		case VDL2HIP_E_INVAL: return "invalid argument";
		case VDL2HIP_E_NOMEM: return "out of memory";
		case VDL2HIP_E_DEVICE: return "HIP device error";
		case VDL2HIP_E_TOOBIG: return "block larger than max_block_bytes";
		case VDL2HIP_E_OVERFLOW: return "device output buffer overflow";
		default: return "unknown error";
	}
}

// Everything a receiver holds is a member that frees itself (hostmem.h) - except its streams, which go to the pool.  Nothing is
// freed while a stream of the receiver may still be running something that reads it: all of them are waited for first.
void vdl2hip_destroy(vdl2hip_ctx *c) {
	if(!c) return;
	OnDevice dev_guard(c);
	c->streams.each([](hipStream_t st) { if(st) (void)hipStreamSynchronize(st); });
	if(c->streams.front && c->pooled) {
		std::lock_guard<std::mutex> lk(g_pool_mutex);
		g_pool.push_back(c->streams);
	} else c->streams.each([](hipStream_t st) { if(st) (void)hipStreamDestroy(st); });
	delete c;
}

// The caller's configuration as this build's structure: one that ends before input_rate (struct_size 56, built against the header
// before it) is taken with input_rate 0.
static int cfg_read(const vdl2hip_cfg *in, vdl2hip_cfg &cfg) {
	if(!in || in->struct_size < VDL2HIP_CFG_SIZE_V1) return VDL2HIP_E_INVAL;
	memset(&cfg, 0, sizeof cfg);
	memcpy(&cfg, in, in->struct_size >= sizeof(vdl2hip_cfg) ? sizeof(vdl2hip_cfg) : (size_t)VDL2HIP_CFG_SIZE_V1);
	cfg.struct_size = sizeof(vdl2hip_cfg); cfg.reserved0 = 0;
	return cfg.reserved1 ? VDL2HIP_E_INVAL : VDL2HIP_OK;
}

int vdl2hip_create(const vdl2hip_cfg *cfg_in, vdl2hip_ctx **out) {
	vdl2hip_cfg cfg_v;
	if(!out || cfg_read(cfg_in, cfg_v) != VDL2HIP_OK) return VDL2HIP_E_INVAL;
	const vdl2hip_cfg *cfg = &cfg_v;
	if(!cfg->freqs || cfg->nchan == 0) return VDL2HIP_E_INVAL;
	if(cfg->oversample == 0 || cfg->oversample > (uint32_t)kMaxOversample) return VDL2HIP_E_INVAL;
	const int fmt = fmt_code(cfg->sample_fmt);
	if(fmt < 0) return VDL2HIP_E_INVAL;
	uint32_t first = cfg->chan_first, count = cfg->chan_count ? cfg->chan_count : cfg->nchan - first;
	if(first >= cfg->nchan || first + count > cfg->nchan || count > (uint32_t)kK5MaxChan) return VDL2HIP_E_INVAL;
	// a receiver that resamples: the ratio must be one the resampler takes, and a block must stay a block
	const bool resample = cfg->input_rate != 0 && cfg->input_rate != (uint32_t)kSymbolRate * kSps * cfg->oversample;
	ResamplerDesign rd;
	uint64_t rs_max_out = 0;
	if(resample) {
		if(!design_resampler(cfg->input_rate, (uint32_t)kSymbolRate * kSps * cfg->oversample, rd, false)) return VDL2HIP_E_INVAL;
		const uint64_t max_in = (cfg->max_block_bytes ? cfg->max_block_bytes : 320000u) / raw_bytes(fmt);
		rs_max_out = (max_in * rd.L + rd.M - 1) / rd.M + 1;
		if(rs_max_out >= (1ull << 31)) return VDL2HIP_E_INVAL;
	}
	*out = nullptr;
	int ndev = 0;
	if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		fprintf(stderr, "vdl2hip: no HIP device available - this library has no CPU path\n");
		return VDL2HIP_E_DEVICE;
	}
	if(cfg->device < 0 || cfg->device >= ndev) return VDL2HIP_E_INVAL;
	struct Restore { int prev = -1; Restore() { (void)hipGetDevice(&prev); } ~Restore() { if(prev >= 0) (void)hipSetDevice(prev); } } restore_device;
	HIPCHK(hipSetDevice(cfg->device));
	vdl2hip_ctx *c = new(std::nothrow) vdl2hip_ctx();
	if(!c) return VDL2HIP_E_NOMEM;
	c->cfg = *cfg; c->cfg.freqs = nullptr;
	c->C = (int)count; c->chan_first = (int)first; c->os = (int)cfg->oversample; c->fmt = fmt;
	c->in_fmt = c->fmt;
	if(resample) { c->rs.on = true; c->fmt = kFmtCF32; }    // what the channeliser and the referee read is r[]
	c->freqs.assign(cfg->freqs + first, cfg->freqs + first + count);
	c->all_freqs.assign(cfg->freqs, cfg->freqs + cfg->nchan);
	const uint32_t fs = (uint32_t)kSymbolRate * kSps * cfg->oversample;
	c->lpf = design_lpf(8000.f / (float)fs, 0.5f);                // input_lpf_init(), demod.c:45-46,367-370
	c->specialised = (c->os == 10 || c->os == 13 || c->os == 20);
	c->run = c->specialised ? kRun : kRunGeneric;
	c->cr = c->C >= 16 ? 4 : c->C >= 8 ? 2 : 1;                   // channels per wave: keep >= 4 channel groups where possible
	c->bf = derive_block_form(c->lpf, c->os, c->run);
	c->dphi.resize(count);
	for(uint32_t i = 0; i < count; i++) c->dphi[i] = nco_step(cfg->centerfreq, c->freqs[i], fs) & 0xffffffu;

	const uint32_t max_bytes = cfg->max_block_bytes ? cfg->max_block_bytes : 320000u;
	const size_t sb = raw_bytes(c->fmt);
	const uint64_t max_samples = (resample ? rs_max_out : max_bytes / sb) + c->os;
	const uint64_t dmax = max_samples / c->os + 1;
	c->dmax = dmax;
	uint32_t cap = 1; while(cap < kSlots * dmax + kHistory + 1024) cap <<= 1;   // kSlots feeds may be in flight (fronts of i+1, i+2 over back of i)
	c->cap = cap;
	c->in_cap = max_bytes;
	c->nseg_cap = (uint32_t)(dmax / (64 * c->run) + 2);

	// (every way out of here that is a failure ends in vdl2hip_destroy(c): what the receiver holds by then goes with it)
	// DEV_ALLOC(buffer, elements[, true: zeroed])
	#define DEV_ALLOC(buf, ...) do { const hipError_t e_ = (buf).alloc(__VA_ARGS__); if(e_ != hipSuccess) { vdl2hip_destroy(c); return e_ == hipErrorOutOfMemory ? VDL2HIP_E_NOMEM : VDL2HIP_E_DEVICE; } } while(0)
	#define DEV_CHK(expr) do { if((expr) != hipSuccess) { vdl2hip_destroy(c); return VDL2HIP_E_DEVICE; } } while(0)
	{
		int prio_low = 0, prio_high = 0;
		DEV_CHK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
		bool from_pool = false;
		{
			std::lock_guard<std::mutex> lk(g_pool_mutex);
			for(size_t i = 0; i < g_pool.size(); i++) if(g_pool[i].device == cfg->device) {
				c->streams = g_pool[i]; g_pool.erase(g_pool.begin() + (long)i);
				from_pool = true;
				break;
			}
		}
		if(!from_pool) {
		c->streams.device = cfg->device;
		DEV_CHK(hipStreamCreateWithPriority(&c->streams.front, hipStreamNonBlocking, prio_low));
		// The walk goes first whenever it competes with the channeliser of a later feed (every later stage waits for it).  The
		// noise-floor and burst streams do not: their many single-wave workgroups, dispatched with priority, each take the
		// register slot of one of the four waves a channeliser workgroup needs on a CU and so keep whole workgroups out; at
		// the front's priority they fill in while the sync kernels (few registers) run.  Measured at 256 channels
		// (profiles/r02_stream_priorities.txt): all three high 7.10 ms/step, walk only 6.91, none 6.93; no difference at 8.
		DEV_CHK(hipStreamCreateWithPriority(&c->streams.back, hipStreamNonBlocking, prio_high));
		DEV_CHK(hipStreamCreateWithPriority(&c->streams.nf, hipStreamNonBlocking, prio_low));
		for(auto &sp : c->streams.pre) DEV_CHK(hipStreamCreateWithPriority(&sp, hipStreamNonBlocking, prio_high));
		for(auto &sb5 : c->streams.burst) DEV_CHK(hipStreamCreateWithPriority(&sb5, hipStreamNonBlocking, prio_low));
		DEV_CHK(hipStreamCreateWithFlags(&c->streams.copy, hipStreamNonBlocking));
		DEV_CHK(hipStreamCreateWithFlags(&c->streams.out, hipStreamNonBlocking));
		}
		c->pooled = true;
	}
	for(auto &sl : c->slot) {
		DEV_CHK(sl.done.ensure()); for(auto &e : sl.ev) DEV_CHK(e.ensure());
		DEV_CHK(sl.ev_walk.ensure(hipEventDisableTiming)); DEV_CHK(sl.ev_nf.ensure(hipEventDisableTiming));
		DEV_CHK(sl.ev_front.ensure());
	}
	DEV_ALLOC(c->d_bf, 1); DEV_ALLOC(c->d_lut, 256); DEV_ALLOC(c->d_tab, 1);
	if(resample) {
		auto &rs = c->rs;
		if(!design_resampler(cfg->input_rate, fs, rd)) { vdl2hip_destroy(c); return VDL2HIP_E_INVAL; }
		rs.L = rd.L; rs.M = rd.M; rs.T = rd.T; rs.cap = rs_max_out;
		rs.span_cap = (uint32_t)((255ull * rs.M + rs.L - 1) / rs.L) + rs.T;             // a tile's 256 outputs: the span of their b, and the T - 1 samples before
		const size_t ntaps = (size_t)rs.L * rs.T, tap_bytes = ntaps * sizeof(float);
		rs.taps_lds = tap_bytes <= kResTapsLds;
		rs.lds = (size_t)rs.span_cap * sizeof(float2) + (rs.taps_lds ? tap_bytes : 0);
		// walk order (resample.h): column q of the table is phase (q M) mod L, the phase of every output n with n mod L = q
		std::vector<float> walk(ntaps);
		for(uint32_t j = 0; j < rs.T; j++) for(uint32_t q = 0; q < rs.L; q++) walk[(size_t)j * rs.L + q] = rd.taps[(size_t)j * rs.L + (size_t)((uint64_t)q * rs.M % rs.L)];
		DEV_ALLOC(rs.d_taps, ntaps);
		DEV_CHK(hipMemcpy(rs.d_taps, walk.data(), tap_bytes, hipMemcpyHostToDevice));
		for(auto &t : rs.d_tail) DEV_ALLOC(t, rs.T, true);   // x[i < 0] = 0
		for(auto &o : rs.d_out) DEV_ALLOC(o, (size_t)rs.cap + 2);      // (two samples of slack behind a block)
	}
	DEV_ALLOC(c->d_dphi, count); DEV_ALLOC(c->d_freq, count); DEV_ALLOC(c->d_ppmthr, count);
	DEV_ALLOC(c->d_carry[0], sb * kMaxOversample); DEV_ALLOC(c->d_carry[1], sb * kMaxOversample);       // (bytes) fewer than `oversample` samples left over
	const size_t nring = (size_t)count * cap;
	static_assert(sizeof(cf32) == 8 && sizeof(float4) == 16 && sizeof(unsigned long long) == 8, "the sizes the counts below stand for");
	DEV_ALLOC(c->d_y, nring, true); DEV_ALLOC(c->d_pf, nring, true);
	DEV_ALLOC(c->d_cand, nring / 64, true); DEV_ALLOC(c->d_flag, nring / 64, true);      // a bit per sample (cap is a power of two >= 65536)
	DEV_ALLOC(c->d_segend, (size_t)count * c->nseg_cap, true);
	DEV_ALLOC(c->d_qpow, 64);
	DEV_ALLOC(c->d_tcarry[0], count, true); DEV_ALLOC(c->d_tcarry[1], count, true);
	DEV_ALLOC(c->d_segpub, (size_t)count * c->nseg_cap * 4, true); DEV_ALLOC(c->d_synctmo, 1, true);
	// The fused fix-up makes a workgroup wait for the workgroup of the previous segment (one-step look-back, kernels.h).  The wait is
	// short while the workgroups of a launch are dispatched in order and stay resident - one process per GPU, the deployment this
	// library is built for.  On a GPU time-sliced between PROCESSES the driver saves and restores waves in no particular order and
	// waiting consumers can hold the CUs their producers need: a consumer therefore gives up after a few milliseconds and works the
	// state out itself from the previous segment's last tile (stats.front_sync_timeouts counts those; results are unaffected).
	// VDL2HIP_NO_FUSE=1 selects the separate fix-up kernel k_fixup instead (no inter-workgroup wait at all, bit-identical results,
	// ~3 % slower): worth setting where the GPU is permanently shared, so that no time is spent waiting.
	c->fuse_k2 = getenv("VDL2HIP_NO_FUSE") == nullptr;
	DEV_ALLOC(c->d_ws, count); DEV_ALLOC(c->d_cnt, 2 * (size_t)count * kNumCounters, true); c->d_wcnt = c->d_cnt + (size_t)count * kNumCounters;
	DEV_ALLOC(c->d_acnt, (size_t)count * kNumAvlcCounters, true);
	// a decodable burst occupies >= 22 symbols = 220 decimated samples (header + 3 data + 2 FEC octets)
	c->cap_bursts_chan = (uint32_t)(dmax / 220 + 4);
	uint64_t cap_b = (uint64_t)count * c->cap_bursts_chan;
	uint64_t cap_f = cap_b * 2; if(cap_f < 4096) cap_f = 4096;
	cap_f += 2048 * kResSlots;                                    // the burst decoder's wavefronts each own a first share of the records and octets
	uint64_t cap_p = cap_b * 512; if(cap_p < (1u << 22)) cap_p = 1u << 22; if(cap_p > (1u << 30)) cap_p = 1u << 30;
	c->cap_log = 8192; c->cap_comb = c->cap_log + kNfTail; c->cap_hist = (uint32_t)(dmax / 3000 + 8);
	cap_p += 2048 * kResPool;
	c->ctl_template = OutCtl{ 0, 0, 0, 0, (uint32_t)cap_b, (uint32_t)cap_f, (uint32_t)cap_p, c->cap_log, 0, 0, {0, 0} };
	DEV_ALLOC(c->d_nf, count);
	DEV_ALLOC(c->d_scfirst, (size_t)count * (c->cap_comb + 1)); DEV_ALLOC(c->d_sccum, (size_t)count * (c->cap_comb + 1));
	// noise-floor history: a frame looks up the value at its burst's sync, at most kSlots feeds + one burst ago
	c->nf_ring = 64; while(c->nf_ring < (kSlots + 2) * c->cap_hist) c->nf_ring <<= 1;
	DEV_ALLOC(c->d_nfring, (size_t)count * c->nf_ring, true);
	DEV_ALLOC(c->d_lpbuf, (size_t)count * c->cap_hist, true); DEV_ALLOC(c->d_nffeed, count, true);
	{
		// segments per feed: enough wavefronts to cover the walk's latency, not more than the chip holds at once
		const char *e = getenv("VDL2HIP_SEG_MIN");
		if(e && atoll(e) >= 64) c->seg_min = atoll(e);
		int64_t smax = std::min<int64_t>(16, 8192 / (3 * (int64_t)count));   // measured: 8..24 are within noise of each other at 8 channels
		smax = std::min<int64_t>(smax, dmax / c->seg_min);
		e = getenv("VDL2HIP_SEG_MAX");
		if(e) smax = std::min<int64_t>(smax, atoll(e));
		c->seg_max = (int)std::max<int64_t>(1, smax);
		if(c->seg_max >= 2) for(auto &sp_ : c->d_spec) DEV_ALLOC(sp_, (size_t)count * 3 * (c->seg_max - 1));
		DEV_ALLOC(c->d_segstats, (size_t)count * 2, true);
	}
	for(auto &sl : c->slot) {
		DEV_ALLOC(sl.d_bursts, cap_b); DEV_ALLOC(sl.d_nbchan, count, true);
		DEV_ALLOC(sl.d_frames, cap_f); DEV_ALLOC(sl.d_pool, cap_p); DEV_ALLOC(sl.d_mail, 1, true);
		sl.d_ctl = &sl.d_mail.get()->ctl;
		DEV_CHK(hipMemcpy(sl.d_ctl, &c->ctl_template, sizeof(OutCtl), hipMemcpyHostToDevice));
		DEV_ALLOC(sl.d_frames_out, cap_f); DEV_ALLOC(sl.d_pool_out, cap_p);
		DEV_ALLOC(sl.d_log, (size_t)count * c->cap_log); DEV_ALLOC(sl.d_nlog, count, true);
		DEV_CHK(sl.h_mail.alloc(sizeof(OutMail), true));
	}

	if(const char *e = getenv("VDL2HIP_REFEREE")) c->referee = atoi(e) != 0;
	// Referee, long feeds: where do the scans go?  A receiver of few channels has a front of a fraction of a millisecond and its step is
	// the walk's chain - walk, scan, check, walk again - unless the scans run AHEAD of the walk on a stream per slot (`prescan`); with
	// hundreds of channels the front hides the chain and the 2.5x scans of that mode (every marked candidate, not every visited one)
	// cost more than they save.  VDL2HIP_REF_PRESCAN=0/1 overrides the choice.
	c->ref_prescan = count <= 64;
	if(const char *e = getenv("VDL2HIP_REF_PRESCAN")) c->ref_prescan = atoi(e) != 0;
	if(const char *e = getenv("VDL2HIP_REF_RETRY")) { const int v = atoi(e); if(v == 0 || (v >= 2 && v <= 8)) c->ref_retry_mul = v; }
	if(const char *e = getenv("VDL2HIP_REF_WARM")) { const long long v = atoll(e); if(v >= 1024 && v <= (1ll << 24)) c->ref_warm = v; }
	if(c->referee) {
		c->ref_T = std::max(1, c->ref_retry_mul) * c->ref_warm + (int64_t)(kHistory + 256) * c->os + 4096;      // run-up (of a retry: ref_retry_mul times the configured one) + the longest burst (its symbols are sliced when its last one has arrived)
		c->ref_cap = 1; while(c->ref_cap < (uint64_t)(kSlots + 2) * (uint64_t)c->ref_T) c->ref_cap <<= 1;
		DEV_ALLOC(c->d_refhist, c->ref_cap * sb);      // (bytes)
		for(auto &r : c->d_ref) DEV_ALLOC(r, 1, true);
		DEV_ALLOC(c->d_refdone, (size_t)count * kRefCache, true); DEV_ALLOC(c->d_refdonen, count, true); DEV_ALLOC(c->d_refstats, 16, true); DEV_ALLOC(c->d_mix, count);
		std::vector<uint8_t> mix(count);
		for(uint32_t i = 0; i < count; i++) mix[i] = cfg->centerfreq != c->freqs[i];       // v->offset_tuning, demod.c:386
		DEV_CHK(hipMemcpy(c->d_mix, mix.data(), count, hipMemcpyHostToDevice));
		for(int k = 0; k < 2; k++) { DEV_ALLOC(c->d_ws_snap[k], count); DEV_ALLOC(c->d_cnt_snap[k], (size_t)count * kNumCounters); }
		DEV_ALLOC(c->d_ws_tmp, count); DEV_ALLOC(c->d_cnt_tmp, (size_t)count * kNumCounters);
		// Walk ahead (launch_back): for receivers whose front does not hide the chain walk - scans - check (a feed's results then come a
		// feed later: with 256 channels, where the front hides the chain anyway, that extra depth cost 10 % and more)
		c->walk_ahead = (count >= 16 && count <= 64) ? 1 : 0;   // (8 channels: the walk itself is longer than the front, the second walks' extra launches cost more than they save: 1.22 against 1.11 ms)
		c->sq_alloc = defer_scans_for((int64_t)dmax, (int)count);
		for(auto &sl : c->slot) {
			DEV_ALLOC(sl.d_rq, c->rq_cap); DEV_ALLOC(sl.d_rqn, 8, true); DEV_ALLOC(sl.d_retry, 3 * (size_t)kRetryScans); DEV_ALLOC(sl.d_rqflag, count, true);
			DEV_ALLOC(sl.d_dq, c->sq_alloc / 2); DEV_ALLOC(sl.d_sq, c->sq_alloc); DEV_ALLOC(sl.d_mq, c->sq_alloc);
			DEV_ALLOC(sl.d_pq, kPreScans); DEV_CHK(sl.ev_pre.ensure(hipEventDisableTiming));
			DEV_ALLOC(sl.d_rqbad, count, true);
			DEV_ALLOC(sl.d_rqflag2, count, true);
			DEV_CHK(sl.ev_stitch.ensure(hipEventDisableTiming)); DEV_CHK(sl.ev_chk.ensure(hipEventDisableTiming));
		}
	}

	Lut4 lut[256]; build_nco_lut(lut);                            // sincosf_lut_init()
	auto tab = std::make_unique<Tables>(); build_tables(*tab);    // demod_sync_init(), rs_init(), header tables
	std::vector<WalkState> ws(count);
	for(auto &w : ws) { memset(&w, 0, sizeof w); walk_state_init(w); }
	DEV_CHK(hipMemcpy(c->d_bf, &c->bf, sizeof(BlockForm), hipMemcpyHostToDevice));
	DEV_CHK(hipMemcpy(c->d_qpow, c->bf.Qpow, 64 * sizeof(float4), hipMemcpyHostToDevice));
	DEV_CHK(hipMemcpy(c->d_lut, lut, sizeof lut, hipMemcpyHostToDevice));
	DEV_CHK(hipMemcpy(c->d_tab, tab.get(), sizeof(Tables), hipMemcpyHostToDevice));
	DEV_CHK(hipMemcpy(c->d_dphi, c->dphi.data(), 4 * count, hipMemcpyHostToDevice));
	DEV_CHK(hipMemcpy(c->d_freq, c->freqs.data(), 4 * count, hipMemcpyHostToDevice));
	{
		std::vector<float> thr(count);
		for(uint32_t i = 0; i < count; i++) thr[i] = ppm_gate_threshold(c->freqs[i], cfg->max_ppm);
		DEV_CHK(hipMemcpy(c->d_ppmthr, thr.data(), 4 * count, hipMemcpyHostToDevice));
	}
	DEV_CHK(hipMemcpy(c->d_ws, ws.data(), count * sizeof(WalkState), hipMemcpyHostToDevice));
	{
		std::vector<NfState> nfs(count);
		for(auto &n : nfs) { memset(&n, 0, sizeof n); nf_state_init(n); }
		DEV_CHK(hipMemcpy(c->d_nf, nfs.data(), count * sizeof(NfState), hipMemcpyHostToDevice));
	}
	// the generic-oversample build may need more than the default dynamic LDS limit (8192: its static LDS is 6 160 bytes; the builds with parked outputs hold 14 352, under tiles of at most 20 800)
	const size_t lds = (size_t)c->run * c->os * 65 * sizeof(float2) + 8192;
	if(lds > 65536) { vdl2hip_destroy(c); return VDL2HIP_E_INVAL; }
	DEV_CHK(hipDeviceSynchronize());
	#undef DEV_ALLOC
	#undef DEV_CHK
	*out = c;
	return VDL2HIP_OK;
}

// Host-fed blocks: the copy into the device goes to one of kSlots input buffers on the copy stream, the channeliser of the
// block waits for it on the front stream; the buffer was last read by the channeliser of feed i - kSlots, which
// collect_slot() has seen complete.  So the H2D of block i+1 overlaps the kernels of block i (and i-1, i-2 further down).
static int feed_host(vdl2hip_ctx *c, const void *buf, size_t nbytes, bool wait_copy) {
	if(!c || (!buf && nbytes)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	if(nbytes == 0) return VDL2HIP_OK;                             // process_buf_*: len == 0 is a no-op (demod.c:341,358)
	if(nbytes > c->in_cap) return VDL2HIP_E_TOOBIG;
	nbytes -= nbytes % raw_bytes(c->in_fmt);
	if(c->pinned_pending) { HIPCHK(hipEventSynchronize(c->pinned_pending)); c->pinned_pending = nullptr; }
	const int k = (int)(c->feed_no % kSlots);
	{ int r = collect_slot(c, c->slot[k]); if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r; }
	if(!c->d_in[k]) {
		if(c->d_in[k].alloc(c->in_cap + 16) != hipSuccess) return VDL2HIP_E_NOMEM;
		HIPCHK(c->ev_copied[k].ensure(hipEventDisableTiming));
	}
	// (In a stream of blocks this copy costs nothing: 200-step regions run at the same 5.51 ms per 256-channel block host-fed and
	// HBM-resident.  What a short timed region sees is the FIRST copy, which nothing overlaps: 2.6 ms once.  Holding the copy back so that
	// it lands beside the channeliser rather than the sync kernels changes nothing or makes it worse; profiles/r03_h2d_placement.txt)
	// Nothing in flight and a large block from page-locked memory (the first block of a stream, or of a timed region): the copy is cut in
	// kColdParts pieces and the channeliser follows them piece by piece (feed_common), instead of idling for the whole transfer -
	// 2.6 ms for a 134 MB block.  In a running stream the copy of block i+1 is hidden behind the kernels of block i and goes in one piece.
	bool parts = !wait_copy && nbytes >= kColdMinBytes && !c->rs.on && !c->mon.on;      // (a block that is resampled goes through k_resample whole, one the monitor sees through k_spectrum)
	for(auto &sl : c->slot) if(sl.pending) parts = false;
	c->cold.n = 0;
	if(parts) {
		const size_t piece = (nbytes / kColdParts) & ~(size_t)4095;
		static_assert(4096 % 8 == 0 && 4096 % 4 == 0, "a piece of a cold-start block ends on a sample boundary in every format");
		if(piece % raw_bytes(c->fmt)) return VDL2HIP_E_INVAL;
		size_t off = 0;
		for(int p = 0; p < kColdParts; p++) {
			const size_t len = p == kColdParts - 1 ? nbytes - off : piece;
			HIPCHK(c->cold.ev[p].ensure(hipEventDisableTiming));
			HIPCHK(hipMemcpyAsync(c->d_in[k] + off, (const uint8_t *)buf + off, len, hipMemcpyHostToDevice, c->streams.copy));
			HIPCHK(hipEventRecord(c->cold.ev[p], c->streams.copy));
			off += len;
			c->cold.samples[p] = off / raw_bytes(c->fmt);
		}
		c->cold.n = kColdParts;
	} else if(wait_copy) {
		// vdl2hip_feed(): `buf` is only ours during the call, so the copy is the blocking one - and a copy the host has waited for
		// needs no event for the front stream to wait on (0.190 -> 0.174-0.181 ms per 320 000-byte block against the asynchronous copy
		// + event + wait it replaces; profiles/r04_dropin_feed_path_ab.txt)
		// RELIES ON: ROCm's hipMemcpy() returns when the data is in device memory, for pageable and page-locked sources alike (the
		// front stream is hipStreamNonBlocking - no implicit ordering with the null stream the copy runs on - and nothing else makes
		// it wait).  CUDA only promises that much for page-locked sources; on a HIP back end without it, use the asynchronous branch
		// below (copy stream + event).  The call also waits for whatever else the process has on the legacy default stream.
		HIPCHK(hipMemcpy(c->d_in[k], buf, nbytes, hipMemcpyHostToDevice));
	} else {
		HIPCHK(hipMemcpyAsync(c->d_in[k], buf, nbytes, hipMemcpyHostToDevice, c->streams.copy));
	}
	if(!wait_copy) {
		HIPCHK(hipEventRecord(c->ev_copied[k], c->streams.copy));
		c->pinned_pending = c->ev_copied[k];
		if(!parts) HIPCHK(hipStreamWaitEvent(c->streams.front, c->ev_copied[k], 0));
	}
	int r = feed_block(c, c->d_in[k], nbytes, parts);
	if(r == VDL2HIP_E_DEVICE) c->failed = true;          // part of the block's work may be queued, part not: the context is out of step with itself
	return r;
}

int vdl2hip_feed(vdl2hip_ctx *c, const void *buf, size_t nbytes) { return feed_host(c, buf, nbytes, true); }

int vdl2hip_feed_pinned(vdl2hip_ctx *c, const void *buf, size_t nbytes) { return feed_host(c, buf, nbytes, false); }

int vdl2hip_feed_device(vdl2hip_ctx *c, const void *dev_buf, size_t nbytes) {
	if(!c || (!dev_buf && nbytes)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(nbytes == 0) return VDL2HIP_OK;
	if(nbytes > c->in_cap) return VDL2HIP_E_TOOBIG;
	if(((uintptr_t)dev_buf) % raw_bytes(c->in_fmt)) return VDL2HIP_E_INVAL;
	nbytes -= nbytes % raw_bytes(c->in_fmt);
	if(c->failed) return VDL2HIP_E_DEVICE;
	int r = feed_block(c, dev_buf, nbytes);
	if(r == VDL2HIP_E_DEVICE) c->failed = true;
	return r;
}

int vdl2hip_sync(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->pinned_pending) { HIPCHK(hipEventSynchronize(c->pinned_pending)); c->pinned_pending = nullptr; }
	if(c->failed) return VDL2HIP_E_DEVICE;
	return collect_pending(c);
}

int vdl2hip_drain(vdl2hip_ctx *c, vdl2hip_frame_cb cb, void *user) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	int r = collect_pending(c, c->drain_lag);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	sort_queue(c);
	int n = 0;
	for(const HostFrame &h : c->queue) {
		if(cb) {
			vdl2hip_frame f{};
			fill_frame(c, h, f);
			cb(&f, user);
		}
		n++;
	}
	c->queue.clear();
	return n;
}

int vdl2hip_drain_packed(vdl2hip_ctx *c, vdl2hip_packed_frame *frames, size_t cap_frames,
		uint8_t *octets, size_t cap_octets, size_t *octets_used) {
	if(!c || (!frames && cap_frames) || (!octets && cap_octets)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	int r = collect_pending(c, c->drain_lag);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	sort_queue(c);
	size_t n = 0, used = 0;
	for(const HostFrame &h : c->queue) {
		if(n >= cap_frames || used + h.f.len > cap_octets) break;
		fill_frame(c, h, frames[n].frame);
		frames[n].frame.octets = nullptr;
		frames[n].octets_off = used;
		if(h.f.len && h.octets()) memcpy(octets + used, h.octets(), h.f.len);
		used += h.f.len;
		n++;
	}
	c->queue.erase(c->queue.begin(), c->queue.begin() + (long)n);
	if(octets_used) *octets_used = used;
	return (int)n;
}

// ---- proto3 wire format, hand-rolled (no protobuf runtime in the product) ----
namespace {
struct PbOut {
	uint8_t *p; size_t cap, n; bool ok;
	void byte(uint8_t b) { if(n < cap) p[n] = b; else ok = false; n++; }
	void varint(uint64_t v) { while(v >= 0x80) { byte((uint8_t)(v | 0x80)); v >>= 7; } byte((uint8_t)v); }
	void tag(uint32_t field, uint32_t wt) { varint((uint64_t)field << 3 | wt); }
	void u32(uint32_t field, uint32_t v) { if(v) { tag(field, 0); varint(v); } }                       // proto3: defaults are omitted
	void i32(uint32_t field, int32_t v) { if(v) { tag(field, 0); varint((uint64_t)(int64_t)v); } }      // negative int32 -> 10-byte varint
	void i64(uint32_t field, int64_t v) { if(v) { tag(field, 0); varint((uint64_t)v); } }
	void f32(uint32_t field, float v) { uint32_t u; memcpy(&u, &v, 4); if(u) { tag(field, 5); for(int i = 0; i < 4; i++) byte((uint8_t)(u >> (8 * i))); } }
	void bytes(uint32_t field, const uint8_t *d, size_t len) { tag(field, 2); varint(len); for(size_t i = 0; i < len; i++) byte(d[i]); }
};
size_t pack_metadata(PbOut &o, const vdl2hip_frame *f, const char *station_id, int64_t tv_sec, int64_t tv_usec) {
	const size_t start = o.n;
	if(station_id && station_id[0]) o.bytes(1, (const uint8_t *)station_id, strlen(station_id));
	o.u32(2, f->freq); o.u32(3, f->synd_weight); o.u32(4, f->datalen_octets);
	o.f32(5, f->frame_pwr_dbfs); o.f32(6, f->nf_pwr_dbfs); o.f32(7, f->ppm_error);
	o.i32(8, 1 /* metadata->version, src/decode.c:177 */); o.i32(9, f->num_fec_corrections); o.i32(10, f->idx);
	uint8_t tsbuf[24]; PbOut ts{ tsbuf, sizeof tsbuf, 0, true };
	ts.i64(1, tv_sec); ts.i64(2, tv_usec);
	o.bytes(11, tsbuf, ts.n);                                    // the timestamp sub-message is always present (src/fmtr-binary.c:38)
	return o.n - start;
}
}  // namespace

int vdl2hip_pack_raw_frame(const vdl2hip_frame *f, const char *station_id, int64_t tv_sec, int64_t tv_usec, uint8_t *out, size_t cap) {
	if(!f || !out || (f->len && !f->octets)) return VDL2HIP_E_INVAL;
	uint8_t meta[512]; PbOut m{ meta, sizeof meta, 0, true };
	pack_metadata(m, f, station_id, tv_sec, tv_usec);
	if(!m.ok) return VDL2HIP_E_TOOBIG;
	PbOut o{ out, cap, 0, true };
	o.byte(0); o.byte(0);                                         // record length, patched below
	o.bytes(1, meta, m.n);
	if(f->len) o.bytes(2, f->octets, f->len);                    // proto3 omits empty bytes
	if(!o.ok || o.n > 65535) return VDL2HIP_E_TOOBIG;
	out[0] = (uint8_t)(o.n >> 8); out[1] = (uint8_t)o.n;         // htons(payload + 2), src/output-file.c:181-188
	return (int)o.n;
}

int vdl2hip_counters(vdl2hip_ctx *c, uint32_t chan, uint64_t out[VDL2HIP_NUM_COUNTERS]) {
	if(!c || !out || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	uint64_t w[kNumCounters];
	HIPCHK(hipMemcpy(out, c->d_cnt + (size_t)(chan - c->chan_first) * kNumCounters, 8 * kNumCounters, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(w, c->d_wcnt + (size_t)(chan - c->chan_first) * kNumCounters, 8 * kNumCounters, hipMemcpyDeviceToHost));
	for(int k = 0; k < kNumCounters; k++) out[k] += w[k];      // the burst decoder's row + the walker's
	return VDL2HIP_OK;
}

int vdl2hip_avlc_counters(vdl2hip_ctx *c, uint32_t chan, uint64_t out[VDL2HIP_NUM_AVLC_COUNTERS]) {
	if(!c || !out || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	HIPCHK(hipMemcpy(out, c->d_acnt + (size_t)(chan - c->chan_first) * kNumAvlcCounters, 8 * kNumAvlcCounters, hipMemcpyDeviceToHost));
	return VDL2HIP_OK;
}

int vdl2hip_set_avlc_filter(vdl2hip_ctx *c, int on) {
	if(!c) return VDL2HIP_E_INVAL;
	c->avlc_filter = on != 0;
	return VDL2HIP_OK;
}

// counter names in the order of the VDL2HIP_CNT_* / VDL2HIP_ACNT_* enums (statsd.c:34-65); the two diagnostics this
// implementation adds (ppm_reject, slicer_neg_idx) are exported under demod.* as well
static const char *const kCounterNames[VDL2HIP_NUM_COUNTERS] = {
	"demod.sync.good", "decoder.crc.good", "decoder.crc.bad", "decoder.errors.no_header", "decoder.errors.too_long",
	"decoder.errors.no_fec", "decoder.errors.data_truncated", "decoder.errors.fec_truncated", "decoder.errors.deinterleave_data",
	"decoder.errors.deinterleave_fec", "decoder.errors.fec_bad", "decoder.errors.bitstream", "decoder.errors.truncated_octets",
	"decoder.errors.unstuff", "decoder.blocks.processed", "decoder.blocks.fec_ok", "decoder.msg.good", "decoder.msg.good_loud",
	"demod.ppm_reject", "demod.slicer_neg_idx" };
static const char *const kAvlcCounterNames[VDL2HIP_NUM_AVLC_COUNTERS] = {
	"avlc.frames.processed", "avlc.errors.too_short", "avlc.frames.good", "avlc.errors.bad_fcs", "avlc.msg.air2gnd",
	"avlc.msg.air2air", "avlc.msg.air2all", "avlc.msg.gnd2air", "avlc.msg.gnd2gnd", "avlc.msg.gnd2all" };

int vdl2hip_statsd_lines(vdl2hip_ctx *c, const char *ns, char *out, size_t cap) {
	if(!c || !ns || !out) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	const size_t per = VDL2HIP_NUM_COUNTERS + VDL2HIP_NUM_AVLC_COUNTERS;
	std::vector<uint64_t> now((size_t)c->C * per);
	{
		std::vector<uint64_t> a(2 * (size_t)c->C * kNumCounters), b((size_t)c->C * kNumAvlcCounters);      // two copies, whatever the channel count
		HIPCHK(hipMemcpy(a.data(), c->d_cnt, a.size() * 8, hipMemcpyDeviceToHost));
		for(size_t k = 0, n = a.size() / 2; k < n; k++) a[k] += a[n + k];                               // the burst decoder's rows + the walker's
		HIPCHK(hipMemcpy(b.data(), c->d_acnt, b.size() * 8, hipMemcpyDeviceToHost));
		for(int ch = 0; ch < c->C; ch++) {
			std::copy(a.begin() + (size_t)ch * kNumCounters, a.begin() + (size_t)(ch + 1) * kNumCounters, now.begin() + ch * per);
			std::copy(b.begin() + (size_t)ch * kNumAvlcCounters, b.begin() + (size_t)(ch + 1) * kNumAvlcCounters, now.begin() + ch * per + kNumCounters);
		}
	}
	const bool first = c->statsd_prev.empty();
	if(first) c->statsd_prev.assign(now.size(), 0);
	std::string txt;
	char line[320];
	for(int ch = 0; ch < c->C; ch++)
		for(size_t k = 0; k < per; k++) {
			const uint64_t d = now[ch * per + k] - c->statsd_prev[ch * per + k];
			if(!first && d == 0) continue;
			const char *name = k < (size_t)kNumCounters ? kCounterNames[k] : kAvlcCounterNames[k - kNumCounters];
			snprintf(line, sizeof line, "%s.%u.%s:%llu|c\n", ns, c->freqs[ch], name, (unsigned long long)d);
			txt += line;
		}
	if(txt.size() + 1 > cap) { if(first) c->statsd_prev.clear(); return VDL2HIP_E_TOOBIG; }
	memcpy(out, txt.c_str(), txt.size() + 1);
	c->statsd_prev = now;
	return (int)txt.size();
}

int vdl2hip_set_profiling(vdl2hip_ctx *c, int on) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	c->profiling = on < 0 ? 0 : on > 2 ? 2 : on;
	return r == VDL2HIP_E_OVERFLOW ? VDL2HIP_OK : r;
}

int vdl2hip_get_stats_sized(vdl2hip_ctx *c, vdl2hip_stats *out, size_t size) {
	if(!c || !out) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	{
		std::vector<uint32_t> ss((size_t)c->C * 2);
		if(hipMemcpy(ss.data(), c->d_segstats, ss.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return VDL2HIP_E_DEVICE;
		c->stats.seg_adopted = c->stats.seg_walked = 0;
		uint32_t tmo = 0;
		if(hipMemcpy(&tmo, c->d_synctmo, 4, hipMemcpyDeviceToHost) != hipSuccess) return VDL2HIP_E_DEVICE;
		c->stats.front_sync_timeouts = tmo;
		for(int i = 0; i < c->C; i++) { c->stats.seg_adopted += ss[2 * i]; c->stats.seg_walked += ss[2 * i + 1]; }
	}
	if(c->d_refstats) {
		uint32_t rs[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		if(hipMemcpy(rs, c->d_refstats, sizeof rs, hipMemcpyDeviceToHost) != hipSuccess) return VDL2HIP_E_DEVICE;
		c->stats.referee_scans = rs[0]; c->stats.referee_cached = rs[1]; c->stats.referee_refused = rs[2]; c->stats.referee_short = rs[3];
		c->stats.referee_candidate_scans = rs[4]; c->stats.referee_header_scans = rs[5]; c->stats.referee_symbol_scans = rs[6]; c->stats.referee_rewalks = rs[7]; c->stats.referee_redone_next = rs[8]; c->stats.referee_unmet = rs[9]; c->stats.referee_retried = rs[10];
		c->stats.referee_symbol_pieces_ahead = rs[11]; c->stats.referee_symbol_pieces_late = rs[12];
	}
	memcpy(out, &c->stats, std::min(size, sizeof c->stats));
	return (r == VDL2HIP_E_OVERFLOW || c->failed) ? VDL2HIP_OK : r;
}
int vdl2hip_get_stats(vdl2hip_ctx *c, vdl2hip_stats *out) { return vdl2hip_get_stats_sized(c, out, sizeof(vdl2hip_stats)); }

void *vdl2hip_stream(vdl2hip_ctx *c) { return c ? (void *)c->streams.front : nullptr; }

int vdl2hip_set_drain_lag(vdl2hip_ctx *c, int lag) {
	if(!c || lag < 0 || lag > kSlots - 1) return VDL2HIP_E_INVAL;
	c->drain_lag = lag;
	return VDL2HIP_OK;
}

int vdl2hip_get_lpf(vdl2hip_ctx *c, float A[3], float B[3]) {
	if(!c) return VDL2HIP_E_INVAL;
	memcpy(A, c->lpf.A, sizeof c->lpf.A); memcpy(B, c->lpf.B, sizeof c->lpf.B);
	return VDL2HIP_OK;
}

int vdl2hip_get_nco_step(vdl2hip_ctx *c, uint32_t chan, uint32_t *dphi) {
	if(!c || !dphi || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C)) return VDL2HIP_E_INVAL;
	*dphi = nco_step(c->cfg.centerfreq, c->freqs[chan - c->chan_first], (uint32_t)kSymbolRate * kSps * c->os);
	return VDL2HIP_OK;
}

int vdl2hip_read_decimated(vdl2hip_ctx *c, uint32_t chan, int64_t first, float *dst, size_t cap) {
	if(!c || !dst || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	if(first < 0 || first > c->k_total || c->k_total - first > (int64_t)c->cap) return VDL2HIP_E_INVAL;
	size_t n = std::min<size_t>(cap, (size_t)(c->k_total - first));
	const cf32 *base = c->d_y + (size_t)(chan - c->chan_first) * c->cap;
	size_t done = 0;
	while(done < n) {
		uint32_t slot = (uint32_t)(first + (int64_t)done) & (c->cap - 1);
		size_t m = std::min<size_t>(n - done, c->cap - slot);
		HIPCHK(hipMemcpy(dst + 2 * done, base + slot, m * sizeof(cf32), hipMemcpyDeviceToHost));
		done += m;
	}
	return (int)n;
}

int vdl2hip_read_resampled(vdl2hip_ctx *c, int64_t first, float *dst, size_t cap) {
	if(!c || !dst || !c->rs.on) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	if(first < 0 || (uint64_t)first > c->rs.n_out) return VDL2HIP_E_INVAL;
	size_t done = 0;
	const size_t n = (size_t)std::min<uint64_t>(cap, c->rs.n_out - (uint64_t)first);
	while(done < n) {
		// the slot whose block holds r[pos] (the blocks of the last kSlots feeds, one after the other)
		const uint64_t pos = (uint64_t)first + done;
		int k = -1;
		for(int i = 0; i < kSlots; i++) if(c->rs.count[i] && pos >= c->rs.first[i] && pos < c->rs.first[i] + c->rs.count[i]) k = i;
		if(k < 0) return done ? (int)done : VDL2HIP_E_INVAL;      // older than what the device keeps
		const size_t m = (size_t)std::min<uint64_t>(n - done, c->rs.first[k] + c->rs.count[k] - pos);
		HIPCHK(hipMemcpy(dst + 2 * done, c->rs.d_out[k] + (pos - c->rs.first[k]), m * sizeof(float2), hipMemcpyDeviceToHost));
		done += m;
	}
	return (int)n;
}

int vdl2hip_resampler_design(uint32_t input_rate, uint32_t output_rate, uint32_t *L, uint32_t *M, uint32_t *T, float *taps, size_t cap) {
	ResamplerDesign d;
	if(!design_resampler(input_rate, output_rate, d, false)) return VDL2HIP_E_INVAL;       // (a refused ratio)
	if(L) *L = d.L;
	if(M) *M = d.M;
	if(T) *T = d.T;
	if(!taps || (size_t)d.L * d.T > cap) return VDL2HIP_E_TOOBIG;
	if(!design_resampler(input_rate, output_rate, d)) return VDL2HIP_E_INVAL;
	memcpy(taps, d.taps.data(), d.taps.size() * sizeof(float));
	return (int)d.taps.size();
}

}  // extern "C"

#include "debug_hooks.inc"   // vdl2hip_debug_*: the test and measurement hooks (needs the statics above)
#include "group.inc"   // vdl2hip_group_*: one receiver over several GPUs of this process (needs the statics above)
#include "ubench.inc"  // vdl2hip_debug_ubench(): issue and LDS-gather rates measured on the spot (bench.py's roofline line)
