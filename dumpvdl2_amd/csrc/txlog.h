// txlog.h - the transmission log: every transmission the activity monitor sees on a channel, one record each, once it has closed.
// Not in the reference.  Definition: vdl2hip.h, "Transmission log".  It sits on top of the activity monitor (activity.h): it reads the
// series p_c[m] that k_activity_power wrote, applies the monitor's threshold and hang rule, and keeps a per-channel state OF ITS OWN
// (TxState) - ActChan, ActState, the series and the carries are read and never written.  Two kernels on the front stream directly
// behind k_activity_scan of the same feed:
//
// k_txlog_plan: one wavefront per channel over the bins the feed completed, 64 at a time.  The busy flags are one ballot mask; the
// transmissions that CLOSE in the word - busy bins with no busy bin among the H + 1 bins after them, the close being bin last + H + 1 -
// come from bit operations on it (txl_masks), with what the state carried in from earlier words and feeds.  The channel's number of
// closes goes to cnt[c]; the state is left as it was.
//
// k_txlog_emit: one wavefront per channel again.  Every workgroup turns the channels' counts into offsets in LDS (k_capture_copy's
// idiom: a load per lane and 64 channels, a scan), so a channel knows where its records go without a third kernel or an atomic.  It
// walks the channel's words again from the saved state.  Per word a SEGMENTED inclusive scan over the wavefront - segments begin at
// the word's transmission starts, six levels of __shfl_up, lane i taking in lane i - d only if no start lies in (i - d, i] - gives
// every lane busy_bins, the float64 sum, the peak and the lowest peak bin of its transmission from that transmission's first bin in
// the word up to the lane.  The lane of a close bin therefore holds the whole of its transmission's share of this word; what earlier
// words and feeds held of it is in the state (TxState.acc) and is combined in front.  That lane builds the record and stores it at
// the channel's offset + the closes before it, if it lies inside the pool (vector stores, no atomics).  The last lane's value is
// what the state carries on.  Order of the float64 additions: fixed by the bins and by where words (that is, feeds) were cut.
// The per-word steps are functions that also compile for the host: vdl2hip_debug_txlog_words runs them lane by lane (tests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "activity.h"

namespace vdl2 {

constexpr uint32_t kTxMaxPool = 1u << 22, kTxDefPool = 1u << 16;
constexpr uint32_t kTxPartial = 1u;      // VDL2HIP_TX_PARTIAL
constexpr int kTxMaxChan = 1024;         // (= kK5MaxChan: vdl2hip.hip asserts it)

// what a lane, and the state, hold of a transmission: busy bins, their float64 sum, the largest p and the lowest bin that has it
struct TxPart { double sum; uint64_t pbin; uint32_t cnt; float peak; };
// the log's own state per channel: the transmission under way as ActState has it, what the log has of it so far, and its flags
struct TxState { uint32_t open, idle; uint64_t first; TxPart acc; uint32_t flags, pad_; };
// the record as the device writes it: the first 64 bytes of vdl2hip_tx (vdl2hip.hip asserts size and offsets)
struct TxRec {
	uint32_t chan, freq; uint64_t first_bin, last_bin, peak_bin; int64_t first_sample, last_sample; uint32_t busy_bins, flags; float peak_power, mean_power;
};
struct TxHdr { uint32_t nrec, dropped; uint64_t pad_; };      // records written to the pool; records that found no room (16 bytes: the records behind it stay 16-byte aligned)
struct TxMasks { uint64_t starts, closes; };

struct TxArgs {
	const float *series; const uint32_t *freq;               // series: [C][S], the activity monitor's
	TxState *st; uint32_t *cnt; TxRec *rec; TxHdr *hdr;       // st, cnt: [C]
	int64_t k_on; uint64_t m0; float thr;
	uint32_t nb, H, B, S, smask, nchan, chan_first, pool;     // nb: bins the feed completed, from m0
};

__host__ __device__ __forceinline__ uint64_t txl_low(uint32_t r) { return r >= 64u ? ~0ull : (1ull << r) - 1ull; }     // bits 0 .. r - 1
__host__ __device__ __forceinline__ uint32_t txl_top(uint64_t v) { return 63u - (uint32_t)__builtin_clzll(v); }         // (v != 0)
__host__ __device__ __forceinline__ TxPart txl_none() { return TxPart{ 0.0, 0ull, 0u, -__builtin_inff() }; }
__host__ __device__ __forceinline__ TxPart txl_lane(bool busy, float p, uint64_t bin) { return busy ? TxPart{ (double)p, bin, 1u, p } : txl_none(); }
// lo: the part over the lower bins, hi: over the higher ones; of equal peaks the lower bin stays
__host__ __device__ __forceinline__ TxPart txl_combine(const TxPart &lo, const TxPart &hi) {
	const bool up = hi.peak > lo.peak;
	return TxPart{ lo.sum + hi.sum, up ? hi.pbin : lo.pbin, lo.cnt + hi.cnt, up ? hi.peak : lo.peak };
}
// The starts and the closes of one word of n <= 64 bins (bit i: bin base + i is busy; nothing set at or above n), with the state
// inherited from the bins before:
//   starts: act_scan_word's - busy bins with no busy bin among the H + 1 bins before them
//   after  = bins that have a busy bin among the H + 1 bins after them (busy >> 1 spread downwards by 0 .. H)
//   last   = busy & ~after: busy bins with no busy bin among the H + 1 bins after them, as far as the word shows.  Bin l of them
//            closes its transmission at bin l + H + 1 if that bin lies in the word - then the H + 1 bins were all in the word and
//            idle; if it does not, l is the word's highest busy bin and the transmission stays open
//   and the transmission that was open with `idle` idle bins behind it closes at bin H - idle of the word if no bin up to there is busy
__host__ __device__ __forceinline__ TxMasks txl_masks(uint64_t busy, uint32_t n, uint32_t H, uint32_t open, uint32_t idle) {
	uint64_t cov = busy, after = busy >> 1;
	for(uint32_t k = 0; k < H && k < 63u; ) { const uint32_t step = k + 1 < H - k ? k + 1 : H - k; cov |= cov << step; after |= after >> step; k += step; }
	const uint32_t r = open ? H - idle : 0u;
	if(open && r) cov |= txl_low(r);
	TxMasks w;
	w.starts = busy & ~((cov << 1) | (open ? 1ull : 0ull));
	w.closes = H + 1u < 64u ? (busy & ~after) << (H + 1u) : 0ull;
	if(open && r < n && !(busy & txl_low(r + 1u))) w.closes |= 1ull << r;
	w.closes &= txl_low(n);
	return w;
}
// level d (1, 2, 4 .. 32) of the segmented scan: does lane `lane` take in lane `lane - d`?  Only if no transmission starts in between
__host__ __device__ __forceinline__ bool txl_take(uint64_t starts, uint32_t lane, uint32_t d) { return lane >= d && ((starts >> (lane - d + 1u)) & txl_low(d)) == 0ull; }
// the record of the transmission that closes at bit q of the word (an idle bin); mine: lane q's value after the scan
__host__ __device__ __forceinline__ void txl_record(uint64_t busy, const TxMasks &w, uint32_t q, uint64_t base, const TxState &s, const TxPart &mine,
		uint32_t chan, uint32_t freq, int64_t k_on, uint32_t B, TxRec &r) {
	const uint64_t sb = w.starts & txl_low(q), bb = busy & txl_low(q);
	// (no start below q: it is the transmission the state carried in, and what the state has of it comes first)
	const TxPart t = sb ? mine : txl_combine(s.acc, mine);
	r.chan = chan; r.freq = freq;
	r.first_bin = sb ? base + txl_top(sb) : s.first;
	r.last_bin = bb ? base + txl_top(bb) : base - 1ull - s.idle;
	r.flags = sb ? 0u : s.flags;
	r.busy_bins = t.cnt;
	// (a transmission open when the log took effect that shows no busy bin afterwards: nothing of it was seen)
	r.peak_bin = t.cnt ? t.pbin : r.first_bin; r.peak_power = t.cnt ? t.peak : 0.f; r.mean_power = t.cnt ? (float)(t.sum / (double)t.cnt) : 0.f;
	r.first_sample = k_on + (int64_t)(r.first_bin * B); r.last_sample = k_on + (int64_t)((r.last_bin + 1ull) * B) - 1;
}
// the state behind the word; last: lane n - 1's value after the scan (the share of the word's last transmission)
__host__ __device__ __forceinline__ void txl_next(uint64_t busy, const TxMasks &w, uint32_t n, uint32_t H, uint64_t base, const TxPart &last, TxState &s) {
	if(busy) {
		const uint32_t idle = n - 1u - txl_top(busy);
		if(idle <= H) {
			if(w.starts) { s.first = base + txl_top(w.starts); s.flags = 0u; s.acc = last; }
			else s.acc = txl_combine(s.acc, last);
			s.open = 1u; s.idle = idle;
		} else s.open = 0u;
	} else if(s.open) { s.idle += n; if(s.idle > H) s.open = 0u; }
	if(!s.open) { s.idle = 0u; s.flags = 0u; s.acc = txl_none(); }
}

#ifdef __HIPCC__
// at enable: the log's state from the activity monitor's, a lane per channel - a transmission under way is taken over with nothing seen of it yet
__global__ __launch_bounds__(64) void k_txlog_init(const ActState *act, TxState *st, uint32_t nchan) {
	const uint32_t c = blockIdx.x * 64u + threadIdx.x;
	if(c >= nchan) return;
	const ActState a = act[c];
	TxState s;
	s.open = a.open; s.idle = a.open ? a.idle : 0u; s.first = a.first; s.acc = txl_none(); s.flags = a.open ? kTxPartial : 0u; s.pad_ = 0u;
	st[c] = s;
}

__global__ __launch_bounds__(64) void k_txlog_plan(const TxArgs a) {
	const uint32_t c = blockIdx.x, lane = threadIdx.x;
	TxState s = a.st[c];
	const float *sr = a.series + (size_t)c * a.S;
	uint32_t closes = 0;
	float pn = lane < a.nb ? sr[(uint32_t)((a.m0 + lane) & a.smask)] : 0.f;
	for(uint32_t w = 0; w < a.nb; w += 64) {                                // (uniform)
		const float pv = pn;
		const uint32_t n = a.nb - w < 64u ? a.nb - w : 64u;
		if(w + 64 + lane < a.nb) pn = sr[(uint32_t)((a.m0 + w + 64 + lane) & a.smask)];
		const uint64_t busy = __ballot(lane < n && pv > a.thr);
		const TxMasks m = txl_masks(busy, n, a.H, s.open, s.idle);
		closes += (uint32_t)__popcll(m.closes);
		txl_next(busy, m, n, a.H, a.m0 + w, txl_none(), s);                  // (only open and idle matter here)
	}
	if(lane == 0) a.cnt[c] = closes;
}

__global__ __launch_bounds__(64) void k_txlog_emit(const TxArgs a) {
	__shared__ uint32_t bb[kTxMaxChan + 1];
	const uint32_t c = blockIdx.x, lane = threadIdx.x, C = a.nchan;
	{
		uint32_t total = 0;
		for(uint32_t c0 = 0; c0 < C; c0 += 64) {
			const bool in = c0 + lane < C;
			const uint32_t v = in ? a.cnt[c0 + lane] : 0u;
			uint32_t inc = v;
			#pragma unroll
			for(int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if(lane >= (uint32_t)d) inc += o; }
			if(in) bb[c0 + lane] = total + inc - v;
			total += __shfl(inc, 63);
		}
		if(lane == 0) bb[C] = total;
	}
	__syncthreads();
	const uint32_t total = bb[C];
	if(c == 0 && lane == 0) { TxHdr h; h.nrec = total < a.pool ? total : a.pool; h.dropped = total - h.nrec; h.pad_ = 0; *a.hdr = h; }
	uint32_t at = bb[c];                                                   // where this channel's next record goes
	TxState s = a.st[c];
	const uint32_t chan = c + a.chan_first, freq = a.freq[c];
	const float *sr = a.series + (size_t)c * a.S;
	float pn = lane < a.nb ? sr[(uint32_t)((a.m0 + lane) & a.smask)] : 0.f;
	for(uint32_t w = 0; w < a.nb; w += 64) {                                // (uniform)
		const float pv = pn;
		const uint32_t n = a.nb - w < 64u ? a.nb - w : 64u;
		const uint64_t base = a.m0 + w;
		if(w + 64 + lane < a.nb) pn = sr[(uint32_t)((a.m0 + w + 64 + lane) & a.smask)];
		const bool isbusy = lane < n && pv > a.thr;
		const uint64_t busy = __ballot(isbusy);
		const TxMasks m = txl_masks(busy, n, a.H, s.open, s.idle);
		TxPart v = txl_lane(isbusy, pv, base + lane);
		if(busy) {                                                       // (an idle word adds nothing to anything)
			#pragma unroll
			for(uint32_t d = 1; d < 64; d <<= 1) {
				const TxPart o{ __shfl_up(v.sum, d), __shfl_up(v.pbin, d), __shfl_up(v.cnt, d), __shfl_up(v.peak, d) };
				if(txl_take(m.starts, lane, d)) v = txl_combine(o, v);
			}
		}
		if((m.closes >> lane) & 1ull) {
			const uint32_t i = at + (uint32_t)__popcll(m.closes & txl_low(lane));
			if(i < a.pool) { TxRec r; txl_record(busy, m, lane, base, s, v, chan, freq, a.k_on, a.B, r); a.rec[i] = r; }
		}
		at += (uint32_t)__popcll(m.closes);
		const TxPart last{ __shfl(v.sum, (int)n - 1), __shfl(v.pbin, (int)n - 1), __shfl(v.cnt, (int)n - 1), __shfl(v.peak, (int)n - 1) };
		txl_next(busy, m, n, a.H, base, last, s);
	}
	if(lane == 0) a.st[c] = s;
}
#endif  // __HIPCC__

}  // namespace vdl2
