// txsearch.h - the preamble search: for every transmission the transmission log closes, the reference's own sync metric at every
// decimated sample of it - the best match, where it was, the frequency error it implies, and whether the reference's 3-sample
// evaluation grid could have locked on it.  Not in the reference.  Definition: vdl2hip.h, "Preamble search".  A read-only pass behind
// k_frame_finish of the feed that closes the transmission (the burst capture's placement): it reads the log's records of the feed
// and y, writes buffers of its own, and touches nothing the decoder, the activity monitor or the log read or write.
//
// k_txsearch_plan: one workgroup over the feed's records, 256 at a time.  Each lane works out the range of one record (txs_range) and
// its number of pieces of kTxsPiece samples; an inclusive scan - per wavefront by __shfl_up, the four wavefronts' totals through LDS -
// carried from one round of 256 to the next, gives every record the offset of its pieces among the feed's: off[i], off[nrec] the total.
//
// k_txsearch_piece: 256 lanes, a workgroup per piece, grid-stride over the feed's pieces.  A piece's record is found by a search in
// off[].  The piece n0 .. n0 + cnt - 1:
//   phases: Phi(n) = phase_of(y[n]) - the reference's double-precision atan2, narrowed - ONCE per sample of [n0 - 153, n0 + cnt) into
//     LDS, lane l taking samples l, l + 256, ...: some 1 180 evaluations a piece where the 16 taps of every window would have asked
//     for 16 a sample.
//   metric: sync_metric() for n0 - 3 .. n0 + cnt - 1, element e = n - (n0 - 3) by lane e mod 256, its taps phi[e + 10 i]: consecutive
//     lanes read consecutive words.  p goes to LDS; a lane keeps the best of its own samples (float32 <, ascending n: the lowest n
//     of the smallest p), its slope and its count below the threshold in registers.
//   lock test: n is a lock point iff n - 3 >= search_first and is_candidate(p(n - 3), p(n)).
//   the 256 partial results are combined by a fixed tree through LDS - lane i takes in lane i + 128, then i + 64, ... i + 1.
//     Every field is a minimum under a total order, an integer sum or an OR: the result does not depend on the tree.
// k_txsearch_reduce: a lane per record combines the record's pieces in ascending order and writes the record.
// The per-piece steps are functions that also compile for the host: vdl2hip_debug_txsearch_range runs them lane by lane (tests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vdl2_core.h"
#include "txlog.h"

namespace vdl2 {

constexpr int kTxsThreads = 256;
constexpr uint32_t kTxsPiece = 1024;                 // samples of a piece
constexpr int64_t kTxsSpan = 57344;                  // the longest range: 56 pieces, more than the longest burst (56 090 samples)
constexpr uint32_t kTxsMaxBack = 4096;               // (hang_bins + 1) * bin_samples at the most: how far a record's last sample lies behind the feed that closes it
constexpr int kTxsLead = 150 + kSyncSkip;            // samples ahead of a piece whose phases it needs: the taps of p(n0 - 3)
constexpr int kTxsPhi = (int)kTxsPiece + kTxsLead;   // phases of a piece: [n0 - 153, n0 + 1023]
constexpr int kTxsP = (int)kTxsPiece + kSyncSkip;    // metric values of a piece: n0 - 3 .. n0 + 1023
constexpr uint32_t kTxsClipped = 2u;                 // VDL2HIP_TXS_CLIPPED (bit 0 is VDL2HIP_TX_PARTIAL, passed on)
static_assert(kTxsSpan % kTxsPiece == 0 && kPreamble == 16 && kSpsDec == 10, "a window is 16 taps, 10 samples apart");

// the record as the device writes it; the layout is vdl2hip_tx_search's (vdl2hip.hip asserts size and offsets): the host copies it
// as it is and fills in frames, frames_ok and why
struct TxsRec {
	uint32_t chan, freq; uint64_t first_bin; int64_t search_first, search_last, best_sample, first_lock; float best_pherr, best_slope, best_ppm;
	uint32_t lock_points, below_thr, lock_phases, flags, frames, frames_ok, why, reserved, reserved2;
};
// what a lane, a piece and a record hold: the smallest p with the lowest n that has it (n = -1, p = +inf: none) and its slope, the
// samples below the threshold, the lock points, the lowest of them (INT64_MAX: none) and the phases they fall on
struct TxsPart { int64_t n, first_lock; float p, s; uint32_t below, locks, phases, pad_; };
struct TxsHdr { uint32_t nrec, npieces; uint64_t pad_; };      // records and pieces of the feed (16 bytes: the records behind it stay 16-byte aligned)

struct TxsArgs {
	const cf32 *y; const Tables *tab; const TxHdr *txhdr; const TxRec *txrec;      // txhdr, txrec: the log's, of the same feed
	uint32_t *off; TxsPart *part; TxsRec *rec; TxsHdr *hdr;                        // off: [pool + 1], part: [piece_cap]
	uint32_t pool, piece_cap, cap, mask, chan_first;
};

// the range of a record: [max(first, last - (kTxsSpan - 1)), last]
__host__ __device__ __forceinline__ void txs_range(int64_t first, int64_t last, int64_t &sfirst, uint32_t &flags) {
	const int64_t lo = last - (kTxsSpan - 1);
	sfirst = first >= lo ? first : lo; flags = first >= lo ? 0u : kTxsClipped;
}
__host__ __device__ __forceinline__ uint32_t txs_pieces(int64_t sfirst, int64_t slast) { return slast >= sfirst ? (uint32_t)((slast - sfirst + (int64_t)kTxsPiece) / (int64_t)kTxsPiece) : 0u; }
__host__ __device__ __forceinline__ TxsPart txs_none() { return TxsPart{ -1, INT64_MAX, __builtin_inff(), 0.f, 0u, 0u, 0u, 0u }; }
// record i with off[i] <= g < off[i + 1] (off: exclusive offsets of the records' piece counts, off[nrec] the total; g below it)
__host__ __device__ __forceinline__ uint32_t txs_find_rec(const uint32_t *off, uint32_t nrec, uint32_t g) {
	uint32_t lo = 0, hi = nrec;
	while(hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if(off[mid] <= g) lo = mid; else hi = mid; }
	return lo;
}
// one lane's share of the phases of a piece: phi[j] = Phi(n0 - kTxsLead + j), j < cnt + kTxsLead; the ring index is masked per element
__host__ __device__ __forceinline__ void txs_phase_step(const cf32 *yc, uint32_t mask, int64_t n0, uint32_t cnt, uint32_t lane, uint32_t nl, float *phi) {
	for(uint32_t j = lane; j < cnt + (uint32_t)kTxsLead; j += nl) {
		const int64_t n = n0 - kTxsLead + (int64_t)j;
		phi[j] = n < 0 ? 0.f : phase_of(yc[(uint32_t)(n & (int64_t)mask)]);
	}
}
// one lane's share of the metric: p[e] = p(n0 - 3 + e), e < cnt + 3, in ascending e; what it finds in the piece itself (e >= 3) goes to `mine`
__host__ __device__ __forceinline__ void txs_metric_step(const float *phi, const Tables &T, int64_t n0, uint32_t cnt, uint32_t lane, uint32_t nl, float *p, TxsPart &mine) {
	for(uint32_t e = lane; e < cnt + (uint32_t)kSyncSkip; e += nl) {
		float ph[kPreamble], pv, sv;
		#pragma unroll
		for(int i = 0; i < kPreamble; i++) ph[i] = phi[e + 10u * (uint32_t)i];
		sync_metric(ph, T, pv, sv);
		p[e] = pv;
		if(e >= (uint32_t)kSyncSkip) {
			if(pv < mine.p) { mine.p = pv; mine.s = sv; mine.n = n0 + (int64_t)(e - (uint32_t)kSyncSkip); }
			mine.below += pv < kSyncThr ? 1u : 0u;
		}
	}
}
// one lane's share of the lock test (p complete: a barrier before it)
__host__ __device__ __forceinline__ void txs_lock_step(const float *p, int64_t n0, uint32_t cnt, int64_t sfirst, uint32_t lane, uint32_t nl, TxsPart &mine) {
	for(uint32_t i = lane; i < cnt; i += nl) {
		const int64_t n = n0 + (int64_t)i;
		if(n - kSyncSkip >= sfirst && is_candidate(p[i], p[i + (uint32_t)kSyncSkip])) {
			mine.locks++; mine.phases |= 1u << (uint32_t)(n % 3);
			if(n < mine.first_lock) mine.first_lock = n;
		}
	}
}
// b taken into a: of equal p the lower n stays (two parts without a best have p = +inf and n = -1 both)
__host__ __device__ __forceinline__ void txs_combine(TxsPart &a, const TxsPart &b) {
	if(b.p < a.p || (b.p == a.p && b.n < a.n)) { a.p = b.p; a.s = b.s; a.n = b.n; }
	a.below += b.below; a.locks += b.locks; a.phases |= b.phases;
	if(b.first_lock < a.first_lock) a.first_lock = b.first_lock;
}
// the tree's level s (128, 64, ... 1) as lane `lane` takes it; a barrier between two levels
__host__ __device__ __forceinline__ void txs_tree_step(TxsPart *part, uint32_t lane, uint32_t s) { if(lane < s) txs_combine(part[lane], part[lane + s]); }
// the record of a transmission from its combined pieces
__host__ __device__ __forceinline__ void txs_record(uint32_t chan, uint32_t freq, uint64_t first_bin, uint32_t txflags, int64_t sfirst, int64_t slast, uint32_t flags, const TxsPart &t, TxsRec &r) {
	r.chan = chan; r.freq = freq; r.first_bin = first_bin; r.search_first = sfirst; r.search_last = slast;
	r.best_sample = t.n; r.first_lock = t.locks ? t.first_lock : -1;
	r.best_pherr = t.p; r.best_slope = t.n >= 0 ? t.s : 0.f; r.best_ppm = t.n >= 0 ? ppm_of(t.s, freq) : 0.f;
	r.lock_points = t.locks; r.below_thr = t.below; r.lock_phases = t.phases; r.flags = flags | (txflags & kTxPartial);
	r.frames = 0; r.frames_ok = 0; r.why = 0; r.reserved = 0; r.reserved2 = 0;
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kTxsThreads) void k_txsearch_plan(const TxsArgs a) {
	__shared__ uint32_t wsum[kTxsThreads / 64];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t nlog = a.txhdr->nrec, nrec = nlog < a.pool ? nlog : a.pool;
	uint32_t carry = 0;
	for(uint32_t w = 0; w < nrec; w += kTxsThreads) {                      // (uniform)
		const uint32_t i = w + t;
		uint32_t v = 0;
		if(i < nrec) { const TxRec r = a.txrec[i]; int64_t sf; uint32_t fl; txs_range(r.first_sample, r.last_sample, sf, fl); v = txs_pieces(sf, r.last_sample); }
		uint32_t inc = v;
		#pragma unroll
		for(int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if(lane >= (uint32_t)d) inc += o; }
		if(lane == 63) wsum[wave] = inc;
		__syncthreads();
		uint32_t before = 0, total = 0;
		#pragma unroll
		for(uint32_t k = 0; k < (uint32_t)kTxsThreads / 64; k++) { const uint32_t s = wsum[k]; if(k < wave) before += s; total += s; }
		if(i < nrec) a.off[i] = carry + before + inc - v;
		carry += total;
		__syncthreads();                                                // (wsum is written again by the next round)
	}
	if(t == 0) { a.off[nrec] = carry; TxsHdr h; h.nrec = nrec; h.npieces = carry < a.piece_cap ? carry : a.piece_cap; h.pad_ = 0; *a.hdr = h; }
}

__global__ __launch_bounds__(kTxsThreads) void k_txsearch_piece(const TxsArgs a) {
	__shared__ float phi[kTxsPhi];
	__shared__ float p[kTxsP];
	__shared__ TxsPart part[kTxsThreads];
	const uint32_t lane = threadIdx.x;
	const uint32_t nrec = a.hdr->nrec, total = a.hdr->npieces;
	const Tables &T = *a.tab;
	for(uint32_t g = blockIdx.x; g < total; g += gridDim.x) {               // (uniform)
		const uint32_t i = txs_find_rec(a.off, nrec, g);
		const TxRec r = a.txrec[i];
		int64_t sf; uint32_t fl;
		txs_range(r.first_sample, r.last_sample, sf, fl);
		const int64_t n0 = sf + (int64_t)(g - a.off[i]) * (int64_t)kTxsPiece, left = r.last_sample - n0 + 1;
		const uint32_t cnt = left < (int64_t)kTxsPiece ? (uint32_t)left : kTxsPiece;
		const cf32 *yc = a.y + (size_t)(r.chan - a.chan_first) * a.cap;
		txs_phase_step(yc, a.mask, n0, cnt, lane, kTxsThreads, phi);
		__syncthreads();
		TxsPart mine = txs_none();
		txs_metric_step(phi, T, n0, cnt, lane, kTxsThreads, p, mine);
		__syncthreads();
		txs_lock_step(p, n0, cnt, sf, lane, kTxsThreads, mine);
		part[lane] = mine;
		__syncthreads();
		#pragma unroll
		for(uint32_t s = kTxsThreads / 2; s >= 1; s >>= 1) { txs_tree_step(part, lane, s); __syncthreads(); }
		if(lane == 0) a.part[g] = part[0];
		__syncthreads();                                                // (phi, p and part are written again by the next piece)
	}
}

__global__ __launch_bounds__(64) void k_txsearch_reduce(const TxsArgs a) {
	const uint32_t nrec = a.hdr->nrec;
	for(uint32_t i = blockIdx.x * 64u + threadIdx.x; i < nrec; i += gridDim.x * 64u) {
		const TxRec r = a.txrec[i];
		int64_t sf; uint32_t fl;
		txs_range(r.first_sample, r.last_sample, sf, fl);
		TxsPart t = txs_none();
		const uint32_t g0 = a.off[i], g1 = a.off[i + 1];
		for(uint32_t g = g0; g < g1 && g < a.piece_cap; g++) txs_combine(t, a.part[g]);      // (g < piece_cap: always - txsearch_piece_cap())
		TxsRec o;
		txs_record(r.chan, r.freq, r.first_bin, r.flags, sf, r.last_sample, fl, t, o);
		a.rec[i] = o;
	}
}
#endif  // __HIPCC__

}  // namespace vdl2
