// relook.h - the second look: for every transmission the transmission log closes, a decode attempt anchored on every preamble in it,
// whatever the walker's state was when it passed by.  Not in the reference, whose FSM evaluates the preamble metric only while it is
// idle.  Definition: vdl2hip.h, "Second look".  A pass behind the preamble search of the feed that closes the transmission: it reads
// the log's records, the search's plan (off[], TxsHdr) and y, and writes buffers of its own - no frame, counter or record of the
// receiver's main path, of the log or of the search.
//
// k_relook_anchors: 256 lanes, a workgroup per piece of the search's plan, grid-stride.  A piece n0 .. n0 + cnt - 1 of a record with
//   the range [sf, last] needs p(n) for lo = max(n0 - 160, sf) .. hi = min(n0 + cnt - 1 + 160, last): the phases of [lo - 150, hi] once
//   per sample into LDS (txs_phase_step) and the metric from them (txs_metric_step), as the search takes them - the same functions on
//   the same operands, so the same floats.  A lane then applies the local-minimum test (rl_is_anchor) to its samples of the piece from
//   LDS; two anchors lie at least 161 samples apart, so a piece has at most seven.  One lane sorts them by n, evaluates the metric once
//   more for their slopes and writes the piece's list.
// k_relook_select: one workgroup over the feed's records, 256 at a time, a lane per record.  The lane merges its pieces' anchors in
//   ascending order, keeps the best max_anchors under the total order (p ascending, n ascending), puts them back in ascending n and
//   plans each attempt (rl_plan_attempt): the --max-ppm gate, the nine header symbols sliced and decoded, the limit, and what the attempt
//   may need of the frame pool at the most - its claim.  An exclusive scan over the records (attempts, claimed records, claimed octets;
//   integers, carried from one round of 256 to the next) gives every attempt its place in the feed's list and every claim its place in
//   the pool: both depend on nothing but the records in their order.  An attempt whose claim does not fit is marked, not decoded.
// k_relook_decode: a wavefront per attempt, grid-stride, on BurstShared and FrameShared in dynamic LDS.  It counts the header's
//   outcome into the attempt's private counter row, builds the Burst the walker would have handed over had it locked at the anchor and
//   calls decode_burst() with the referee off on the attempt's claim as the wavefront's reserve (no atomics on a shared counter), then
//   finish_frame() on every frame that came out.
// The per-lane steps are functions that also compile for the host: vdl2hip_debug_relook_range runs them lane by lane (tests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vdl2_core.h"
#include "txlog.h"
#include "txsearch.h"

namespace vdl2 {

constexpr int kRlThreads = 256;
constexpr int kRlSep = 160;                                      // R: two preambles cannot lie closer (16 symbols of 10 samples)
constexpr int kRlPieceAnchors = 7;                               // anchors of one piece at the most
constexpr int kRlPhi = (int)kTxsPiece + 2 * kRlSep + 150;        // phases of a piece: [n0 - 160 - 150, n0 + 1023 + 160]
constexpr int kRlP = (int)kTxsPiece + 2 * kRlSep;                // metric values of a piece
constexpr uint32_t kRlMaxAnchors = 16, kRlDefAnchors = 4;
constexpr uint32_t kRlDefFrames = 4096, kRlMaxFrames = 1u << 20, kRlDefOctets = 1u << 20, kRlMaxOctets = 1u << 26;
constexpr uint32_t kRlMaxRecs = 1u << 15;                        // attempts of one feed at the most (what is beyond is counted as dropped)
constexpr uint32_t kRlPpmReject = 2u, kRlTruncated = 4u, kRlNoRoom = 8u;      // VDL2HIP_RELOOK_* (bit 0 is VDL2HIP_TX_PARTIAL, passed on)
constexpr uint32_t kRlNoHeader = 0xffu;                          // RlAtt::status of an attempt whose header was not read
static_assert(((int)kTxsPiece - 1) / (kRlSep + 1) + 1 == kRlPieceAnchors, "anchors are at least kRlSep + 1 samples apart");

struct RlAnchor { int64_t n; float p, s; };                      // 16 bytes
struct RlPiece { uint32_t n, pad_[3]; RlAnchor a[kRlPieceAnchors]; };      // 128 bytes: the anchors of a piece in ascending n
// the record as the device writes it; the layout is vdl2hip_relook's (vdl2hip.hip asserts size and offsets): the host copies it as it
// is, fills in frames_new and turns frame_first into an index of the read
struct RlRec {
	uint32_t chan, freq; uint64_t first_bin; int64_t anchor, end_sample; float pherr, slope, ppm_error, prev_phase;
	uint32_t tl_bits, nsym, synd_weight; int32_t stop; uint32_t frames, frames_ok, frames_new; int32_t fec_corrections;
	uint32_t frame_first, flags, reserved[2]; unsigned long long counters[kNumCounters];
};
// an attempt as it is planned: the anchor, the header's outcome and the claim
struct RlAtt { int64_t n, end_sample; float p, s, phi0, ppm; uint32_t flags, status, tl_bits, nsym, syndrome, negs, claim_f, claim_p; };
// what k_relook_decode needs beside the record: where the claim lies in the pool, the header's outcome
struct RlPlan { uint32_t off_f, claim_f, off_p, claim_p, status, syndrome, negs, pad_; };
// frames_used, octets_used: what the attempts produced, packed (k_relook_pack_plan): what the host copies
struct RlHdr { uint32_t nrec, ntx, anchors_found, dropped, frames_claimed, frames_used, octets_claimed, octets_used; };      // 32 bytes

struct RlArgs {
	const cf32 *y; const Tables *tab; const TxHdr *txhdr; const TxRec *txrec; const uint32_t *off; const TxsHdr *shdr;      // off, shdr: the search's plan of the same feed
	RlPiece *piece; RlRec *rec; RlPlan *plan; RlHdr *hdr; OutFrame *frames; uint8_t *pool; unsigned long long *acnt; const float *nfring;
	OutFrame *frames_out; uint8_t *pool_out;                          // what is delivered: the frames the attempts produced, without the unused parts of their claims
	float thr, max_ppm; uint32_t max_anchors, pool_frames, pool_octets, rec_cap, piece_cap, cap, mask, chan_first, back;      // back: (H + 1) B
};

// the metric values a piece needs: p(lo .. lo + E - 1)
__host__ __device__ __forceinline__ void rl_span(int64_t n0, uint32_t cnt, int64_t sf, int64_t last, int64_t &lo, uint32_t &E) {
	lo = n0 - kRlSep >= sf ? n0 - kRlSep : sf;
	const int64_t hi = n0 + (int64_t)cnt - 1 + kRlSep <= last ? n0 + (int64_t)cnt - 1 + kRlSep : last;
	E = (uint32_t)(hi - lo + 1);
}
// is element i of p[0 .. E) an anchor?  p[e] = p(lo + e), and [lo, lo + E) holds all of [n - R, n + R] that lies inside the range.
// (written so that a NaN neither is one nor beats one)
__host__ __device__ __forceinline__ bool rl_is_anchor(const float *p, uint32_t i, uint32_t E, float thr) {
	const float v = p[i];
	if(!(v < thr)) return false;
	const uint32_t b0 = i >= (uint32_t)kRlSep ? i - (uint32_t)kRlSep : 0u, e1 = i + (uint32_t)kRlSep < E ? i + (uint32_t)kRlSep : E - 1u;
	for(uint32_t m = b0; m < i; m++) if(p[m] <= v) return false;
	for(uint32_t m = i + 1u; m <= e1; m++) if(p[m] < v) return false;
	return true;
}
// the anchor at element i: the metric once more, for its slope (the same function on the same phases: the same p)
__host__ __device__ __forceinline__ RlAnchor rl_anchor_at(const float *phi, const Tables &T, int64_t lo, uint32_t i) {
	float ph[kPreamble], pv, sv;
	#pragma unroll
	for(int k = 0; k < kPreamble; k++) ph[k] = phi[i + 10u * (uint32_t)k];
	sync_metric(ph, T, pv, sv);
	return RlAnchor{ lo + (int64_t)i, pv, sv };
}
// c taken into the best nb <= K anchors, kept in (p ascending, n ascending) order
__host__ __device__ __forceinline__ void rl_keep(RlAnchor *best, uint32_t &nb, uint32_t K, const RlAnchor &c) {
	uint32_t j = nb;
	while(j > 0 && (c.p < best[j - 1].p || (c.p == best[j - 1].p && c.n < best[j - 1].n))) j--;
	if(j >= K) return;
	const uint32_t top = nb < K ? nb : K - 1u;
	for(uint32_t k = top; k > j; k--) best[k] = best[k - 1];
	best[j] = c;
	if(nb < K) nb++;
}
__host__ __device__ __forceinline__ void rl_sort_by_n(RlAnchor *best, uint32_t nb) {
	for(uint32_t i = 1; i < nb; i++) {
		const RlAnchor c = best[i];
		uint32_t j = i;
		while(j > 0 && best[j - 1].n > c.n) { best[j] = best[j - 1]; j--; }
		best[j] = c;
	}
}
// what an attempt with a header of tl_bits may need of the pool at the most.  A frame is at least one octet behind a flag of eight
// bits, and bit un-stuffing only removes bits: at most octets / 2 + 1 frames, their octets no more than the burst's, each frame's
// space rounded up to four.
__host__ __device__ __forceinline__ void rl_claim(uint32_t tl_bits, uint32_t &claim_f, uint32_t &claim_p) {
	const uint32_t octets = tl_bits / 8 + (tl_bits % 8 != 0);
	claim_f = octets / 2 + 1;
	claim_p = (octets + 3u * claim_f + 3u) & ~3u;
}
// The attempt at anchor c: the reference's DM_SYNC from a channel reset with prev_phi = Phi(c.n), dphi = s(c.n); symbol m at
// c.n + 10 (m + 1).  The gate, the header (decode.c:198-258 as the walker takes it), the limit, the claim.
__host__ __device__ __forceinline__ void rl_plan_attempt(const cf32 *yc, uint32_t mask, const Tables &T, uint32_t freq, float max_ppm, int64_t limit, const RlAnchor &c, RlAtt &o) {
	o.n = c.n; o.p = c.p; o.s = c.s; o.phi0 = phase_of(yc[(uint32_t)(c.n & (int64_t)mask)]); o.ppm = ppm_of(c.s, freq);
	o.flags = 0; o.status = kRlNoHeader; o.tl_bits = 0; o.nsym = 0; o.syndrome = 0; o.negs = 0; o.claim_f = 0; o.claim_p = 0;
	o.end_sample = c.n + 9 * kSpsDec;
	if(max_ppm != 0.f && fabsf(o.ppm) > max_ppm) { o.flags = kRlPpmReject; return; }
	if(o.end_sample > limit) { o.flags = kRlTruncated; return; }
	float prev = o.phi0;
	uint32_t hdr = 0; int negs = 0;
	for(int l = 0; l < 9; l++) {
		const float cur = phase_of(yc[(uint32_t)((c.n + (int64_t)(l + 1) * kSpsDec) & (int64_t)mask)]);
		const uint32_t sym = T.gray[slice_symbol(cur, prev, c.s, negs)];
		prev = cur;
		for(int k = 0; k < 3; k++) {
			const int b = 3 * l + k;
			if(b < kHdrBits) hdr |= (((sym >> (2 - k)) & 1u) ^ (uint32_t)T.prbs[b]) << (kHdrBits - 1 - b);
		}
	}
	const Geometry g = header_to_geometry(hdr, T.hdr_H, T.hdr_fix);
	o.status = (uint32_t)g.status; o.syndrome = g.syndrome; o.negs = (uint32_t)negs;
	if(g.status != HDR_OK) return;
	o.tl_bits = g.tl_bits; o.nsym = (g.want_bits + kHdrBits + 2) / 3;
	o.syndrome = g.syndrome | ((uint32_t)popc32(T.hdr_fix[g.syndrome]) << 8);
	o.end_sample = c.n + (int64_t)o.nsym * kSpsDec;
	if(o.end_sample > limit) { o.flags = kRlTruncated; return; }
	rl_claim(g.tl_bits, o.claim_f, o.claim_p);
}
// the record of an attempt before it is decoded, and its plan: off_f, off_p the exclusive sums of the claims before it
__host__ __device__ __forceinline__ void rl_record(uint32_t chan, uint32_t freq, uint64_t first_bin, uint32_t txflags, const RlAtt &t, uint32_t off_f, unsigned long long off_p,
		uint32_t pool_frames, uint32_t pool_octets, RlRec &r, RlPlan &pl) {
	r.chan = chan; r.freq = freq; r.first_bin = first_bin; r.anchor = t.n; r.end_sample = t.end_sample;
	r.pherr = t.p; r.slope = t.s; r.ppm_error = t.ppm; r.prev_phase = t.phi0;
	r.tl_bits = t.tl_bits; r.nsym = t.nsym; r.synd_weight = t.syndrome >> 8; r.stop = -1;
	r.frames = 0; r.frames_ok = 0; r.frames_new = 0; r.fec_corrections = -1; r.frame_first = 0; r.flags = t.flags | (txflags & kTxPartial);
	r.reserved[0] = r.reserved[1] = 0;
	for(int k = 0; k < kNumCounters; k++) r.counters[k] = 0;
	pl.off_f = off_f; pl.claim_f = t.claim_f; pl.off_p = (uint32_t)off_p; pl.claim_p = t.claim_p; pl.status = t.status; pl.syndrome = t.syndrome; pl.negs = t.negs; pl.pad_ = 0;
	if(t.claim_f && ((unsigned long long)off_f + t.claim_f > pool_frames || off_p + t.claim_p > pool_octets)) { r.flags |= kRlNoRoom; pl.claim_f = 0; pl.claim_p = 0; }
}
// the error counter that ended an attempt: the one of CNT_CRC_BAD .. CNT_ERR_UNSTUFF that is not 0 (-1: none)
__host__ __device__ __forceinline__ int32_t rl_stop(const unsigned long long *cnt) {
	for(int k = CNT_CRC_BAD; k <= CNT_ERR_UNSTUFF; k++) if(cnt[k]) return k;
	return -1;
}

// One attempt, by one wavefront (host: its phases one after the other): the header's outcome counted, the burst decoded into the
// attempt's claim, its frames finished.  r, pl: as rl_record left them; cnt: the attempt's counter row, zeroed (the kernel keeps it in
// LDS and copies it to the record); burst_shared_init() and frame_shared_init() first.
VDL2_HD __attribute__((always_inline)) void rl_decode(RlRec &r, const RlPlan &pl, int32_t chan_local, const cf32 *yc, uint32_t mask, const Tables &T,
		OutFrame *frames, uint8_t *pool, OutCtl *ctl, unsigned long long *cnt, unsigned long long *acnt, const float *nfring, BurstShared &sh, FrameShared &fs) {
	if(pl.status == kRlNoHeader || (r.flags & (kRlTruncated | kRlNoRoom))) return;
	LANE0
		if((pl.syndrome & 0xffu) == 0) VDL2_CNT_ADD(cnt, CNT_CRC_GOOD, 1);
		if(pl.status != HDR_OK) {
			VDL2_CNT_ADD(cnt, CNT_SLICER_NEG_IDX, pl.negs);
			VDL2_CNT_ADD(cnt, pl.status == HDR_CRC_BAD ? CNT_CRC_BAD : pl.status == HDR_TOO_LONG ? CNT_ERR_TOO_LONG : CNT_ERR_NO_FEC, 1);
		}
	LANE0_END
	if(pl.status == HDR_OK) {
		Burst b;
		b.chan = chan_local; b.nsym = (int32_t)r.nsym; b.t_first = r.anchor + kSpsDec; b.sync_sample = r.anchor; b.end_sample = r.end_sample; b.ord = -1;
		b.prev_phi0 = r.prev_phase; b.vdphi = r.slope; b.ppm = r.ppm_error; b.vdphi_err = 0.f; b.prev_n = r.anchor;
		b.tl_bits = r.tl_bits; b.syndrome = pl.syndrome; b.nf_upd = 0; b.sync_evals = 0;
		// the claim is the wavefront's reserve: decode_burst() hands out its records and octets without going to the shared counters
		LANE0
			sh.res_slot = pl.off_f; sh.res_nslot = pl.claim_f; sh.res_off = pl.off_p; sh.res_npool = pl.claim_p;
			sh.res_capf = pl.off_f + pl.claim_f; sh.res_capp = pl.off_p + pl.claim_p;
		LANE0_END
		ChanView v{ yc, nullptr, nullptr, mask };
		decode_burst(b, r.freq, T, v, cnt, frames, pool, ctl, sh);
		WAVE_SYNC_GLOBAL();                                           // (the records below were written by other lanes of this wavefront)
		const uint32_t nf = (uint32_t)cnt[CNT_MSG_GOOD] < pl.claim_f ? (uint32_t)cnt[CNT_MSG_GOOD] : pl.claim_f;
		uint32_t ok = 0; int32_t fec = -1;
		for(uint32_t k = 0; k < nf; k++) {
			OutFrame &f = frames[pl.off_f + k];
			finish_frame(f, pool, T, acnt, nfring, 0u, fs);
			WAVE_SYNC_GLOBAL();
			if(f.avlc_status == AVLC_OK) ok++;
			fec = f.num_fec_corrections;
		}
		LANE0
			for(uint32_t k = 0; k < nf; k++) frames[pl.off_f + k].nf_pwr_dbfs = __builtin_nanf("");
			r.frames = nf; r.frames_ok = ok; r.fec_corrections = fec; r.frame_first = pl.off_f;
		LANE0_END
	}
	LANE0
		r.stop = rl_stop(cnt);
	LANE0_END
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kRlThreads) void k_relook_anchors(const RlArgs a) {
	__shared__ float phi[kRlPhi];
	__shared__ float p[kRlP];
	__shared__ uint32_t s_n, s_idx[kRlPieceAnchors + 1];
	const uint32_t lane = threadIdx.x;
	const uint32_t nrec = a.shdr->nrec, total = a.shdr->npieces;
	const Tables &T = *a.tab;
	for(uint32_t g = blockIdx.x; g < total; g += gridDim.x) {               // (uniform)
		const uint32_t i = txs_find_rec(a.off, nrec, g);
		const TxRec r = a.txrec[i];
		int64_t sf; uint32_t fl;
		txs_range(r.first_sample, r.last_sample, sf, fl);
		const int64_t n0 = sf + (int64_t)(g - a.off[i]) * (int64_t)kTxsPiece, left = r.last_sample - n0 + 1;
		const uint32_t cnt = left < (int64_t)kTxsPiece ? (uint32_t)left : kTxsPiece;
		int64_t lo; uint32_t E;
		rl_span(n0, cnt, sf, r.last_sample, lo, E);
		const cf32 *yc = a.y + (size_t)(r.chan - a.chan_first) * a.cap;
		if(lane == 0) s_n = 0;
		// (the search's steps with the piece lo + 3 .. lo + E - 1: they stage the phases of [lo - 150, lo + E) and p(lo .. lo + E - 1))
		txs_phase_step(yc, a.mask, lo + kSyncSkip, E - (uint32_t)kSyncSkip, lane, kRlThreads, phi);
		__syncthreads();
		TxsPart unused = txs_none();
		txs_metric_step(phi, T, lo + kSyncSkip, E - (uint32_t)kSyncSkip, lane, kRlThreads, p, unused);
		__syncthreads();
		const uint32_t base = (uint32_t)(n0 - lo);
		for(uint32_t k = lane; k < cnt; k += kRlThreads)
			if(rl_is_anchor(p, base + k, E, a.thr)) { const uint32_t q = atomicAdd(&s_n, 1u); if(q < (uint32_t)kRlPieceAnchors) s_idx[q] = base + k; }
		__syncthreads();
		if(lane == 0) {
			const uint32_t n = s_n < (uint32_t)kRlPieceAnchors ? s_n : (uint32_t)kRlPieceAnchors;      // (never more: they are 161 samples apart)
			for(uint32_t x = 1; x < n; x++) { const uint32_t c = s_idx[x]; uint32_t j = x; while(j > 0 && s_idx[j - 1] > c) { s_idx[j] = s_idx[j - 1]; j--; } s_idx[j] = c; }
			RlPiece &o = a.piece[g];
			o.n = n; o.pad_[0] = o.pad_[1] = o.pad_[2] = 0;
			for(uint32_t x = 0; x < n; x++) o.a[x] = rl_anchor_at(phi, T, lo, s_idx[x]);
		}
		__syncthreads();                                                // (phi, p and the list are written again by the next piece)
	}
}

__global__ __launch_bounds__(kRlThreads) void k_relook_select(const RlArgs a) {
	__shared__ uint32_t s_att[kRlThreads], s_fr[kRlThreads];
	__shared__ unsigned long long s_oc[kRlThreads];
	__shared__ uint32_t s_found, s_dropped;
	const uint32_t t = threadIdx.x;
	const uint32_t nrec = a.shdr->nrec;
	const Tables &T = *a.tab;
	if(t == 0) { s_found = 0; s_dropped = 0; }
	__syncthreads();
	uint32_t c_att = 0, c_fr = 0; unsigned long long c_oc = 0;
	for(uint32_t w = 0; w < nrec; w += kRlThreads) {                      // (uniform)
		const uint32_t i = w + t;
		RlAtt att[kRlMaxAnchors];
		uint32_t nb = 0, v_fr = 0; unsigned long long v_oc = 0;
		TxRec r{};
		if(i < nrec) {
			r = a.txrec[i];
			RlAnchor best[kRlMaxAnchors];
			uint32_t found = 0;
			const uint32_t g0 = a.off[i], g1 = a.off[i + 1];
			for(uint32_t g = g0; g < g1 && g < a.piece_cap; g++) {          // (g < piece_cap: always - txsearch_piece_cap())
				const uint32_t n = a.piece[g].n < (uint32_t)kRlPieceAnchors ? a.piece[g].n : (uint32_t)kRlPieceAnchors;
				for(uint32_t x = 0; x < n; x++) { rl_keep(best, nb, a.max_anchors, a.piece[g].a[x]); found++; }
			}
			rl_sort_by_n(best, nb);
			const cf32 *yc = a.y + (size_t)(r.chan - a.chan_first) * a.cap;
			const int64_t limit = r.last_sample + (int64_t)a.back;
			for(uint32_t k = 0; k < nb; k++) { rl_plan_attempt(yc, a.mask, T, r.freq, a.max_ppm, limit, best[k], att[k]); v_fr += att[k].claim_f; v_oc += att[k].claim_p; }
			if(found) atomicAdd(&s_found, found);
		}
		// exclusive sums over the round's 256 records, through LDS (integers: the result does not depend on the order)
		s_att[t] = nb; s_fr[t] = v_fr; s_oc[t] = v_oc;
		__syncthreads();
		for(uint32_t d = 1; d < (uint32_t)kRlThreads; d <<= 1) {
			const uint32_t x0 = t >= d ? s_att[t - d] : 0u, x1 = t >= d ? s_fr[t - d] : 0u; const unsigned long long x2 = t >= d ? s_oc[t - d] : 0ull;
			__syncthreads();
			s_att[t] += x0; s_fr[t] += x1; s_oc[t] += x2;
			__syncthreads();
		}
		uint32_t o_att = c_att + s_att[t] - nb, o_fr = c_fr + s_fr[t] - v_fr; unsigned long long o_oc = c_oc + s_oc[t] - v_oc;
		c_att += s_att[kRlThreads - 1]; c_fr += s_fr[kRlThreads - 1]; c_oc += s_oc[kRlThreads - 1];
		uint32_t lost = 0;
		for(uint32_t k = 0; k < nb; k++) {
			if(o_att < a.rec_cap) rl_record(r.chan, r.freq, r.first_bin, r.flags, att[k], o_fr, o_oc, a.pool_frames, a.pool_octets, a.rec[o_att], a.plan[o_att]);
			else lost++;
			o_att++; o_fr += att[k].claim_f; o_oc += att[k].claim_p;
		}
		if(lost) atomicAdd(&s_dropped, lost);
		__syncthreads();                                                // (the sums are written again by the next round)
	}
	__syncthreads();
	if(t == 0) {
		RlHdr h;
		h.nrec = c_att < a.rec_cap ? c_att : a.rec_cap; h.ntx = nrec; h.anchors_found = s_found; h.dropped = s_dropped;
		h.frames_claimed = c_fr < a.pool_frames ? c_fr : a.pool_frames; h.frames_used = 0; h.octets_claimed = (uint32_t)(c_oc < a.pool_octets ? c_oc : a.pool_octets); h.octets_used = 0;
		*a.hdr = h;
	}
}

__global__ __launch_bounds__(64) void k_relook_decode(const RlArgs a) {
	extern __shared__ __align__(16) unsigned char rl_lds[];           // a BurstShared, then a FrameShared
	BurstShared &sh = *reinterpret_cast<BurstShared *>(rl_lds);
	FrameShared &fs = *reinterpret_cast<FrameShared *>(rl_lds + ((sizeof(BurstShared) + 15) & ~(size_t)15));
	__shared__ OutCtl ctl;                                            // the attempt's own: capacity 0 - a record beyond the claim is refused, not written
	__shared__ unsigned long long cnt[kNumCounters];                  // the attempt's counter row
	const uint32_t n = a.hdr->nrec;
	if(blockIdx.x >= n) return;
	const Tables &T = *a.tab;
	if(threadIdx.x == 0) { ctl = OutCtl{}; ctl.nframes = 0xf0000000u; ctl.pool_used = 0xf0000000u; }
	burst_shared_init(T, 0u, &ctl, sh, true);
	frame_shared_init(T, fs);
	for(uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
		RlRec &r = a.rec[i];
		const RlPlan pl = a.plan[i];
		WAVE_FOR(l)
			if(l < kNumCounters) cnt[l] = 0;
		WAVE_END
		rl_decode(r, pl, (int32_t)(r.chan - a.chan_first), a.y + (size_t)(r.chan - a.chan_first) * a.cap, a.mask, T, a.frames, a.pool, &ctl, cnt,
		          a.acnt + (size_t)blockIdx.x * kNumAvlcCounters, a.nfring, sh, fs);
		WAVE_FOR(l)
			if(l < kNumCounters) r.counters[l] = cnt[l];
		WAVE_END
	}
}

// What the host copies is what the attempts produced, not what they claimed (a claim is the worst case of a header's length).
// k_relook_pack_plan: one workgroup, a lane per attempt, 256 a round: the attempt's frames and the octets they take (each frame's
//   rounded up to four), an exclusive scan over the attempts in their order (integers, carried from round to round): the attempt's
//   place among the delivered frames goes to its record's frame_first, its octets' place to reserved[0] (the host clears it).
// k_relook_pack_copy: a wavefront per attempt, grid-stride: records and octets to their places.
__global__ __launch_bounds__(kRlThreads) void k_relook_pack_plan(const RlArgs a) {
	__shared__ uint32_t s_fr[kRlThreads], s_oc[kRlThreads];
	const uint32_t t = threadIdx.x, n = a.hdr->nrec;
	uint32_t c_fr = 0, c_oc = 0;
	for(uint32_t w = 0; w < n; w += kRlThreads) {                         // (uniform)
		const uint32_t i = w + t;
		uint32_t v_fr = 0, v_oc = 0;
		if(i < n) {
			v_fr = a.rec[i].frames;
			const uint32_t off = a.plan[i].off_f;
			for(uint32_t k = 0; k < v_fr; k++) v_oc += (a.frames[off + k].len + 3u) & ~3u;
		}
		s_fr[t] = v_fr; s_oc[t] = v_oc;
		__syncthreads();
		for(uint32_t d = 1; d < (uint32_t)kRlThreads; d <<= 1) {
			const uint32_t x0 = t >= d ? s_fr[t - d] : 0u, x1 = t >= d ? s_oc[t - d] : 0u;
			__syncthreads();
			s_fr[t] += x0; s_oc[t] += x1;
			__syncthreads();
		}
		if(i < n) { a.rec[i].frame_first = v_fr ? c_fr + s_fr[t] - v_fr : 0u; a.rec[i].reserved[0] = c_oc + s_oc[t] - v_oc; }
		c_fr += s_fr[kRlThreads - 1]; c_oc += s_oc[kRlThreads - 1];
		__syncthreads();                                                // (the sums are written again by the next round)
	}
	if(t == 0) { a.hdr->frames_used = c_fr; a.hdr->octets_used = c_oc; }      // (no more than was claimed: within the pools)
}
__global__ __launch_bounds__(64) void k_relook_pack_copy(const RlArgs a) {
	const uint32_t n = a.hdr->nrec, lane = threadIdx.x;
	for(uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
		const uint32_t nf = a.rec[i].frames, src = a.plan[i].off_f, dst = a.rec[i].frame_first;
		uint32_t at = a.rec[i].reserved[0];
		for(uint32_t k = 0; k < nf; k++) {
			OutFrame f = a.frames[src + k];
			const uint32_t from = f.pool_off, len = f.len;
			for(uint32_t j = lane; j < len; j += 64u) a.pool_out[at + j] = a.pool[from + j];
			f.pool_off = at;
			if(lane == 0) a.frames_out[dst + k] = f;
			at += (len + 3u) & ~3u;
		}
	}
}
#endif  // __HIPCC__

}  // namespace vdl2
