// capture.h - the burst capture: for every burst the walker has handed to the burst decoder, a window of the channel's decimated
// stream around it and a phase-error quality record computed from the same samples.  Not in the reference.
// Definition: vdl2hip.h, "Burst capture".  A read-only pass behind k_frame_finish of the feed that decodes the burst: it reads the
// feed's burst lists and y, writes buffers of its own, and touches nothing the decoder reads or writes.
//
// k_capture_plan: one wavefront per channel over the channel's burst list.  64 bursts at a time, each lane works out the clipped
// window of one burst (cap_window); an inclusive scan over the wavefront, carried from one round of 64 to the next, gives every
// burst the offset of its window among the channel's windows; the channel's total goes to tot[c].
//
// k_capture_copy: 256 lanes, a workgroup per burst, grid-stride over the feed's bursts in record order (channel, position in the
// channel's list).  Every workgroup turns the channels' burst counts and window totals into offsets in LDS (burst_body()'s idiom: a
// load per lane and 64 channels, a scan), finds a burst's channel by a search there, and so knows the burst's place in the pool
// without a third kernel or an atomic.  A window that ends beyond pool_samples is not copied (VDL2HIP_BURST_NO_ROOM); offsets only
// grow, so every burst behind it is refused too and the pairs in use are those up to the last burst that fitted.
//   copy: the destination decides the shape - a single pair first where the burst's place in the pool is odd, then 16-byte stores,
//     fed by one 16-byte load where the ring index is even too and by two 8-byte loads where it is not, then a single pair if one is
//     left.  The ring index is masked per element: a 16-byte load starts at an even index and the ring's length is even.
//   quality: a lane takes a run of consecutive symbols, so that phase_of() of a symbol also serves as the next symbol's previous
//     phase (decode_burst step 1); its sums are float64, in symbol order; the 256 partial results are combined by a fixed tree
//     through LDS - lane i takes in lane i + 128, then i + 64, ... i + 1 - the same on every launch.
// The per-burst steps are functions that also compile for the host: vdl2hip_debug_capture_* run them lane by lane (tests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vdl2_core.h"

namespace vdl2 {

constexpr int kCapThreads = 256;
constexpr uint32_t kCapMaxPre = 4096, kCapMaxPost = 1024, kCapMaxPool = 1u << 24, kCapDefPool = 1u << 20;
constexpr uint32_t kCapNoRoom = 1u;      // VDL2HIP_BURST_NO_ROOM
constexpr int kCapMaxChan = 1024;        // (= kK5MaxChan: vdl2hip.hip asserts it)

// the record as the device writes it; the layout is vdl2hip_burst's (vdl2hip.hip asserts size and offsets): the host copies it as it
// is and fills in frames, frames_ok and fec_corrections
struct CapRec {
	uint32_t chan, freq; int64_t burst_ord, sync_sample, end_sample, first_symbol; uint32_t nsym, tl_bits; float ppm_error, dphi, prev_phase; uint32_t flags;
	int64_t iq_first; uint32_t iq_count, reserved; uint64_t iq_off; uint32_t frames, frames_ok; int32_t fec_corrections; uint32_t weak_symbols;
	float mean_power, min_power, max_power, phase_err_rms, phase_err_mean, phase_err_max;
};
struct CapPlan { uint64_t off; int64_t first; uint32_t count, pad_; };     // a burst's window, and where it begins among its channel's windows
struct CapHdr { uint32_t nrec, pad_; uint64_t pairs; };                  // records of the feed; pairs of the pool in use
struct CapPart { double se, se2, sp; float emax, pmin, pmax; uint32_t weak; };

struct CapArgs {
	const cf32 *y; const Burst *bursts; const uint32_t *nb_chan; const uint32_t *freq;
	CapPlan *plan; uint64_t *tot; CapRec *rec; cf32 *pool; CapHdr *hdr;
	int64_t k_end; uint64_t pool_samples; uint32_t cap_bursts_chan, nchan, chan_first, cap, mask, pre, post;
};

// the clipped window of a burst: iq_first = max(0, sync - pre), iq_last = min(end + post, k_end - 1)
__host__ __device__ __forceinline__ void cap_window(const Burst &b, uint32_t pre, uint32_t post, int64_t k_end, int64_t &first, uint32_t &count) {
	first = b.sync_sample - (int64_t)pre; if(first < 0) first = 0;
	int64_t last = b.end_sample + (int64_t)post; if(last > k_end - 1) last = k_end - 1;
	count = last >= first ? (uint32_t)(last - first + 1) : 0u;
}
// channel c with bb[c] <= g < bb[c + 1] (bb: exclusive offsets of the channels' burst counts, bb[nchan] the total)
__host__ __device__ __forceinline__ int cap_find_chan(const uint32_t *bb, int nchan, uint32_t g) {
	int lo = 0, hi = nchan;
	while(hi - lo > 1) { const int mid = (lo + hi) >> 1; if(bb[mid] <= g) lo = mid; else hi = mid; }
	return lo;
}
// burst g (channel c, position i) fits and its window ends at pair `end`: is it the last one that fits?  Offsets only grow, so it is
// if there is no next burst or the next one's window ends beyond the pool - that workgroup says how much of the pool is in use
__host__ __device__ __forceinline__ bool cap_is_last_fit(const uint32_t *bbn, int nchan, const CapPlan *plan, uint32_t cap_bursts_chan, uint32_t g, int c, uint32_t i,
		uint64_t end, uint64_t pool_samples, uint32_t total) {
	if(g + 1 >= total) return true;
	const int c2 = i + 1 < bbn[c + 1] - bbn[c] ? c : cap_find_chan(bbn, nchan, g + 1);
	return end + plan[(size_t)c2 * cap_bursts_chan + (g + 1 - bbn[c2])].count > pool_samples;
}
// one lane's share of the copy of y[first .. first + count) to dst[0 .. count), dst being pair `off` of a 16-byte aligned pool
__host__ __device__ __forceinline__ void cap_copy(const cf32 *yc, uint32_t mask, int64_t first, uint32_t count, cf32 *dst, uint64_t off, uint32_t lane, uint32_t nl) {
	if(!count) return;
	const uint32_t head = (uint32_t)(off & 1u), npair = (count - head) >> 1;
	if(lane == 0 && head) dst[0] = yc[(uint32_t)(first & (int64_t)mask)];
	for(uint32_t q = lane; q < npair; q += nl) {
		const uint32_t i = head + 2 * q, s = (uint32_t)((first + (int64_t)i) & (int64_t)mask);
		float4 v;
		if(!(s & 1u)) v = *(const float4 *)(yc + s);
		else { const cf32 a0 = yc[s], a1 = yc[(s + 1u) & mask]; v = make_float4(a0.re, a0.im, a1.re, a1.im); }
		*(float4 *)(dst + i) = v;
	}
	if(lane == nl - 1 && ((count - head) & 1u)) dst[count - 1] = yc[(uint32_t)((first + (int64_t)count - 1) & (int64_t)mask)];
}
// what slice_symbol() rounds (vdl2_core.h, demod.c:256-263): the phase step less the burst's slope, wrapped, in units of pi / 4
__host__ __device__ __forceinline__ float cap_slice_arg(float phi, float prev_phi, float vdphi) {
	float dphi = phi - prev_phi - vdphi;
	if(dphi < 0) dphi = (float)((double)dphi + 2.0f * M_PI);
	else if((double)dphi > 2.0f * M_PI) dphi = (float)((double)dphi - 2.0f * M_PI);
	return (float)((double)dphi / M_PI_4);
}
// one lane's run of symbols: m0 = lane * ceil(nsym / nl) .. in order
__host__ __device__ __forceinline__ CapPart cap_quality_run(const cf32 *yc, uint32_t mask, const Burst &b, uint32_t lane, uint32_t nl) {
	CapPart q{ 0.0, 0.0, 0.0, 0.f, __builtin_inff(), 0.f, 0u };
	const int64_t nsym = b.nsym > 0 ? b.nsym : 0, per = (nsym + nl - 1) / nl, m0 = (int64_t)lane * per, m1 = m0 + per < nsym ? m0 + per : nsym;
	if(m0 >= nsym) return q;
	float prev = m0 ? phase_of(yc[(uint32_t)((b.t_first + (m0 - 1) * kSpsDec) & (int64_t)mask)]) : b.prev_phi0;
	for(int64_t m = m0; m < m1; m++) {
		const cf32 v = yc[(uint32_t)((b.t_first + m * kSpsDec) & (int64_t)mask)];
		const float cur = phase_of(v), u = cap_slice_arg(cur, prev, b.vdphi), e = u - roundf(u), ae = fabsf(e);
		const float p = v.re * v.re + v.im * v.im;
		q.se += (double)e; q.se2 += (double)e * (double)e; q.sp += (double)p;
		q.emax = ae > q.emax ? ae : q.emax; q.pmin = p < q.pmin ? p : q.pmin; q.pmax = p > q.pmax ? p : q.pmax;
		q.weak += ae > 0.25f ? 1u : 0u;
		prev = cur;
	}
	return q;
}
__host__ __device__ __forceinline__ void cap_combine(CapPart &a, const CapPart &b) {
	a.se += b.se; a.se2 += b.se2; a.sp += b.sp; a.weak += b.weak;
	a.emax = b.emax > a.emax ? b.emax : a.emax; a.pmin = b.pmin < a.pmin ? b.pmin : a.pmin; a.pmax = b.pmax > a.pmax ? b.pmax : a.pmax;
}
// the tree's level s (128, 64, ... 1) as lane `lane` takes it; a barrier between two levels
__host__ __device__ __forceinline__ void cap_tree_step(CapPart *part, uint32_t lane, uint32_t s) { if(lane < s) cap_combine(part[lane], part[lane + s]); }
// the record of a burst from the combined sums
__host__ __device__ __forceinline__ void cap_record(const Burst &b, uint32_t chan, uint32_t freq, const CapPlan &p, uint64_t off, bool fits, const CapPart &q, CapRec &r) {
	r.chan = chan; r.freq = freq; r.burst_ord = b.ord; r.sync_sample = b.sync_sample; r.end_sample = b.end_sample; r.first_symbol = b.t_first;
	r.nsym = (uint32_t)b.nsym; r.tl_bits = b.tl_bits; r.ppm_error = b.ppm; r.dphi = b.vdphi; r.prev_phase = b.prev_phi0; r.flags = fits ? 0u : kCapNoRoom;
	r.iq_first = p.first; r.iq_count = fits ? p.count : 0u; r.reserved = 0; r.iq_off = fits ? off : 0u;
	r.frames = 0; r.frames_ok = 0; r.fec_corrections = -1; r.weak_symbols = q.weak;
	const double n = b.nsym > 0 ? (double)b.nsym : 1.0;
	r.mean_power = (float)(q.sp / n); r.min_power = b.nsym > 0 ? q.pmin : 0.f; r.max_power = q.pmax;
	r.phase_err_rms = (float)(sqrt(q.se2 / n) * M_PI_4); r.phase_err_mean = (float)((q.se / n) * M_PI_4); r.phase_err_max = (float)((double)q.emax * M_PI_4);
}

#ifdef __HIPCC__
__global__ __launch_bounds__(64) void k_capture_plan(const CapArgs a) {
	const uint32_t c = blockIdx.x, lane = threadIdx.x;
	const uint32_t nbc = a.nb_chan[c], nb = nbc < a.cap_bursts_chan ? nbc : a.cap_bursts_chan;
	const Burst *bl = a.bursts + (size_t)c * a.cap_bursts_chan;
	CapPlan *pl = a.plan + (size_t)c * a.cap_bursts_chan;
	uint64_t carry = 0;
	for(uint32_t w = 0; w < nb; w += 64) {                                // (uniform)
		const uint32_t i = w + lane;
		int64_t first = 0; uint32_t cnt = 0;
		if(i < nb) cap_window(bl[i], a.pre, a.post, a.k_end, first, cnt);
		uint32_t inc = cnt;                                             // (64 windows of < 2^16 pairs)
		#pragma unroll
		for(int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if(lane >= (uint32_t)d) inc += o; }
		if(i < nb) pl[i] = CapPlan{ carry + inc - cnt, first, cnt, 0u };
		carry += __shfl(inc, 63);
	}
	if(lane == 0) { a.tot[c] = carry; if(c == 0) { a.hdr->nrec = 0; a.hdr->pad_ = 0; a.hdr->pairs = 0; } }
}

__global__ __launch_bounds__(kCapThreads) void k_capture_copy(const CapArgs a) {
	__shared__ uint32_t bbn[kCapMaxChan + 1];
	__shared__ uint64_t bbo[kCapMaxChan + 1];
	__shared__ CapPart part[kCapThreads];
	const uint32_t lane = threadIdx.x, C = a.nchan;
	if(lane < 64) {
		uint32_t total = 0; uint64_t ototal = 0;
		for(uint32_t c0 = 0; c0 < C; c0 += 64) {
			const bool in = c0 + lane < C;
			const uint32_t nbc = in ? a.nb_chan[c0 + lane] : 0u, v = nbc < a.cap_bursts_chan ? nbc : a.cap_bursts_chan;
			const uint64_t t = in ? a.tot[c0 + lane] : 0ull;
			uint32_t inc = v; uint64_t oinc = t;
			#pragma unroll
			for(int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); const uint64_t oo = __shfl_up(oinc, d); if(lane >= (uint32_t)d) { inc += o; oinc += oo; } }
			if(in) { bbn[c0 + lane] = total + inc - v; bbo[c0 + lane] = ototal + oinc - t; }
			total += __shfl(inc, 63); ototal += __shfl(oinc, 63);
		}
		if(lane == 0) { bbn[C] = total; bbo[C] = ototal; }
	}
	__syncthreads();
	const uint32_t total = bbn[C];
	if(blockIdx.x == 0 && lane == 0) a.hdr->nrec = total;
	for(uint32_t g = blockIdx.x; g < total; g += gridDim.x) {             // (uniform)
		const int c = cap_find_chan(bbn, (int)C, g);
		const uint32_t i = g - bbn[c];
		const size_t at = (size_t)c * a.cap_bursts_chan + i;
		const Burst b = a.bursts[at];
		const CapPlan p = a.plan[at];
		const uint64_t off = bbo[c] + p.off;
		const bool fits = off + p.count <= a.pool_samples;
		const cf32 *yc = a.y + (size_t)c * a.cap;
		if(fits) cap_copy(yc, a.mask, p.first, p.count, a.pool + off, off, lane, kCapThreads);
		part[lane] = cap_quality_run(yc, a.mask, b, lane, kCapThreads);
		__syncthreads();
		#pragma unroll
		for(uint32_t s = kCapThreads / 2; s >= 1; s >>= 1) { cap_tree_step(part, lane, s); __syncthreads(); }
		if(lane == 0) {
			cap_record(b, (uint32_t)c + a.chan_first, a.freq[c], p, off, fits, part[0], a.rec[g]);
			if(fits && cap_is_last_fit(bbn, (int)C, a.plan, a.cap_bursts_chan, g, c, i, off + p.count, a.pool_samples, total)) a.hdr->pairs = off + p.count;
		}
		__syncthreads();                                                // (part is written again by the next burst)
	}
}
#endif  // __HIPCC__

}  // namespace vdl2
