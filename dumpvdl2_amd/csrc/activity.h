// activity.h - the channel activity monitor: a power envelope of every channel's decimated stream in fixed time bins, and from it
// busy / idle decisions, transmission counts, a level histogram and a short per-channel series.  Not in the reference.
// Definition (vdl2hip.h, "Activity monitor"): with t = k - k_on the position in the stream since the monitor was enabled, bin m
// covers t = m B .. (m + 1) B - 1 and p[m] = (1 / B) sum (re^2 + im^2) of y over it, in float32.
//
// k_activity_power: a workgroup takes a run of consecutive bins of one channel (grid: bin runs x channels, so a shard of few
// channels still fills the chip).  It goes through the samples of its bins in chunks of kActChunk: every lane loads 16 bytes (two
// samples) at a time, lane i the pair i, i + 256, ... of the chunk - coalesced whatever B is - and stores re^2 + im^2 to LDS (a
// word of padding per 16, so that the strided reads below spread over the banks).  A chunk starts where a bin starts in this
// feed (or a whole number of chunks further into a bin longer than a chunk) and holds whole bins from there.  The sum of a bin's
// samples IN THIS FEED is taken in an order that depends on the bin and on where the feed begins and ends, and on nothing else:
//   16 samples in sequence -> a sub-block;  16 sub-blocks in sequence -> a group (256 samples);  the groups in sequence,
// all counted from the bin's first sample in this feed; what does not exist counts as +0, which changes no sum.  The bin the feed
// starts in begins from the channel's carried float32 partial sum; what the feed leaves of an incomplete bin - the last "bin" of
// the last workgroup's run - becomes the new carry (two buffers, alternating: a workgroup reads one and another writes the other).
// No atomics, no dependence on the grid.  The monitor never reads y outside the feed's own samples: a 16-byte pair that would
// reach over either end is read as one sample.
//
// k_activity_scan: one wavefront per channel over the bins the feed completed, 64 at a time.  The 64 busy flags are one ballot
// mask; where transmissions begin, how long they are and what state the next word (and feed) inherits come from bit operations
// on it (below).  The histogram is counted in LDS and added to the channel's 64 counters at the end; sum_power is the words'
// sums in order, each a butterfly over the 64 lanes in float64 - the same tree on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace vdl2 {

constexpr int kActThreads = 256;
constexpr int kActChunk = 2048;          // samples staged at a time: 16 KiB of y, four 16-byte loads per lane
constexpr int kActSub = 16;              // samples per sub-block, sub-blocks per group
constexpr int kActBuckets = 64;
constexpr uint32_t kActMinBin = 10, kActMaxBin = 10500, kActMaxHang = 255, kActMaxSeries = 1u << 20;
// a chunk holds at most 1 + (kActChunk - 1) / kActMinBin bins, and sub-blocks: (len + 15 per bin) / 16
constexpr int kActMaxSegs = 1 + (kActChunk - 1) / (int)kActMinBin;                 // 205 <= kActThreads: a lane per bin at the last level
constexpr int kActMaxSubs = (kActChunk + 15 * kActMaxSegs) / kActSub + 1;
static_assert(kActMaxSegs <= kActThreads, "one lane per bin of a chunk");

// what the scan keeps per channel; the layout is vdl2hip_activity_chan's (vdl2hip.hip asserts the size): the host copies it as it is
struct ActChan {
	uint64_t bins, busy_bins, transmissions, longest_bins; double sum_power; float max_power, min_power; uint32_t open, reserved; uint64_t hist[kActBuckets];
};
// ... and what a reset leaves alone: the transmission under way (open: the idle bins since its last busy one are <= H), its first bin
struct ActState { uint32_t open, idle; uint64_t first; };

struct ActArgs {
	const float2 *y;           // [C][cap]: the decimated ring
	float *series;             // [C][S]: p[m] at m & (S - 1)
	const float *carry_in;     // [C]: the float32 sum of what earlier feeds held of the bin this feed starts in
	float *carry_out;          // [C]: the same for the next feed
	int64_t k0;                // the feed's first decimated sample
	uint64_t m0;               // the bin it starts in
	int32_t off;               // where that bin begins relative to the feed's first sample: -(B - 1) .. 0
	uint32_t D, B, nbt, run;   // the feed's samples; bins it touches, the incomplete last one included (= completed + 1); bins per workgroup
	uint32_t cap, mask, S, smask;
};
struct ActScanArgs {
	const float *series; ActChan *acc; ActState *st; const float *edges;       // edges: [63]
	float thr; uint64_t m0; uint32_t nb, H, S, smask;                          // nb: bins the feed completed, from m0
};

// bucket(p) = #{ i : E[i] <= p } for ascending E[0 .. 62], E[63] = +inf: a binary search that never reads past E[63]
__host__ __device__ __forceinline__ uint32_t act_bucket(const float *E, float p) {
	uint32_t n = 0;
	for(uint32_t s = 32; s >= 1; s >>= 1) if(E[n + s - 1] <= p) n += s;
	return n;
}
// The transmissions of one word of n <= 64 bins (bit i: bin base + i is busy; nothing set at or above n), with the state inherited
// from the bins before:
//   cov    = bins that are busy or have a busy bin at most H bins before them (the busy mask spread upwards by 0 .. H, and the low
//            H - idle bits if a transmission is open): a bin after which a transmission is still under way
//   starts = busy & ~(cov << 1 | open): busy bins with no busy bin among the H + 1 bins before them - transmissions begin there
// Between two starts lies one transmission; its last busy bin is the highest busy bit below the next start.
__host__ __device__ __forceinline__ void act_scan_word(uint64_t busy, uint32_t n, uint32_t H, uint64_t base, ActState &s, uint64_t &tx, uint64_t &longest) {
	uint64_t cov = busy;
	for(uint32_t k = 0; k < H && k < 63u; ) { const uint32_t step = k + 1 < H - k ? k + 1 : H - k; cov |= cov << step; k += step; }
	if(s.open) { const uint32_t r = H - s.idle; if(r) cov |= r >= 64u ? ~0ull : (1ull << r) - 1ull; }
	uint64_t starts = busy & ~((cov << 1) | (s.open ? 1ull : 0ull));
	tx += (uint64_t)__builtin_popcountll(starts);
	if(busy) {
		const uint64_t head = busy & (starts ? (starts & (0ull - starts)) - 1ull : ~0ull);            // busy bins of the transmission that was open
		if(head) { const uint64_t len = base + (63u - (uint32_t)__builtin_clzll(head)) - s.first + 1; longest = len > longest ? len : longest; }
		uint64_t first = s.first;
		while(starts) {
			const uint32_t b = (uint32_t)__builtin_ctzll(starts);
			starts &= starts - 1ull;
			const uint64_t seg = busy & (starts ? (starts & (0ull - starts)) - 1ull : ~0ull) & ~((1ull << b) - 1ull);
			const uint64_t len = (63u - (uint32_t)__builtin_clzll(seg)) - b + 1u;
			longest = len > longest ? len : longest;
			first = base + b;
		}
		const uint32_t after = n - 1u - (63u - (uint32_t)__builtin_clzll(busy));
		if(after <= H) { s.open = 1u; s.idle = after; s.first = first; } else s.open = 0u;
	} else if(s.open) { s.idle += n; if(s.idle > H) s.open = 0u; }
}
__host__ __device__ __forceinline__ uint32_t act_pad(uint32_t i) { return i + (i >> 4); }

__host__ __device__ __forceinline__ float act_pow(float2 v) { return __builtin_fmaf(v.x, v.x, v.y * v.y); }

// One chunk of a workgroup's run: it starts at sample `pos` of the feed inside bin j (`fresh`: at the bin's first sample in this
// feed) and holds len samples in nseg pieces - len0 of bin j, then whole bins of B (the incomplete last bin: what the feed has of it).
// fin0: bin j ends in this chunk.  Sub-blocks and groups are numbered piece after piece: nsb0 / ngr0 of the first, nsbB / ngrB of each other.
struct ActPlan {
	int64_t pos, kabs; uint32_t j, len0, nseg, len, o, nsb0, nsb, ngr0, ngr, nsbB, ngrB; bool fin0, fresh;
};
constexpr int kActLdsP = kActChunk + 2 + (kActChunk + 2) / 16 + 1, kActLdsG = kActMaxSegs + kActChunk / (kActSub * kActSub) + 1;
__host__ __device__ __forceinline__ ActPlan act_plan(const ActArgs &a, uint32_t j, uint32_t jend, int64_t pos, bool fresh) {
	ActPlan k{};
	const uint32_t B = a.B;
	int64_t e = (int64_t)(j + 1) * B + a.off; if(j == a.nbt - 1 || e > (int64_t)a.D) e = a.D;
	const int64_t rem = e - pos;
	k.pos = pos; k.j = j; k.fresh = fresh; k.fin0 = rem <= kActChunk;
	if(!k.fin0) { k.len0 = k.len = kActChunk; k.nseg = 1; }
	else {
		k.len0 = (uint32_t)rem;
		uint32_t extra = ((uint32_t)kActChunk - k.len0) / B; if(extra > jend - j - 1) extra = jend - j - 1;
		k.nseg = 1 + extra;
		int64_t lend = pos + k.len0 + (int64_t)extra * B; if(lend > (int64_t)a.D) lend = a.D;      // (the incomplete bin ends with the feed)
		k.len = (uint32_t)(lend - pos);
	}
	k.kabs = a.k0 + pos; k.o = (uint32_t)(k.kabs & 1);
	k.nsbB = (B + kActSub - 1) / kActSub; k.ngrB = (k.nsbB + kActSub - 1) / kActSub;
	k.nsb0 = (k.len0 + kActSub - 1) / kActSub; k.nsb = k.nsb0 + (k.nseg - 1) * k.nsbB;
	k.ngr0 = (k.nsb0 + kActSub - 1) / kActSub; k.ngr = k.ngr0 + (k.nseg - 1) * k.ngrB;
	return k;
}
// The four steps of a chunk as one lane of the workgroup takes them, a barrier between each two (the host build runs them lane by
// lane: vdl2hip_debug_activity_power, the tests' model of the order of additions).
// PHASE 0: stage re^2 + im^2 of [pos, pos + len): p[pad(o + i)] is sample pos + i
// PHASE 1: sub-blocks - 16 samples in sequence, counted from each bin's first sample in the chunk
// PHASE 2: groups - 16 sub-blocks in sequence
// PHASE 3: a lane per bin of the chunk - the groups in sequence, on top of what the bin has so far (acc: lane 0's, of a bin longer than a chunk)
template<int PHASE>
__host__ __device__ __forceinline__ void act_step(const ActArgs &a, const ActPlan &k, uint32_t c, uint32_t lane, float *p, float *sb, float *gr, float &acc) {
	const uint32_t B = a.B, o = k.o;
	if(PHASE == 0) {
		const float2 *yc = a.y + (size_t)c * a.cap;
		const int64_t kb = k.kabs - o;
		const uint32_t lo2 = o, hi2 = (o + k.len) >> 1;                    // pairs lo2 .. hi2 - 1 lie inside whole
		for(uint32_t q0 = 0; q0 < hi2; q0 += 4 * kActThreads) {
			float4 v[4];
			#pragma unroll
			for(int u = 0; u < 4; u++) {
				const uint32_t q = q0 + (uint32_t)u * kActThreads + lane;
				v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
				if(q >= lo2 && q < hi2) v[u] = *(const float4 *)(yc + (uint32_t)((kb + 2 * (int64_t)q) & a.mask));
			}
			#pragma unroll
			for(int u = 0; u < 4; u++) {
				const uint32_t q = q0 + (uint32_t)u * kActThreads + lane;
				if(q >= lo2 && q < hi2) { p[act_pad(2 * q)] = act_pow(make_float2(v[u].x, v[u].y)); p[act_pad(2 * q + 1)] = act_pow(make_float2(v[u].z, v[u].w)); }
			}
		}
		if(k.len) {
			if(lane == 0 && o) p[act_pad(1)] = act_pow(yc[(uint32_t)(k.kabs & a.mask)]);                       // the first sample is the odd half of a pair
			if(lane == 64 && ((o + k.len) & 1)) p[act_pad(o + k.len - 1)] = act_pow(yc[(uint32_t)((k.kabs + k.len - 1) & a.mask)]);   // the last one the even half
		}
	}
	if(PHASE == 1) {
		for(uint32_t i = lane; i < k.nsb; i += kActThreads) {
			uint32_t sub = i, s0 = 0, L = k.len0;
			if(i >= k.nsb0) { const uint32_t t = i - k.nsb0, seg1 = t / k.nsbB; sub = t - seg1 * k.nsbB; s0 = k.len0 + seg1 * B; L = k.len - s0 < B ? k.len - s0 : B; }
			const uint32_t first = kActSub * sub, n = L > first ? L - first : 0, base = o + s0 + first;
			float s = 0.f;
			#pragma unroll
			for(uint32_t t = 0; t < (uint32_t)kActSub; t++) s += t < n ? p[act_pad(base + t)] : 0.f;
			sb[i] = s;
		}
	}
	if(PHASE == 2) {
		for(uint32_t g = lane; g < k.ngr; g += kActThreads) {
			uint32_t grp = g, sbase = 0, ns = k.nsb0;
			if(g >= k.ngr0) { const uint32_t t = g - k.ngr0, seg1 = t / k.ngrB; grp = t - seg1 * k.ngrB; sbase = k.nsb0 + seg1 * k.nsbB; ns = k.nsbB; }
			const uint32_t first = kActSub * grp, n = ns > first ? ns - first : 0;
			float s = 0.f;
			#pragma unroll
			for(uint32_t t = 0; t < (uint32_t)kActSub; t++) s += t < n ? sb[sbase + first + t] : 0.f;
			gr[g] = s;
		}
	}
	if(PHASE == 3) {
		if(lane < k.nseg) {
			const uint32_t gbase = lane ? k.ngr0 + (lane - 1) * k.ngrB : 0, n = lane ? k.ngrB : k.ngr0;
			float v = 0.f;
			if(lane == 0) v = !k.fresh ? acc : k.j == 0 ? a.carry_in[c] : 0.f;
			for(uint32_t t = 0; t < n; t++) v += gr[gbase + t];
			if(lane == 0 && !k.fin0) acc = v;
			else {
				const uint32_t jj = k.j + lane;
				if(jj == a.nbt - 1) a.carry_out[c] = v;
				else a.series[(size_t)c * a.S + (uint32_t)((a.m0 + jj) & a.smask)] = v / (float)B;
			}
		}
	}
}
// where the run of workgroup bx begins: its first bin (counted from m0; nbt - 1 is the incomplete one) and that bin's first sample in the feed
__host__ __device__ __forceinline__ int64_t act_run_start(const ActArgs &a, uint32_t j) { const int64_t pos = (int64_t)j * a.B + a.off; return pos < 0 ? 0 : pos; }

#ifdef __HIPCC__
__global__ __launch_bounds__(kActThreads) void k_activity_power(const ActArgs a) {
	__shared__ float p[kActLdsP];
	__shared__ float sb[kActMaxSubs];
	__shared__ float gr[kActLdsG];
	const uint32_t c = blockIdx.y, lane = threadIdx.x;
	uint32_t j = blockIdx.x * a.run;
	const uint32_t jend = j + a.run < a.nbt ? j + a.run : a.nbt;
	if(j >= jend) return;
	int64_t pos = act_run_start(a, j);
	bool fresh = true;
	float acc = 0.f;
	while(j < jend) {                                                      // (everything that steers this loop is uniform)
		const ActPlan k = act_plan(a, j, jend, pos, fresh);
		act_step<0>(a, k, c, lane, p, sb, gr, acc);
		__syncthreads();
		act_step<1>(a, k, c, lane, p, sb, gr, acc);
		__syncthreads();
		act_step<2>(a, k, c, lane, p, sb, gr, acc);
		__syncthreads();
		act_step<3>(a, k, c, lane, p, sb, gr, acc);
		// (the next chunk's stores to p, sb and gr come behind barriers every lane passes only after these reads)
		if(!k.fin0) { pos += kActChunk; fresh = false; }
		else { j += k.nseg; pos += k.len; fresh = true; }
	}
}

// One wavefront per channel over the bins a feed completed (act_scan_word: what a word of 64 of them does to the transmissions)
__global__ __launch_bounds__(64) void k_activity_scan(const ActScanArgs a) {
	__shared__ float E[kActBuckets];
	__shared__ uint32_t hcnt[kActBuckets];
	const uint32_t c = blockIdx.x, lane = threadIdx.x, H = a.H;
	E[lane] = lane < (uint32_t)kActBuckets - 1 ? a.edges[lane] : __builtin_inff();
	hcnt[lane] = 0;
	__syncthreads();
	ActChan *ac = a.acc + c;
	ActState s = a.st[c];
	uint64_t bins = ac->bins, busy_bins = ac->busy_bins, tx = ac->transmissions, longest = ac->longest_bins;
	double sum = ac->sum_power; float mx = ac->max_power, mn = ac->min_power;
	const float *sr = a.series + (size_t)c * a.S;
	float pn = lane < a.nb ? sr[(uint32_t)((a.m0 + lane) & a.smask)] : 0.f;
	for(uint32_t w = 0; w < a.nb; w += 64) {
		const float pv = pn;
		const uint32_t n = a.nb - w < 64u ? a.nb - w : 64u;
		const bool valid = lane < n;
		if(w + 64 + lane < a.nb) pn = sr[(uint32_t)((a.m0 + w + 64 + lane) & a.smask)];      // the next word's, while this one is worked on
		const uint64_t busy = __ballot(valid && pv > a.thr);
		if(valid) atomicAdd(&hcnt[act_bucket(E, pv)], 1u);
		double d = valid ? (double)pv : 0.0;
		float hi = valid ? pv : 0.f, lo = valid ? pv : __builtin_inff();
		#pragma unroll
		for(int x = 32; x >= 1; x >>= 1) { d += __shfl_xor(d, x); hi = __builtin_fmaxf(hi, __shfl_xor(hi, x)); lo = __builtin_fminf(lo, __shfl_xor(lo, x)); }
		sum += d;
		mx = bins ? __builtin_fmaxf(mx, hi) : hi; mn = bins ? __builtin_fminf(mn, lo) : lo;
		bins += n; busy_bins += (uint64_t)__popcll(busy);
		act_scan_word(busy, n, H, a.m0 + w, s, tx, longest);               // (the same in every lane)
	}
	if(lane == 0) {
		ac->bins = bins; ac->busy_bins = busy_bins; ac->transmissions = tx; ac->longest_bins = longest;
		ac->sum_power = sum; ac->max_power = mx; ac->min_power = mn;
		a.st[c] = s;
	}
	__syncthreads();
	if(hcnt[lane]) ac->hist[lane] += hcnt[lane];
}
#endif  // __HIPCC__

}  // namespace vdl2
