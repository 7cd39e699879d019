// resample.h - K0: the rational resampler in front of the channeliser (a receiver created with vdl2hip_cfg.input_rate).
//
// One wideband stream, not one per channel: a block of the caller's IQ (any format, any supported rate) becomes a block of complex
// float32 at 105000 * oversample, which the rest of the receiver takes as a VDL2HIP_FMT_CF32 block.  Definition (vdl2hip.h):
//   r[n] = sum_{j < T} h[j L + p_n] x[b_n - j],   p_n = (n M) mod L,   b_n = floor(n M / L),   x[i < 0] = 0
// in float32, real and imaginary part each one chain of T fused multiply-adds, j = 0 first - whatever the feed, the workgroup or
// the lane an output falls to, so the stream is a function of the input stream alone.
//
// Mapping: one lane per output, 256 outputs per tile, kResTiles tiles per workgroup.  The input a tile needs (its outputs' span of
// ~256 M / L samples plus the T - 1 before it) is converted once and staged in LDS as float2; a lane then reads T consecutive staged
// samples downwards.  The samples before the block come from the tail the feed before left (the last T - 1 samples of the stream, as
// floats: converted once, and independent of the format), workgroup 0 writes the next feed's.
//
// The tap table is kept in WALK order: ht[j L + q] = h[j L + (q M) mod L], so that output n reads column q = n mod L - the lanes of a
// wavefront, consecutive outputs, read consecutive words of row j (ds_read_b32 banks on address mod 32 words per half-wavefront:
// no conflict, except for the few lanes behind a wrap of q where L is no multiple of 32; lanes L apart share an address, which
// broadcasts) whatever M is.  In prototype order the 32 phases of a half-wavefront would be 32 arbitrary columns of a row.
// The table sits in LDS while it is small beside the tile (kResTapsLds bytes); the large ones (525 phases x 29 taps) are read through
// the cache, with consecutive lanes on consecutive words as well.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "rawfmt.h"

namespace vdl2 {

constexpr int kResTile = 256;            // outputs per tile = lanes per workgroup
constexpr int kResTiles = 4;             // tiles per workgroup: the taps are loaded and the position is divided out once per workgroup
constexpr uint32_t kResTapsLds = 24576;  // bytes of tap table that go to LDS (beside a tile of at most (255 * 8 + 1 + 224 + 1) * 8 = 18 128 bytes)

struct K0Args {
	const void *in;            // the block: nin samples in the caller's format
	const float2 *tail_in;     // x[N0 - (T - 1) .. N0 - 1] (N0: the stream index of in[0]); zeros before the stream
	float2 *tail_out;          // the same for the next feed (the other of two buffers)
	const float *taps;         // L * T, walk order
	float2 *out;               // r[n0 .. n0 + nout)
	uint64_t q0;               // n0 mod L
	uint64_t t0;               // (n0 M) mod L + L (b_{n0} - N0): the position of output n0 relative to the block, in units of 1 / L input samples
	uint32_t nin, nout, L, M, T, span_cap;
};

// sample `rel` of the stream relative to the block's first: the tail before it, the block (the format's conversion: rawfmt.h),
// nothing after it
template<int FMT>
__device__ __forceinline__ float2 res_sample(const K0Args &a, int64_t rel) {
	if(rel < 0) return rel >= -(int64_t)(a.T - 1) ? a.tail_in[rel + (int64_t)(a.T - 1)] : make_float2(0.f, 0.f);
	if(rel >= (int64_t)a.nin) return make_float2(0.f, 0.f);
	return RawFmt<FMT>::level(((const typename RawFmt<FMT>::word *)a.in)[rel]);
}

template<int FMT, bool TAPS_LDS>
__global__ __launch_bounds__(kResTile) void k_resample(const K0Args a) {
	extern __shared__ float2 res_lds[];
	float2 *xs = res_lds;                                      // [span_cap]
	float *ht = (float *)(res_lds + a.span_cap);               // [L * T] (TAPS_LDS)
	const uint32_t lane = threadIdx.x, L = a.L, M = a.M, T = a.T;
	if(TAPS_LDS) for(uint32_t i = lane; i < L * T; i += kResTile) ht[i] = a.taps[i];
	// the workgroup's first output: its position in 1 / L input samples, divided out once (64-bit); what follows stays within 32 bits
	// (a tile moves on by 256 M <= 2^21, a lane by at most 255 M)
	const uint64_t iw = (uint64_t)blockIdx.x * (uint64_t)(kResTile * kResTiles);
	const uint64_t tw = a.t0 + iw * (uint64_t)M;
	const int64_t bw = (int64_t)(tw / L);
	const uint32_t pw = (uint32_t)(tw % L), qw = (uint32_t)((a.q0 + iw) % L);
	for(int k = 0; k < kResTiles; k++) {
		const uint64_t i0 = iw + (uint64_t)k * kResTile;
		if(i0 >= a.nout) break;                                // (uniform)
		const uint32_t nv = (uint32_t)(a.nout - i0 < (uint64_t)kResTile ? a.nout - i0 : (uint64_t)kResTile);
		const uint32_t tt = pw + (uint32_t)k * (uint32_t)kResTile * M;
		const int64_t bt = bw + (int64_t)(tt / L);             // b of the tile's first output, relative to the block
		const uint32_t pt = tt % L;
		const int64_t lo = bt - (int64_t)(T - 1);              // first sample the tile reads
		uint32_t span = (pt + (nv - 1) * M) / L + T;           // ... and how many: up to its last output's b
		if(span > a.span_cap) span = a.span_cap;               // (never: span_cap is this expression's maximum)
		__syncthreads();                                       // the tile before has been read; the taps are in place
		for(uint32_t i = lane; i < span; i += kResTile) xs[i] = res_sample<FMT>(a, lo + (int64_t)i);
		__syncthreads();
		if(lane < nv) {
			const uint32_t tl = pt + lane * M;
			uint32_t xi = tl / L + (T - 1);                    // this output's b in the tile: it reads xs[xi], xs[xi - 1], ... xs[xi - (T - 1)]
			if(xi >= span) xi = span - 1;                      // (never)
			const uint32_t q = (qw + (uint32_t)k * kResTile + lane) % L;
			const float *hq = (TAPS_LDS ? (const float *)ht : a.taps) + q;
			const float2 *xp = xs + xi;
			float ar = 0.f, ai = 0.f;
			#pragma unroll 4
			for(uint32_t j = 0; j < T; j++) {
				const float h = hq[j * L];
				const float2 x = xp[-(int)j];
				ar = __builtin_fmaf(h, x.x, ar);
				ai = __builtin_fmaf(h, x.y, ai);
			}
			a.out[i0 + lane] = make_float2(ar, ai);
		}
	}
	// the last T - 1 samples of the stream so far, for the feed that follows (a block shorter than that keeps part of the old tail)
	if(blockIdx.x == 0 && lane < T - 1) a.tail_out[lane] = res_sample<FMT>(a, (int64_t)a.nin - (int64_t)(T - 1) + (int64_t)lane);
}

}  // namespace vdl2
