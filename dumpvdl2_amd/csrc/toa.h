// toa.h - burst timing: for every burst the walker has handed to the burst decoder, the correlation of the channel's decimated stream
// with the unique word's waveform (toa_design.h) at 2 W + 1 lags round the decoder's own symbol clock - the peak, its parabola vertex,
// its strength, the carrier's phase and slope there.  Not in the reference.
// Definition: vdl2hip.h, "Burst timing".  A read-only pass behind k_frame_finish of the feed that decodes the burst, where the burst
// capture runs: it reads the feed's burst lists and y, writes buffers of its own, and touches nothing the decoder reads or writes.
//
// k_toa: 256 lanes, a workgroup per burst, grid-stride over the feed's bursts in record order (channel, position in the channel's
// list).  Every workgroup turns the channels' burst counts into offsets in LDS (k_capture_copy's idiom) and finds a burst's channel by
// a search there; every record has a fixed size and a fixed place, so there is no plan kernel and no atomic.
//   stage: u[0 .. 151) = conj(s[n]) rotated by the burst's slope, and y[t0 - W .. t0 + W + 151) through the ring mask (zero before the
//     stream's start) go to LDS once: at most 215 pairs.
//   lags: wavefront w takes the lags w, w + 4, ...; lane l of it the taps l, l + 64, l + 128 in that order (fused multiply-adds from
//     zero), and the 64 partial sums are combined by a fixed tree of shuffles - lane i takes in lane i + 32, then i + 16, ... i + 1.
//   peak: every lane reads the 2 W + 1 powers in ascending order (uniform: LDS broadcasts); the wavefront that owns the peak's lag forms
//     the two half sums and the energy under the template the same way - the energy in float64 -, writes the curve if the record has
//     one, and its lane 0 the record.
// The per-burst steps are functions that also compile for the host: vdl2hip_debug_toa_burst runs them lane by lane (tests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vdl2_core.h"
#include "capture.h"
#include "toa_design.h"

namespace vdl2 {

constexpr int kToaThreads = 256, kToaWaves = 4;
constexpr uint32_t kToaMaxLag = 32, kToaDefLag = 8, kToaMaxLags = 2 * kToaMaxLag + 1, kToaWin = kToaTaps + 2 * kToaMaxLag;
constexpr uint32_t kToaMaxPool = 1u << 24, kToaDefCurves = 4096;
constexpr int kToaLead = kPreamble * kSpsDec;       // the unique word ahead of a burst's first symbol: t0 = first_symbol - 160
constexpr int kToaHalf = 75;                        // the two half sums: n = 0 .. 74 and 75 .. 149
constexpr uint32_t kToaEarly = 1u, kToaEdge = 2u, kToaFlat = 4u, kToaNoCurve = 8u;      // VDL2HIP_TOA_*

// the record as the device writes it; the layout is vdl2hip_burst_toa's (taps.inc asserts size and offsets): the host copies it as it
// is and fills in frames, frames_ok and curve_off
struct ToaRec {
	uint32_t chan, freq; int64_t burst_ord, sync_sample, first_symbol, peak_sample; int32_t peak_lag; uint32_t nlags;
	float toa_frac, peak_power, energy, rho, carrier_phase, cfo_hz, dphi, resid; uint32_t flags, frames, frames_ok, curve_off;
};
struct ToaHdr { uint32_t nrec, pad_[3]; };          // records of the feed
struct ToaSums { cf32 c, ca, cb; double ey; };      // at the peak: the whole sum, the two halves, the energy under the template

struct ToaArgs {
	const cf32 *y; const Burst *bursts; const uint32_t *nb_chan; const uint32_t *freq; const cf32 *s;
	ToaRec *rec; float *curve; ToaHdr *hdr;
	double e_s; uint32_t cap_bursts_chan, nchan, chan_first, cap, mask, W, pool_curves;
};

// sample i of the window, y_c[t0 - W + i]: 0 before the stream's start
__host__ __device__ __forceinline__ cf32 toa_window(const cf32 *yc, uint32_t mask, int64_t t0, uint32_t W, uint32_t i) {
	const int64_t m = t0 - (int64_t)W + (int64_t)i;
	return m < 0 ? cf32{ 0.f, 0.f } : yc[(uint32_t)(m & (int64_t)mask)];
}
// u[n] = conj(s[n]) (cos th, sin th), th = -(double)dphi n / 10: cosine and sine in double, narrowed; the product in float32
__host__ __device__ __forceinline__ cf32 toa_u(cf32 s, float dphi, uint32_t n) {
	const double th = -(double)dphi * (double)n / 10.0;
	const float c = (float)cos(th), sn = (float)sin(th);
	return cf32{ fmaf(s.re, c, s.im * sn), fmaf(s.re, sn, -(s.im * c)) };
}
// lane `lane` of 64's share of sum u[n] yw[k + n] over n0 <= n < n1: its taps lane, lane + 64, lane + 128 in that order, from zero
__host__ __device__ __forceinline__ cf32 toa_lane_sum(const cf32 *u, const cf32 *yw, uint32_t k, uint32_t lane, uint32_t n0, uint32_t n1) {
	cf32 acc{ 0.f, 0.f };
	for(uint32_t n = lane; n < n1; n += 64) {
		if(n < n0) continue;
		const cf32 a = u[n], b = yw[k + n];
		acc.re = fmaf(a.re, b.re, acc.re); acc.re = fmaf(-a.im, b.im, acc.re);
		acc.im = fmaf(a.re, b.im, acc.im); acc.im = fmaf(a.im, b.re, acc.im);
	}
	return acc;
}
// ... and of the energy under the template at lag k: float32 re^2 + im^2 (a product, a fused multiply-add) per sample, summed in double
__host__ __device__ __forceinline__ double toa_lane_energy(const cf32 *yw, uint32_t k, uint32_t lane) {
	double e = 0.0;
	for(uint32_t n = lane; n < (uint32_t)kToaTaps; n += 64) { const cf32 b = yw[k + n]; e += (double)fmaf(b.re, b.re, b.im * b.im); }
	return e;
}
__host__ __device__ __forceinline__ cf32 toa_add(cf32 a, cf32 b) { return cf32{ a.re + b.re, a.im + b.im }; }
__host__ __device__ __forceinline__ float toa_power(cf32 c) { return fmaf(c.re, c.re, c.im * c.im); }
// the tree's level s (32, 16, ... 1) as lane `lane` takes it on the host (the device's is a shuffle: what lane 0 ends up with is the same)
template<typename T, typename F>
__host__ __forceinline__ void toa_tree_step(T *part, uint32_t lane, uint32_t s, F add) { if(lane < s) part[lane] = add(part[lane], part[lane + s]); }
// the lowest lag index among those with the largest power: a float32 >, taken in ascending order
__host__ __device__ __forceinline__ uint32_t toa_peak(const float *P, uint32_t nlags) {
	uint32_t kp = 0; float best = P[0];
	for(uint32_t k = 1; k < nlags; k++) { const float v = P[k]; if(v > best) { best = v; kp = k; } }
	return kp;
}
// the angle of (re, im) by the decoder's double atan2, after a scaling by the larger magnitude that keeps its float quotient in range
__host__ __device__ __forceinline__ double toa_angle(double im, double re) {
	const double m = fabs(re) > fabs(im) ? fabs(re) : fabs(im);
	return m > 0.0 ? atan2_f64(im / m, re / m) : 0.0;
}
// the record of a burst from its curve and the sums at the peak (curve: the record has room for its curve)
__host__ __device__ __forceinline__ void toa_record(const Burst &b, uint32_t chan, uint32_t freq, uint32_t W, const float *P, uint32_t kp, const ToaSums &q, double e_s,
		bool curve, ToaRec &r) {
	const uint32_t nlags = 2 * W + 1;
	const int64_t t0 = b.t_first - kToaLead;
	r.chan = chan; r.freq = freq; r.burst_ord = b.ord; r.sync_sample = b.sync_sample; r.first_symbol = b.t_first;
	r.peak_lag = (int32_t)kp - (int32_t)W; r.peak_sample = t0 + r.peak_lag; r.nlags = nlags;
	uint32_t flags = (t0 - (int64_t)W < 0 ? kToaEarly : 0u) | (curve ? 0u : kToaNoCurve);
	// the vertex of the parabola through the peak and its neighbours (one beyond +-W counts as 0 for the sign of den)
	const double pa = kp > 0 ? (double)P[kp - 1] : 0.0, pb = (double)P[kp], pc = kp + 1 < nlags ? (double)P[kp + 1] : 0.0;
	const double den = (pa - 2.0 * pb) + pc;
	const bool edge = kp == 0 || kp + 1 == nlags, flat = den >= 0.0;
	flags |= (edge ? kToaEdge : 0u) | (flat ? kToaFlat : 0u);
	r.toa_frac = edge || flat ? 0.f : (float)(0.5 * (pa - pc) / den);
	r.peak_power = P[kp]; r.energy = (float)q.ey;
	r.rho = q.ey == 0.0 ? 0.f : (float)((double)P[kp] / (e_s * q.ey));
	r.carrier_phase = phase_of(q.c);
	// c_b conj(c_a), in double from the float32 sums
	const double zr = fma((double)q.cb.re, (double)q.ca.re, (double)q.cb.im * (double)q.ca.im);
	const double zi = fma((double)q.cb.im, (double)q.ca.re, -((double)q.cb.re * (double)q.ca.im));
	r.dphi = b.vdphi; r.resid = (float)(toa_angle(zi, zr) / (double)kToaHalf);
	r.cfo_hz = (float)(((double)b.vdphi / 10.0 + (double)r.resid) * (105000.0 / (2.0 * kToaPi)));
	r.flags = flags; r.frames = 0; r.frames_ok = 0; r.curve_off = 0;
}

#ifdef __HIPCC__
__device__ __forceinline__ cf32 toa_wave_sum(cf32 v) {
	#pragma unroll
	for(int s = 32; s >= 1; s >>= 1) v = toa_add(v, cf32{ __shfl_down(v.re, s), __shfl_down(v.im, s) });
	return v;                                                           // (lane 0's is the tree's result)
}
__device__ __forceinline__ double toa_wave_sum(double v) {
	#pragma unroll
	for(int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
	return v;
}

__global__ __launch_bounds__(kToaThreads) void k_toa(const ToaArgs a) {
	__shared__ uint32_t bbn[kCapMaxChan + 1];
	__shared__ cf32 u[kToaTaps], yw[kToaWin], cl[kToaMaxLags];
	__shared__ float P[kToaMaxLags];
	const uint32_t lane = threadIdx.x, wave = lane >> 6, wl = lane & 63u, C = a.nchan, W = a.W, nlags = 2 * W + 1, nwin = (uint32_t)kToaTaps + 2 * W;
	if(lane < 64) {
		uint32_t total = 0;
		for(uint32_t c0 = 0; c0 < C; c0 += 64) {
			const bool in = c0 + lane < C;
			const uint32_t nbc = in ? a.nb_chan[c0 + lane] : 0u, v = nbc < a.cap_bursts_chan ? nbc : a.cap_bursts_chan;
			uint32_t inc = v;
			#pragma unroll
			for(int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if(lane >= (uint32_t)d) inc += o; }
			if(in) bbn[c0 + lane] = total + inc - v;
			total += __shfl(inc, 63);
		}
		if(lane == 0) bbn[C] = total;
	}
	__syncthreads();
	const uint32_t total = bbn[C];
	if(blockIdx.x == 0 && lane == 0) { a.hdr->nrec = total; a.hdr->pad_[0] = a.hdr->pad_[1] = a.hdr->pad_[2] = 0; }
	for(uint32_t g = blockIdx.x; g < total; g += gridDim.x) {             // (uniform)
		const int c = cap_find_chan(bbn, (int)C, g);
		const Burst b = a.bursts[(size_t)c * a.cap_bursts_chan + (g - bbn[c])];
		const cf32 *yc = a.y + (size_t)c * a.cap;
		const int64_t t0 = b.t_first - kToaLead;
		if(lane < (uint32_t)kToaTaps) u[lane] = toa_u(a.s[lane], b.vdphi, lane);
		if(lane < nwin) yw[lane] = toa_window(yc, a.mask, t0, W, lane);      // (nwin <= 215 < 256)
		__syncthreads();
		for(uint32_t k = wave; k < nlags; k += kToaWaves) {                 // (uniform per wavefront)
			const cf32 v = toa_wave_sum(toa_lane_sum(u, yw, k, wl, 0u, (uint32_t)kToaTaps));
			if(wl == 0) { cl[k] = v; P[k] = toa_power(v); }
		}
		__syncthreads();
		const uint32_t kp = toa_peak(P, nlags);
		if(wave == (kp & (kToaWaves - 1))) {
			ToaSums q;
			q.ca = toa_wave_sum(toa_lane_sum(u, yw, kp, wl, 0u, (uint32_t)kToaHalf));
			q.cb = toa_wave_sum(toa_lane_sum(u, yw, kp, wl, (uint32_t)kToaHalf, 2u * kToaHalf));
			q.ey = toa_wave_sum(toa_lane_energy(yw, kp, wl));
			const bool curve = g < a.pool_curves;
			if(curve) for(uint32_t k = wl; k < nlags; k += 64) a.curve[(size_t)g * nlags + k] = P[k];
			if(wl == 0) {
				q.c = cl[kp];
				ToaRec r;
				toa_record(b, (uint32_t)c + a.chan_first, a.freq[c], W, P, kp, q, a.e_s, curve, r);
				a.rec[g] = r;
			}
		}
		__syncthreads();                                                // (u, yw, P and cl are written again by the next burst)
	}
}
#endif  // __HIPCC__

}  // namespace vdl2
