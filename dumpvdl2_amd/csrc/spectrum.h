// spectrum.h - the input monitor: a Welch-averaged, windowed-FFT power spectrum and level statistics of the caller's stream, as
// fed (ahead of the resampler).  Not in the reference.  Definition (vdl2hip.h, "Input monitor"): the stream is cut into segments
// of N = nfft samples, segment j is analysed iff it is complete and j % stride == 0,
//   X_s[k] = sum_n w[n] x[j N + n] exp(-2 pi i k n / N),   acc[i] += |X_s[(i + N / 2) mod N]|^2
// the transform and |X|^2 in float32, the sums over segments in float64.  The host divides by S (sum w)^2 when it reads.
//
// k_spectrum: one workgroup takes a run of consecutive analysed segments.  Per segment every sample is loaded once (lane i takes
// samples i, i + T, ...: coalesced), converted as the resampler converts it, counted into the level statistics as it is and stored
// to LDS times w[n]; then a Stockham autosort FFT between two LDS buffers - radix 4 while 4 divides what is left, one radix-2 pass
// at the end where log2 N is odd - with every twiddle read from the host's table (no device sin / cos, no recurrence).  A lane
// keeps the bins i = lane, lane + T, ... of the run's sum in float64 registers and writes them, with the workgroup's level
// partials, as one row: plain stores, no atomics.  k_spectrum_reduce adds the rows in index order into the accumulators, a lane per
// bin, so the result is a function of the sequence of feeds alone.
//
// LDS: a butterfly of a pass with stride s reads x[b + k N / 4] (b: the butterfly, consecutive over the lanes - no conflict) and
// writes y[q + s (4 p + k)], q = b mod s, p = b / s: in the first pass (s = 1) a stride of 4 float2 = 8 dwords, which would put
// the 32 lanes of a ds_write_b64 phase on 8 of the 64 dword banks.  Every 32 float2 are followed by one of padding (spec_pad),
// which spreads them over all of them; the later passes write runs of s consecutive elements.
// The samples a feed leaves in an incomplete segment that will be analysed are carried as float2 (the format no longer matters),
// in two buffers that alternate like the resampler's tail; workgroup 0 writes the next feed's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "resample.h"

namespace vdl2 {

constexpr int kSpecMaxThreads = 256;     // lanes per workgroup: N / 4 butterflies per pass, at most this many at a time
constexpr int kSpecMaxPerLane = 16;      // bins (and samples) per lane at the most: 4096 / 256
constexpr uint32_t kSpecMaxRows = 1024;  // workgroups of one launch = rows the reduction adds
constexpr int kSpecLevels = 5;           // a row's tail: sum of re^2 + im^2, sum re, sum im (float64), clipped count, peak (as float64: exact)

struct SpecArgs {
	const void *in;            // the block: nin samples in the caller's format
	const float2 *carry_in;    // the ncarry samples of the segment the block starts in (it is analysed and was begun by earlier feeds)
	float2 *carry_out;         // the same for the next feed: ncarry_out samples, the first of them at rel = carry_rel
	const float *w;            // [N]
	const float2 *tw;          // [N]: exp(-2 pi i k / N)
	double *rows;              // [grid][N + kSpecLevels]
	int64_t rel0;              // first sample of the first analysed segment relative to the block's first (>= -ncarry)
	int64_t carry_rel;
	uint64_t seg_step;         // stride N
	uint32_t nin, ncarry, ncarry_out, nseg, run, N, log2n;
};

__host__ __device__ __forceinline__ uint32_t spec_pad(uint32_t i) { return i + (i >> 5); }
__host__ __device__ __forceinline__ float2 spec_cmul(float2 a, float2 w) {
	return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// Butterfly b (0 .. n_total / 4 - 1) of the Stockham radix-4 pass that works on sub-transforms of length n = n_total / s:
//   y[q + s (4 p + k)] = w_n^{k p} sum_m x[q + s (p + m n / 4)] (-i)^{k m},   q = b mod s, p = b / s
__host__ __device__ __forceinline__ void spec_pass4(const float2 *x, float2 *y, const float2 *tw, uint32_t ntot, uint32_t log2s, uint32_t b) {
	const uint32_t s = 1u << log2s, q = b & (s - 1), p = b >> log2s, n4 = ntot >> 2;
	const float2 a0 = x[spec_pad(b)], a1 = x[spec_pad(b + n4)], a2 = x[spec_pad(b + 2 * n4)], a3 = x[spec_pad(b + 3 * n4)];
	const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
	const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
	const float2 jd = make_float2(-d13.y, d13.x);                       // i (a1 - a3)
	const uint32_t t = p << log2s;                                      // p (n_total / n): the twiddle's index in the table of n_total
	const uint32_t o = q + ((4 * p) << log2s);
	y[spec_pad(o)] = make_float2(s02.x + s13.x, s02.y + s13.y);
	y[spec_pad(o + s)] = spec_cmul(make_float2(d02.x - jd.x, d02.y - jd.y), tw[t]);
	y[spec_pad(o + 2 * s)] = spec_cmul(make_float2(s02.x - s13.x, s02.y - s13.y), tw[2 * t]);
	y[spec_pad(o + 3 * s)] = spec_cmul(make_float2(d02.x + jd.x, d02.y + jd.y), tw[3 * t]);
}
// The last pass where log2 N is odd: sub-transforms of length 2 (s = N / 2), no twiddle.  Butterfly b: 0 .. N / 2 - 1
__host__ __device__ __forceinline__ void spec_pass2(const float2 *x, float2 *y, uint32_t ntot, uint32_t b) {
	const uint32_t h = ntot >> 1;
	const float2 a0 = x[spec_pad(b)], a1 = x[spec_pad(b + h)];
	y[spec_pad(b)] = make_float2(a0.x + a1.x, a0.y + a1.y);
	y[spec_pad(b + h)] = make_float2(a0.x - a1.x, a0.y - a1.y);
}

#ifdef __HIPCC__
// sample `rel` of the stream relative to the block's first, as a float value: the carried part of the segment, then the block
template<int FMT>
__device__ __forceinline__ float2 spec_sample(const SpecArgs &a, int64_t rel) {
	if(rel < 0) { const int64_t i = rel + (int64_t)a.ncarry; return i >= 0 ? a.carry_in[i] : make_float2(0.f, 0.f); }
	if(rel >= (int64_t)a.nin) return make_float2(0.f, 0.f);                  // (never: the host lists complete segments only)
	return RawFmt<FMT>::level(((const typename RawFmt<FMT>::word *)a.in)[rel]);
}

// PER = N / T: the samples (and bins) a lane holds - 1 at N = 64, 4 from 256 to 1024, 16 at 4096: a build per value, so that the
// loops over them have no idle iterations and a small transform does not pay for the registers of a large one
template<int FMT, int PER>
__global__ __launch_bounds__(kSpecMaxThreads) void k_spectrum(const SpecArgs a) {
	extern __shared__ float2 spec_lds[];
	const uint32_t N = a.N, T = blockDim.x, lane = threadIdx.x, half = spec_pad(N) + 1;
	float2 *bufa = spec_lds, *bufb = spec_lds + half;
	if(blockIdx.x == 0) for(uint32_t i = lane; i < a.ncarry_out; i += T) a.carry_out[i] = spec_sample<FMT>(a, a.carry_rel + (int64_t)i);
	double acc[PER];
	#pragma unroll
	for(int r = 0; r < PER; r++) acc[r] = 0.0;
	double sp = 0.0, si = 0.0, sq = 0.0;
	uint32_t nclip = 0;
	float peak = 0.f;
	const uint32_t m0 = blockIdx.x * a.run;
	for(uint32_t m = m0; m < m0 + a.run && m < a.nseg; m++) {              // (uniform)
		const int64_t rel = a.rel0 + (int64_t)((uint64_t)m * a.seg_step);
		#pragma unroll
		for(int r = 0; r < PER; r++) {
			const uint32_t i = lane + (uint32_t)r * T;
			if(i < N) {
				const float2 v = spec_sample<FMT>(a, rel + (int64_t)i);
				sp += (double)v.x * (double)v.x + (double)v.y * (double)v.y; si += (double)v.x; sq += (double)v.y;
				peak = __builtin_fmaxf(peak, __builtin_fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)));
				nclip += (RawFmt<FMT>::at_rail(v.x) || RawFmt<FMT>::at_rail(v.y)) ? 1u : 0u;       // (at the converter's rail, stated on the float value: vdl2hip.h)
				const float wn = a.w[i];
				bufa[spec_pad(i)] = make_float2(v.x * wn, v.y * wn);
			}
		}
		__syncthreads();
		float2 *x = bufa, *y = bufb;
		uint32_t log2s = 0;
		for(; log2s + 2 <= a.log2n; log2s += 2) {
			for(uint32_t b = lane; b < (N >> 2); b += T) spec_pass4(x, y, a.tw, N, log2s, b);
			__syncthreads();
			float2 *t = x; x = y; y = t;
		}
		if(log2s < a.log2n) {
			for(uint32_t b = lane; b < (N >> 1); b += T) spec_pass2(x, y, N, b);
			__syncthreads();
			float2 *t = x; x = y; y = t;
		}
		#pragma unroll
		for(int r = 0; r < PER; r++) {
			const uint32_t i = lane + (uint32_t)r * T;
			if(i < N) {
				const float2 X = x[spec_pad((i + (N >> 1)) & (N - 1))];         // bin i of the ascending-frequency order is X[(i + N / 2) mod N]
				acc[r] += (double)(X.x * X.x + X.y * X.y);
			}
		}
		__syncthreads();                                                    // the next segment overwrites both buffers
	}
	double *row = a.rows + (size_t)blockIdx.x * (N + kSpecLevels);
	#pragma unroll
	for(int r = 0; r < PER; r++) {
		const uint32_t i = lane + (uint32_t)r * T;
		if(i < N) row[i] = acc[r];
	}
	// the level partials of the workgroup: a tree over the lanes, always the same one
	double *red = (double *)spec_lds;                                       // [kSpecLevels][T]: over the transform's buffers (spec_lds_bytes() covers both)
	red[lane] = sp; red[T + lane] = si; red[2 * T + lane] = sq; red[3 * T + lane] = (double)nclip; red[4 * T + lane] = (double)peak;
	__syncthreads();
	for(uint32_t h = T >> 1; h > 0; h >>= 1) {
		if(lane < h) {
			red[lane] += red[lane + h]; red[T + lane] += red[T + lane + h]; red[2 * T + lane] += red[2 * T + lane + h];
			red[3 * T + lane] += red[3 * T + lane + h];
			red[4 * T + lane] = red[4 * T + lane] > red[4 * T + lane + h] ? red[4 * T + lane] : red[4 * T + lane + h];
		}
		__syncthreads();
	}
	if(lane < (uint32_t)kSpecLevels) row[N + lane] = red[lane * T];
}

// acc[i] += rows[0][i] + rows[1][i] + ...: one lane per bin and per level figure, the rows in index order (the peak: their maximum)
__global__ __launch_bounds__(256) void k_spectrum_reduce(const double *rows, double *acc, uint32_t nrows, uint32_t N) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x, W = N + kSpecLevels;
	if(i >= W) return;
	double s = acc[i];
	if(i == N + 4) {
		for(uint32_t r = 0; r < nrows; r++) { const double v = rows[(size_t)r * W + i]; s = v > s ? v : s; }
	} else {
		#pragma unroll 8
		for(uint32_t r = 0; r < nrows; r++) s += rows[(size_t)r * W + i];
	}
	acc[i] = s;
}
#endif  // __HIPCC__

// threads and dynamic LDS of k_spectrum for a transform of N points (the two padded buffers; the level tree reuses them)
inline uint32_t spec_threads(uint32_t N) { const uint32_t t = N / 4; return t < 64 ? 64 : t > (uint32_t)kSpecMaxThreads ? (uint32_t)kSpecMaxThreads : t; }
inline size_t spec_lds_bytes(uint32_t N) {
	const size_t fft = 2 * (size_t)(spec_pad(N) + 1) * sizeof(float2), red = (size_t)kSpecLevels * spec_threads(N) * sizeof(double);
	return fft > red ? fft : red;
}

}  // namespace vdl2
