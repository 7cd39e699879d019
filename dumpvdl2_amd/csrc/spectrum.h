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
//
// The spectrogram tap (vdl2hip.h, "Spectrogram") is a second build of the same kernel, k_spectrum_lines: beside the run's float64 sums
// a lane keeps, per bin it owns, the float32 maximum and the float64 sum of the line under way, and flushes them where the run crosses
// a line boundary (specgram_plan.h: head, whole lines, tail).  A whole line goes straight to the ring; head and tail are left as pieces
// - float64 sums, float32 maxima; their line and segment count follow from the plan - with the run's maximum per bin and the smallest
// mean of its whole lines.  k_specgram_combine, a lane per bin, starts from the carried partial line, adds the pieces in workgroup
// order, writes the lines that become complete, stores the new carry and updates the holds.  Plain coalesced stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "resample.h"
#include "specgram_plan.h"

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

// what the spectrogram build of the kernel and the combine kernel share.  piece_*: [rows][2][N], head then tail; run_max: [rows][N] the
// largest |X|^2 of the run; run_floor: [rows][N] the smallest line mean among the run's whole lines (+inf: none); ring_*: [ring_lines][N];
// carry_*: [N] the line under way between feeds; hold: [2][N] max_hold, then floor_hold (+inf while no line has been completed)
struct SpgArgs {
	double *piece_sum; float *piece_max, *run_max, *run_floor;
	float *ring_mean, *ring_max;
	double *carry_sum; float *carry_max, *hold;
	double norm;               // 1 / (sum w)^2
	SpgFeed f;
};
// a line's values as the ring receives them
__host__ __device__ __forceinline__ float spg_mean(double sum, double norm, uint32_t R) { return (float)(sum * norm / (double)R); }
__host__ __device__ __forceinline__ float spg_peak(float mx, double norm) { return (float)((double)mx * norm); }

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
// SPG: the spectrogram build (sg: its arguments; unused otherwise)
template<int FMT, int PER, bool SPG>
__device__ __forceinline__ void spectrum_run(const SpecArgs &a, const SpgArgs &sg) {
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
	// the line under way in this run: its sum and maximum per bin; the run's maximum; the smallest mean of the run's whole lines
	double lsum[SPG ? PER : 1]; float lmax[SPG ? PER : 1], gmax[SPG ? PER : 1], wmin[SPG ? PER : 1];
	SpgRun rn{}; uint32_t cnt = 0, until = 0; uint64_t line = 0; bool inside = false;
	if constexpr(SPG) {
		#pragma unroll
		for(int r = 0; r < PER; r++) { lsum[r] = 0.0; lmax[r] = 0.f; gmax[r] = 0.f; wmin[r] = __builtin_inff(); }
		rn = spg_run(sg.f, blockIdx.x);
		inside = rn.to_boundary == 0; until = inside ? sg.f.R : rn.to_boundary; line = inside ? rn.whole_first : rn.head_line;
	}
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
				const float q = X.x * X.x + X.y * X.y;
				acc[r] += (double)q;
				if constexpr(SPG) { lsum[r] += (double)q; lmax[r] = __builtin_fmaxf(lmax[r], q); gmax[r] = __builtin_fmaxf(gmax[r], q); }
			}
		}
		if constexpr(SPG) {
			if(++cnt == until) {                                            // (uniform) a line ends with this segment
				#pragma unroll
				for(int r = 0; r < PER; r++) {
					const uint32_t i = lane + (uint32_t)r * T;
					if(i < N) {
						if(inside) {                                            // it began in this run: to the ring
							const size_t o = (size_t)(line & sg.f.ring_mask) * N + i;
							const float mean = spg_mean(lsum[r], sg.norm, sg.f.R);
							sg.ring_mean[o] = mean; sg.ring_max[o] = spg_peak(lmax[r], sg.norm);
							wmin[r] = __builtin_fminf(wmin[r], mean);
						} else {                                                // it began earlier: the head piece
							const size_t o = (size_t)blockIdx.x * 2 * N + i;
							sg.piece_sum[o] = lsum[r]; sg.piece_max[o] = lmax[r];
						}
					}
					lsum[r] = 0.0; lmax[r] = 0.f;
				}
				inside = true; cnt = 0; until = sg.f.R; line++;
			}
		}
		__syncthreads();                                                    // the next segment overwrites both buffers
	}
	if constexpr(SPG) {
		// what is left of a line: the tail piece, or the head where the run never reached a boundary
		#pragma unroll
		for(int r = 0; r < PER; r++) {
			const uint32_t i = lane + (uint32_t)r * T;
			if(i < N) {
				if(cnt) { const size_t o = ((size_t)blockIdx.x * 2 + (inside ? 1 : 0)) * N + i; sg.piece_sum[o] = lsum[r]; sg.piece_max[o] = lmax[r]; }
				sg.run_max[(size_t)blockIdx.x * N + i] = gmax[r]; sg.run_floor[(size_t)blockIdx.x * N + i] = wmin[r];
			}
		}
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
template<int FMT, int PER>
__global__ __launch_bounds__(kSpecMaxThreads) void k_spectrum(const SpecArgs a) { spectrum_run<FMT, PER, false>(a, SpgArgs{}); }
template<int FMT, int PER>
__global__ __launch_bounds__(kSpecMaxThreads) void k_spectrum_lines(const SpecArgs a, const SpgArgs sg) { spectrum_run<FMT, PER, true>(a, sg); }

// One lane per bin: the carried partial line, then this feed's pieces in workgroup order.  Every line that becomes complete goes to
// the ring; max_hold takes every run's maximum (x -> (float)((double)x norm) is monotone: the maximum of the rounded values is the
// rounded maximum), floor_hold every completed line's mean, exactly as the ring received it.  carry_n: the segments the carry holds
__global__ __launch_bounds__(256) void k_specgram_combine(const SpgArgs sg, uint32_t N, uint32_t carry_n) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if(i >= N) return;
	const SpgFeed &f = sg.f;
	double csum = carry_n ? sg.carry_sum[i] : 0.0;
	float cmax = carry_n ? sg.carry_max[i] : 0.f;
	float hold = sg.hold[i], floor = sg.hold[N + i];
	uint32_t cnt = carry_n;
	for(uint32_t g = 0; g < f.grid; g++) {
		const SpgRun rn = spg_run(f, g);                                    // (uniform)
		if(rn.m0 >= rn.m1) break;
		hold = __builtin_fmaxf(hold, spg_peak(sg.run_max[(size_t)g * N + i], sg.norm));
		if(rn.head_n) {
			const size_t o = (size_t)g * 2 * N + i;
			csum += sg.piece_sum[o]; cmax = __builtin_fmaxf(cmax, sg.piece_max[o]); cnt += rn.head_n;
			if(cnt == f.R) {
				const size_t w = (size_t)(rn.head_line & f.ring_mask) * N + i;
				const float mean = spg_mean(csum, sg.norm, f.R);
				sg.ring_mean[w] = mean; sg.ring_max[w] = spg_peak(cmax, sg.norm);
				floor = __builtin_fminf(floor, mean);
				csum = 0.0; cmax = 0.f; cnt = 0;
			}
		}
		if(rn.whole_n) floor = __builtin_fminf(floor, sg.run_floor[(size_t)g * N + i]);
		if(rn.tail_n) { const size_t o = ((size_t)g * 2 + 1) * N + i; csum = sg.piece_sum[o]; cmax = sg.piece_max[o]; cnt = rn.tail_n; }
	}
	sg.carry_sum[i] = csum; sg.carry_max[i] = cmax;
	sg.hold[i] = hold; sg.hold[N + i] = floor;
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
