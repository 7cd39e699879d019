// resample_design.h - host-side, one-time design of the rational resampler in front of the channeliser (K0, resample.h).
//
// Not in the reference: dumpvdl2 sets its radio to 105000 * oversample samples per second itself (src/dumpvdl2.c:1073) and never
// resamples.  A receiver that is handed IQ at another rate converts it to that rate first:
//   fout = 105000 * oversample, g = gcd(input_rate, fout), L = fout / g, M = input_rate / g
//   r[n] = sum_{j < T} h[j L + p_n] x[b_n - j],   p_n = (n M) mod L,   b_n = floor(n M / L)
// h[] is a Kaiser-windowed sinc at the rate L * input_rate, designed in double precision and rounded to float32 once:
//   cutoff 0.50 fmin, transition 0.40 .. 0.60 fmin (fmin = min(input_rate, fout)), designed for 86 dB - the textbook length for 80 dB
//   misses it by up to 0.9 dB once the taps are float32 - which gives, over every supported ratio (tests/test_resampler_design.py):
//   ripple <= 0.001 dB over |f| <= 0.40 fmin, >= 85 dB down for |f| >= 0.60 fmin, every phase's DC gain within 3e-5 of 1.
// What folds back from beyond 0.60 fmin lands outside 0.40 fmin: the channels of a receiver lie within that.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace vdl2 {

constexpr uint32_t kResMaxL = 1024;      // phases: keeps the tap table small (1024 x 29 floats = 116 KiB, read through the cache)
constexpr uint32_t kResMaxDown = 8;      // input_rate <= 8 fout: T grows with M / L (219 at 8)
constexpr uint32_t kResMaxUp = 4;        // 4 input_rate >= fout: bounds the output a block can become
constexpr uint32_t kResMaxT = 224;       // taps per phase at the ratios above (the kernel's tail update relies on T - 1 < 256)

struct ResamplerDesign {
	uint32_t L = 0, M = 0, T = 0;
	std::vector<float> taps;             // L * T, prototype order: h[j * L + p]
};

inline uint32_t res_gcd(uint32_t a, uint32_t b) { while(b) { const uint32_t t = a % b; a = b; b = t; } return a; }

// false: a ratio this library does not take (vdl2hip.h, vdl2hip_cfg.input_rate); L, M are written either way when the rates are non-zero
inline bool resampler_ratio(uint32_t input_rate, uint32_t output_rate, uint32_t &L, uint32_t &M) {
	L = M = 0;
	if(input_rate == 0 || output_rate == 0) return false;
	const uint32_t g = res_gcd(input_rate, output_rate);
	L = output_rate / g; M = input_rate / g;
	if(L > kResMaxL) return false;
	if((uint64_t)input_rate > (uint64_t)kResMaxDown * output_rate) return false;
	if((uint64_t)kResMaxUp * input_rate < (uint64_t)output_rate) return false;
	return true;
}

inline double res_bessel_i0(double x) {      // the series: x <= 9 here, converges in a few dozen terms
	double s = 1.0, t = 1.0;
	const double q = x * x / 4.0;
	for(int k = 1; k < 200; k++) { t *= q / ((double)k * (double)k); s += t; if(t < 1e-18 * s) break; }
	return s;
}

inline uint32_t resampler_taps_per_phase(uint32_t input_rate, uint32_t output_rate, uint32_t L) {
	const double A = 86.0, fmin = (double)(input_rate < output_rate ? input_rate : output_rate);
	const double dw = 2.0 * M_PI * 0.2 * fmin / ((double)L * (double)input_rate);      // transition width at the prototype's rate, rad / sample
	return (uint32_t)std::ceil((A - 8.0) / (2.285 * dw) / (double)L) + 1u;
}

inline bool design_resampler(uint32_t input_rate, uint32_t output_rate, ResamplerDesign &d, bool want_taps = true) {
	if(!resampler_ratio(input_rate, output_rate, d.L, d.M)) return false;
	d.T = resampler_taps_per_phase(input_rate, output_rate, d.L);
	if(d.T > kResMaxT) return false;      // (cannot happen within the ratios above: 219 at 8 : 1)
	if(!want_taps) return true;
	const double A = 86.0, beta = 0.1102 * (A - 8.7);
	const double fmin = (double)(input_rate < output_rate ? input_rate : output_rate);
	const double fc = 0.5 * fmin / ((double)d.L * (double)input_rate);                 // cutoff, cycles / sample at the prototype's rate
	const size_t N = (size_t)d.L * d.T;
	std::vector<double> h(N);
	const double mid = ((double)N - 1.0) / 2.0, i0b = res_bessel_i0(beta);
	double sum = 0.0;
	for(size_t k = 0; k < N; k++) {
		const double t = (double)k - mid, a = 2.0 * fc * t * M_PI;
		const double sinc = std::fabs(a) < 1e-12 ? 1.0 : std::sin(a) / a;
		const double u = 2.0 * t / ((double)N - 1.0), w = res_bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - u * u))) / i0b;
		h[k] = sinc * w;
		sum += h[k];
	}
	d.taps.resize(N);
	for(size_t k = 0; k < N; k++) d.taps[k] = (float)(h[k] * (double)d.L / sum);      // every phase's DC gain ~ 1
	return true;
}

}  // namespace vdl2
