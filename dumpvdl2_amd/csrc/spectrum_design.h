// spectrum_design.h - host-side, one-time design of the input monitor's tables (spectrum.h): the analysis window and the FFT's
// twiddle factors, in double precision, each value rounded to float32 once.  Plain C++: nothing of HIP is needed to compile it.
//
// Not in the reference (dumpvdl2 has no view of its wideband input).  Definition (vdl2hip.h, "Input monitor"): all three windows
// are periodic, w[n], n = 0 .. N - 1, t = 2 pi n / N:
//   rect  1
//   Hann  0.5 - 0.5 cos t
//   BH4   0.35875 - 0.48829 cos t + 0.14128 cos 2t - 0.01168 cos 3t      (4-term Blackman-Harris: sidelobes 92 dB down, below
//                                                                         what a float32 transform resolves)
// and the twiddles are tw[k] = exp(-2 pi i k / N), k = 0 .. N - 1.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace vdl2 {

constexpr uint32_t kSpecMinN = 64, kSpecMaxN = 4096;
constexpr uint32_t kSpecWindows = 3;     // VDL2HIP_WIN_RECT, _HANN, _BH4
constexpr double kSpecPi = 3.14159265358979323846264338327950288;

inline bool spectrum_nfft_ok(uint32_t n) { return n >= kSpecMinN && n <= kSpecMaxN && (n & (n - 1)) == 0; }

struct SpectrumDesign {
	uint32_t nfft = 0, window = 0, log2n = 0;
	std::vector<float> w;                // nfft
	std::vector<float> tw;               // 2 nfft: (re, im) of exp(-2 pi i k / nfft)
	double sum_w = 0.0, sum_w2 = 0.0;    // of the float32 values, in double
	double enbw_bins = 0.0;              // nfft sum_w2 / sum_w^2
};

inline double spectrum_window_value(uint32_t window, uint32_t n, uint32_t nfft) {
	const double t = 2.0 * kSpecPi * (double)n / (double)nfft;
	if(window == 1) return 0.5 - 0.5 * std::cos(t);
	if(window == 2) return 0.35875 - 0.48829 * std::cos(t) + 0.14128 * std::cos(2.0 * t) - 0.01168 * std::cos(3.0 * t);
	return 1.0;
}

// false: an nfft or a window this library does not take
inline bool design_spectrum(uint32_t nfft, uint32_t window, SpectrumDesign &d, bool want_twiddles = true) {
	if(!spectrum_nfft_ok(nfft) || window >= kSpecWindows) return false;
	d.nfft = nfft; d.window = window; d.log2n = 0;
	while((1u << d.log2n) < nfft) d.log2n++;
	d.w.resize(nfft);
	d.sum_w = d.sum_w2 = 0.0;
	for(uint32_t n = 0; n < nfft; n++) {
		d.w[n] = (float)spectrum_window_value(window, n, nfft);
		d.sum_w += (double)d.w[n];
		d.sum_w2 += (double)d.w[n] * (double)d.w[n];
	}
	d.enbw_bins = (double)nfft * d.sum_w2 / (d.sum_w * d.sum_w);
	d.tw.clear();
	if(!want_twiddles) return true;
	d.tw.resize(2 * (size_t)nfft);
	for(uint32_t k = 0; k < nfft; k++) {
		// the octant's own function of the angle folded into [0, pi / 4]: the eight symmetric values come out as the same float32
		// numbers, and the axes exactly 0 and +-1
		const uint32_t oct = (8 * k) / nfft, r = k % (nfft / 8);
		const uint32_t m = (oct & 1) ? nfft / 8 - r : r;                   // distance from the nearest axis, in steps of 2 pi / nfft
		const double a = 2.0 * kSpecPi * (double)m / (double)nfft;
		const double c = std::cos(a), s = std::sin(a);
		double re, im;                                                   // of exp(+2 pi i k / nfft)
		switch(oct) {
			case 0: re = c; im = s; break;
			case 1: re = s; im = c; break;
			case 2: re = -s; im = c; break;
			case 3: re = -c; im = s; break;
			case 4: re = -c; im = -s; break;
			case 5: re = -s; im = -c; break;
			case 6: re = s; im = -c; break;
			default: re = c; im = -s; break;
		}
		d.tw[2 * k] = (float)re + 0.0f;
		d.tw[2 * k + 1] = (float)(-im) + 0.0f;
	}
	return true;
}

}  // namespace vdl2
