// toa_design.h - host-side, one-time design of the burst timing tap's template (toa.h): the unique word as a raised-cosine waveform
// at the decimated rate, in double precision, each value rounded to float32 once.  Plain C++: nothing of HIP is needed to compile it.
//
// Not in the reference (dumpvdl2 never correlates with the unique word's waveform: its sync grid works on phases, demod.c:105-198).
// Definition (vdl2hip.h, "Burst timing"):
//   s[n] = sum_{i = 0 .. 15} exp(j P[i]) p((n - 10 i) / 10),  n = 0 .. 150
//   P[i]   the cumulative unique-word phases of demod.c:107-124 (tables.h builds the same list for the sync kernels)
//   p(t) = sinc(t) cos(0.6 pi t) / (1 - (1.2 t)^2), sinc(t) = sin(pi t) / (pi t): the raised cosine of roll-off 0.6 the synthesiser
//          shapes its symbols with, here without its truncation to +-4 symbols.  t is a multiple of 0.1 and 1.2 t = +-1 would need
//          t = +-5/6, so the singular point is never met; p(0) = 1 and p(k) = 0 at every other integer, so s[10 i] = exp(j P[i]) up to
//          the rounding of sin(pi k).
// Index 0 is the centre of unique-word symbol 0, index 150 that of symbol 15: the template stops at the two outer centres, because
// the constant-phase ramp-up symbols ahead of the unique word correlate with anything that reaches beyond them.
#pragma once
#include <cmath>
#include <cstdint>

namespace vdl2 {

constexpr int kToaTaps = 151;            // 15 symbols of 10 samples and the last centre
constexpr double kToaPi = 3.14159265358979323846264338327950288;

struct ToaDesign {
	float s[2 * kToaTaps];               // (re, im)
	double energy;                       // E_s: sum |s[n]|^2 of the float32 values, in double, in ascending n
};

inline double toa_pulse(int tenths) {
	if(tenths == 0) return 1.0;
	const double t = (double)tenths / 10.0, x = 1.2 * t;
	return std::sin(kToaPi * t) / (kToaPi * t) * std::cos(0.6 * kToaPi * t) / (1.0 - x * x);
}

inline void design_toa(ToaDesign &d) {
	static const int q[16] = { 0, 3, -3, 1, 1, 2, 0, 4, -3, 4, -2, 3, 1, -2, -3, 0 };      // P[i] in units of pi / 4
	d.energy = 0.0;
	for(int n = 0; n < kToaTaps; n++) {
		double re = 0.0, im = 0.0;
		for(int i = 0; i < 16; i++) {
			const double p = toa_pulse(n - 10 * i), a = (double)q[i] * (kToaPi / 4.0);
			re += std::cos(a) * p; im += std::sin(a) * p;
		}
		d.s[2 * n] = (float)re; d.s[2 * n + 1] = (float)im;
		d.energy += (double)d.s[2 * n] * (double)d.s[2 * n] + (double)d.s[2 * n + 1] * (double)d.s[2 * n + 1];
	}
}

}  // namespace vdl2
