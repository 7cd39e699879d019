// rawfmt.h - the one place that knows a raw IQ sample: the internal format codes, a sample's size, the word it is loaded as and its
// conversion to the (re, im) float pair of the reference's sbuf[] (src/demod.c:349-365).  Every reader of raw input - the
// channeliser's staging, the referee's scans, the resampler, the input monitor, k_carry - and the host's dispatch go through it.
// A new format supplies: a code, a RawFmt<> (word, level, ref_level, at_rail), a case in raw_bytes(), in with_fmt() and in the
// kernels' spelled-out chains (kernels.h: ref_raw_sample, ref_exact_window_dev, load_sample, k_carry), its public value in
// fmt_code() (vdl2hip.hip) - and, if it is to have a channeliser build that stages it without range checks, a line in
// has_fast_build() (kernels.h).
// Compiles as plain host C++17 too (tests/rawfmt/rawfmt_host.cpp holds every conversion to numpy's, exhaustively).
#pragma once
#include <cstdint>
#include <type_traits>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RAWFMT_HD __host__ __device__ __forceinline__
#else
#define RAWFMT_HD inline
#endif

namespace vdl2 {

#if defined(__HIPCC__)
typedef float2 raw2;
#else
struct raw2 { float x, y; };
#endif
RAWFMT_HD raw2 raw_pair(float re, float im) { raw2 v; v.x = re; v.y = im; return v; }

// The format inside the library (vdl2hip_ctx.fmt / in_fmt, K1Args.fmt, RefChan.fmt, the kernels' template FMT) is a small code: the
// public value for U8, S16LE and CF32, and 3 for VDL2HIP_FMT_S8, whose public value is 4 (fmt_code(), vdl2hip.hip, maps one to the other)
constexpr int kFmtU8 = 0, kFmtS16 = 1, kFmtCF32 = 2, kFmtS8 = 3;
constexpr unsigned fmt_bit(int fmt) { return 1u << fmt; }
constexpr unsigned kFmtAny = fmt_bit(kFmtU8) | fmt_bit(kFmtS16) | fmt_bit(kFmtCF32) | fmt_bit(kFmtS8);
template<int FMT> using FmtC = std::integral_constant<int, FMT>;

// bytes per complex sample
constexpr unsigned raw_bytes(int fmt) { return fmt == kFmtCF32 ? 8u : fmt == kFmtS16 ? 4u : 2u; }

// (i - 127.5f) / 127.5f of an unsigned byte (demod.c:349-354) without the division: d = i - 127.5 is exact, q = d * fl(1 / 127.5) is within an
// ulp, one Newton step on the residual d - 127.5 q makes it the correctly rounded quotient - for all 256 values (checked on the device
// against the division: tests/test_gpu_parity.py::test_uint8_conversion_without_the_division)
RAWFMT_HD float u8_level(uint32_t i) {
	const float d = (float)i - 127.5f, r = 1.0f / 127.5f;
	const float q = d * r;
	return __builtin_fmaf(__builtin_fmaf(-127.5f, q, d), r, q);
}
// (float)b / 128.0f of the two signed bytes of a 16-bit word (I in the low byte): one XOR per word turns both bytes into u = b + 128, an
// unsigned byte converts with a byte-select v_cvt_f32_ubyte*, and fma(u, 2^-7, -1) is exact (u 2^-7 is, and so is the difference: a
// multiple of 2^-7 in [-1, 1)) - two VALU operations per component where u8_level needs four, and never a negative zero (u = 128 gives
// 1 - 1 = +0).  Checked on the device for all 256 values: tests/test_gpu_s8.py::test_conversion_is_exact
RAWFMT_HD raw2 s8_level(uint32_t w) {
	const uint32_t u = w ^ 0x8080u;
	return raw_pair(__builtin_fmaf((float)(u & 0xffu), 0.0078125f, -1.0f), __builtin_fmaf((float)((u >> 8) & 0xffu), 0.0078125f, -1.0f));
}
// CF32: process_buf_short() / process_buf_uchar() do nothing but fill the float array sbuf[] (src/demod.c:349-365) that every later
// stage reads, so a CF32 sample IS the reference's sbuf[] value - unscaled, unclipped - but for this: a negative zero is read as a
// positive one.  The integer conversions never produce -0; the scan's shortcut for channels that are not mixed (k_ref_scan_multi:
// q_dphi) multiplies by (sin, cos) = (0, 1) and would turn (+0, -0) into (+0, +0) where the reference leaves it, and atan2 of a
// silent sample would land on the other side of its branch cut.
RAWFMT_HD float cf32_level(float x) { return x + 0.0f; }
RAWFMT_HD float raw_float(uint32_t bits) { float f; __builtin_memcpy(&f, &bits, 4); return f; }

// Per format: `word`, what a sample is loaded as; level(), THE conversion of the format, of the loaded word to a pair (the staging of
// the channeliser, the resampler, the monitor); ref_level(), the conversion as the referee and the generic staging execute it (the
// referee re-runs the reference's arithmetic: it differs from level() for U8 only), into two floats, of the sample held as 32-bit words
// (the scans: w, and for CF32 w2 - the same bits as the loaded word); at_rail(): is this level at the converter's rail (vdl2hip.h,
// "Input monitor").
template<int FMT> struct RawFmt;
// U8 (VDL2HIP_FMT_U8): (i - 127.5f) / 127.5f (demod.c:349-354).  Two conversions, equal for all 256 bytes (the test named at
// u8_level): ref_level() is the reference's own division - what the referee's scans and load_sample execute; level() is the
// division-free u8_level - what the U8 build of the channeliser, the resampler and the monitor execute.  Each site keeps the one it
// has: the other would be other instructions.
template<> struct RawFmt<kFmtU8> {
	typedef uint16_t word;
	static RAWFMT_HD raw2 level(uint32_t w, uint32_t = 0) { return raw_pair(u8_level(w & 0xffu), u8_level((w >> 8) & 0xffu)); }
	static RAWFMT_HD void ref_level(uint32_t w, uint32_t, float &re, float &im) { re = ((float)(w & 0xff) - 127.5f) / 127.5f; im = ((float)((w >> 8) & 0xff) - 127.5f) / 127.5f; }
	static RAWFMT_HD bool at_rail(float v) { return __builtin_fabsf(v) == 1.0f; }
};
// S16 (VDL2HIP_FMT_S16LE, I in the low half): (float)v / 32768.0f (demod.c:362-363)
template<> struct RawFmt<kFmtS16> {
	typedef uint32_t word;
	static RAWFMT_HD void ref_level(uint32_t w, uint32_t, float &re, float &im) { re = (float)(int16_t)(w & 0xffff) / 32768.0f; im = (float)(int16_t)(w >> 16) / 32768.0f; }
	static RAWFMT_HD raw2 level(uint32_t w, uint32_t = 0) { float re, im; ref_level(w, 0u, re, im); return raw_pair(re, im); }
	static RAWFMT_HD bool at_rail(float v) { return v == -1.0f || v == 32767.0f / 32768.0f; }
};
// CF32 (VDL2HIP_FMT_CF32: interleaved I, Q as float32): cf32_level on both
template<> struct RawFmt<kFmtCF32> {
	typedef raw2 word;
	static RAWFMT_HD raw2 level(raw2 w) { return raw_pair(cf32_level(w.x), cf32_level(w.y)); }
	static RAWFMT_HD void ref_level(uint32_t w, uint32_t w2, float &re, float &im) { re = cf32_level(raw_float(w)); im = cf32_level(raw_float(w2)); }
	static RAWFMT_HD bool at_rail(float v) { return __builtin_fabsf(v) >= 1.0f; }                      // (false for a NaN)
};
// S8 (VDL2HIP_FMT_S8: interleaved I, Q as signed bytes): (float)b / 128.0f, the float process_buf_short() makes of the int16 256 b
template<> struct RawFmt<kFmtS8> {
	typedef uint16_t word;
	static RAWFMT_HD raw2 level(uint32_t w, uint32_t = 0) { return s8_level(w); }
	static RAWFMT_HD void ref_level(uint32_t w, uint32_t, float &re, float &im) { const raw2 v = s8_level(w); re = v.x; im = v.y; }
	static RAWFMT_HD bool at_rail(float v) { return v == -1.0f || v == 127.0f / 128.0f; }              // (bytes -128 and 127)
};

// A run-time format code as a compile-time constant, for the host's pick among the builds of a kernel template: f(FmtC<code>{}).
// (The kernels that learn the format at run time - ref_raw_sample, ref_exact_window_dev, load_sample, k_carry - spell their chain
// of comparisons out, over the names above: through this helper and a lambda the device code came out with its loads in another
// order.)
template<class F>
inline void with_fmt(int code, F &&f) {
	switch(code) {
		case kFmtCF32: f(FmtC<kFmtCF32>{}); break;
		case kFmtS16: f(FmtC<kFmtS16>{}); break;
		case kFmtS8: f(FmtC<kFmtS8>{}); break;
		default: f(FmtC<kFmtU8>{}); break;
	}
}

// the loaded word as the sample's 32-bit words
RAWFMT_HD void raw_words(uint32_t v, uint32_t &w, uint32_t &w2) { w = v; w2 = 0u; }
RAWFMT_HD void raw_words(raw2 v, uint32_t &w, uint32_t &w2) { __builtin_memcpy(&w, &v.x, 4); __builtin_memcpy(&w2, &v.y, 4); }
// sample i of the raw samples at p, as the referee and the generic staging convert it
template<int FMT>
RAWFMT_HD void raw_ref_sample(const void *p, int64_t i, float &re, float &im) {
	uint32_t w, w2;
	raw_words(((const typename RawFmt<FMT>::word *)p)[i], w, w2);
	RawFmt<FMT>::ref_level(w, w2, re, im);
}

}  // namespace vdl2
