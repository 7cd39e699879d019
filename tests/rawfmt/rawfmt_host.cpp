// rawfmt_host.cpp - the host build of dumpvdl2_amd/csrc/rawfmt.h: every conversion over its whole domain, as raw bits on stdout for
// tests/test_rawfmt_host.py to hold against numpy's float32 arithmetic.
//   U8 <i> <byte> <level lo> <level hi> <ref_level lo> <ref_level hi>      i = 0..255: the byte in the low and in the high position
//   S8 <byte> <level lo> <level hi> <ref lo> <ref hi>
//   S16 <value> <level lo> <level hi> <ref lo> <ref hi>                    all 65 536 values in the low and in the high half
//   CF32 <bits in> <level> <ref_level>                                     for every word given on the command line (hex)
//   BYTES <u8> <s16> <cf32> <s8>
// (floats as the hex of their bits; lo / hi: the component read from that position, the other position holding the complement
// pattern so that a conversion that mixes the two up is caught)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "rawfmt.h"

using namespace vdl2;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

template<int FMT>
static void both(const char *tag, uint32_t v, uint32_t lo_word, uint32_t hi_word) {
	const raw2 a = RawFmt<FMT>::level((typename RawFmt<FMT>::word)lo_word), b = RawFmt<FMT>::level((typename RawFmt<FMT>::word)hi_word);
	float rl, ri, rl2, ri2;
	RawFmt<FMT>::ref_level(lo_word, 0u, rl, ri);
	RawFmt<FMT>::ref_level(hi_word, 0u, rl2, ri2);
	(void)ri; (void)rl2;
	printf("%s %u %08x %08x %08x %08x\n", tag, v, bits(a.x), bits(b.y), bits(rl), bits(ri2));
}

int main(int argc, char **argv) {
	for(uint32_t i = 0; i < 256; i++) {
		const uint32_t other = (~i) & 0xffu;
		both<kFmtU8>("U8", i, i | (other << 8), (i << 8) | other);
		both<kFmtS8>("S8", i, i | (other << 8), (i << 8) | other);
	}
	for(uint32_t i = 0; i < 65536; i++) {
		const uint32_t other = (~i) & 0xffffu;
		both<kFmtS16>("S16", i, i | (other << 16), (i << 16) | other);
	}
	for(int k = 1; k < argc; k++) {
		const uint32_t u = (uint32_t)strtoul(argv[k], nullptr, 16);
		float f; memcpy(&f, &u, 4);
		const raw2 a = RawFmt<kFmtCF32>::level(raw_pair(f, 1.0f)), b = RawFmt<kFmtCF32>::level(raw_pair(1.0f, f));
		float re, im, re2, im2;
		RawFmt<kFmtCF32>::ref_level(u, 0x3f800000u, re, im);
		RawFmt<kFmtCF32>::ref_level(0x3f800000u, u, re2, im2);
		if(bits(a.y) != 0x3f800000u || bits(b.x) != 0x3f800000u || bits(im) != 0x3f800000u || bits(re2) != 0x3f800000u || bits(a.x) != bits(b.y) || bits(re) != bits(im2)) { printf("CF32 components mixed up\n"); return 1; }
		printf("CF32 %08x %08x %08x\n", u, bits(a.x), bits(re));
	}
	static_assert(raw_bytes(kFmtU8) == 2 && raw_bytes(kFmtS16) == 4 && raw_bytes(kFmtCF32) == 8 && raw_bytes(kFmtS8) == 2, "sample sizes");
	static_assert(sizeof(RawFmt<kFmtU8>::word) == 2 && sizeof(RawFmt<kFmtS16>::word) == 4 && sizeof(RawFmt<kFmtCF32>::word) == 8 && sizeof(RawFmt<kFmtS8>::word) == 2, "a word is a sample");
	printf("BYTES %u %u %u %u\n", raw_bytes(kFmtU8), raw_bytes(kFmtS16), raw_bytes(kFmtCF32), raw_bytes(kFmtS8));
	// the run-time form picks the format it is asked for
	for(int code = 0; code < 4; code++) {
		int got = -1;
		with_fmt(code, [&](auto F) { got = F(); });
		printf("WITH %d %d\n", code, got);
	}
	return 0;
}
