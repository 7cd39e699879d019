// specgram_plan.h - the spectrogram tap's plan of a feed (vdl2hip.h, "Spectrogram"; kernels: spectrum.h): which workgroup of k_spectrum
// takes which analysed segments, where the line boundaries fall in its run, which pieces it leaves for the combine kernel and which ring
// slots the feed writes.  Plain C++ - no HIP include, like rawfmt.h - so that the host tests run it against brute force
// (tests/specgram/specgram_plan_host.cpp); the device code calls the same functions.
//
// The tap numbers the segments it sees t = 0, 1, ... (t = a - a0).  Line l is t in [l R, (l + 1) R).  A feed brings t0 .. t0 + nseg - 1;
// workgroup g takes the feed's segments [g run, min((g + 1) run, nseg)), as the monitor's launch always did.  Of its run
//   head: what lies ahead of the first line boundary, if the run does not begin on one (the line began in an earlier workgroup or feed)
//   whole lines: those that begin and end inside the run - written straight to the ring by the workgroup
//   tail: what follows the last boundary in the run, if the run does not end on one
// so a workgroup leaves at most two pieces, and the pieces of one line are met in ascending segment order by whoever walks the
// workgroups in index order (k_specgram_combine), starting from what the feeds before left of the line under way.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SPG_FN __host__ __device__ inline
#else
#define SPG_FN inline
#endif

namespace vdl2 {

constexpr uint32_t kSpgDefLineSegments = 16, kSpgMaxLineSegments = 1u << 20;
constexpr uint64_t kSpgMaxRingFloats = 1ull << 25;     // ring_lines * nfft at the most, per plane

struct SpgFeed {
	uint64_t t0;              // segments the tap has seen before this feed
	uint32_t nseg, run, grid; // analysed segments of the feed, segments per workgroup, workgroups (at least 1, also for no segment)
	uint32_t R, ring_mask;    // line_segments, ring_lines - 1
};
struct SpgRun {
	uint32_t m0, m1;          // the feed's segments [m0, m1) this workgroup takes
	uint32_t to_boundary;     // segments from m0 to the first line boundary at or behind it (0: the run begins on one)
	uint32_t head_n;          // min(to_boundary, m1 - m0): the head piece's segments (0: none)
	uint32_t whole_n;         // whole lines
	uint32_t tail_n;          // the tail piece's segments (0: none)
	uint64_t head_line;       // the line the head belongs to; the whole lines are whole_first .., the tail's is whole_first + whole_n
	uint64_t whole_first;
};

// the monitor's split of nseg segments over at most max_rows workgroups
SPG_FN void spg_split(uint64_t nseg, uint32_t max_rows, uint32_t &run, uint32_t &grid) {
	const uint64_t r = (nseg + max_rows - 1) / max_rows;
	run = (uint32_t)(r > 1 ? r : 1);
	const uint64_t g = (nseg + run - 1) / run;
	grid = (uint32_t)(g > 1 ? g : 1);
}
SPG_FN SpgFeed spg_feed(uint64_t t0, uint64_t nseg, uint32_t R, uint32_t ring_lines, uint32_t max_rows) {
	SpgFeed f{};
	f.t0 = t0; f.nseg = (uint32_t)nseg; f.R = R; f.ring_mask = ring_lines - 1;
	spg_split(nseg, max_rows, f.run, f.grid);
	return f;
}
SPG_FN SpgRun spg_run(const SpgFeed &f, uint32_t g) {
	SpgRun r{};
	const uint64_t m0 = (uint64_t)g * f.run, m1 = m0 + f.run < f.nseg ? m0 + f.run : f.nseg;
	if(m0 >= f.nseg) { r.m0 = r.m1 = f.nseg; return r; }
	r.m0 = (uint32_t)m0; r.m1 = (uint32_t)m1;
	const uint64_t s = f.t0 + m0, len = m1 - m0;
	const uint32_t ph = (uint32_t)(s % f.R);
	r.head_line = s / f.R;
	r.to_boundary = ph ? f.R - ph : 0;
	r.head_n = (uint32_t)(r.to_boundary < len ? r.to_boundary : len);
	r.whole_first = ph ? r.head_line + 1 : r.head_line;
	const uint64_t rest = len - r.head_n;
	r.whole_n = (uint32_t)(rest / f.R);
	r.tail_n = (uint32_t)(rest % f.R);
	return r;
}
// lines complete before and after the feed: [first, last) are the lines it completes, each written to slot l & ring_mask
SPG_FN uint64_t spg_lines_before(const SpgFeed &f) { return f.t0 / f.R; }
SPG_FN uint64_t spg_lines_after(const SpgFeed &f) { return (f.t0 + f.nseg) / f.R; }

// analysed segments one feed of max_samples samples can complete (the segment under way may lack one sample only), and from that the
// smallest ring: a power of two of at least the lines such a feed can complete - R - 1 segments of a line may be carried - plus one
inline uint64_t spg_feed_segments(uint64_t max_samples, uint32_t N, uint32_t stride) {
	const uint64_t segs = (max_samples + N - 1) / N;
	return (segs + stride - 1) / stride;
}
inline uint64_t spg_ring_min(uint64_t feed_segments, uint32_t R) {
	const uint64_t need = (feed_segments + R - 1) / R + 1;
	uint64_t p = 1;
	while(p < need) p <<= 1;
	return p;
}

}  // namespace vdl2
