// specgram_plan_host.cpp - the spectrogram's plan of a feed (dumpvdl2_amd/csrc/specgram_plan.h) against brute force, on the CPU.
// A stand-alone program (tests/test_specgram_plan.py builds it with -fsanitize=address,undefined): random streams of feeds, and the
// edges R = 1, no segment, a feed that completes no line, a feed that completes more than 1024 lines.  For every feed it checks
//   - every analysed segment is taken exactly once, in order, by the workgroups in index order; the split keeps the workgroup limit;
//   - what spg_run() says of a run - head, whole lines, tail - is what a walk over its segments finds; no workgroup has more than
//     two pieces, each piece is one stretch of one line;
//   - walking the workgroups in order (as k_specgram_combine does) from the carried count, the pieces of a line come in ascending
//     segment order and close the line exactly where it ends; every line the feed completes is written once, to slot l mod ring_lines,
//     and no two lines of one feed share a slot;
// and for every stream that the lines assembled over its feeds are those of the whole stream in one feed: line l = segments
// [l R, (l + 1) R) in order.  Prints "ok <tuples> <feeds>" or the first failure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>
#include "specgram_plan.h"

using namespace vdl2;

static int fails = 0;
#define CHECK(cond, ...) do { if(!(cond)) { if(fails++ < 10) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while(0)

struct Line { uint64_t next; uint32_t slot; int writes; };     // next: the tap ordinal the line waits for; written `writes` times

// one feed of nseg analysed segments after t0 seen; lines: what the stream has assembled so far (carried between feeds)
static void check_feed(uint64_t t0, uint64_t nseg, uint32_t R, uint32_t ring, uint32_t max_rows, std::map<uint64_t, Line> &lines, uint64_t &carry_n) {
	const SpgFeed f = spg_feed(t0, nseg, R, ring, max_rows);
	CHECK(f.grid >= 1 && f.grid <= max_rows && f.run >= 1, "grid %u run %u", f.grid, f.run);
	CHECK((uint64_t)f.grid * f.run >= nseg && (nseg == 0 || (uint64_t)(f.grid - 1) * f.run < nseg), "split of %" PRIu64, nseg);
	CHECK(carry_n == t0 % R, "carry %" PRIu64, carry_n);
	uint64_t next_m = 0, cnt = carry_n;
	std::map<uint32_t, uint64_t> slot_of;                      // ring slots this feed writes -> line
	auto write_line = [&](uint64_t l, bool by_workgroup) {
		(void)by_workgroup;
		const uint32_t slot = (uint32_t)(l & f.ring_mask);
		CHECK(slot == l % ring, "slot");
		CHECK(!slot_of.count(slot), "two lines of one feed in slot %u", slot);
		slot_of[slot] = l;
		lines[l].writes++; lines[l].slot = slot;
	};
	auto take = [&](uint64_t l, uint64_t first, uint32_t n) {  // a stretch of line l: must be what the line waits for
		auto it = lines.find(l);
		if(it == lines.end()) { CHECK(first == l * R, "line %" PRIu64 " begins at %" PRIu64, l, first); it = lines.emplace(l, Line{ l * R, 0, 0 }).first; }
		CHECK(it->second.next == first, "line %" PRIu64 " waits for %" PRIu64 ", gets %" PRIu64, l, it->second.next, first);
		it->second.next = first + n;
		CHECK(it->second.next <= (l + 1) * R, "line %" PRIu64 " overruns", l);
	};
	for(uint32_t g = 0; g < f.grid; g++) {
		const SpgRun r = spg_run(f, g);
		if(nseg == 0) { CHECK(r.m0 == r.m1 && !r.head_n && !r.whole_n && !r.tail_n, "an empty feed has a run"); continue; }
		CHECK(r.m0 == next_m && r.m1 > r.m0 && r.m1 <= nseg, "run %u: [%u, %u) after %" PRIu64, g, r.m0, r.m1, next_m);
		next_m = r.m1;
		// brute force over the run's segments
		const uint64_t s = t0 + r.m0, e = t0 + r.m1;
		uint32_t head = 0, tail = 0; uint64_t whole_segs = 0, head_line = 0, tail_line = 0, whole_first = UINT64_MAX, whole_last = 0;
		for(uint64_t t = s; t < e; t++) {
			const uint64_t l = t / R;
			if(l * R < s) { if(head) CHECK(head_line == l, "head over two lines"); head_line = l; head++; }
			else if((l + 1) * R > e) { if(tail) CHECK(tail_line == l, "tail over two lines"); tail_line = l; tail++; }
			else { whole_segs++; if(l < whole_first) whole_first = l; if(l > whole_last) whole_last = l; }
		}
		CHECK(r.head_n == head && r.tail_n == tail && (uint64_t)r.whole_n * R == whole_segs, "run %u: head %u/%u whole %u/%" PRIu64 " tail %u/%u", g, r.head_n, head, r.whole_n, whole_segs, r.tail_n, tail);
		if(head) CHECK(r.head_line == head_line, "head line");
		if(whole_segs) CHECK(r.whole_first == whole_first && whole_last == whole_first + r.whole_n - 1, "whole lines");
		if(tail) CHECK(r.whole_first + r.whole_n == tail_line, "tail line");
		CHECK(r.to_boundary == (s % R ? R - s % R : 0), "to_boundary");
		// the combine kernel's walk
		if(r.head_n) {
			take(r.head_line, s, r.head_n);
			cnt += r.head_n;
			CHECK(cnt <= R, "carry overruns a line");
			if(cnt == R) { CHECK(lines[r.head_line].next == (r.head_line + 1) * R, "line closed early"); write_line(r.head_line, false); cnt = 0; }
			else CHECK(!r.whole_n && !r.tail_n, "a head that does not close its line is followed by more");
		}
		for(uint32_t k = 0; k < r.whole_n; k++) { CHECK(cnt == 0, "whole line over a carry"); take(r.whole_first + k, (r.whole_first + k) * R, R); write_line(r.whole_first + k, true); }
		if(r.tail_n) { CHECK(cnt == 0, "tail over a carry"); take(r.whole_first + r.whole_n, (r.whole_first + r.whole_n) * R, r.tail_n); cnt = r.tail_n; }
	}
	CHECK(next_m == nseg, "segments taken %" PRIu64 " of %" PRIu64, next_m, nseg);
	carry_n = cnt;
	const uint64_t l0 = spg_lines_before(f), l1 = spg_lines_after(f);
	CHECK(l0 == t0 / R && l1 == (t0 + nseg) / R && slot_of.size() == l1 - l0, "lines [%" PRIu64 ", %" PRIu64 "): %zu written", l0, l1, slot_of.size());
	CHECK(l1 - l0 < ring, "a feed completes %" PRIu64 " lines, the ring has %u", l1 - l0, ring);
	for(auto &kv : slot_of) CHECK(kv.second >= l0 && kv.second < l1, "a line outside the feed's was written");
}

// the analysed segments complete at stream position pos: ceil(floor(pos / N) / stride)
static uint64_t ordinal(uint64_t pos, uint32_t N, uint32_t stride) { return (pos / N + stride - 1) / stride; }

// a stream from pos0 on, cut into the given feeds: checks every feed, then the lines against the stream in one piece
static void check_stream(uint64_t pos0, const std::vector<uint32_t> &feeds, uint32_t N, uint32_t stride, uint32_t R, uint64_t a0_back, uint32_t max_rows, uint64_t max_len, uint64_t &nfeeds) {
	const uint64_t a0 = ordinal(pos0, N, stride) - (a0_back < ordinal(pos0, N, stride) ? a0_back : 0);     // the tap was enabled a0_back segments ago
	const uint32_t ring = (uint32_t)spg_ring_min(spg_feed_segments(max_len, N, stride), R);
	CHECK((ring & (ring - 1)) == 0, "ring %u", ring);
	std::map<uint64_t, Line> lines;
	uint64_t pos = pos0, carry = (ordinal(pos0, N, stride) - a0) % R;
	// (what the feeds before pos0 left of the line under way)
	if(carry) lines.emplace((ordinal(pos0, N, stride) - a0) / R, Line{ ordinal(pos0, N, stride) - a0, 0, 0 });
	for(uint32_t len : feeds) {
		// the monitor's count of the segments a feed completes and analyses, by brute force
		uint64_t nseg = 0;
		for(uint64_t j = pos / N; j < (pos + len) / N; j++) if(j % stride == 0) nseg++;
		CHECK(nseg == ordinal(pos + len, N, stride) - ordinal(pos, N, stride), "ordinals");
		CHECK(nseg <= spg_feed_segments(max_len, N, stride), "a feed's segments");
		check_feed(ordinal(pos, N, stride) - a0, nseg, R, ring, max_rows, lines, carry);
		pos += len; nfeeds++;
	}
	const uint64_t seen = ordinal(pos, N, stride) - a0, first_line = (ordinal(pos0, N, stride) - a0) / R;
	for(uint64_t l = first_line; l < seen / R; l++) {
		auto it = lines.find(l);
		CHECK(it != lines.end() && it->second.writes == 1 && it->second.next == (l + 1) * R && it->second.slot == l % ring, "line %" PRIu64 " of the stream", l);
	}
	for(auto &kv : lines) if(kv.first >= seen / R) CHECK(kv.second.writes == 0 && kv.second.next == seen, "the line under way");
	CHECK(lines.size() == seen / R - first_line + (seen % R ? 1 : 0), "lines %zu", lines.size());
}

int main(int argc, char **argv) {
	const uint32_t tuples = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 3000;
	std::mt19937_64 rng(20250607);
	auto pick = [&](std::initializer_list<uint32_t> v) { return v.begin()[rng() % v.size()]; };
	const uint64_t max_len = 300000;
	uint64_t nfeeds = 0;
	// the edges, each against one feed and against a cut
	check_stream(0, { 300000 }, 64, 1, 1, 0, 1024, max_len, nfeeds);                       // R = 1, more than 1024 lines (4687), several per workgroup
	check_stream(0, { 300000 }, 64, 1, 3, 0, 1024, max_len, nfeeds);                       // more than 1024 lines, runs that straddle them
	check_stream(5, { 0, 10, 40, 8, 1 }, 64, 1, 16, 0, 1024, max_len, nfeeds);             // no segment (and one, at the end)
	check_stream(0, { 64 * 7, 64 * 5, 64 * 3 }, 64, 1, 16, 0, 1024, max_len, nfeeds);      // a feed that completes no line (7, 12, then 15 of 16)
	check_stream(0, { 64 * 1500 }, 64, 1, 1000, 0, 1024, max_len, nfeeds);                 // many workgroups, a piece of one line each
	check_stream(1000, { 64 * 1100 }, 64, 1, 1000, 17, 7, max_len, nfeeds);                // few workgroups
	for(uint32_t i = 0; i < tuples; i++) {
		const uint32_t N = pick({ 64, 1024, 4096 }), stride = 1 + (uint32_t)(rng() % 5), R = pick({ 1, 2, 3, 16, 1000 });
		const uint32_t max_rows = pick({ 1, 2, 3, 7, 64, 1000, 1024, 1024 });
		const uint64_t pos0 = rng() % 3 ? rng() % (20ull * N * stride) : (1ull << 40) + rng() % (1ull << 33);
		const uint64_t a0_back = rng() % 2 ? 0 : rng() % 2000;
		std::vector<uint32_t> feeds;
		const int nf = 1 + (int)(rng() % 5);
		for(int k = 0; k < nf; k++) {
			const uint32_t kind = (uint32_t)(rng() % 4);
			feeds.push_back(kind == 0 ? (uint32_t)(rng() % (max_len + 1)) : kind == 1 ? (uint32_t)(rng() % (3 * N)) : kind == 2 ? (uint32_t)(rng() % (2ull * N * stride * R < max_len ? 2ull * N * stride * R : max_len)) : (uint32_t)max_len);
		}
		check_stream(pos0, feeds, N, stride, R, a0_back, max_rows, max_len, nfeeds);
		// ... and the same stretch of stream in one feed, where it fits
		uint64_t total = 0;
		for(uint32_t len : feeds) total += len;
		if(total <= max_len) check_stream(pos0, { (uint32_t)total }, N, stride, R, a0_back, max_rows, max_len, nfeeds);
	}
	if(fails) { printf("failed: %d\n", fails); return 1; }
	printf("ok %u %" PRIu64 "\n", tuples, nfeeds);
	return 0;
}
