// mark_ahead_host.cpp - TEST INFRASTRUCTURE (tests/test_mark_ahead_host.py builds and runs it; never linked into libvdl2hip.so).
// A stand-alone host program: the source of the walker and the burst decoder (dumpvdl2_amd/csrc/vdl2_core.h, through the host
// simulation tests/hostsim/hostsim.cpp) walks a decimated stream feed by feed, and every burst descriptor that comes out is given to
//   A  the burst decoder's first pass (decode_burst with a BurstDefer of pass 1 and nothing scanned yet): the pieces it lists;
//   B  the marking step on its own (burst_mark + burst_piece_range, as k_burst_mark calls them): the pieces of its mask.
// A is printed, a line per burst with marked symbols, and must be the same as B, burst for burst (exit status 1 if not).  The test
// compares the printed lines with tests/golden/mark_ahead_*.txt - what route A printed BEFORE the marking step was factored out of
// decode_burst (this file compiled with -DMARK_AHEAD_BASELINE, which leaves route B out, against that older vdl2_core.h).
//
// Input (argv[1]): int32 nchan, nfeeds, seg_min, seg_max; float max_ppm; int32 wide_back; int64 D; uint32 freqs[nchan];
// int64 feed_len[nfeeds]; float trace[nchan][D][2] - the oracle's decimated stream, which is both y and the referee's exact samples
// (so a scan changes nothing and every route sees the same y).  wide_back > 0: one more, made-up descriptor - the last burst with
// marked symbols, its prev_n moved wide_back samples back, into silence: the one way to a `wide` request (a real burst is too short).
#include <cstdint>
#include "hostsim.cpp"

struct Piece { int64_t lo, hi; bool operator==(const Piece &o) const { return lo == o.lo && hi == o.hi; } };

int main(int argc, char **argv) {
	if(argc < 2) { fprintf(stderr, "usage: %s input.bin\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if(!f) { perror(argv[1]); return 2; }
	int32_t hdr[4]; float max_ppm; int32_t wide_back; int64_t D;
	if(fread(hdr, 4, 4, f) != 4 || fread(&max_ppm, 4, 1, f) != 1 || fread(&wide_back, 4, 1, f) != 1 || fread(&D, 8, 1, f) != 1) return 2;
	const int nchan = hdr[0], nfeeds = hdr[1];
	if(nchan < 1 || nchan > 64 || nfeeds < 1 || nfeeds > 4096 || D < 1 || D > (1 << 22)) return 2;
	std::vector<uint32_t> freqs(nchan); std::vector<int64_t> flen(nfeeds); std::vector<float> tr((size_t)nchan * D * 2);
	if(fread(freqs.data(), 4, nchan, f) != (size_t)nchan || fread(flen.data(), 8, nfeeds, f) != (size_t)nfeeds || fread(tr.data(), 4, tr.size(), f) != tr.size()) return 2;
	fclose(f);
	int cap_log2 = 10; while((1ll << cap_log2) < D + 70000) cap_log2++;
	Sim *s = hostsim_create(nchan, freqs.data(), max_ppm, cap_log2);
	hostsim_set_exact(s, tr.data(), D);
	if(hdr[2] > 0) hostsim_set_segments(s, hdr[2], hdr[3]);

	// the descriptors, each with the first sample of the feed that handed it over
	std::vector<int64_t> feed_k0;
	std::vector<float> part;
	int64_t k = 0;
	for(int i = 0; i < nfeeds; i++) {
		const int64_t n = flen[i];
		if(n < 1 || k + n > D) return 2;
		part.resize((size_t)nchan * n * 2);
		for(int c = 0; c < nchan; c++) memcpy(&part[(size_t)c * n * 2], &tr[((size_t)c * D + k) * 2], (size_t)n * 8);
		if(hostsim_feed(s, part.data(), n) < 0) { fprintf(stderr, "hostsim output overflow\n"); return 2; }
		feed_k0.resize(s->all_bursts.size(), k);
		k += n;
	}
	std::vector<Burst> bursts = s->all_bursts;

	// the ring as the channeliser leaves it: the stream itself (the decoder's scans above wrote the same values over it)
	std::vector<RefChan> rc(nchan);
	for(int c = 0; c < nchan; c++) rc[c] = RefChan{ s->exact.data() + (size_t)c * D * 2, D, &s->y[(size_t)c * s->cap], s->mask, 0, 0, nullptr };   // (no `done` map: nothing counts as scanned before)
	std::vector<OutFrame> frames(4096); std::vector<uint8_t> pool(1 << 20); std::vector<unsigned long long> cnt((size_t)nchan * kNumCounters);
	std::vector<uint32_t> dq(16); std::vector<ScanReq> sq(256);
	static BurstShared sh;
	long n_marked = 0, n_redo = 0, n_prevfeed = 0, n_wide = 0, n_bad = 0, n_pieces = 0;
	int last_marked = -1;
	const size_t nreal = bursts.size();
	for(size_t i = 0; i < bursts.size(); i++) {
		const Burst b = bursts[i];
		const int c = b.chan;
		ChanView v{ &s->y[(size_t)c * s->cap], nullptr, nullptr, s->mask };
		v.ref = &rc[c]; v.ref_chan = c;
		// A: the first pass
		OutCtl ctl; memset(&ctl, 0, sizeof ctl);
		ctl.cap_frames = (uint32_t)frames.size(); ctl.cap_pool = (uint32_t)pool.size();
		ctl.nframes = burst_reserve_initial_frames(1); ctl.pool_used = burst_reserve_initial_pool(1);
		burst_shared_init(s->T, 0, &ctl, sh);
		uint32_t dq_n = 0, sq_n = 0;
		BurstDefer df{ dq.data(), &dq_n, (uint32_t)dq.size(), sq.data(), &sq_n, (uint32_t)sq.size(), 1 };
		const int64_t calls0 = rc[c].calls;
		decode_burst(b, freqs[c], s->T, v, &cnt[(size_t)c * kNumCounters], frames.data(), pool.data(), &ctl, sh, &df, (uint32_t)i);
		burst_reserve_done(frames.data(), sh);
		if(rc[c].calls != calls0 || sq_n > sq.size() || dq_n > 1 || (dq_n == 0) != (sq_n == 0)) { printf("BAD burst %zu: the first pass scanned or its lists ran over (%u, %u)\n", i, dq_n, sq_n); n_bad++; continue; }
		std::vector<Piece> A;
		for(uint32_t j = 0; j < sq_n; j++) { if(sq[j].chan != c || sq[j].kind != REF_SYMBOLS) n_bad++; A.push_back(Piece{ sq[j].lo, sq[j].hi }); }
		bool redo = false, wide = false;
#ifndef MARK_AHEAD_BASELINE
		// B: the marking step on its own
		BurstMarks mk;
		burst_mark(b, v, sh, mk);
		std::vector<Piece> B;
		if(mk.mfirst != 0xffffffffu) {
			for(int q = 0; q < 128; q++) {
				if(!((sh.u_pm[q >> 5] >> (q & 31)) & 1u)) continue;
				int64_t lo, hi;
				burst_piece_range(mk, q, q, lo, hi);
				B.push_back(Piece{ lo, hi });
			}
			redo = mk.redo_slope; wide = mk.wide;
		}
		if(!(A == B)) { printf("MISMATCH burst %zu chan %d sync %lld: first pass %zu pieces, marking step %zu\n", i, c, (long long)b.sync_sample, A.size(), B.size()); n_bad++; }
		if(i >= nreal && !wide) { printf("BAD: the made-up burst is not wide\n"); n_bad++; }
#else
		redo = b.vdphi_err > 0.f; wide = i >= nreal;
#endif
		if(!A.empty() && i < nreal) last_marked = (int)i;
		if(i + 1 == nreal && wide_back > 0 && last_marked >= 0 && bursts[last_marked].t_first - wide_back >= 0) {
			Burst w = bursts[last_marked];
			w.prev_n = w.t_first - wide_back;
			bursts.push_back(w);
		}
		if(A.empty()) continue;
		const bool prevfeed = b.prev_n >= 0 && i < nreal && b.prev_n < feed_k0[i];
		n_marked++; n_redo += redo; n_prevfeed += prevfeed; n_wide += wide; n_pieces += (long)A.size();
		printf("B %d %lld %lld %d %lld %d %d %d |", c, (long long)b.sync_sample, (long long)b.t_first, b.nsym, (long long)b.prev_n, redo ? 1 : 0, prevfeed ? 1 : 0, wide ? 1 : 0);
		for(const Piece &p : A) printf(" %lld:%lld", (long long)p.lo, (long long)p.hi);
		printf("\n");
	}
	printf("SUMMARY bursts %zu marked %ld pieces %ld redo_slope %ld prev_n_in_previous_feed %ld wide %ld bad %ld\n", nreal, n_marked, n_pieces, n_redo, n_prevfeed, n_wide, n_bad);
	hostsim_destroy(s);
	return n_bad ? 1 : 0;
}
