// debug_hooks.inc - included at the end of vdl2hip.hip (uses its file-local helpers: collect_pending, launch_scans, HIPCHK ...).
// Every vdl2hip_debug_* entry point: the hooks the tests and the measurement scripts reach the library's pieces through.  None is
// declared in vdl2hip.h.  What a hook allocates it holds in DevBuf / Event locals (hostmem.h): every way out releases everything.

// What the hooks below say three times over each: was the call good, a host block to a buffer (all of it, or its first `bytes`), a
// buffer filled with a byte, a buffer back to the host, the decoder's tables built and sent
static bool hip_ok(hipError_t e) { return e == hipSuccess; }
#include <random>
template<typename T> static bool dbg_up(const DevBuf<T> &d, const void *src, size_t bytes) { return hip_ok(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice)); }
template<typename T> static bool dbg_up(const DevBuf<T> &d, const void *src) { return dbg_up(d, src, d.bytes()); }
template<typename T> static bool dbg_fill(const DevBuf<T> &d, int v) { return hip_ok(hipMemset(d, v, d.bytes())); }
template<typename T> static bool dbg_down(void *dst, const DevBuf<T> &d, size_t bytes) { return hip_ok(hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost)); }
template<typename T> static bool dbg_down(void *dst, const DevBuf<T> &d) { return dbg_down(dst, d, d.bytes()); }
static bool dbg_tables(const DevBuf<Tables> &d) { auto tab = std::make_unique<Tables>(); build_tables(*tab); return dbg_up(d, tab.get()); }

// Builds with a VDL2_*_PROF switch (kernels.h): the kernel's per-slot counters, [64][K] in a device symbol, summed over the slots
// into out[K], and set back to zero if asked
template<int K> static int prof_read(const void *symbol, unsigned long long *out, int reset) {
	unsigned long long h[64][K];
	if(hipMemcpyFromSymbol(h, symbol, sizeof h) != hipSuccess) return -3;
	for(int k = 0; k < K; k++) { out[k] = 0; for(int s = 0; s < 64; s++) out[k] += h[s][k]; }
	if(reset) { memset(h, 0, sizeof h); if(hipMemcpyToSymbol(symbol, h, sizeof h) != hipSuccess) return -3; }
	return 0;
}

extern "C" {

// test hook (not declared in vdl2hip.h; host only, needs no receiver and no GPU): what the process holds through the owners of
// hostmem.h right now -> out = { device buffers, page-locked buffers, events }
int vdl2hip_debug_live_resources(long long out[3]) {
	if(!out) return VDL2HIP_E_INVAL;
	for(int i = 0; i < 3; i++) out[i] = hostmem::g_live[i].load();
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_parity.py): "no_fuse" = run the segment-start fix-up as the separate kernel
// k_fixup instead of inside K1 (bit-identical results); "force_timeout" = make every look-back hand-off fail (producers publish
// under a wrong epoch), so that the fall-back path is taken by every workgroup and can be tested
int vdl2hip_debug_option(vdl2hip_ctx *c, const char *name, long value) {
	if(!c || !name) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	if(strcmp(name, "no_fuse") == 0) { c->fuse_k2 = value == 0; return VDL2HIP_OK; }
	if(strcmp(name, "force_timeout") == 0) { c->debug_force_timeout = value != 0; return VDL2HIP_OK; }
	if(strcmp(name, "force_mismatch") == 0) { c->debug_force_mismatch = value != 0; return VDL2HIP_OK; }   // every channel walked again with the next feed's walk already done is taken to have ended differently: the next feed is redone for it
	if(strcmp(name, "walk_ahead_below") == 0) { c->walk_ahead_below = (double)value; c->walk_ahead_auto = true; return VDL2HIP_OK; }   // (tests: feeds of fewer channel-samples than this let the next walk go ahead)
	if(strcmp(name, "mark_cap") == 0) { if(value < 0 || value > (long long)kDeferScansMax) return VDL2HIP_E_INVAL; c->debug_mark_cap = (uint32_t)value; return VDL2HIP_OK; }   // the list of pieces marked ahead of the check (k_burst_mark) holds at most this many (0: as sized): what runs over goes the burst decoder's own list-and-second-pass way
	if(strcmp(name, "walk_ahead") == 0) { if(value != 0 && value != 1) return VDL2HIP_E_INVAL; c->walk_ahead = (int)value; c->walk_ahead_auto = false; return VDL2HIP_OK; }   // 1: the next feed's walk goes ahead of a feed's check, for every feed; 0: a feed's walk waits for the check of the feed before (round 5's schedule)
	if(strcmp(name, "exact_tier") == 0) { if(value != 0 && value != 1) return VDL2HIP_E_INVAL; c->debug_exact_tier = (int)value; return VDL2HIP_OK; }   // 1 (default): the exact sync tier's dense form, k_sync_dense; 0: the word-at-a-time form it replaced, k_sync_exact4 (bit-identical results)
	if(strcmp(name, "screen_all") == 0) { c->debug_screen_all = value != 0; return VDL2HIP_OK; }   // the screening tier flags every sample (flags are only ever conservative: same frames), so that the exact tier runs at its worst-case density
	if(strcmp(name, "force_again") == 0) { c->debug_force_again = value != 0; return VDL2HIP_OK; }   // every channel of every long feed is stitched a second time (the referee's walk-again path)
	if(strcmp(name, "referee") == 0) { if(value && !c->d_refhist) return VDL2HIP_E_INVAL; c->referee = value != 0; return VDL2HIP_OK; }   // (on only where it was on at create: the history ring)
	if(strcmp(name, "ref_warm") == 0) { if(value < 0 || value > c->ref_T - 4096) return VDL2HIP_E_INVAL; c->ref_warm = value; return VDL2HIP_OK; }
	return VDL2HIP_E_INVAL;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_position.py; host code only - no kernel and no kernel argument knows of it): a
// receiver that has not been fed becomes one whose stream BEGINS at input sample n, at rest - not one that was silent before n.  Every
// position the receiver keeps is an absolute index since the stream began (n_total / K1Args::n0 and the NCO phase taken from it, k_total /
// k0, the walker's a, e, e0 and intervals, Burst::t_first / sync_sample / end_sample / prev_n, the evaluation log, ScanReq::lo / hi,
// RefPiece::s0, the cache of finished stretches, nbase, the taps' k_on): the tests start it hours in, past 2^31 and 2^32, this way.
//   n_total = n, k_total = K = n / os; every channel's WalkState - and every snapshot copy the walk-ahead path keeps (d_ws_snap[], d_ws_tmp) -
//   is walk_state_init()'s with a = K, e = e0 = K + 2; noise floor, evaluation counts, burst ordinals, counters stay at their initial values.
//   Taps enabled afterwards take their k_on from k_total, as ever.
// What lies before n is rest, and the code must see that:
//   - at position 0 "before the stream" is a negative index (ChanView::Phi, ref_eps2, the walker's history taps, Burst::prev_n == -1,
//     txs_range, the scans' n_lo < 0 / s_beg < 0); at n none of those branches is taken, the code reads ring slots (K - j) & mask instead.
//     d_y, d_pf, d_cand and d_flag are zero from vdl2hip_create (DEV_ALLOC(..., true)) and nothing has written them before the first feed,
//     and phase_of({+0, +0}) is +0.0f in both builds (device: atan2_f64's !(mx > 0) branch, copysign(0.0, +0.0); host: libm's
//     atan2(+0, +0)), phase_fast({0, 0}) is 0 likewise: the slots read as position 0's "before the stream" does.  The walker's first
//     evaluation of a run cannot fire and it never reads pf[] before e0 = K + 2, so the zero metric values before K are never looked at.
//     One difference: ref_eps2() of a zero sample INSIDE the stream is kRefBig where position 0 has 0 - windows whose taps reach before
//     K are "cannot tell" and go to the referee, which decides them on the reference's own samples: the same frames, more scans in the
//     first 150 decimated samples.  Burst::prev_n may be K - 1 where position 0 has -1 (the phase there is 0 either way).
//   - the referee's scans know the start of the stream from s_beg < 0 at position 0: they begin there in the reference's state, zero,
//     exactly, and k_ref_scan_multi's witness with them.  At n a scan cannot know, so the history ring gets min(n, ref_T) raw samples
//     registered as the one piece { s0 = n - that, that many }, ref_wp behind them: seeded noise of a few percent of full scale, then
//     kPosQuiet samples of zeros up to n.  Over the zeros the recursion decays (0.985 per input sample at oversample 20) through the
//     subnormal range, where it comes to a stop at 1e-41 or less - not at 0 exactly: (B1 + B2) k rounds to k for small k - and a state
//     of 1e-41 is absorbed by the first addition of a sample's A0 x (1e-9 for one count of S16), so the stretch comes out bit for bit as
//     from rest (tests/test_gpu_position.py reads the first samples after n back).  Zeros alone would do that too, but the witness
//     (started from another state wherever s_beg > 0) could not meet a scan that stays at 0 exactly while its own state stops in the
//     subnormals: every scan whose run-up lies in the zeros was counted as unmet and run again (measured: 24 of 116 scans of an
//     8-channel capture of 1 s fed whole, none at position 0).  Over the noise the two meet as they do anywhere in a stream and stay
//     together through the zeros.  That holds for the formats whose all-zero code is the sample 0 (S16, S8, CF32).  FMT_U8 has no such
//     code ((b - 127.5) / 127.5) and no history of bytes leaves every channel's filter at rest: a U8 receiver takes a position only with
//     the referee switched off (debug_option "referee" 0) - its channeliser, walker, noise floor and burst decoder are then held at large
//     indices, its scans are not.
// Refused (VDL2HIP_E_INVAL): a receiver that has been fed or has anything carried or queued, or whose activity monitor is on already; n
// not a multiple of the oversampling; a receiver that resamples (cfg.input_rate) - K0's position pair (q0, t0) is not set by this hook; a
// receiver of unsigned bytes whose referee is on.
int vdl2hip_debug_set_position(vdl2hip_ctx *c, uint64_t n) {
	if(!c || c->failed || c->feed_no != 0 || c->ncarry != 0 || c->n_total != 0 || c->k_total != 0 || !c->queue.empty() || !c->ref_pieces.empty()) return VDL2HIP_E_INVAL;
	if(c->rs.on || c->act.on || n % (uint64_t)c->os != 0 || n > (1ull << 60) || (c->fmt == kFmtU8 && c->referee)) return VDL2HIP_E_INVAL;      // (an activity monitor that is on has taken its k_on already)
	OnDevice dev_guard(c);
	const int64_t K = (int64_t)(n / (uint64_t)c->os);
	std::vector<WalkState> ws((size_t)c->C);
	for(auto &w : ws) { memset(&w, 0, sizeof w); walk_state_init(w); w.a = K; w.e = w.e0 = K + 2; }
	const size_t wb = ws.size() * sizeof(WalkState);
	HIPCHK(hipMemcpy(c->d_ws, ws.data(), wb, hipMemcpyHostToDevice));
	for(auto *d : { &c->d_ws_snap[0], &c->d_ws_snap[1], &c->d_ws_tmp }) if(d->get()) HIPCHK(hipMemcpy(d->get(), ws.data(), wb, hipMemcpyHostToDevice));
	if(c->d_refhist && c->referee) {
		const uint64_t w = std::min<uint64_t>(n, (uint64_t)c->ref_T);      // (ref_T < ref_cap: the piece does not wrap)
		if(w) {
			constexpr uint64_t kPosQuiet = 32768;                             // zeros up to n: hundreds of decay times of the filter at any oversampling up to 32
			const size_t sb = raw_bytes(c->fmt);
			const uint64_t noisy = w > kPosQuiet ? w - kPosQuiet : 0;
			std::vector<uint8_t> h((size_t)w * sb, 0);
			std::mt19937 rng(20950u);
			for(uint64_t i = 0; i < 2 * noisy; i++) {                        // (I and Q of every sample)
				const int v = (int)(rng() % 2001u) - 1000;                    // +-1000 counts of S16: 3 % of full scale
				if(c->fmt == kFmtS16) { const int16_t q = (int16_t)v; memcpy(&h[2 * i], &q, 2); }
				else if(c->fmt == kFmtS8) h[i] = (uint8_t)(int8_t)(v / 32);
				else { const float q = (float)v / 32768.0f; memcpy(&h[4 * i], &q, 4); }
			}
			HIPCHK(hipMemcpy(c->d_refhist, h.data(), h.size(), hipMemcpyHostToDevice));
			c->ref_pieces.push_back(vdl2hip_ctx::HistPiece{ (int64_t)(n - w), (int64_t)w, 0 });
			c->ref_wp = w % c->ref_cap;
		}
	}
	HIPCHK(hipDeviceSynchronize());
	c->n_total = n; c->k_total = K;
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h): the referee's scan on [n_lo, n_hi] of one channel, with the raw input the most recent feed could
// reach - the decimated stream there is then the reference's own, to be read back with vdl2hip_read_decimated().  1: done, 0: refused
int vdl2hip_debug_exact_window_many(vdl2hip_ctx *c, uint32_t chan, int64_t n_lo, int64_t n_hi, uint32_t count, int64_t stride, float *ms) {
	if(!c || !c->d_refhist || chan >= (uint32_t)c->C || c->feed_no == 0 || count == 0 || count > 65536) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	DevBuf<int> d_out; std::vector<int> h(count, 0);
	if(!hip_ok(d_out.alloc(count))) return VDL2HIP_E_NOMEM;
	Event e0, e1;
	if(!hip_ok(e0.ensure()) || !hip_ok(e1.ensure())) return VDL2HIP_E_DEVICE;
	hipExtLaunchKernelGGL(k_ref_probe, dim3(count), dim3(64), 0, c->streams.front, e0, e1, 0, c->d_ref[(c->feed_no - 1) % kSlots].get(), (int)chan, c->C, n_lo, n_hi, stride, d_out.get());
	if(!hip_ok(hipStreamSynchronize(c->streams.front)) || !dbg_down(h.data(), d_out)) return VDL2HIP_E_DEVICE;
	if(ms) { float t = 0.f; (void)hipEventElapsedTime(&t, e0, e1); *ms = t; }
	int n = 0; for(int v : h) n += v;
	return n;            // stretches done (of `count`)
}
// test hook (not declared in vdl2hip.h): the same through k_ref_scan_multi - `count` stretches (chan[i], lo[i], hi[i]) side by side;
// returns the number of scans run, *ms = the kernels' time.  with_retry: as the product's launches do it - the scans that have not met
// their witness are listed and run again from ref_retry_mul times further back (without: they are counted as unmet and published)
int vdl2hip_debug_scan_multi2(vdl2hip_ctx *c, const int32_t *chan, const int64_t *lo, const int64_t *hi, uint32_t count, int with_retry, float *ms) {
	if(!c || !c->d_refhist || c->feed_no == 0 || count == 0 || count > 65536 || !chan || !lo || !hi) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	std::vector<ScanReq> h(count);
	for(uint32_t i = 0; i < count; i++) { if(chan[i] < 0 || chan[i] >= c->C) return VDL2HIP_E_INVAL; h[i] = ScanReq{ chan[i], REF_CANDIDATE, lo[i], hi[i] }; }
	DevBuf<ScanReq> d_sq, d_rt; DevBuf<uint32_t> d_n;
	if(!hip_ok(d_sq.alloc(count)) || !hip_ok(d_n.alloc(2)) || !hip_ok(d_rt.alloc(kRetryScans))) return VDL2HIP_E_NOMEM;
	uint32_t before[8] = {0}, after[8] = {0};
	const uint32_t nn[2] = { count, 0u };
	Event e0, e1;
	if(!hip_ok(e0.ensure()) || !hip_ok(e1.ensure()) || !dbg_up(d_sq, h.data()) || !dbg_up(d_n, nn) || !dbg_down(before, c->d_refstats, sizeof before)) return VDL2HIP_E_DEVICE;
	RefChan *ref = c->d_ref[(c->feed_no - 1) % kSlots];
	launch_scans(c, c->streams.front, ref, 0xfffeu, d_sq, nullptr, d_n, count, c->k_total, with_retry ? d_rt.get() : nullptr, d_n + 1, e0, e1);
	if(!hip_ok(hipStreamSynchronize(c->streams.front)) || !dbg_down(after, c->d_refstats, sizeof after)) return VDL2HIP_E_DEVICE;
	if(ms) { float t = 0.f; (void)hipEventElapsedTime(&t, e0, e1); *ms = t; }
	return (int)(after[0] - before[0]);
}
int vdl2hip_debug_exact_window(vdl2hip_ctx *c, uint32_t chan, int64_t n_lo, int64_t n_hi) { return vdl2hip_debug_exact_window_many(c, chan, n_lo, n_hi, 1, 0, nullptr); }

// test hook (not declared in vdl2hip.h): what the DPP controls the channeliser's scan relies on do on this device
int vdl2hip_debug_u8_levels(float out[512]) {        // out[0..255]: the channeliser's division-free (i - 127.5) / 127.5, out[256..511]: the division (tests)
	DevBuf<float> d;
	if(!hip_ok(d.alloc(512))) return VDL2HIP_E_NOMEM;
	hipLaunchKernelGGL(k_u8_level_probe, dim3(1), dim3(256), 0, 0, d);
	return dbg_down(out, d) ? VDL2HIP_OK : VDL2HIP_E_DEVICE;
}

int vdl2hip_debug_s8_levels(float out[512]) {        // out[0..255]: s8_level() of the byte patterns 0..255, out[256..511]: (float)(int8_t)i / 128.0f the plain way (tests)
	DevBuf<float> d;
	if(!hip_ok(d.alloc(512))) return VDL2HIP_E_NOMEM;
	hipLaunchKernelGGL(k_s8_level_probe, dim3(1), dim3(256), 0, 0, d);
	return dbg_down(out, d) ? VDL2HIP_OK : VDL2HIP_E_DEVICE;
}

int vdl2hip_debug_dpp_probe(const float in[64], float out[256]) {
	DevBuf<float> d_in, d_out;
	if(!hip_ok(d_in.alloc(64)) || !hip_ok(d_out.alloc(256))) return VDL2HIP_E_NOMEM;
	if(!dbg_up(d_in, in)) return VDL2HIP_E_DEVICE;
	hipLaunchKernelGGL(k_dpp_probe, dim3(1), dim3(64), 0, 0, (const float *)d_in, d_out);
	return dbg_down(out, d_out) ? VDL2HIP_OK : VDL2HIP_E_DEVICE;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_core_probe.py): the device builds of vdl2_core.h's element-wise pieces on n elements.
// kind 0 phase_of, 1 phase_fast, 2 mag_of: in (re, im), out 1 float; 3 sync_metric: in 16 phases, out (pherr, slope); 4 sync_metric_screen:
// in 16 phases in turns, out (16 taps, kScreenEarly taps); 5 slice_symbol: in (phi, prev_phi, vdphi), out int32 (index, neg);
// 6 parabola_vertex: in (y1, y2, y3), out 1 float; 7 in (vdphi, freq as uint32, max_ppm), out (ppm_of, ppm_gate_threshold); 8 header_to_geometry:
// in a 25-bit header word (uint32), out uint32 (status, syndrome, tl_bits, want_bits); 9 / 10 sync_metric_ref with `full` / without: in 16 phases and
// the 16 ref_eps2() figures of their taps, out (pherr, slope, E, alo, ahi); 11 ref_pherr_range x 3 and ref_candidate_verdict: in (p, alo, ahi, E) of n,
// (p, alo, ahi, E, slope) of n-3, (p, alo, ahi, E) of n-6, max_ppm, the gate's threshold, out (verdict as int32, r0.lo, r0.hi, r3.lo, r3.hi, r6.lo, r6.hi);
// 12 ref_vertex_marginal: in three (lo, hi), out int32 0/1; 13 in (phi, prev_phi, vdphi, e_sum), out (ref_symbol_dist, ref_symbol_marginal as int32).
// Needs no receiver
int vdl2hip_debug_core_probe(int kind, const void *in, size_t n, void *out) {
	if(kind < 0 || kind >= PROBE_KINDS || !in || !out || n == 0 || n > (size_t)1 << 26) return VDL2HIP_E_INVAL;
	DevBuf<float> d_in, d_out; DevBuf<Tables> d_tab;
	if(!hip_ok(d_in.alloc(n * (size_t)core_probe_in_words(kind))) || !hip_ok(d_out.alloc(n * (size_t)core_probe_out_words(kind))) || !hip_ok(d_tab.alloc(1))) return VDL2HIP_E_NOMEM;
	if(!dbg_tables(d_tab) || !dbg_up(d_in, in) || !dbg_fill(d_out, 0)) return VDL2HIP_E_DEVICE;
	hipLaunchKernelGGL(k_core_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, kind, (const float *)d_in, (uint32_t)n, d_out, (const Tables *)d_tab);
	return hip_ok(hipGetLastError()) && dbg_down(out, d_out) ? VDL2HIP_OK : VDL2HIP_E_DEVICE;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_burst_probe.py): the device build of the burst decoder's pieces on n elements, `grid`
// workgroups of kBurstWaves wavefronts (kernels.h: k_burst_probe_wave, k_burst_probe_rs, k_burst_probe).  Needs no receiver.
//   kind 0 (wave primitives)  in uint32 [n][64], out uint32 [n][68]: first flag, flag count, 64 scanned values, their total, the minimum
//   kind 1 (rs_decode_row)    in uint8 [n][256]: 255 octets and npar (0, 2, 4 or 6); out uint8 [n][256]: the row, then int32 [n]: the return value
//   kind 2 (decode_burst)     in Burst [n], element i on ring y[i][ring_len] (cf32, ring_len a power of two), freq [nchan], referee off.  The output
//                             control block starts as a feed's does (the counters behind the wavefronts' own shares) with capacities cap_frames and
//                             cap_pool; behind the records and behind the pool lie guard_frames records and guard_pool octets, everything filled with
//                             0xA5 beforehand.  Returned: frames [cap_frames + guard_frames], pool [cap_pool + guard_pool], ctl (an OutCtl), cnt
//                             [nchan][20]; `out` is not used
int vdl2hip_debug_burst_probe(int kind, const void *in, size_t n, unsigned grid, void *out, const uint32_t *freq, uint32_t nchan, const float *y, uint32_t ring_len,
		uint32_t cap_frames, uint32_t cap_pool, uint32_t guard_frames, uint32_t guard_pool, void *frames, uint8_t *pool, void *ctl, unsigned long long *cnt) {
	if(kind < 0 || kind >= BPROBE_KINDS || !in || n == 0 || n > (size_t)1 << 20 || grid == 0 || grid > 1024) return VDL2HIP_E_INVAL;
	const uint32_t nwaves = grid * (uint32_t)kBurstWaves;
	const bool burst = kind == BPROBE_BURST;
	size_t nin = 0, nout = 0;
	if(kind == BPROBE_WAVE) { nin = n * 64 * 4; nout = n * (size_t)kBProbeWaveOut * 4; }
	else if(kind == BPROBE_RS) {
		nin = n * (size_t)kBProbeRsStride; nout = n * (size_t)kBProbeRsStride + n * 4;
		for(size_t i = 0; i < n; i++) { const uint8_t np = ((const uint8_t *)in)[i * kBProbeRsStride + kRsN]; if(np > kRsPar || (np & 1)) return VDL2HIP_E_INVAL; }
	} else {
		nin = n * sizeof(Burst);
		if(!freq || nchan == 0 || !y || ring_len < 64 || (ring_len & (ring_len - 1)) || ring_len > 1u << 20 || !frames || !pool || !ctl || !cnt) return VDL2HIP_E_INVAL;
		if(cap_frames > 1u << 20 || cap_pool > 1u << 26 || guard_frames > 1u << 16 || guard_pool > 1u << 20 || n * (size_t)ring_len > (size_t)1 << 26) return VDL2HIP_E_INVAL;
		for(size_t i = 0; i < n; i++) {
			const Burst &b = ((const Burst *)in)[i];
			if(b.chan < 0 || (uint32_t)b.chan >= nchan || b.nsym < 1 || b.nsym > kMaxSyms || b.tl_bits == 0 || b.tl_bits > kMaxTl || b.t_first < 0 || b.prev_n < -2) return VDL2HIP_E_INVAL;
		}
	}
	if(!burst && !out) return VDL2HIP_E_INVAL;
	const size_t nfr = (size_t)cap_frames + guard_frames, npool = (size_t)cap_pool + guard_pool;
	DevBuf<uint8_t> d_in, d_out, d_pool; DevBuf<Tables> d_tab; DevBuf<OutCtl> d_ctl;
	DevBuf<uint32_t> d_freq; DevBuf<cf32> d_y; DevBuf<unsigned long long> d_cnt; DevBuf<OutFrame> d_frames;
	if(!hip_ok(d_in.alloc(nin)) || !hip_ok(d_tab.alloc(1)) || !hip_ok(d_ctl.alloc(1)) || (nout && !hip_ok(d_out.alloc(nout)))) return VDL2HIP_E_NOMEM;
	if(burst && (!hip_ok(d_freq.alloc(nchan)) || !hip_ok(d_y.alloc(n * (size_t)ring_len)) || !hip_ok(d_cnt.alloc((size_t)nchan * kNumCounters))
	             || !hip_ok(d_frames.alloc(nfr + 1)) || !hip_ok(d_pool.alloc(npool + 4)))) return VDL2HIP_E_NOMEM;
	OutCtl h_ctl; memset(&h_ctl, 0, sizeof h_ctl);
	h_ctl.cap_frames = cap_frames; h_ctl.cap_pool = cap_pool;
	h_ctl.nframes = burst_reserve_initial_frames(nwaves); h_ctl.pool_used = burst_reserve_initial_pool(nwaves);     // (kernels.h: reset_out_ctl)
	if(!dbg_tables(d_tab) || !dbg_up(d_in, in) || !dbg_up(d_ctl, &h_ctl) || (nout && !dbg_fill(d_out, 0))) return VDL2HIP_E_DEVICE;
	if(burst && (!dbg_up(d_freq, freq) || !dbg_up(d_y, y) || !dbg_fill(d_cnt, 0) || !dbg_fill(d_frames, 0xA5) || !dbg_fill(d_pool, 0xA5))) return VDL2HIP_E_DEVICE;
	BurstProbeArgs a{ (uint32_t)n, d_tab, d_ctl, (const uint32_t *)d_in.get(), (uint32_t *)d_out.get(), d_in, d_out,
	                  (int32_t *)(d_out.get() + n * (size_t)kBProbeRsStride), (const Burst *)d_in.get(), d_freq, d_y, ring_len, ring_len - 1, d_cnt, d_frames, d_pool };
	const unsigned lds = (unsigned)(sizeof(BurstShared) * kBurstWaves);
	if(kind == BPROBE_WAVE) hipLaunchKernelGGL(k_burst_probe_wave, dim3(grid), dim3(64 * kBurstWaves), lds, 0, a);
	else if(kind == BPROBE_RS) hipLaunchKernelGGL(k_burst_probe_rs, dim3(grid), dim3(64 * kBurstWaves), lds, 0, a);
	else hipLaunchKernelGGL(k_burst_probe, dim3(grid), dim3(64 * kBurstWaves), lds, 0, a);
	if(!hip_ok(hipGetLastError()) || !hip_ok(hipDeviceSynchronize())) return VDL2HIP_E_DEVICE;
	if(nout && !dbg_down(out, d_out)) return VDL2HIP_E_DEVICE;
	if(burst && (!dbg_down(frames, d_frames, nfr * sizeof(OutFrame)) || !dbg_down(pool, d_pool, npool) || !dbg_down(ctl, d_ctl) || !dbg_down(cnt, d_cnt))) return VDL2HIP_E_DEVICE;
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_burst_probe.py): k_frame_finish itself, `grid` workgroups, on the caller's record list
// (nrec records, tombstones - chan < 0 - among them), octet pool, control block (an OutCtl: nframes, cap_frames; nvalid and pool_out_used zero)
// and noise-floor rings ring[nchan][ring_len] (ring_len a power of two).  Returned: frames_out [nrec], pool_out [pool_out_cap] (both 0xA5 where
// nothing was delivered), the whole OutMail (mail_out: sizeof(OutMail) octets, see vdl2hip_debug_sizeof_outmail) and the AVLC counters acnt [nchan][10].
// Needs no receiver
int vdl2hip_debug_sizeof_outmail(void) { return (int)sizeof(OutMail); }
int vdl2hip_debug_frame_finish(unsigned grid, const void *frames_in, uint32_t nrec, const uint8_t *pool, uint32_t pool_len, const void *ctl_in, const float *ring, uint32_t ring_len,
		uint32_t nchan, void *frames_out, uint8_t *pool_out, uint32_t pool_out_cap, void *mail_out, unsigned long long *acnt) {
	if(grid == 0 || grid > 1024 || !ctl_in || !ring || ring_len == 0 || (ring_len & (ring_len - 1)) || ring_len > 1u << 20 || nchan == 0 || nchan > 1024 || !frames_out || !pool_out || !mail_out || !acnt
	   || nrec > 1u << 20 || pool_len > 1u << 28 || (nrec && !frames_in) || (pool_len && !pool)) return VDL2HIP_E_INVAL;
	OutCtl h_ctl; memcpy(&h_ctl, ctl_in, sizeof h_ctl);
	const uint32_t nf = h_ctl.nframes < h_ctl.cap_frames ? h_ctl.nframes : h_ctl.cap_frames;
	if(nf > nrec || h_ctl.nvalid != 0 || h_ctl.pool_out_used != 0) return VDL2HIP_E_INVAL;
	size_t need = 0;
	for(uint32_t i = 0; i < nf; i++) {
		const OutFrame &f = ((const OutFrame *)frames_in)[i];
		if(f.chan < 0) continue;
		if((uint32_t)f.chan >= nchan || f.len > 1u << 20 || (size_t)f.pool_off + f.len > pool_len) return VDL2HIP_E_INVAL;
		need += ((size_t)f.len + 3) & ~(size_t)3;
	}
	if(need > pool_out_cap) return VDL2HIP_E_INVAL;
	DevBuf<OutFrame> d_frames, d_fout; DevBuf<uint8_t> d_pool, d_pout; DevBuf<OutMail> d_mail; DevBuf<Tables> d_tab; DevBuf<float> d_ring; DevBuf<unsigned long long> d_acnt;
	if(!hip_ok(d_frames.alloc((size_t)nrec + 1)) || !hip_ok(d_fout.alloc((size_t)nrec + 1)) || !hip_ok(d_pool.alloc((size_t)pool_len + 4)) || !hip_ok(d_pout.alloc((size_t)pool_out_cap + 4))
	   || !hip_ok(d_mail.alloc(1)) || !hip_ok(d_tab.alloc(1)) || !hip_ok(d_ring.alloc((size_t)nchan * ring_len)) || !hip_ok(d_acnt.alloc((size_t)nchan * kNumAvlcCounters))) return VDL2HIP_E_NOMEM;
	auto mail = std::make_unique<OutMail>(); memset(mail.get(), 0xA5, sizeof(OutMail)); mail->ctl = h_ctl;
	if(!dbg_tables(d_tab) || !dbg_up(d_mail, mail.get()) || (nrec && !dbg_up(d_frames, frames_in, (size_t)nrec * sizeof(OutFrame))) || (pool_len && !dbg_up(d_pool, pool, pool_len))
	   || !dbg_up(d_ring, ring) || !dbg_fill(d_acnt, 0) || !dbg_fill(d_fout, 0xA5) || !dbg_fill(d_pout, 0xA5)) return VDL2HIP_E_DEVICE;
	hipLaunchKernelGGL(k_frame_finish, dim3(grid), dim3(64 * kFrameWaves), 0, 0, d_frames, (const uint8_t *)d_pool, d_mail, (const Tables *)d_tab, d_acnt, (const float *)d_ring, ring_len - 1, d_fout, d_pout);
	if(!hip_ok(hipGetLastError()) || !hip_ok(hipDeviceSynchronize())) return VDL2HIP_E_DEVICE;
	if((nrec && !dbg_down(frames_out, d_fout, (size_t)nrec * sizeof(OutFrame))) || (pool_out_cap && !dbg_down(pool_out, d_pout, pool_out_cap))
	   || !dbg_down(mail_out, d_mail) || !dbg_down(acnt, d_acnt)) return VDL2HIP_E_DEVICE;
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_nf_probe.py): K4b, the noise-floor replay, on the caller's inputs - one call is one feed
// of nchan channels.  y [nchan][ring_len] (cf32, ring_len a power of two), the feed's evaluation logs chunks [nchan][cap_log] (EvalChunk) and
// nlog [nchan], the channels' NfState (nf: nchan * vdl2hip_debug_sizeof_nfstate() octets, in and out) and the history rings ring [nchan][nf_ring]
// (in and out, nf_ring a power of two).  mode 0: k_nf_prepare, k_nf_replay on dim3(grid, nchan), k_nf_finish, as a long feed launches them;
// mode 1: k_nf_all, as a short one does (grid is not used).  The dynamic LDS is the product's; cap_comb is the product's cap_log + kNfTail plus
// a guard of 64 entries behind every channel's row of the two scratch lists.
// Returned besides: lpbuf [nchan][cap_hist] (0xA5 where nothing was written) and the feed records (NfFeed [nchan]).
// Refused (VDL2HIP_E_INVAL) is what the product cannot have: nlog > cap_log, a state that does not add up, a feed with more than cap_hist - 1
// updates, a history ring shorter than cap_hist.  Behind lpbuf, the rings and the two scratch lists lie kNfProbeGuard octets each, and behind every
// channel's rows of the scratch lists the row guard, all filled with 0xA5 beforehand: VDL2HIP_E_DEVICE if any of it has changed (in lpbuf and
// the rings a store beyond a channel's own row lands in the next channel's, which the caller sees in what comes back).  Needs no receiver
int vdl2hip_debug_sizeof_nfstate(void) { return (int)sizeof(NfState); }
int vdl2hip_debug_sizeof_nffeed(void) { return (int)sizeof(NfFeed); }
int vdl2hip_debug_nf_probe(int mode, unsigned grid, uint32_t nchan, const float *y, uint32_t ring_len, const void *chunks, const uint32_t *nlog, uint32_t cap_log,
		void *nf, float *ring, uint32_t nf_ring, uint32_t cap_hist, float *lpbuf, void *feeds) {
	constexpr size_t kNfProbeGuard = 4096;
	if(mode < 0 || mode > 1 || grid == 0 || grid > 64 || nchan == 0 || nchan > 1024 || !y || ring_len < 64 || (ring_len & (ring_len - 1)) || ring_len > 1u << 20 || !chunks || !nlog
	   || cap_log == 0 || cap_log > 1u << 16 || !nf || !ring || nf_ring == 0 || (nf_ring & (nf_ring - 1)) || nf_ring > 1u << 20 || cap_hist < 2 || cap_hist > nf_ring || !lpbuf || !feeds) return VDL2HIP_E_INVAL;
	const EvalChunk *hc = static_cast<const EvalChunk *>(chunks);
	const NfState *hs = static_cast<const NfState *>(nf);
	for(uint32_t c = 0; c < nchan; c++) {
		const NfState &s = hs[c];
		if(nlog[c] > cap_log || s.ntail < 0 || s.ntail > kNfTail || s.evals < 0 || s.tail_ord < 0) return VDL2HIP_E_INVAL;
		int64_t ord = s.tail_ord;
		for(int i = 0; i < s.ntail; i++) { if(s.tail[i].count < 1 || s.tail[i].count > (int64_t)1 << 32 || s.tail[i].first < 0) return VDL2HIP_E_INVAL; ord += s.tail[i].count; }
		if(ord != s.evals) return VDL2HIP_E_INVAL;
		for(uint32_t i = 0; i < nlog[c]; i++) { const EvalChunk &k = hc[(size_t)c * cap_log + i]; if(k.count < 1 || k.count > (int64_t)1 << 32 || k.first < 0) return VDL2HIP_E_INVAL; ord += k.count; }
		if(ord / 1000 - s.evals / 1000 > (int64_t)cap_hist - 1) return VDL2HIP_E_INVAL;
	}
	// (the scratch lists' rows are cap_comb + 1 long in the kernels: the row guard is part of cap_comb here, which changes nothing else -
	// cap_comb only bounds ntail + nlog, and that is kNfTail + cap_log at the most)
	constexpr uint32_t kNfRowGuard = 64;
	const uint32_t cap_comb = cap_log + (uint32_t)kNfTail + kNfRowGuard;
	const size_t nsc = (size_t)nchan * (cap_comb + 1), nlp = (size_t)nchan * cap_hist, nring = (size_t)nchan * nf_ring, gw = kNfProbeGuard / 4, gq = kNfProbeGuard / 8;
	DevBuf<cf32> d_y; DevBuf<NfState> d_nf; DevBuf<EvalChunk> d_log; DevBuf<uint32_t> d_nlog; DevBuf<int64_t> d_scf, d_scc; DevBuf<NfFeed> d_feed; DevBuf<float> d_lp, d_ring;
	if(!hip_ok(d_y.alloc((size_t)nchan * ring_len)) || !hip_ok(d_nf.alloc(nchan)) || !hip_ok(d_log.alloc((size_t)nchan * cap_log)) || !hip_ok(d_nlog.alloc(nchan)) || !hip_ok(d_scf.alloc(nsc + gq))
	   || !hip_ok(d_scc.alloc(nsc + gq)) || !hip_ok(d_feed.alloc(nchan)) || !hip_ok(d_lp.alloc(nlp + gw)) || !hip_ok(d_ring.alloc(nring + gw))) return VDL2HIP_E_NOMEM;
	if(!dbg_up(d_y, y) || !dbg_up(d_nf, nf) || !dbg_up(d_log, chunks) || !dbg_up(d_nlog, nlog) || !dbg_fill(d_scf, 0xA5) || !dbg_fill(d_scc, 0xA5) || !dbg_fill(d_feed, 0xA5) || !dbg_fill(d_lp, 0xA5)
	   || !dbg_fill(d_ring, 0xA5) || !dbg_up(d_ring, ring, nring * sizeof(float))) return VDL2HIP_E_DEVICE;
	K4bArgs a{ d_y, d_nf, d_log, d_nlog, d_scf, d_scc, d_feed, d_lp, d_ring, nf_ring - 1, ring_len, ring_len - 1, cap_log, cap_comb, cap_hist, (int32_t)nchan };
	const unsigned nf_lds = (unsigned)(sizeof(NfShared) * kNfWaves), nf_grid = (unsigned)((nchan + kNfWaves - 1) / kNfWaves);
	if(mode == 0) {
		hipLaunchKernelGGL(k_nf_prepare, dim3(nf_grid), dim3(64 * kNfWaves), nf_lds, 0, a);
		hipLaunchKernelGGL(k_nf_replay, dim3(grid, nchan), dim3(64 * kNfWaves), nf_lds, 0, a);
		hipLaunchKernelGGL(k_nf_finish, dim3(nf_grid), dim3(64 * kNfWaves), nf_lds, 0, a);
	} else hipLaunchKernelGGL(k_nf_all, dim3(nf_grid), dim3(64 * kNfWaves), nf_lds, 0, a);
	if(!hip_ok(hipGetLastError()) || !hip_ok(hipDeviceSynchronize())) return VDL2HIP_E_DEVICE;
	std::vector<uint8_t> g(4 * kNfProbeGuard);
	if(!hip_ok(hipMemcpy(g.data(), d_scf.get() + nsc, kNfProbeGuard, hipMemcpyDeviceToHost)) || !hip_ok(hipMemcpy(g.data() + kNfProbeGuard, d_scc.get() + nsc, kNfProbeGuard, hipMemcpyDeviceToHost))
	   || !hip_ok(hipMemcpy(g.data() + 2 * kNfProbeGuard, d_lp.get() + nlp, kNfProbeGuard, hipMemcpyDeviceToHost))
	   || !hip_ok(hipMemcpy(g.data() + 3 * kNfProbeGuard, d_ring.get() + nring, kNfProbeGuard, hipMemcpyDeviceToHost))) return VDL2HIP_E_DEVICE;
	if(!dbg_down(nf, d_nf) || !dbg_down(ring, d_ring, nring * sizeof(float)) || !dbg_down(lpbuf, d_lp, nlp * sizeof(float)) || !dbg_down(feeds, d_feed)) return VDL2HIP_E_DEVICE;
	for(uint8_t b : g) if(b != 0xA5) return VDL2HIP_E_DEVICE;
	// every channel's rows of the scratch lists: what lies behind the ncomb + 1 entries the channel has is untouched
	std::vector<int64_t> hf(nsc), hcm(nsc);
	if(!dbg_down(hf.data(), d_scf, nsc * sizeof(int64_t)) || !dbg_down(hcm.data(), d_scc, nsc * sizeof(int64_t))) return VDL2HIP_E_DEVICE;
	const NfFeed *hfd = static_cast<const NfFeed *>(feeds);
	for(uint32_t c = 0; c < nchan; c++) {
		if(hfd[c].ncomb > cap_log + (uint32_t)kNfTail) return VDL2HIP_E_DEVICE;
		for(size_t i = (size_t)hfd[c].ncomb + 1; i <= cap_comb; i++)
			if(hf[(size_t)c * (cap_comb + 1) + i] != (int64_t)0xA5A5A5A5A5A5A5A5ull || hcm[(size_t)c * (cap_comb + 1) + i] != (int64_t)0xA5A5A5A5A5A5A5A5ull) return VDL2HIP_E_DEVICE;
	}
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_walk_probe.py): K4, the walker, on the caller's inputs - one call is one feed [k0, k_end) of
// nchan channels.  y and pf [nchan][ring_len] (cf32, ring_len a power of two) and cand [nchan][ring_len / 64] as ChanView defines them, the
// channels' WalkState (ws: nchan * vdl2hip_debug_sizeof_walkstate() octets, in and out) and counters (cnt [nchan][20], in and out).
// mode 0: k_walk; mode 1: k_walk_spec and k_walk_stitch over nseg segments of seglen samples, with the grids, the blocks and the dynamic LDS of
// launch_back() / launch_stitch().  The referee is off (no RefChan, no request list, no snapshots).
// Returned besides: bursts [nchan][cap_bursts_chan] and log [nchan][cap_log] (EvalChunk), both 0xA5 where nothing was written - a store beyond
// a channel's own row lands in the next channel's, which the caller sees - nb_chan and nlog [nchan], the control block (an OutCtl), and in mode 1
// seg_stats [nchan][2] and the speculative walks spec [nchan][3 * (nseg - 1)] (SpecOut: vdl2hip_debug_sizeof_specout() octets each).
// Refused (VDL2HIP_E_INVAL) is what the product cannot have: segments shorter than 64 samples, more than kMaxSeg of them, a segment count
// that is not the feed's length over seglen rounded up, a feed longer than the ring, a state that is not a walker's.  Behind every output buffer
// lie kWalkProbeGuard octets filled with 0xA5 beforehand: VDL2HIP_E_DEVICE if any of them has changed.  Needs no receiver
int vdl2hip_debug_sizeof_walkstate(void) { return (int)sizeof(WalkState); }
int vdl2hip_debug_sizeof_burst(void) { return (int)sizeof(Burst); }
int vdl2hip_debug_sizeof_specout(void) { return (int)sizeof(SpecOut); }
int vdl2hip_debug_walk_probe(int mode, uint32_t nchan, const float *y, const float *pf, const uint64_t *cand, uint32_t ring_len, const uint32_t *freq, float max_ppm,
		int64_t k0, int64_t k_end, int32_t nseg, int64_t seglen, void *ws, unsigned long long *cnt, uint32_t cap_bursts_chan, uint32_t cap_log,
		void *bursts, uint32_t *nb_chan, void *log, uint32_t *nlog, void *ctl, uint32_t *seg_stats, void *spec) {
	constexpr size_t kWalkProbeGuard = 4096;
	if(mode < 0 || mode > 1 || nchan == 0 || nchan > 1024 || !y || !pf || !cand || ring_len < 64 || (ring_len & (ring_len - 1)) || ring_len > 1u << 20 || !freq || !(max_ppm >= 0.f)
	   || k0 < 0 || k_end < k0 || k_end - k0 > (int64_t)ring_len || !ws || !cnt || cap_bursts_chan == 0 || cap_bursts_chan > 1u << 16 || cap_log == 0 || cap_log > 1u << 16
	   || !bursts || !nb_chan || !log || !nlog || !ctl) return VDL2HIP_E_INVAL;
	const int64_t D = k_end - k0;
	if(mode == 1 && (!seg_stats || !spec || nseg < 2 || nseg > kMaxSeg || seglen < 64 || (int64_t)(nseg - 1) * seglen >= D || (int64_t)nseg * seglen < D)) return VDL2HIP_E_INVAL;
	const WalkState *hw = static_cast<const WalkState *>(ws);
	for(uint32_t c = 0; c < nchan; c++) {
		const WalkState &s = hw[c];
		if(s.mode < 0 || s.mode > 2 || s.niv < 0 || s.niv > kNumIv || s.a < 0 || s.evals < 0 || s.bursts < 0) return VDL2HIP_E_INVAL;
		if(s.mode == 0 && (s.e0 < s.a + 2 || s.e < s.e0 || s.e < k0 || s.e > k0 + 2 || s.a > k0)) return VDL2HIP_E_INVAL;
		if(s.mode != 0 && (s.pb.sync_sample < 0 || s.pb.sync_sample >= k0 || s.pb.t_first <= s.pb.sync_sample || s.pb.t_first > s.pb.sync_sample + kSpsDec || s.pb.prev_n < -2 || s.pb.prev_n > s.pb.sync_sample)) return VDL2HIP_E_INVAL;
		if(s.mode == 1 && s.pb.t_first + 8 * kSpsDec < k0) return VDL2HIP_E_INVAL;
		if(s.mode == 2 && (s.pb.nsym < 1 || s.pb.nsym > kMaxSyms || s.pb.end_sample != s.pb.t_first + (int64_t)(s.pb.nsym - 1) * kSpsDec || s.pb.end_sample < k0)) return VDL2HIP_E_INVAL;
	}
	const uint32_t nspec = mode == 1 ? 3u * (uint32_t)(nseg - 1) : 0u;
	const size_t b_ws = (size_t)nchan * sizeof(WalkState), b_cnt = (size_t)nchan * kNumCounters * sizeof(unsigned long long), b_bursts = (size_t)nchan * cap_bursts_chan * sizeof(Burst),
	             b_nb = (size_t)nchan * 4, b_log = (size_t)nchan * cap_log * sizeof(EvalChunk), b_ctl = sizeof(OutCtl), b_seg = (size_t)nchan * 8, b_spec = (size_t)nchan * nspec * sizeof(SpecOut);
	DevBuf<cf32> d_y, d_pf; DevBuf<uint64_t> d_cand; DevBuf<uint32_t> d_freq; DevBuf<float> d_thr; DevBuf<Tables> d_tab;
	DevBuf<uint8_t> d_ws, d_cnt, d_bursts, d_nb, d_log, d_nlog, d_ctl, d_seg, d_spec;
	struct Out { DevBuf<uint8_t> *d; size_t used; void *host; };
	const Out outs[] = { { &d_ws, b_ws, ws }, { &d_cnt, b_cnt, cnt }, { &d_bursts, b_bursts, bursts }, { &d_nb, b_nb, nb_chan }, { &d_log, b_log, log }, { &d_nlog, b_nb, nlog },
	                     { &d_ctl, b_ctl, ctl }, { &d_seg, b_seg, seg_stats }, { &d_spec, b_spec, spec } };
	if(!hip_ok(d_y.alloc((size_t)nchan * ring_len)) || !hip_ok(d_pf.alloc((size_t)nchan * ring_len)) || !hip_ok(d_cand.alloc((size_t)nchan * (ring_len >> 6))) || !hip_ok(d_freq.alloc(nchan))
	   || !hip_ok(d_thr.alloc(nchan)) || !hip_ok(d_tab.alloc(1))) return VDL2HIP_E_NOMEM;
	for(const Out &o : outs) if(!hip_ok(o.d->alloc(o.used + kWalkProbeGuard))) return VDL2HIP_E_NOMEM;
	std::vector<float> thr(nchan);
	for(uint32_t c = 0; c < nchan; c++) thr[c] = ppm_gate_threshold(freq[c], max_ppm);
	OutCtl h_ctl; memset(&h_ctl, 0, sizeof h_ctl);
	h_ctl.cap_bursts = nchan * cap_bursts_chan; h_ctl.cap_log = cap_log;
	if(!dbg_tables(d_tab) || !dbg_up(d_y, y) || !dbg_up(d_pf, pf) || !dbg_up(d_cand, cand) || !dbg_up(d_freq, freq) || !dbg_up(d_thr, thr.data())) return VDL2HIP_E_DEVICE;
	for(const Out &o : outs) if(!dbg_fill(*o.d, 0xA5)) return VDL2HIP_E_DEVICE;
	if(!dbg_up(d_ws, ws, b_ws) || !dbg_up(d_cnt, cnt, b_cnt) || !dbg_up(d_ctl, &h_ctl, b_ctl) || !hip_ok(hipMemset(d_seg, 0, b_seg))) return VDL2HIP_E_DEVICE;
	K4Args k4{};
	k4.y = d_y; k4.pf = d_pf; k4.cand = d_cand; k4.tab = d_tab; k4.ws = reinterpret_cast<WalkState *>(d_ws.get()); k4.cnt = reinterpret_cast<unsigned long long *>(d_cnt.get());
	k4.bursts = reinterpret_cast<Burst *>(d_bursts.get()); k4.nb_chan = reinterpret_cast<uint32_t *>(d_nb.get()); k4.cap_bursts_chan = cap_bursts_chan; k4.ctl = reinterpret_cast<OutCtl *>(d_ctl.get());
	k4.freq = d_freq; k4.log = reinterpret_cast<EvalChunk *>(d_log.get()); k4.nlog = reinterpret_cast<uint32_t *>(d_nlog.get()); k4.cap_log = cap_log; k4.k_end = k_end; k4.max_ppm = max_ppm;
	k4.cap = ring_len; k4.mask = ring_len - 1; k4.chan_first = 0; k4.nchan = (int32_t)nchan; k4.ppm_thr = d_thr;
	if(mode == 0) hipLaunchKernelGGL(k_walk, dim3(nchan), dim3(64), 0, 0, k4);
	else {
		K4sArgs k4s{ k4, reinterpret_cast<SpecOut *>(d_spec.get()), nspec, nseg, k0, seglen, reinterpret_cast<uint32_t *>(d_seg.get()), 0 };
		hipLaunchKernelGGL(k_walk_spec, dim3((unsigned)((1 + 3 * (nseg - 1) + kWalkWaves - 1) / kWalkWaves), nchan), dim3(64 * kWalkWaves), 0, 0, k4s);
		hipLaunchKernelGGL(k_walk_stitch, dim3((unsigned)((nchan + kStitchWaves - 1) / kStitchWaves)), dim3(64 * kStitchWaves), (unsigned)(sizeof(StitchLds) * kStitchWaves), 0, k4s);
	}
	if(!hip_ok(hipGetLastError()) || !hip_ok(hipDeviceSynchronize())) return VDL2HIP_E_DEVICE;
	std::vector<uint8_t> g(kWalkProbeGuard);
	bool clean = true;
	for(const Out &o : outs) {
		if(!hip_ok(hipMemcpy(g.data(), o.d->get() + o.used, kWalkProbeGuard, hipMemcpyDeviceToHost))) return VDL2HIP_E_DEVICE;
		for(uint8_t b : g) clean = clean && b == 0xA5;
		if(o.host && o.used && !dbg_down(o.host, *o.d, o.used)) return VDL2HIP_E_DEVICE;
	}
	return clean ? VDL2HIP_OK : VDL2HIP_E_DEVICE;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_nf_probe.py): the noise floor as the receiver holds it after everything fed so far -
// nf[i] = v->mag_nf after first_update + i updates of channel chan, from the history ring (which holds the last nf_ring of them), and
// *evals = the got_sync() evaluations the replay has accounted for.  Returns the number of entries delivered (fewer than `count` where the
// channel has had fewer updates)
int vdl2hip_debug_read_noise_floor(vdl2hip_ctx *c, uint32_t chan, int64_t first_update, size_t count, float *nf, int64_t *evals) {
	if(!c || !evals || (count && !nf) || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C) || first_update < 0) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	const size_t ch = chan - c->chan_first;
	auto st = std::make_unique<NfState>();
	HIPCHK(hipMemcpy(st.get(), c->d_nf + ch, sizeof(NfState), hipMemcpyDeviceToHost));
	*evals = st->evals;
	const int64_t upd = st->evals / 1000;                              // entries 0 .. upd exist; the ring keeps the newest nf_ring of them
	if(first_update > upd || upd - first_update >= (int64_t)c->nf_ring) return VDL2HIP_E_INVAL;
	const size_t n = std::min<size_t>(count, (size_t)(upd - first_update + 1));
	std::vector<float> h(c->nf_ring);
	HIPCHK(hipMemcpy(h.data(), c->d_nfring + ch * c->nf_ring, h.size() * sizeof(float), hipMemcpyDeviceToHost));
	for(size_t i = 0; i < n; i++) nf[i] = h[(uint32_t)(first_update + (int64_t)i) & (c->nf_ring - 1)];
	return (int)n;
}

// Builds with a VDL2_*_PROF switch (kernels.h): the kernels' own counters (prof_read)
#ifdef VDL2_K1_PROF
int vdl2hip_debug_k1_prof(unsigned long long out[16], int reset) { return prof_read<16>(HIP_SYMBOL(vdl2_k1_prof), out, reset); }
#endif
#ifdef VDL2_K3B_PROF
int vdl2hip_debug_k3b_prof(unsigned long long out[16], int reset) { return prof_read<16>(HIP_SYMBOL(vdl2_k3b_prof), out, reset); }
#endif
#ifdef VDL2_K5_PROF
int vdl2hip_debug_k5_prof(unsigned long long out[16], int reset) { return prof_read<16>(HIP_SYMBOL(vdl2_k5_prof), out, reset); }
int vdl2hip_debug_nf_prof(unsigned long long out[16], int reset) { return prof_read<16>(HIP_SYMBOL(vdl2_nf_prof), out, reset); }
int vdl2hip_debug_k4_prof(unsigned long long out[24], int reset) { return prof_read<24>(HIP_SYMBOL(vdl2_k4_prof), out, reset); }
#endif

// test hook (not declared in vdl2hip.h; host only): the scan's word step (act_scan_word) over `count` words of nbits[i] <= 64 busy flags
// each, from an idle start -> out = { transmissions, longest_bins, open, first bin of the open transmission }
int vdl2hip_debug_activity_words(const uint64_t *busy, const uint32_t *nbits, uint32_t count, uint32_t hang_bins, uint64_t out[4]) {
	if(!busy || !nbits || !out || hang_bins > kActMaxHang) return VDL2HIP_E_INVAL;
	ActState st{}; uint64_t tx = 0, longest = 0, base = 0;
	for(uint32_t i = 0; i < count; i++) {
		if(nbits[i] == 0 || nbits[i] > 64 || (nbits[i] < 64 && (busy[i] >> nbits[i]) != 0)) return VDL2HIP_E_INVAL;
		act_scan_word(busy[i], nbits[i], hang_bins, base, st, tx, longest);
		base += nbits[i];
	}
	out[0] = tx; out[1] = longest; out[2] = st.open; out[3] = st.open ? st.first : 0;
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; host only, needs no GPU): the transmission log's word steps (txlog.h) for one channel, lane by
// lane and level by level as k_txlog_emit takes them, over `count` words of nbits[i] <= 64 bins each - p: the bins' powers, one after
// the other, the first being bin `base`; init: NULL for an idle start, else { open, idle, first bin } of a transmission under way, as
// k_txlog_init takes it over from the activity monitor.  The records that close go to recs[0 .. cap_recs) with chan and freq 0 and the
// host's fields as the library delivers a record without frames; k_txlog_plan's count is taken beside and must agree
// (VDL2HIP_E_DEVICE if not).  Returns the number of records; out = { open, idle, first bin, busy bins so far } of the state behind the last word.
int vdl2hip_debug_txlog_words(const float *p, const uint32_t *nbits, uint32_t count, float thr, uint32_t hang_bins, uint32_t B, int64_t k_on, uint64_t base,
		const uint64_t *init, vdl2hip_tx *recs, uint32_t cap_recs, uint64_t out[4]) {
	if(!p || !nbits || !out || (!recs && cap_recs) || hang_bins > kActMaxHang || !B) return VDL2HIP_E_INVAL;
	TxState s{}; s.acc = txl_none();
	if(init && init[0]) { if(init[1] > hang_bins) return VDL2HIP_E_INVAL; s.open = 1u; s.idle = (uint32_t)init[1]; s.first = init[2]; s.flags = kTxPartial; }
	TxState sp = s;                                                       // (k_txlog_plan's copy)
	uint32_t nrec = 0, planned = 0;
	for(uint32_t i = 0; i < count; i++) {
		const uint32_t n = nbits[i];
		if(n == 0 || n > 64) return VDL2HIP_E_INVAL;
		uint64_t busy = 0;
		for(uint32_t l = 0; l < n; l++) if(p[l] > thr) busy |= 1ull << l;
		{
			const TxMasks m = txl_masks(busy, n, hang_bins, sp.open, sp.idle);
			planned += (uint32_t)__builtin_popcountll(m.closes);
			txl_next(busy, m, n, hang_bins, base, txl_none(), sp);
		}
		const TxMasks m = txl_masks(busy, n, hang_bins, s.open, s.idle);
		TxPart v[64];
		for(uint32_t l = 0; l < 64; l++) v[l] = txl_lane(l < n && ((busy >> l) & 1ull), l < n ? p[l] : 0.f, base + l);
		for(uint32_t d = 1; d < 64; d <<= 1) {
			TxPart o[64];
			for(uint32_t l = 0; l < 64; l++) o[l] = v[l >= d ? l - d : l];      // (__shfl_up)
			for(uint32_t l = 0; l < 64; l++) if(txl_take(m.starts, l, d)) v[l] = txl_combine(o[l], v[l]);
		}
		for(uint32_t l = 0; l < 64; l++) if((m.closes >> l) & 1ull) {
			if(nrec >= cap_recs) return VDL2HIP_E_TOOBIG;
			vdl2hip_tx r{};
			TxRec t;
			txl_record(busy, m, l, base, s, v[l], 0u, 0u, k_on, B, t);
			memcpy(&r, &t, sizeof t);
			r.first_burst_ord = -1;
			recs[nrec++] = r;
		}
		txl_next(busy, m, n, hang_bins, base, v[n - 1], s);
		p += n; base += n;
	}
	if(planned != nrec || sp.open != s.open || sp.idle != s.idle) return VDL2HIP_E_DEVICE;
	out[0] = s.open; out[1] = s.idle; out[2] = s.open ? s.first : 0; out[3] = s.open ? s.acc.cnt : 0;
	return (int)nrec;
}

// test hook (not declared in vdl2hip.h; host only, needs no GPU): the preamble search's per-piece steps (txsearch.h) for one record,
// lane by lane and level by level as k_txsearch_piece and k_txsearch_reduce take them - y: the channel's ring of ring_len (re, im)
// pairs (a power of two), the record's first_sample and last_sample, its frequency -> rec: a vdl2hip_tx_search with chan, first_bin
// and the host's fields 0.  The staging arrays have a guard zone of NaNs behind each: VDL2HIP_E_DEVICE if a store went beyond a piece's sizes.
int vdl2hip_debug_txsearch_range(const float *y, uint32_t ring_len, int64_t first, int64_t last, uint32_t freq, void *rec) {
	if(!y || !rec || ring_len < 2 || (ring_len & (ring_len - 1)) || first < 0 || last < first || !freq) return VDL2HIP_E_INVAL;
	const cf32 *yc = reinterpret_cast<const cf32 *>(y);
	auto tab = std::make_unique<Tables>(); build_tables(*tab);
	int64_t sf; uint32_t fl;
	txs_range(first, last, sf, fl);
	const uint32_t np = txs_pieces(sf, last);
	if(np == 0 || np > (uint32_t)(kTxsSpan / kTxsPiece)) return VDL2HIP_E_DEVICE;
	constexpr int G = 16;
	std::vector<float> phi(kTxsPhi + G), p(kTxsP + G);
	std::vector<TxsPart> part(kTxsThreads), piece(np);
	bool bad = false;
	for(uint32_t g = 0; g < np; g++) {
		const int64_t n0 = sf + (int64_t)g * (int64_t)kTxsPiece, left = last - n0 + 1;
		const uint32_t cnt = left < (int64_t)kTxsPiece ? (uint32_t)left : kTxsPiece;
		std::fill(phi.begin(), phi.end(), NAN); std::fill(p.begin(), p.end(), NAN);
		for(uint32_t l = 0; l < (uint32_t)kTxsThreads; l++) txs_phase_step(yc, ring_len - 1, n0, cnt, l, kTxsThreads, phi.data());
		for(uint32_t l = 0; l < (uint32_t)kTxsThreads; l++) { part[l] = txs_none(); txs_metric_step(phi.data(), *tab, n0, cnt, l, kTxsThreads, p.data(), part[l]); }
		for(uint32_t l = 0; l < (uint32_t)kTxsThreads; l++) txs_lock_step(p.data(), n0, cnt, sf, l, kTxsThreads, part[l]);
		for(uint32_t s = kTxsThreads / 2; s >= 1; s >>= 1) for(uint32_t l = 0; l < (uint32_t)kTxsThreads; l++) txs_tree_step(part.data(), l, s);
		piece[g] = part[0];
		for(int i = 0; i < G; i++) bad = bad || !std::isnan(phi[kTxsPhi + i]) || !std::isnan(p[kTxsP + i]);
	}
	TxsPart t = txs_none();
	for(uint32_t g = 0; g < np; g++) txs_combine(t, piece[g]);
	TxsRec r;
	txs_record(0u, freq, 0ull, 0u, sf, last, fl, t, r);
	memcpy(rec, &r, sizeof r);
	return bad ? VDL2HIP_E_DEVICE : VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; host only, needs no GPU): the second look's steps (relook.h) for one record, lane by lane as
// k_relook_anchors, k_relook_select and k_relook_decode take them - y: the channel's ring of ring_len (re, im) pairs (a power of two),
// the record's first_sample and last_sample, the limit (last_sample + (H + 1) B in the receiver), its frequency, the configuration as
// vdl2hip_relook_enable() takes it (0: the defaults) -> recs: the attempt records with chan and first_bin 0 and frames_new 0, frames /
// octets: as vdl2hip_relook_read() packs them, out = { anchors found, attempts, frames, octets }.  Returns the attempts.  The staging
// arrays have a guard zone of NaNs behind each: VDL2HIP_E_DEVICE if a store went beyond a piece's sizes.
int vdl2hip_debug_relook_range(const float *y, uint32_t ring_len, int64_t first, int64_t last, int64_t limit, uint32_t freq, float threshold, uint32_t max_anchors, float max_ppm,
		uint32_t pool_frames, uint32_t pool_octets, vdl2hip_relook *recs, uint32_t cap_recs, vdl2hip_packed_frame *frames, uint32_t cap_frames, uint8_t *octets, uint32_t cap_octets, uint64_t out[4]) {
	if(!y || !out || ring_len < 2 || (ring_len & (ring_len - 1)) || first < 0 || last < first || limit < last || !freq) return VDL2HIP_E_INVAL;
	if((!recs && cap_recs) || (!frames && cap_frames) || (!octets && cap_octets)) return VDL2HIP_E_INVAL;
	if(!(threshold >= 0.f && threshold <= 30.f) || !(max_ppm >= 0.f) || max_anchors > kRlMaxAnchors || pool_frames > kRlMaxFrames || pool_octets > kRlMaxOctets) return VDL2HIP_E_INVAL;
	const float thr = threshold != 0.f ? threshold : kSyncThr;
	const uint32_t K = max_anchors ? max_anchors : kRlDefAnchors, pf = pool_frames ? pool_frames : kRlDefFrames, po = pool_octets ? pool_octets : kRlDefOctets;
	const cf32 *yc = reinterpret_cast<const cf32 *>(y);
	const uint32_t mask = ring_len - 1;
	auto tab = std::make_unique<Tables>(); build_tables(*tab);
	int64_t sf; uint32_t fl;
	txs_range(first, last, sf, fl);
	const uint32_t np = txs_pieces(sf, last);
	if(np == 0 || np > (uint32_t)(kTxsSpan / kTxsPiece)) return VDL2HIP_E_DEVICE;
	constexpr int G = 16;
	std::vector<float> phi(kRlPhi + G), p(kRlP + G);
	std::vector<RlPiece> piece(np);
	bool bad = false;
	for(uint32_t g = 0; g < np; g++) {
		const int64_t n0 = sf + (int64_t)g * (int64_t)kTxsPiece, left = last - n0 + 1;
		const uint32_t cnt = left < (int64_t)kTxsPiece ? (uint32_t)left : kTxsPiece;
		int64_t lo; uint32_t E;
		rl_span(n0, cnt, sf, last, lo, E);
		std::fill(phi.begin(), phi.end(), NAN); std::fill(p.begin(), p.end(), NAN);
		for(uint32_t l = 0; l < (uint32_t)kRlThreads; l++) txs_phase_step(yc, mask, lo + kSyncSkip, E - (uint32_t)kSyncSkip, l, kRlThreads, phi.data());
		for(uint32_t l = 0; l < (uint32_t)kRlThreads; l++) { TxsPart unused = txs_none(); txs_metric_step(phi.data(), *tab, lo + kSyncSkip, E - (uint32_t)kSyncSkip, l, kRlThreads, p.data(), unused); }
		const uint32_t base = (uint32_t)(n0 - lo);
		uint32_t idx[kRlPieceAnchors + 1], n = 0;
		for(uint32_t l = 0; l < (uint32_t)kRlThreads; l++)
			for(uint32_t k = l; k < cnt; k += kRlThreads)
				if(rl_is_anchor(p.data(), base + k, E, thr)) { if(n < (uint32_t)kRlPieceAnchors) idx[n] = base + k; n++; }
		if(n > (uint32_t)kRlPieceAnchors) return VDL2HIP_E_DEVICE;         // (never: they are 161 samples apart)
		std::sort(idx, idx + n);
		piece[g].n = n;
		for(uint32_t x = 0; x < n; x++) piece[g].a[x] = rl_anchor_at(phi.data(), *tab, lo, idx[x]);
		for(int i = 0; i < G; i++) bad = bad || !std::isnan(phi[kRlPhi + i]) || !std::isnan(p[kRlP + i]);
	}
	RlAnchor best[kRlMaxAnchors]; uint32_t nb = 0; uint64_t found = 0;
	for(uint32_t g = 0; g < np; g++) for(uint32_t x = 0; x < piece[g].n; x++) { rl_keep(best, nb, K, piece[g].a[x]); found++; }
	rl_sort_by_n(best, nb);
	if(nb > cap_recs) return VDL2HIP_E_TOOBIG;
	std::vector<RlRec> rec(nb); std::vector<RlPlan> plan(nb);
	uint32_t o_fr = 0; unsigned long long o_oc = 0;
	for(uint32_t k = 0; k < nb; k++) {
		RlAtt t;
		rl_plan_attempt(yc, mask, *tab, freq, max_ppm, limit, best[k], t);
		rl_record(0u, freq, 0ull, 0u, t, o_fr, o_oc, pf, po, rec[k], plan[k]);
		o_fr += t.claim_f; o_oc += t.claim_p;
	}
	std::vector<OutFrame> fr(pf); std::vector<uint8_t> pool((size_t)po + 4);
	auto sh = std::make_unique<BurstShared>(); auto fs = std::make_unique<FrameShared>();
	OutCtl ctl{}; ctl.nframes = 0xf0000000u; ctl.pool_used = 0xf0000000u;
	unsigned long long acnt[kNumAvlcCounters] = {};
	const float nfring = 0.f;
	burst_shared_init(*tab, 0u, &ctl, *sh, true);
	frame_shared_init(*tab, *fs);
	size_t nfr = 0, used = 0;
	for(uint32_t k = 0; k < nb; k++) {
		rl_decode(rec[k], plan[k], 0, yc, mask, *tab, fr.data(), pool.data(), &ctl, rec[k].counters, acnt, &nfring, *sh, *fs);
		memcpy(recs + k, &rec[k], sizeof(RlRec));
		recs[k].frame_first = (uint32_t)(rec[k].frames ? nfr : 0);
		for(uint32_t j = 0; j < rec[k].frames; j++) {
			const OutFrame &f = fr[rec[k].frame_first + j];
			if(nfr >= cap_frames || used + f.len > cap_octets) return VDL2HIP_E_TOOBIG;
			vdl2hip_packed_frame &o = frames[nfr++];
			memset(&o, 0, sizeof o);
			o.frame.chan = 0; o.frame.freq = freq; o.frame.idx = f.idx; o.frame.len = f.len; o.frame.octets = nullptr;
			o.frame.synd_weight = f.synd_weight; o.frame.datalen_octets = f.datalen_octets; o.frame.num_fec_corrections = f.num_fec_corrections;
			o.frame.frame_pwr_dbfs = f.frame_pwr_dbfs; o.frame.nf_pwr_dbfs = f.nf_pwr_dbfs; o.frame.ppm_error = f.ppm_error;
			o.frame.burst_ord = f.burst_ord; o.frame.sync_sample = f.sync_sample; o.frame.end_sample = f.end_sample;
			o.frame.avlc_status = f.avlc_status; o.frame.dst_addr = f.dst_addr; o.frame.src_addr = f.src_addr;
			o.octets_off = used;
			memcpy(octets + used, pool.data() + f.pool_off, f.len);
			used += f.len;
		}
	}
	out[0] = found; out[1] = nb; out[2] = nfr; out[3] = used;
	return bad || ctl.overflow ? VDL2HIP_E_DEVICE : (int)nb;
}

// test hook (not declared in vdl2hip.h; host only, needs no GPU): the transmission capture's plan (txcap.h) for the nrec records of one
// feed, as k_txcap_plan takes it - tx: the log's records (first_sample, last_sample, flags, chan, freq, first_bin are read), cfg: as
// vdl2hip_txcap_enable() takes it (nfft 0, pool_samples 0 and pool_spectra 0 mean their defaults) -> recs: the records as the device
// writes them (iq_off in pairs of the pool, spec_off in floats of the feed's spectra), poff[nrec + 1]: the offsets of their pieces,
// out = { pairs of the pool in use, pieces }
int vdl2hip_debug_txcap_plan(const vdl2hip_tx *tx, uint32_t nrec, const vdl2hip_txcap_cfg *cfg, vdl2hip_tx_capture *recs, uint32_t *poff, uint64_t out[2]) {
	if((!tx && nrec) || !cfg || (!recs && nrec) || !poff || !out || cfg->struct_size != sizeof(vdl2hip_txcap_cfg)) return VDL2HIP_E_INVAL;
	const uint32_t N = cfg->nfft ? cfg->nfft : kTxcDefN;
	if(N < kTxcMinN || N > kTxcMaxN || (N & (N - 1)) || cfg->pre_samples > kTxcMaxPre) return VDL2HIP_E_INVAL;
	const TxcCfg k{ cfg->pool_samples ? cfg->pool_samples : kTxcDefPool, cfg->flags, cfg->pre_samples, cfg->post_samples, cfg->max_iq_samples, N, cfg->pool_spectra ? cfg->pool_spectra : kTxcDefSpectra };
	uint64_t off = 0, used = 0; uint32_t pieces = 0;
	for(uint32_t i = 0; i < nrec; i++) {
		TxRec t; memcpy(&t, tx + i, sizeof t);
		TxcRec r; uint32_t cnt, np;
		txc_plan_rec(t, i, k, r, cnt, np);
		if(txc_place(r, off, k) && cnt) used = std::max(used, off + cnt);
		memcpy(recs + i, &r, sizeof r);
		poff[i] = pieces; off += cnt; pieces += np;
	}
	poff[nrec] = pieces; out[0] = used; out[1] = pieces;
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; host only, needs no GPU): the transmission capture's per-piece steps (txcap.h) for one record,
// lane by lane, pass by pass and round by round as k_txcap_spectrum and k_txcap_reduce take them - y: the channel's ring of ring_len
// (re, im) pairs (a power of two), the record's first_sample and last_sample -> power[nfft], *segments.  The staging arrays have a
// guard zone of NaNs behind each: VDL2HIP_E_DEVICE if a store went beyond the kernel's sizes.
int vdl2hip_debug_txcap_spectrum(const float *y, uint32_t ring_len, int64_t first, int64_t last, uint32_t nfft, uint32_t window, float *power, uint32_t *segments) {
	if(!y || !power || !segments || ring_len < 2 || (ring_len & (ring_len - 1)) || first < 0 || last < first) return VDL2HIP_E_INVAL;
	const uint32_t N = nfft ? nfft : kTxcDefN;
	SpectrumDesign d;
	if(N < kTxcMinN || N > kTxcMaxN || !design_spectrum(N, window, d)) return VDL2HIP_E_INVAL;
	const cf32 *yc = reinterpret_cast<const cf32 *>(y);
	const float2 *tw = reinterpret_cast<const float2 *>(d.tw.data());
	int64_t ef; uint32_t efl;
	txs_range(first, last, ef, efl);
	const uint32_t S = txc_segments(last - ef + 1, N), np = txc_pieces(S, N), G = txc_groups(N), L = N >> 2, npass = txc_passes(d.log2n);
	*segments = S;
	constexpr int GZ = 16;
	const size_t span = txc_span(N), half = txc_half(N);
	std::vector<float2> smp(span + GZ), buf((size_t)G * 2 * half + GZ);
	std::vector<double> gacc((size_t)G * N), part((size_t)std::max(1u, np) * N);
	const float2 nan2 = make_float2(NAN, NAN);
	bool bad = false;
	for(uint32_t pc = 0; pc < np; pc++) {
		uint32_t s0, ns;
		txc_piece(S, N, pc, s0, ns);
		std::fill(smp.begin(), smp.end(), nan2); std::fill(buf.begin(), buf.end(), nan2);
		for(uint32_t l = 0; l < (uint32_t)kTxcThreads; l++) txc_load_step(yc, ring_len - 1, ef + (int64_t)s0 * (int64_t)(N >> 1), (ns + 1) * (N >> 1), l, kTxcThreads, smp.data());
		std::vector<double> acc((size_t)kTxcThreads * 4, 0.0);
		for(uint32_t rd = 0; rd < kTxcRounds; rd++) {
			auto each = [&](auto f) { for(uint32_t lane = 0; lane < (uint32_t)kTxcThreads; lane++) { const uint32_t g = lane / L, l = lane % L, s = rd * G + g; if(s < ns) f(lane, g, l, s); } };
			each([&](uint32_t, uint32_t g, uint32_t l, uint32_t s) { txc_fill_step(smp.data(), d.w.data(), N, s, l, buf.data() + (size_t)g * 2 * half); });
			for(uint32_t p = 0; p < npass; p++)
				each([&](uint32_t, uint32_t g, uint32_t l, uint32_t) { float2 *a = buf.data() + (size_t)g * 2 * half, *b = a + half; txc_pass_step(p & 1 ? b : a, p & 1 ? a : b, tw, N, d.log2n, p, l); });
			each([&](uint32_t lane, uint32_t g, uint32_t l, uint32_t) { const float2 *a = buf.data() + (size_t)g * 2 * half; txc_power_step(npass & 1 ? a + half : a, N, l, &acc[(size_t)lane * 4]); });
		}
		for(uint32_t lane = 0; lane < (uint32_t)kTxcThreads; lane++) for(uint32_t r = 0; r < 4; r++) gacc[(size_t)(lane / L) * N + lane % L + r * L] = acc[(size_t)lane * 4 + r];
		for(uint32_t b = 0; b < N; b++) part[(size_t)pc * N + b] = txc_group_sum(gacc.data(), G, N, b);
		for(int i = 0; i < GZ; i++) bad = bad || !std::isnan(smp[span + i].x) || !std::isnan(buf[(size_t)G * 2 * half + i].x);
	}
	const double norm = 1.0 / (d.sum_w * d.sum_w);
	for(uint32_t b = 0; b < N; b++) power[b] = S ? txc_reduce_bin(part.data(), 0, np, N, b, norm, S) : 0.f;
	return bad ? VDL2HIP_E_DEVICE : VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h; host only): k_activity_power's own code, lane by lane and barrier by barrier, for one channel of
// one feed - y: the channel's ring of `cap` (re, im) pairs, the feed its samples k0 .. k0 + D - 1, t0 of them after the monitor was enabled;
// series: a ring of S values.  Every index into the staging arrays is checked: VDL2HIP_E_DEVICE if one is out of range.
int vdl2hip_debug_activity_power(const float *y, uint32_t cap, int64_t k0, uint32_t D, uint32_t B, uint64_t t0, uint32_t run, float carry_in, float *series, uint32_t S, float *carry_out) {
	if(!y || !series || !carry_out || !cap || (cap & (cap - 1)) || !S || (S & (S - 1)) || B < kActMinBin || B > kActMaxBin || !D || D > cap || !run || k0 < 0 || ((uintptr_t)y & 15)) return VDL2HIP_E_INVAL;
	const uint64_t m0 = t0 / B, nb = (t0 + D) / B - m0;
	if(nb > S) return VDL2HIP_E_TOOBIG;
	ActArgs a{};
	a.y = (const float2 *)y; a.series = series; a.carry_in = &carry_in; a.carry_out = carry_out; a.k0 = k0; a.m0 = m0;
	a.off = (int32_t)((int64_t)(m0 * B) - (int64_t)t0); a.D = D; a.B = B; a.nbt = (uint32_t)nb + 1; a.run = run; a.cap = cap; a.mask = cap - 1; a.S = S; a.smask = S - 1;
	// staging arrays with a guard zone of NaNs behind each: a store or a load beyond the kernel's sizes shows
	constexpr int G = 64;
	std::vector<float> p(kActLdsP + G), sb(kActMaxSubs + G), gr(kActLdsG + G);
	bool bad = false;
	for(uint32_t bx = 0; bx * run < a.nbt; bx++) {
		uint32_t j = bx * run;
		const uint32_t jend = j + run < a.nbt ? j + run : a.nbt;
		int64_t pos = act_run_start(a, j);
		bool fresh = true;
		float acc[kActThreads] = {};
		while(j < jend) {
			const ActPlan k = act_plan(a, j, jend, pos, fresh);
			if(k.pos < 0 || k.pos + k.len > D || k.nseg > (uint32_t)kActMaxSegs || k.nsb > (uint32_t)kActMaxSubs || k.ngr > (uint32_t)kActLdsG || act_pad(k.o + k.len) >= (uint32_t)kActLdsP) return VDL2HIP_E_DEVICE;
			for(auto *v : { &p, &sb, &gr }) std::fill(v->begin(), v->end(), NAN);
			for(uint32_t l = 0; l < (uint32_t)kActThreads; l++) act_step<0>(a, k, 0, l, p.data(), sb.data(), gr.data(), acc[l]);
			for(uint32_t l = 0; l < (uint32_t)kActThreads; l++) act_step<1>(a, k, 0, l, p.data(), sb.data(), gr.data(), acc[l]);
			for(uint32_t l = 0; l < (uint32_t)kActThreads; l++) act_step<2>(a, k, 0, l, p.data(), sb.data(), gr.data(), acc[l]);
			for(uint32_t l = 0; l < (uint32_t)kActThreads; l++) act_step<3>(a, k, 0, l, p.data(), sb.data(), gr.data(), acc[l]);
			for(int i = 0; i < G; i++) bad = bad || !std::isnan(p[kActLdsP + i]) || !std::isnan(sb[kActMaxSubs + i]) || !std::isnan(gr[kActLdsG + i]);
			if(!k.fin0) { pos += kActChunk; fresh = false; }
			else { j += k.nseg; pos += k.len; fresh = true; }
		}
	}
	return bad ? VDL2HIP_E_DEVICE : VDL2HIP_OK;
}

// test hooks (not declared in vdl2hip.h; host only, need no GPU): the capture's per-burst steps on the CPU, lane by lane and level by level.
// A burst as the hooks take it (64 bytes):
struct CapDebugBurst { int32_t nsym; uint32_t tl_bits; int64_t t_first, sync_sample, end_sample, ord, prev_n; float prev_phi0, vdphi, ppm; uint32_t pad_; };
static Burst cap_debug_burst(const CapDebugBurst &d) {
	Burst b{};
	b.nsym = d.nsym; b.tl_bits = d.tl_bits; b.t_first = d.t_first; b.sync_sample = d.sync_sample; b.end_sample = d.end_sample; b.ord = d.ord; b.prev_n = d.prev_n;
	b.prev_phi0 = d.prev_phi0; b.vdphi = d.vdphi; b.ppm = d.ppm;
	return b;
}
// One burst over y, a channel's ring of ring_len (re, im) pairs (a power of two, 16-byte aligned), its window placed at pair `off`
// of a pool: -> the record (iq_off = off) and iq[0 .. iq_count).  VDL2HIP_E_DEVICE if a store went outside the window's place.
int vdl2hip_debug_capture_burst(const float *y, uint32_t ring_len, const void *burst, uint32_t pre, uint32_t post, int64_t k_end, uint64_t off, uint32_t chan, uint32_t freq,
		vdl2hip_burst *rec, float *iq, size_t cap_pairs) {
	if(!y || !burst || !rec || (ring_len & (ring_len - 1)) || ring_len < 2 || ((uintptr_t)y & 15) || pre > kCapMaxPre || post > kCapMaxPost || off > (1u << 24)) return VDL2HIP_E_INVAL;
	const Burst b = cap_debug_burst(*static_cast<const CapDebugBurst *>(burst));
	if(b.nsym < 0 || b.sync_sample < 0 || b.end_sample < b.sync_sample || b.end_sample >= k_end || b.t_first < 0 || b.t_first + (int64_t)(b.nsym > 0 ? b.nsym - 1 : 0) * kSpsDec >= k_end) return VDL2HIP_E_INVAL;
	CapPlan p{};
	cap_window(b, pre, post, k_end, p.first, p.count);
	if(iq && p.count > cap_pairs) return VDL2HIP_E_TOOBIG;               // (a window longer than the ring goes round it: the steps mask every index)
	const cf32 *yc = reinterpret_cast<const cf32 *>(y);
	constexpr size_t G = 4;                                           // guard pairs of NaN on either side of the window's place
	const size_t base = (size_t)(off & 1u) + 2 * G;                  // (the pool begins on a 16-byte boundary; the window at a pair of off's parity)
	std::vector<float4> store((base + p.count + 2 * G + 3) / 2 + 1);
	cf32 *pool = reinterpret_cast<cf32 *>(store.data());
	for(size_t i = 0; i < 2 * store.size(); i++) pool[i] = cf32{ NAN, NAN };
	for(uint32_t l = 0; l < (uint32_t)kCapThreads; l++) cap_copy(yc, ring_len - 1, p.first, p.count, pool + base, off, l, kCapThreads);
	bool bad = false;
	for(size_t i = 0; i < 2 * store.size(); i++) if(i < base || i >= base + p.count) bad = bad || !std::isnan(pool[i].re) || !std::isnan(pool[i].im);
	std::vector<CapPart> part(kCapThreads);
	for(uint32_t l = 0; l < (uint32_t)kCapThreads; l++) part[l] = cap_quality_run(yc, ring_len - 1, b, l, kCapThreads);
	for(uint32_t s = kCapThreads / 2; s >= 1; s >>= 1) for(uint32_t l = 0; l < (uint32_t)kCapThreads; l++) cap_tree_step(part.data(), l, s);
	CapRec r{};
	cap_record(b, chan, freq, p, off, true, part[0], r);
	memcpy(rec, &r, sizeof r);
	if(iq && p.count) memcpy(iq, pool + base, (size_t)p.count * sizeof(cf32));
	return bad ? VDL2HIP_E_DEVICE : VDL2HIP_OK;
}
// The offsets of a feed's bursts as the two kernels work them out - bursts[c * cap_bursts_chan + i], i < nb_chan[c]; the scans go in
// rounds of 64 with a carry as the wavefronts' do (integer sums: their order changes nothing) - and the room decision:
// -> iq_off, iq_count, flags per burst in record order, hdr = { records, pairs of the pool in use }.  Returns the number of records.
int vdl2hip_debug_capture_plan(const void *bursts, const uint32_t *nb_chan, uint32_t nchan, uint32_t cap_bursts_chan, uint32_t pre, uint32_t post, int64_t k_end,
		uint64_t pool_samples, uint64_t *iq_off, uint32_t *iq_count, uint32_t *flags, size_t cap_recs, uint64_t hdr[2]) {
	if(!bursts || !nb_chan || !hdr || !nchan || nchan > (uint32_t)kCapMaxChan || !cap_bursts_chan || pre > kCapMaxPre || post > kCapMaxPost) return VDL2HIP_E_INVAL;
	const CapDebugBurst *db = static_cast<const CapDebugBurst *>(bursts);
	std::vector<CapPlan> plan((size_t)nchan * cap_bursts_chan);
	std::vector<uint64_t> tot(nchan), bbo(nchan + 1);
	std::vector<uint32_t> bbn(nchan + 1);
	for(uint32_t c = 0; c < nchan; c++) {                                // k_capture_plan
		const uint32_t nb = std::min(nb_chan[c], cap_bursts_chan);
		uint64_t carry = 0;
		for(uint32_t w = 0; w < nb; w += 64) {
			uint32_t inc = 0;
			for(uint32_t l = 0; l < 64 && w + l < nb; l++) {
				CapPlan &p = plan[(size_t)c * cap_bursts_chan + w + l];
				cap_window(cap_debug_burst(db[(size_t)c * cap_bursts_chan + w + l]), pre, post, k_end, p.first, p.count);
				p.off = carry + inc; inc += p.count;
			}
			carry += inc;
		}
		tot[c] = carry;
	}
	uint32_t total = 0; uint64_t ototal = 0;                             // k_capture_copy: the channels' offsets
	for(uint32_t c = 0; c < nchan; c++) { bbn[c] = total; bbo[c] = ototal; total += std::min(nb_chan[c], cap_bursts_chan); ototal += tot[c]; }
	bbn[nchan] = total; bbo[nchan] = ototal;
	hdr[0] = total; hdr[1] = 0;
	if((iq_off || iq_count || flags) && cap_recs < total) return VDL2HIP_E_TOOBIG;
	for(uint32_t g = 0; g < total; g++) {
		const int c = cap_find_chan(bbn.data(), (int)nchan, g);
		const uint32_t i = g - bbn[c];
		const CapPlan &p = plan[(size_t)c * cap_bursts_chan + i];
		const uint64_t off = bbo[c] + p.off;
		const bool fits = off + p.count <= pool_samples;
		if(iq_off) iq_off[g] = fits ? off : 0;
		if(iq_count) iq_count[g] = fits ? p.count : 0;
		if(flags) flags[g] = fits ? 0u : kCapNoRoom;
		if(fits && cap_is_last_fit(bbn.data(), (int)nchan, plan.data(), cap_bursts_chan, g, c, i, off + p.count, pool_samples, total)) hdr[1] = off + p.count;
	}
	return (int)total;
}

// test hook (not declared in vdl2hip.h; host only, needs no GPU): k_toa's per-burst steps on the CPU, lane by lane and level by level.
// One burst - its first symbol at first_symbol, its slope dphi - over y, a channel's ring of ring_len (re, im) pairs (a power of two,
// at least 256), W = max_lag (0: 8): -> the record (chan, freq, burst_ord, sync_sample 0; curve_off 0) and curve[0 .. 2 W + 1).
int vdl2hip_debug_toa_burst(const float *y, uint32_t ring_len, int64_t first_symbol, float dphi, uint32_t max_lag, vdl2hip_burst_toa *rec, float *curve, size_t cap_floats) {
	if(!y || !rec || (ring_len & (ring_len - 1)) || ring_len < 256 || max_lag > kToaMaxLag) return VDL2HIP_E_INVAL;
	const uint32_t W = max_lag ? max_lag : kToaDefLag, nlags = 2 * W + 1, nwin = (uint32_t)kToaTaps + 2 * W;
	if(curve && cap_floats < nlags) return VDL2HIP_E_TOOBIG;
	const cf32 *yc = reinterpret_cast<const cf32 *>(y);
	ToaDesign d;
	design_toa(d);
	Burst b{};
	b.t_first = first_symbol; b.vdphi = dphi;
	const int64_t t0 = b.t_first - kToaLead;
	cf32 u[kToaTaps], yw[kToaWin], cl[kToaMaxLags], part[64];
	float P[kToaMaxLags];
	double dpart[64];
	auto add = [](cf32 p, cf32 q) { return toa_add(p, q); };
	auto dadd = [](double p, double q) { return p + q; };
	auto sum = [&](uint32_t k, uint32_t n0, uint32_t n1) {
		for(uint32_t l = 0; l < 64; l++) part[l] = toa_lane_sum(u, yw, k, l, n0, n1);
		for(uint32_t s = 32; s >= 1; s >>= 1) for(uint32_t l = 0; l < 64; l++) toa_tree_step(part, l, s, add);
		return part[0];
	};
	for(uint32_t l = 0; l < (uint32_t)kToaTaps; l++) u[l] = toa_u(cf32{ d.s[2 * l], d.s[2 * l + 1] }, dphi, l);
	for(uint32_t l = 0; l < nwin; l++) yw[l] = toa_window(yc, ring_len - 1, t0, W, l);
	for(uint32_t w = 0; w < (uint32_t)kToaWaves; w++) for(uint32_t k = w; k < nlags; k += kToaWaves) { cl[k] = sum(k, 0u, (uint32_t)kToaTaps); P[k] = toa_power(cl[k]); }
	const uint32_t kp = toa_peak(P, nlags);
	ToaSums q;
	q.c = cl[kp]; q.ca = sum(kp, 0u, (uint32_t)kToaHalf); q.cb = sum(kp, (uint32_t)kToaHalf, 2u * kToaHalf);
	for(uint32_t l = 0; l < 64; l++) dpart[l] = toa_lane_energy(yw, kp, l);
	for(uint32_t s = 32; s >= 1; s >>= 1) for(uint32_t l = 0; l < 64; l++) toa_tree_step(dpart, l, s, dadd);
	q.ey = dpart[0];
	ToaRec r{};
	toa_record(b, 0u, 0u, W, P, kp, q, d.energy, curve != nullptr, r);
	memcpy(rec, &r, sizeof r);
	if(curve) memcpy(curve, P, nlags * sizeof(float));
	return VDL2HIP_OK;
}

// test hook (not declared in vdl2hip.h): what the sync kernels left for decimated samples first .. first+count-1 of one channel - the tabulated
// metric {pherr (its sign: the referee's mark), slope} and the candidate bit, one byte per sample
int vdl2hip_debug_read_sync(vdl2hip_ctx *c, uint32_t chan, int64_t first, size_t count, float *pf, uint8_t *cand) {
	if(!c || !pf || !cand || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	if(first < 0 || first > c->k_total || c->k_total - first > (int64_t)c->cap) return VDL2HIP_E_INVAL;
	const size_t n = std::min<size_t>(count, (size_t)(c->k_total - first)), ch = chan - c->chan_first;
	std::vector<uint64_t> words(c->cap >> 6);
	HIPCHK(hipMemcpy(words.data(), c->d_cand + ch * (c->cap >> 6), words.size() * 8, hipMemcpyDeviceToHost));
	for(size_t i = 0; i < n; i++) {
		const uint32_t slot = (uint32_t)(first + (int64_t)i) & (c->cap - 1);
		cand[i] = (uint8_t)((words[slot >> 6] >> (slot & 63)) & 1u);
	}
	size_t done = 0;
	while(done < n) {
		const uint32_t slot = (uint32_t)(first + (int64_t)done) & (c->cap - 1);
		const size_t m = std::min<size_t>(n - done, c->cap - slot);
		HIPCHK(hipMemcpy(pf + 2 * done, c->d_pf + ch * c->cap + slot, m * sizeof(cf32), hipMemcpyDeviceToHost));
		done += m;
	}
	return (int)n;
}

// test hook (not declared in vdl2hip.h; tests/test_gpu_sync_screen.py): the screening tier's verdicts, flag[i] = bit first + i of the d_flag ring
int vdl2hip_debug_read_flags(vdl2hip_ctx *c, uint32_t chan, int64_t first, size_t count, uint8_t *flag) {
	if(!c || !flag || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	int r = collect_pending(c);
	if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
	if(first < 0 || first > c->k_total || c->k_total - first > (int64_t)c->cap) return VDL2HIP_E_INVAL;
	// (up to the end of the last word: the bits past the last valid sample are the kernel's too, and must be zero)
	const size_t n = std::min<size_t>(count, (size_t)(((c->k_total + 63) & ~(int64_t)63) - first)), ch = chan - c->chan_first;
	std::vector<uint64_t> words(c->cap >> 6);
	HIPCHK(hipMemcpy(words.data(), c->d_flag + ch * (c->cap >> 6), words.size() * 8, hipMemcpyDeviceToHost));
	for(size_t i = 0; i < n; i++) {
		const uint32_t slot = (uint32_t)(first + (int64_t)i) & (c->cap - 1);
		flag[i] = (uint8_t)((words[slot >> 6] >> (slot & 63)) & 1u);
	}
	return (int)n;
}

}  // extern "C"
