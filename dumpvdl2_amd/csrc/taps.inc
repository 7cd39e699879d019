// taps.inc - the receiver's nine optional taps, host side (included by vdl2hip.hip behind the context; kernels: spectrum.h - the
// input monitor's and the spectrogram's - capture.h, toa.h, relook.h, txsearch.h, txcap.h, txlog.h, activity.h).  Each tap stands in one place: its share of a feed (launch), of a collected feed
// (collect), what gives its buffers back (free), then its entry points of vdl2hip.h.  A tap stands behind those it calls into: the
// log hands its records to the search and to the transmission capture, the activity monitor launches the log and switches it off,
// the input monitor does both with the spectrogram.
// Six of them deliver records - capture, burst timing, second look, search, transmission capture, log - and share one mechanism: per slot a TapSlot with a RecordMail in it
// (hostmem.h), per context the totals, a queue of collected records and the staging buffer of a feed with more records than come
// with the header.  Their enable is: validate, collect what is in flight, free the old, allocate per slot, zero the totals, on.
// (The entry points have C linkage from their declarations in vdl2hip.h.)

// vdl2hip_<tap>_read of a tap whose records go out as they are queued
template<typename R>
static int pop_records(std::deque<R> &q, R *recs, size_t cap_recs) {
	size_t n = 0;
	while(!q.empty() && n < cap_recs) { recs[n++] = q.front(); q.pop_front(); }
	return (int)n;
}

// ---- the spectrogram (vdl2hip.h, "Spectrogram"; kernels: spectrum.h; the plan of a feed: specgram_plan.h) ----
// A tap on top of the input monitor, which launches it and switches it off (so it stands ahead of it here): max-hold, floor and the
// last ring_lines lines of R analysed segments each.  It has no event, stream or landing place of its own: the monitor's serve.
static_assert(sizeof(vdl2hip_specgram_cfg) == 16 && sizeof(vdl2hip_specgram_info) == 72, "vdl2hip.h states these sizes");
// Its share of a feed that analyses nseg >= 1 segments (monitor_block): the arguments of k_spectrum_lines, which takes k_spectrum's
// place in that feed, and of k_specgram_combine behind the monitor's reduction.  The host's counts move on here.
static bool specgram_plan(vdl2hip_ctx *c, uint64_t nseg, SpgArgs &sg) {
	auto &s = c->spg; auto &b = s.buf;
	sg.piece_sum = b.d_piece_sum; sg.piece_max = b.d_piece_max; sg.run_max = b.d_run_max; sg.run_floor = b.d_run_floor;
	sg.ring_mean = b.d_ring_mean; sg.ring_max = b.d_ring_max; sg.carry_sum = b.d_carry_sum; sg.carry_max = b.d_carry_max; sg.hold = b.d_hold;
	sg.norm = 1.0 / (c->mon.sum_w * c->mon.sum_w);
	sg.f = spg_feed(s.seen, nseg, s.R, s.ring, kSpecMaxRows);
	// (never: a feed is at most max_block_bytes) the pieces have a row per workgroup, the ring a slot per line of one feed
	return sg.f.grid <= s.rows && spg_lines_after(sg.f) - spg_lines_before(sg.f) < s.ring;
}
static void specgram_launch_combine(vdl2hip_ctx *c, const SpgArgs &sg, hipEvent_t e1) {
	auto &s = c->spg;
	hipExtLaunchKernelGGL(k_specgram_combine, dim3((c->mon.nfft + 255) / 256), dim3(256), 0u, c->streams.front, (hipEvent_t) nullptr, e1, 0,
	                      sg, c->mon.nfft, (uint32_t)(sg.f.t0 % s.R));
	const uint64_t l0 = spg_lines_before(sg.f), l1 = spg_lines_after(sg.f);
	s.seen += sg.f.nseg; s.hold_segments += sg.f.nseg; s.hold_lines += l1 - l0;
}
// give its buffers back (the monitor's launches carry it: whoever calls has waited for them, or nothing was queued since the enable)
static void specgram_free(vdl2hip_ctx *c) {
	c->spg.buf = {};
	c->spg.on = false;
}
static int specgram_wait(vdl2hip_ctx *c) {
	auto &m = c->mon;
	if(m.tap.queued && hipEventSynchronize(m.tap.last) != hipSuccess) { (void)hipGetLastError(); return VDL2HIP_E_DEVICE; }
	return VDL2HIP_OK;
}
// the holds as they stand once everything the monitor has queued is done: [nfft] max_hold, [nfft] floor_hold (zero while no line)
static int specgram_fetch_hold(vdl2hip_ctx *c, std::vector<float> &hold) {
	auto &m = c->mon; auto &s = c->spg;
	const size_t N = m.nfft;
	hold.assign(2 * N, 0.f);
	if(s.hold_segments == 0) return VDL2HIP_OK;                      // nothing has touched them since they were zeroed
	HIPCHK(m.tap.fetch(m.tap.land, s.buf.d_hold, s.buf.d_hold.bytes()));
	memcpy(hold.data(), m.tap.land, 2 * N * sizeof(float));
	if(s.hold_lines == 0) std::fill(hold.begin() + (ptrdiff_t)N, hold.end(), 0.f);
	return VDL2HIP_OK;
}
// the holds' start: max_hold 0, floor_hold +inf (the host reports 0 while no line is complete), on the front stream
static hipError_t specgram_clear_hold(vdl2hip_ctx *c) {
	auto &s = c->spg;
	const size_t N = c->mon.nfft;
	hipError_t e = hipMemsetAsync(s.buf.d_hold, 0, N * sizeof(float), c->streams.front);
	if(e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(s.buf.d_hold.get() + N), 0x7f800000, N, c->streams.front);
	return e;
}
int vdl2hip_specgram_enable(vdl2hip_ctx *c, const vdl2hip_specgram_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_specgram_cfg) || cfg->reserved != 0) return VDL2HIP_E_INVAL;
	if(!c->mon.on || cfg->line_segments > kSpgMaxLineSegments || (cfg->ring_lines & (cfg->ring_lines - 1)) != 0) return VDL2HIP_E_INVAL;
	auto &m = c->mon; auto &s = c->spg;
	const uint32_t R = cfg->line_segments ? cfg->line_segments : kSpgDefLineSegments;
	const uint64_t N = m.nfft, feed_segs = spg_feed_segments(c->in_cap / raw_bytes(c->in_fmt), m.nfft, m.stride);
	const uint64_t ring = std::max<uint64_t>(cfg->ring_lines, spg_ring_min(feed_segs, R));
	if(ring * N > kSpgMaxRingFloats) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = specgram_wait(c); if(r != VDL2HIP_OK) return r; }      // nothing of an earlier tap is in flight any more
	specgram_free(c);
	const size_t rows = (size_t)std::min<uint64_t>(kSpecMaxRows, std::max<uint64_t>(1, feed_segs));
	auto &b = s.buf;
	for(hipError_t e : { b.d_piece_sum.alloc(rows * 2 * N), b.d_piece_max.alloc(rows * 2 * N), b.d_run_max.alloc(rows * N), b.d_run_floor.alloc(rows * N),
	                     b.d_ring_mean.alloc(ring * N, true), b.d_ring_max.alloc(ring * N, true), b.d_carry_sum.alloc(N, true), b.d_carry_max.alloc(N, true), b.d_hold.alloc(2 * N) })
		if(e != hipSuccess) { specgram_free(c); return e == hipErrorOutOfMemory ? VDL2HIP_E_NOMEM : VDL2HIP_E_DEVICE; }
	if(specgram_clear_hold(c) != hipSuccess || hipStreamSynchronize(c->streams.front) != hipSuccess) { (void)hipGetLastError(); specgram_free(c); return VDL2HIP_E_DEVICE; }
	s.R = R; s.ring = (uint32_t)ring; s.rows = (uint32_t)rows; s.a0 = m.ordinal; s.seen = 0; s.hold_segments = s.hold_lines = 0;
	s.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_specgram_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->spg.on) (void)specgram_wait(c);
	specgram_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_specgram_read(vdl2hip_ctx *c, vdl2hip_specgram_info *info, float *max_hold, float *floor_hold, size_t cap, int reset) {
	if(!c || !c->spg.on || !c->mon.on || (info && info->struct_size != sizeof(vdl2hip_specgram_info))) return VDL2HIP_E_INVAL;
	auto &m = c->mon; auto &s = c->spg;
	const uint32_t N = m.nfft;
	if((max_hold || floor_hold) && cap < N) return VDL2HIP_E_TOOBIG;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	if(max_hold || floor_hold) {
		std::vector<float> hold;
		{ int r = specgram_fetch_hold(c, hold); if(r != VDL2HIP_OK) return r; }
		if(max_hold) memcpy(max_hold, hold.data(), (size_t)N * sizeof(float));
		if(floor_hold) memcpy(floor_hold, hold.data() + N, (size_t)N * sizeof(float));
	}
	if(info) {
		memset(info, 0, sizeof *info);
		info->struct_size = sizeof *info; info->nfft = N; info->window = m.window; info->stride = m.stride; info->line_segments = s.R; info->ring_lines = s.ring;
		info->sample_rate = c->cfg.input_rate ? c->cfg.input_rate : (uint32_t)kSymbolRate * kSps * c->cfg.oversample;
		info->centerfreq = c->cfg.centerfreq;
		info->first_segment = s.a0; info->first_sample = s.a0 * m.stride * N;
		info->lines = s.seen / s.R; info->hold_segments = s.hold_segments; info->hold_lines = s.hold_lines;
	}
	if(reset) {
		// (on the front stream: behind the launches that are queued, ahead of the next feed's; the ring and the line under way stay)
		HIPCHK(specgram_clear_hold(c));
		HIPCHK(m.tap.mark(c->streams.front));
		s.hold_segments = s.hold_lines = 0;
	}
	return (int)N;
}
int vdl2hip_specgram_lines(vdl2hip_ctx *c, int64_t first_line, float *mean, float *max, size_t cap_lines) {
	if(!c || !c->spg.on || !c->mon.on) return VDL2HIP_E_INVAL;
	auto &m = c->mon; auto &s = c->spg;
	const uint64_t lines = s.seen / s.R;
	if(first_line < 0 || (uint64_t)first_line > lines || lines - (uint64_t)first_line > s.ring) return VDL2HIP_E_INVAL;
	const size_t n = std::min<size_t>(std::min<size_t>(cap_lines, (size_t)(lines - (uint64_t)first_line)), 0x7fffffffu);
	if(n == 0 || (!mean && !max)) return (int)n;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	const size_t N = m.nfft, p0 = (size_t)((uint64_t)first_line & (s.ring - 1)), n0 = std::min<size_t>(n, s.ring - p0);
	for(int k = 0; k < 2; k++) {
		float *dst = k ? max : mean;
		const float *plane = k ? s.buf.d_ring_max : s.buf.d_ring_mean;
		if(!dst) continue;
		HIPCHK(m.tap.fetch(dst, plane + p0 * N, n0 * N * sizeof(float)));
		if(n0 < n) HIPCHK(m.tap.fetch(dst + n0 * N, plane, (n - n0) * N * sizeof(float)));
	}
	return (int)n;
}
// the bins of channel f: those within 12.5 kHz, or the nearest one (vdl2hip_spectrum_channels)
template<typename F>
static void channel_bins(const vdl2hip_ctx *c, double f, F take) {
	const uint32_t N = c->mon.nfft;
	const double fs = (double)(c->cfg.input_rate ? c->cfg.input_rate : (uint32_t)kSymbolRate * kSps * c->cfg.oversample), cf = (double)c->cfg.centerfreq;
	double best = 0.0; bool any = false; uint32_t nearest = 0;
	for(uint32_t i = 0; i < N; i++) {
		const double d = std::fabs(cf + ((double)i - (double)(N / 2)) * fs / (double)N - f);
		if(d <= 12500.0) { take(i); any = true; }
		if(i == 0 || d < best) { best = d; nearest = i; }
	}
	if(!any) take(nearest);
}
int vdl2hip_specgram_channels(vdl2hip_ctx *c, float *peak_dbfs, float *floor_dbfs, size_t cap) {
	if(!c || !c->spg.on || !c->mon.on) return VDL2HIP_E_INVAL;
	const size_t nchan = c->all_freqs.size();
	if((peak_dbfs || floor_dbfs) && cap < nchan) return VDL2HIP_E_TOOBIG;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	std::vector<float> hold;
	{ int r = specgram_fetch_hold(c, hold); if(r != VDL2HIP_OK) return r; }
	const uint32_t N = c->mon.nfft;
	for(size_t ch = 0; ch < nchan; ch++) {
		double peak = 0.0, sum = 0.0;
		channel_bins(c, (double)c->all_freqs[ch], [&](uint32_t i) { peak = std::max(peak, (double)hold[i]); sum += (double)hold[N + i]; });
		if(peak_dbfs) peak_dbfs[ch] = peak > 0.0 ? (float)(10.0 * std::log10(peak)) : -INFINITY;
		if(floor_dbfs) floor_dbfs[ch] = sum > 0.0 ? (float)(10.0 * std::log10(sum / c->mon.enbw)) : -INFINITY;
	}
	return (int)nchan;
}

// ---- the input monitor (vdl2hip.h, "Input monitor"; kernels: spectrum.h) ----
// Its share of a feed: on the front stream ahead of everything else that reads the block, so it is ordered with the copy into
// d_in[k], with that buffer's reuse and with a caller's device buffer exactly as the channeliser is.
// Host bookkeeping: the stream position (64 bits), the segments this feed completes, which of them are analysed, what is carried.
template<int FMT>
static void launch_spectrum(vdl2hip_ctx *c, const SpecArgs &a, unsigned grid, hipEvent_t e0, hipEvent_t e1) {
	#define SPEC_LAUNCH(PER) hipExtLaunchKernelGGL((k_spectrum<FMT, PER>), dim3(grid), dim3(c->mon.threads), (uint32_t)c->mon.lds, c->streams.front, e0, e1, 0, a)
	switch(c->mon.nfft / c->mon.threads) {                           // samples per lane (spec_threads(): 1, 2, 4 up to N = 1024, 8, 16)
		case 1: SPEC_LAUNCH(1); break;
		case 2: SPEC_LAUNCH(2); break;
		case 4: SPEC_LAUNCH(4); break;
		case 8: SPEC_LAUNCH(8); break;
		default: SPEC_LAUNCH(16); break;
	}
	#undef SPEC_LAUNCH
}
// the spectrogram's build of the same launch (specgram_plan)
template<int FMT>
static void launch_spectrum_lines(vdl2hip_ctx *c, const SpecArgs &a, const SpgArgs &sg, unsigned grid, hipEvent_t e0, hipEvent_t e1) {
	#define SPEC_LAUNCH(PER) hipExtLaunchKernelGGL((k_spectrum_lines<FMT, PER>), dim3(grid), dim3(c->mon.threads), (uint32_t)c->mon.lds, c->streams.front, e0, e1, 0, a, sg)
	switch(c->mon.nfft / c->mon.threads) {
		case 1: SPEC_LAUNCH(1); break;
		case 2: SPEC_LAUNCH(2); break;
		case 4: SPEC_LAUNCH(4); break;
		case 8: SPEC_LAUNCH(8); break;
		default: SPEC_LAUNCH(16); break;
	}
	#undef SPEC_LAUNCH
}
static int monitor_block(vdl2hip_ctx *c, const void *dev_in, size_t nbytes) {
	auto &m = c->mon;
	const uint64_t nin = nbytes / raw_bytes(c->in_fmt);
	if(nin == 0) return VDL2HIP_OK;
	if(nin >= (1ull << 32)) return VDL2HIP_E_TOOBIG;
	const uint64_t N = m.nfft, pos0 = m.pos, pos1 = pos0 + nin;
	const uint64_t j0 = pos0 / N, j1 = pos1 / N;                          // the segments the stream stands in before and after: [j0, j1) are completed
	const uint64_t ja = (j0 + m.stride - 1) / m.stride * m.stride;        // the first of them that is analysed
	const uint64_t nseg = ja < j1 ? (j1 - 1 - ja) / m.stride + 1 : 0;
	const uint32_t o1 = (uint32_t)(pos1 % N);
	const uint32_t ncarry_out = j1 % m.stride == 0 ? o1 : 0;               // (a segment that stride skips is not kept)
	m.pos = pos1;
	if(nseg == 0 && ncarry_out == 0) { m.ncarry = 0; return VDL2HIP_OK; }
	SpecArgs a{};
	a.in = dev_in; a.carry_in = m.buf.d_carry[m.carry_sel]; a.carry_out = m.buf.d_carry[m.carry_sel ^ 1]; a.w = m.buf.d_w; a.tw = m.buf.d_tw; a.rows = m.buf.d_rows;
	a.rel0 = (int64_t)(ja * N) - (int64_t)pos0; a.carry_rel = (int64_t)(j1 * N) - (int64_t)pos0; a.seg_step = (uint64_t)m.stride * N;
	a.nin = (uint32_t)nin; a.ncarry = m.ncarry; a.ncarry_out = ncarry_out; a.nseg = (uint32_t)nseg;
	a.N = m.nfft; a.log2n = m.log2n;
	uint32_t grid = 1;
	spg_split(nseg, kSpecMaxRows, a.run, grid);                                             // (no segment: workgroup 0 still moves the carry on)
	if(grid > kSpecMaxRows || (int64_t)a.ncarry + a.rel0 < 0) return VDL2HIP_E_INVAL;       // (never)
	// the spectrogram, where it is on and the feed analyses a segment: its build of the kernel, and its combine kernel behind the reduction
	const bool lines = c->spg.on && nseg != 0;
	SpgArgs sg{};
	if(lines && !specgram_plan(c, nseg, sg)) return VDL2HIP_E_INVAL;                        // (never)
	OutSlot &sl = c->slot[c->feed_no % kSlots];
	{ int r = collect_slot(c, sl); if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r; }   // (the feed is about to do the same) its events are about to be reused
	KernelTimes &t = sl.mon_t;
	t.arm(c->profiling >= 2);
	if(lines) with_fmt(c->in_fmt, [&](auto F) { launch_spectrum_lines<F()>(c, a, sg, grid, t.e(0), t.e(1)); });
	else with_fmt(c->in_fmt, [&](auto F) { launch_spectrum<F()>(c, a, grid, t.e(0), t.e(1)); });
	if(nseg) {
		const uint32_t W = m.nfft + kSpecLevels;
		hipExtLaunchKernelGGL(k_spectrum_reduce, dim3((W + 255) / 256), dim3(256), 0u, c->streams.front, t.e(2), lines ? (hipEvent_t) nullptr : t.e(3), 0,
		                      (const double *)m.buf.d_rows, m.buf.d_acc.get(), (uint32_t)grid, m.nfft);
		if(lines) specgram_launch_combine(c, sg, t.e(3));                                   // (the second pair of events spans both)
	}
	HIPCHK(hipGetLastError());
	HIPCHK(m.tap.mark(c->streams.front));
	t.launched(nseg ? 2 : 1);
	m.segments += nseg; m.ordinal += nseg; m.carry_sel ^= 1; m.ncarry = ncarry_out;
	return VDL2HIP_OK;
}
// wait for what the monitor has queued and give its buffers back (event, stream and landing place stay with the context: m.tap;
// what its launches took of the slots' feeds is not a later monitor's)
static void monitor_free(vdl2hip_ctx *c) {
	auto &m = c->mon;
	if(m.tap.queued) (void)hipEventSynchronize(m.tap.last);
	specgram_free(c);                                                // (a spectrogram's state would no longer mean anything)
	m.buf = {};
	for(auto &sl : c->slot) sl.mon_t.n = 0;
	m.on = false; m.tap.queued = false; m.nfft = 0;
}
// the accumulators as they stand once everything the monitor has queued is done: [nfft] sums of |X|^2, then the level sums
static int monitor_fetch(vdl2hip_ctx *c, std::vector<double> &acc) {
	auto &m = c->mon;
	acc.assign((size_t)m.nfft + kSpecLevels, 0.0);
	if(!m.tap.queued) return VDL2HIP_OK;                             // nothing has touched them since they were zeroed
	HIPCHK(m.tap.fetch(m.tap.land, m.buf.d_acc, m.buf.d_acc.bytes()));
	memcpy(acc.data(), m.tap.land, m.buf.d_acc.bytes());
	return VDL2HIP_OK;
}
static void monitor_power(const vdl2hip_ctx *c, const std::vector<double> &acc, double *power) {
	const auto &m = c->mon;
	const double scale = m.segments ? 1.0 / ((double)m.segments * m.sum_w * m.sum_w) : 0.0;
	for(uint32_t i = 0; i < m.nfft; i++) power[i] = acc[i] * scale;
}
int vdl2hip_spectrum_window(uint32_t nfft, uint32_t window, float *w, size_t cap) {
	SpectrumDesign d;
	if(!design_spectrum(nfft, window, d, false)) return VDL2HIP_E_INVAL;
	if(!w || cap < nfft) return VDL2HIP_E_TOOBIG;
	memcpy(w, d.w.data(), (size_t)nfft * sizeof(float));
	return (int)nfft;
}
int vdl2hip_spectrum_enable(vdl2hip_ctx *c, const vdl2hip_spectrum_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_spectrum_cfg)) return VDL2HIP_E_INVAL;
	SpectrumDesign d;
	if(cfg->nfft != 0 && !design_spectrum(cfg->nfft, cfg->window, d)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	auto &m = c->mon;
	monitor_free(c);
	if(cfg->nfft == 0) return VDL2HIP_OK;
	HIPCHK(m.tap.last.ensure(hipEventDisableTiming));
	if(!m.tap.rd) HIPCHK(hipStreamCreateWithFlags(&m.tap.rd, hipStreamNonBlocking));
	if(!m.tap.land) HIPCHK(m.tap.land.alloc(((size_t)kSpecMaxN + kSpecLevels) * sizeof(double)));
	const size_t N = cfg->nfft, W = N + kSpecLevels;
	auto &b = m.buf;
	if(b.d_w.alloc(N) != hipSuccess || b.d_tw.alloc(N) != hipSuccess || b.d_carry[0].alloc(N) != hipSuccess || b.d_carry[1].alloc(N) != hipSuccess
	   || b.d_rows.alloc((size_t)kSpecMaxRows * W) != hipSuccess || b.d_acc.alloc(W) != hipSuccess) { monitor_free(c); return VDL2HIP_E_NOMEM; }
	if(hipMemcpy(b.d_w, d.w.data(), b.d_w.bytes(), hipMemcpyHostToDevice) != hipSuccess
	   || hipMemcpy(b.d_tw, d.tw.data(), b.d_tw.bytes(), hipMemcpyHostToDevice) != hipSuccess
	   || hipMemset(b.d_acc, 0, b.d_acc.bytes()) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { monitor_free(c); return VDL2HIP_E_DEVICE; }
	m.nfft = cfg->nfft; m.window = cfg->window; m.stride = cfg->stride ? cfg->stride : 1; m.log2n = d.log2n;
	m.threads = spec_threads(m.nfft); m.lds = spec_lds_bytes(m.nfft);
	m.sum_w = d.sum_w; m.enbw = d.enbw_bins;
	m.pos = 0; m.segments = 0; m.ordinal = 0; m.ncarry = 0; m.carry_sel = 0; m.kernel_ms = 0.0; m.tap.queued = false;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_spectrum_read(vdl2hip_ctx *c, vdl2hip_spectrum_info *info, double *power, size_t cap, int reset) {
	if(!c || !c->mon.on || (info && info->struct_size != sizeof(vdl2hip_spectrum_info))) return VDL2HIP_E_INVAL;
	auto &m = c->mon;
	if(power && cap < m.nfft) return VDL2HIP_E_TOOBIG;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	std::vector<double> acc;
	{ int r = monitor_fetch(c, acc); if(r != VDL2HIP_OK) return r; }
	const uint32_t N = m.nfft;
	if(info) {
		memset(info, 0, sizeof *info);
		info->struct_size = sizeof *info; info->nfft = N; info->window = m.window; info->stride = m.stride;
		info->sample_rate = c->cfg.input_rate ? c->cfg.input_rate : (uint32_t)kSymbolRate * kSps * c->cfg.oversample;
		info->centerfreq = c->cfg.centerfreq;
		info->segments = m.segments; info->samples = m.segments * N; info->clipped = (uint64_t)acc[N + 3];
		info->enbw_bins = m.enbw;
		if(info->samples) { const double n = (double)info->samples; info->mean_power = acc[N] / n; info->dc_i = acc[N + 1] / n; info->dc_q = acc[N + 2] / n; }
		info->peak = (float)acc[N + 4];
		info->kernel_ms = (float)m.kernel_ms;
	}
	if(power) monitor_power(c, acc, power);
	if(reset) {
		// (on the front stream: behind the launches that are queued, ahead of the next feed's)
		HIPCHK(hipMemsetAsync(m.buf.d_acc, 0, m.buf.d_acc.bytes(), c->streams.front));
		HIPCHK(m.tap.mark(c->streams.front));
		m.segments = 0;
	}
	return (int)N;
}
int vdl2hip_spectrum_channels(vdl2hip_ctx *c, float *dbfs, size_t cap) {
	if(!c || !c->mon.on || !dbfs) return VDL2HIP_E_INVAL;
	auto &m = c->mon;
	const size_t nchan = c->all_freqs.size();
	if(cap < nchan) return VDL2HIP_E_TOOBIG;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	std::vector<double> acc;
	{ int r = monitor_fetch(c, acc); if(r != VDL2HIP_OK) return r; }
	const uint32_t N = m.nfft;
	std::vector<double> power(N);
	monitor_power(c, acc, power.data());
	const double fs = (double)(c->cfg.input_rate ? c->cfg.input_rate : (uint32_t)kSymbolRate * kSps * c->cfg.oversample), cf = (double)c->cfg.centerfreq;
	for(size_t ch = 0; ch < nchan; ch++) {
		const double f = (double)c->all_freqs[ch];
		double sum = 0.0, best = 0.0; bool any = false; uint32_t nearest = 0;
		for(uint32_t i = 0; i < N; i++) {
			const double d = std::fabs(cf + ((double)i - (double)(N / 2)) * fs / (double)N - f);
			if(d <= 12500.0) { sum += power[i]; any = true; }
			if(i == 0 || d < best) { best = d; nearest = i; }
		}
		if(!any) sum = power[nearest];
		dbfs[ch] = sum > 0.0 ? (float)(10.0 * std::log10(sum / m.enbw)) : -INFINITY;
	}
	return (int)nchan;
}

// ---- the burst capture (vdl2hip.h, "Burst capture"; kernels: capture.h) ----
// The ring behind the window.  The capture of feed i reads y from iq_first >= sync_sample - kCapMaxPre on, while the channelisers
// of up to kSlots - 1 later feeds may be writing (feed i + kSlots takes feed i's slot, and collect_slot() has waited for feed i
// before that).  They write [k_end, k_end + (kSlots - 1) dmax), which in a ring of `cap` >= kSlots dmax + kHistory + 1024 samples
// (vdl2hip_create) lands on samples older than k_end - dmax - kHistory - 1024 <= k0 - kHistory - 1024, k0 being feed i's first
// sample.  A burst is handed over in the feed that brings its last symbol, so end_sample >= k0; the longest burst is 56 320 samples
// from its first symbol to its last and its sync lies a unique word before that: iq_first > k0 - 56 320 - 200 - 4 096 = k0 - 60 616
// > k0 - kHistory - 1024 = k0 - 66 560.  The 5 944 samples between the two are why pre stops at 4 096.  A window is at most
// 4 096 + 56 520 + 1 024 < 2^16 pairs long.
static_assert(kCapMaxPre + 56320 + 200 < kHistory + 1024, "a window begins inside what the ring keeps behind a feed");
static_assert(sizeof(CapRec) == sizeof(vdl2hip_burst) && sizeof(vdl2hip_burst) == 128 && offsetof(CapRec, iq_first) == offsetof(vdl2hip_burst, iq_first)
              && offsetof(CapRec, frames) == offsetof(vdl2hip_burst, frames) && offsetof(CapRec, mean_power) == offsetof(vdl2hip_burst, mean_power)
              && offsetof(CapRec, phase_err_max) == offsetof(vdl2hip_burst, phase_err_max), "the host copies the device's records as they are");
static_assert(sizeof(vdl2hip_capture_cfg) == 24 && sizeof(vdl2hip_capture_info) == 56 && sizeof(CapHdr) == 16, "vdl2hip.h states these sizes");
static_assert(kCapMaxChan == kK5MaxChan, "k_capture_copy keeps every channel's offsets in LDS");

// Its share of a feed (launch_rest): behind the frame finisher on the feed's burst stream, where both passes of the burst decoder are done
static int capture_launch(vdl2hip_ctx *c, OutSlot &sl, hipStream_t st) {
	auto &m = c->capt;
	CapArgs a{};
	a.y = c->d_y; a.bursts = sl.d_bursts; a.nb_chan = sl.d_nbchan; a.freq = c->d_freq;
	a.plan = sl.cap.d_plan; a.tot = sl.cap.d_tot; a.rec = sl.cap.mail.d_rec(); a.pool = sl.cap.d_pool; a.hdr = sl.cap.mail.d_hdr();
	a.k_end = sl.back_k0 + sl.back_D; a.pool_samples = m.pool; a.cap_bursts_chan = c->cap_bursts_chan; a.nchan = (uint32_t)c->C; a.chan_first = (uint32_t)c->chan_first;
	a.cap = c->cap; a.mask = c->cap - 1; a.pre = m.pre; a.post = m.post;
	KernelTimes &t = sl.cap.times;
	t.arm(c->profiling >= 2);
	hipExtLaunchKernelGGL(k_capture_plan, dim3((unsigned)c->C), dim3(64), 0u, st, t.e(0), t.e(1), 0, a);
	// a workgroup per burst, bounded like the burst decoder's wavefronts (16 .. 2048 of them, by the feed's size): 8 .. 512
	const unsigned grid = std::min(512u, std::max(8u, sl.k5_waves / 4));
	hipExtLaunchKernelGGL(k_capture_copy, dim3(grid), dim3(kCapThreads), 0u, st, t.e(2), t.e(3), 0, a);
	HIPCHK(hipGetLastError());
	HIPCHK(sl.cap.mail.post(st));
	t.launched(2);
	return VDL2HIP_OK;
}
// A collected feed's records and the used part of its IQ pool - one staging buffer, one wait - joined with the feed's frames - all of
// them, whatever the AVLC filter lets through - and appended to the queue.
static int capture_collect(vdl2hip_ctx *c, OutSlot &sl, const OutFrame *fr, uint32_t nf) {
	auto &m = c->capt;
	if(!m.on || !sl.cap.mail) return VDL2HIP_OK;
	const CapHdr h = sl.cap.mail.hdr();
	const uint32_t nrec = (uint32_t)std::min<uint64_t>(h.nrec, (uint64_t)c->C * c->cap_bursts_chan);
	const uint64_t pairs = std::min<uint64_t>(h.pairs, m.pool);
	if(nrec == 0) return VDL2HIP_OK;
	const CapRec *rec = nullptr;
	const size_t rec_bytes = sl.cap.mail.staged(nrec), iq_bytes = (size_t)pairs * sizeof(cf32);
	HIPCHK(sl.cap.mail.fetch(nrec, m.stage, c->streams.out, rec, false, iq_bytes));
	if(pairs) HIPCHK(hipMemcpyAsync(m.stage + rec_bytes, sl.cap.d_pool, iq_bytes, hipMemcpyDeviceToHost, c->streams.out));
	if(rec_bytes + iq_bytes) HIPCHK(hipStreamSynchronize(c->streams.out));
	const float *iqp = reinterpret_cast<const float *>(m.stage + rec_bytes);
	auto iq = pairs ? std::make_shared<std::vector<float>>(iqp, iqp + 2 * (size_t)pairs) : std::make_shared<std::vector<float>>();
	struct Join { uint32_t frames = 0, ok = 0; int32_t fec = -1, last_idx = -1; };
	std::map<std::pair<int32_t, int64_t>, Join> join;
	for(uint32_t i = 0; i < nf; i++) {
		if(fr[i].chan < 0 || fr[i].chan >= c->C) continue;
		Join &j = join[{ fr[i].chan + c->chan_first, fr[i].burst_ord }];
		j.frames++; if(fr[i].avlc_status == AVLC_OK) j.ok++;
		if(fr[i].idx >= j.last_idx) { j.last_idx = fr[i].idx; j.fec = fr[i].num_fec_corrections; }
	}
	for(uint32_t i = 0; i < nrec; i++) {
		vdl2hip_burst r;
		memcpy(&r, rec + i, sizeof r);
		if(r.iq_off + r.iq_count > pairs) { r.iq_count = 0; r.iq_off = 0; r.flags |= VDL2HIP_BURST_NO_ROOM; }      // (never)
		m.bursts++; m.iq_samples += r.iq_count; if(r.flags & VDL2HIP_BURST_NO_ROOM) m.iq_dropped++;
		auto it = join.find({ (int32_t)r.chan, r.burst_ord });
		if(it != join.end()) { r.frames = it->second.frames; r.frames_ok = it->second.ok; r.fec_corrections = it->second.fec; }
		if((m.flags & VDL2HIP_CAPTURE_FAILED_ONLY) && r.frames_ok != 0) continue;
		m.queue.push_back(vdl2hip_ctx::CapItem{ r, iq });
	}
	return VDL2HIP_OK;
}
// give the capture's buffers back (nothing of it may be in flight: the callers have collected every feed)
static void capture_free(vdl2hip_ctx *c) {
	for(auto &sl : c->slot) sl.cap.reset();
	c->capt.queue.clear();
	c->capt.on = false;
}
int vdl2hip_capture_enable(vdl2hip_ctx *c, const vdl2hip_capture_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_capture_cfg) || cfg->reserved != 0) return VDL2HIP_E_INVAL;
	if(cfg->pre_samples > kCapMaxPre || cfg->post_samples > kCapMaxPost || (cfg->flags & ~VDL2HIP_CAPTURE_FAILED_ONLY) || cfg->pool_samples > kCapMaxPool) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }        // nothing of an earlier capture is in flight any more
	auto &m = c->capt;
	capture_free(c);
	const uint32_t pool = cfg->pool_samples ? cfg->pool_samples : kCapDefPool;
	const size_t nb = (size_t)c->C * c->cap_bursts_chan;
	for(auto &sl : c->slot) {
		auto &b = sl.cap;
		const hipError_t mail = b.mail.alloc(nb);
		const bool ok = mail == hipSuccess && b.d_plan.alloc(nb) == hipSuccess && b.d_tot.alloc((size_t)c->C) == hipSuccess && b.d_pool.alloc(pool) == hipSuccess;
		// (a mail that stands and still reports an error: its allocations succeeded, clearing it did not)
		if(!ok) { const bool cleared = mail == hipSuccess || !b.mail; capture_free(c); return cleared ? VDL2HIP_E_NOMEM : VDL2HIP_E_DEVICE; }
	}
	if(hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); capture_free(c); return VDL2HIP_E_DEVICE; }
	m.pre = cfg->pre_samples; m.post = cfg->post_samples; m.flags = cfg->flags; m.pool = pool;
	m.bursts = m.iq_samples = m.iq_dropped = 0; m.kernel_ms = 0.0;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_capture_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->capt.on && !c->failed) { int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	capture_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_capture_info_get(vdl2hip_ctx *c, vdl2hip_capture_info *info) {
	if(!c || !c->capt.on || !info || info->struct_size != sizeof(vdl2hip_capture_info)) return VDL2HIP_E_INVAL;
	const auto &m = c->capt;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info; info->pre_samples = m.pre; info->post_samples = m.post; info->flags = m.flags; info->pool_samples = m.pool;
	info->bursts = m.bursts; info->iq_samples = m.iq_samples; info->iq_dropped = m.iq_dropped; info->kernel_ms = (float)m.kernel_ms;
	return VDL2HIP_OK;
}
// (its own: a record goes out with its IQ, packed behind the IQ of the records before it)
int vdl2hip_capture_read(vdl2hip_ctx *c, vdl2hip_burst *recs, size_t cap_recs, float *iq, size_t cap_pairs, size_t *pairs_used) {
	if(!c || !c->capt.on || (!recs && cap_recs) || (!iq && cap_pairs)) return VDL2HIP_E_INVAL;
	auto &q = c->capt.queue;
	size_t n = 0, used = 0;
	while(!q.empty() && n < cap_recs) {
		const vdl2hip_ctx::CapItem &it = q.front();
		if(used + it.r.iq_count > cap_pairs) break;
		recs[n] = it.r;
		recs[n].iq_off = used;
		if(it.r.iq_count) memcpy(iq + 2 * used, it.iq->data() + 2 * it.r.iq_off, (size_t)it.r.iq_count * 2 * sizeof(float));
		used += it.r.iq_count;
		n++;
		q.pop_front();
	}
	if(pairs_used) *pairs_used = used;
	return (int)n;
}

// ---- burst timing (vdl2hip.h, "Burst timing"; kernel: toa.h; the template: toa_design.h) ----
// The ring behind the window.  Under the burst capture's conditions (above) a burst's first symbol lies after k0 - 56 320, k0 being the
// first sample of the feed that decodes it; the window begins a unique word and W samples before that: t0 - W > k0 - 56 320 - 160 - 32
// > k0 - kHistory - 1024.  It ends at t0 + W + 150 < first_symbol + 32, inside the header the walker has already read.
static_assert(56320 + kToaLead + kToaMaxLag < kHistory + 1024, "a window begins inside what the ring keeps behind a feed");
static_assert(sizeof(ToaRec) == sizeof(vdl2hip_burst_toa) && sizeof(vdl2hip_burst_toa) == 96 && offsetof(ToaRec, peak_sample) == offsetof(vdl2hip_burst_toa, peak_sample)
              && offsetof(ToaRec, peak_lag) == offsetof(vdl2hip_burst_toa, peak_lag) && offsetof(ToaRec, toa_frac) == offsetof(vdl2hip_burst_toa, toa_frac)
              && offsetof(ToaRec, resid) == offsetof(vdl2hip_burst_toa, resid) && offsetof(ToaRec, flags) == offsetof(vdl2hip_burst_toa, flags)
              && offsetof(vdl2hip_burst_toa, flags) == 80 && offsetof(ToaRec, curve_off) == offsetof(vdl2hip_burst_toa, curve_off), "the host copies the device's records as they are");
static_assert(sizeof(vdl2hip_toa_cfg) == 16 && sizeof(vdl2hip_toa_info) == 64 && sizeof(ToaHdr) == 16, "vdl2hip.h states these sizes");
static_assert(VDL2HIP_TOA_EARLY == kToaEarly && VDL2HIP_TOA_EDGE == kToaEdge && VDL2HIP_TOA_FLAT == kToaFlat && VDL2HIP_TOA_NO_CURVE == kToaNoCurve, "the record's flags");
static_assert(kCapMaxChan == kK5MaxChan && kToaWin <= kToaThreads, "k_toa keeps every channel's offsets in LDS and stages a window with a lane per sample");

// Its share of a feed (launch_rest): behind the frame finisher on the feed's burst stream, like the capture
static int toa_launch(vdl2hip_ctx *c, OutSlot &sl, hipStream_t st) {
	auto &m = c->toa;
	ToaArgs a{};
	a.y = c->d_y; a.bursts = sl.d_bursts; a.nb_chan = sl.d_nbchan; a.freq = c->d_freq; a.s = m.d_s;
	a.rec = sl.toa.mail.d_rec(); a.curve = sl.toa.d_curve; a.hdr = sl.toa.mail.d_hdr();
	a.e_s = m.e_s; a.cap_bursts_chan = c->cap_bursts_chan; a.nchan = (uint32_t)c->C; a.chan_first = (uint32_t)c->chan_first;
	a.cap = c->cap; a.mask = c->cap - 1; a.W = m.W; a.pool_curves = m.pool_curves;
	KernelTimes &t = sl.toa.times;
	t.arm(c->profiling >= 2);
	// a workgroup per burst, bounded like the capture's: 8 .. 512
	const unsigned grid = std::min(512u, std::max(8u, sl.k5_waves / 4));
	hipExtLaunchKernelGGL(k_toa, dim3(grid), dim3(kToaThreads), 0u, st, t.e(0), t.e(1), 0, a);
	HIPCHK(hipGetLastError());
	HIPCHK(sl.toa.mail.post(st));
	t.launched(1);
	return VDL2HIP_OK;
}
// A collected feed's records and the curves of the first pool_curves of them - one staging buffer, one wait - joined with the feed's
// frames as the capture's are and appended to the queue.
static int toa_collect(vdl2hip_ctx *c, OutSlot &sl, const OutFrame *fr, uint32_t nf) {
	auto &m = c->toa;
	if(!m.on || !sl.toa.mail) return VDL2HIP_OK;
	const uint32_t nrec = (uint32_t)std::min<uint64_t>(sl.toa.mail.hdr().nrec, (uint64_t)c->C * c->cap_bursts_chan);
	if(nrec == 0) return VDL2HIP_OK;
	const uint32_t nlags = 2 * m.W + 1, ncurve = std::min(nrec, m.pool_curves);
	const ToaRec *rec = nullptr;
	const size_t rec_bytes = sl.toa.mail.staged(nrec), cv_bytes = (size_t)ncurve * nlags * sizeof(float);
	HIPCHK(sl.toa.mail.fetch(nrec, m.stage, c->streams.out, rec, false, cv_bytes));
	HIPCHK(hipMemcpyAsync(m.stage + rec_bytes, sl.toa.d_curve, cv_bytes, hipMemcpyDeviceToHost, c->streams.out));
	HIPCHK(hipStreamSynchronize(c->streams.out));
	const float *cvp = reinterpret_cast<const float *>(m.stage + rec_bytes);
	auto curves = std::make_shared<std::vector<float>>(cvp, cvp + (size_t)ncurve * nlags);
	struct Join { uint32_t frames = 0, ok = 0; };
	std::map<std::pair<int32_t, int64_t>, Join> join;
	for(uint32_t i = 0; i < nf; i++) {
		if(fr[i].chan < 0 || fr[i].chan >= c->C) continue;
		Join &j = join[{ fr[i].chan + c->chan_first, fr[i].burst_ord }];
		j.frames++; if(fr[i].avlc_status == AVLC_OK) j.ok++;
	}
	for(uint32_t i = 0; i < nrec; i++) {
		vdl2hip_burst_toa r;
		memcpy(&r, rec + i, sizeof r);
		if(i < ncurve && !(r.flags & VDL2HIP_TOA_NO_CURVE) && r.nlags == nlags) r.curve_off = i * nlags;
		else { r.flags |= VDL2HIP_TOA_NO_CURVE; r.curve_off = 0; }
		m.bursts++; if(r.flags & VDL2HIP_TOA_NO_CURVE) m.curves_dropped++; else m.curves++;
		if(r.flags & VDL2HIP_TOA_EARLY) m.early++;
		if(r.flags & VDL2HIP_TOA_EDGE) m.edge++;
		auto it = join.find({ (int32_t)r.chan, r.burst_ord });
		if(it != join.end()) { r.frames = it->second.frames; r.frames_ok = it->second.ok; }
		if((m.flags & VDL2HIP_TOA_FAILED_ONLY) && r.frames_ok != 0) continue;
		m.queue.push_back(vdl2hip_ctx::ToaItem{ r, curves });
	}
	return VDL2HIP_OK;
}
// give the tap's buffers back (nothing of it may be in flight: the callers have collected every feed)
static void toa_free(vdl2hip_ctx *c) {
	for(auto &sl : c->slot) sl.toa.reset();
	c->toa.d_s.reset();
	c->toa.queue.clear();
	c->toa.on = false;
}
int vdl2hip_toa_template(float *s, size_t cap_pairs) {
	if(!s) return VDL2HIP_E_INVAL;
	if(cap_pairs < (size_t)kToaTaps) return VDL2HIP_E_TOOBIG;
	ToaDesign d;
	design_toa(d);
	memcpy(s, d.s, sizeof d.s);
	return kToaTaps;
}
int vdl2hip_toa_enable(vdl2hip_ctx *c, const vdl2hip_toa_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_toa_cfg)) return VDL2HIP_E_INVAL;
	if(cfg->max_lag > kToaMaxLag || (cfg->flags & ~VDL2HIP_TOA_FAILED_ONLY)) return VDL2HIP_E_INVAL;
	const uint32_t W = cfg->max_lag ? cfg->max_lag : kToaDefLag, nlags = 2 * W + 1, pool_curves = cfg->pool_curves ? cfg->pool_curves : kToaDefCurves;
	if((uint64_t)pool_curves * nlags > kToaMaxPool) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }        // nothing of an earlier tap is in flight any more
	auto &m = c->toa;
	toa_free(c);
	ToaDesign d;
	design_toa(d);
	const size_t nb = (size_t)c->C * c->cap_bursts_chan;
	bool ok = m.d_s.alloc(kToaTaps) == hipSuccess;
	// (a feed has at most nb records: no more curves than that)
	for(auto &sl : c->slot) ok = ok && sl.toa.mail.alloc(nb) == hipSuccess && sl.toa.d_curve.alloc(std::min<size_t>(nb, pool_curves) * nlags) == hipSuccess;
	if(!ok) { toa_free(c); return VDL2HIP_E_NOMEM; }
	if(hipMemcpy(m.d_s, d.s, sizeof d.s, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); toa_free(c); return VDL2HIP_E_DEVICE; }
	m.W = W; m.flags = cfg->flags; m.pool_curves = pool_curves; m.e_s = d.energy;
	m.bursts = m.curves = m.curves_dropped = m.early = m.edge = 0; m.kernel_ms = 0.0;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_toa_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->toa.on && !c->failed) { int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	toa_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_toa_info_get(vdl2hip_ctx *c, vdl2hip_toa_info *info) {
	if(!c || !c->toa.on || !info || info->struct_size != sizeof(vdl2hip_toa_info)) return VDL2HIP_E_INVAL;
	const auto &m = c->toa;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info; info->max_lag = m.W; info->flags = m.flags; info->pool_curves = m.pool_curves;
	info->bursts = m.bursts; info->curves = m.curves; info->curves_dropped = m.curves_dropped; info->early = m.early; info->edge = m.edge;
	info->kernel_ms = (float)m.kernel_ms;
	return VDL2HIP_OK;
}
// (its own: a record goes out with its curve, packed behind the curves of the records before it)
int vdl2hip_toa_read(vdl2hip_ctx *c, vdl2hip_burst_toa *recs, size_t cap_recs, float *curves, size_t cap_floats, size_t *floats_used) {
	if(!c || !c->toa.on || (!recs && cap_recs) || (!curves && cap_floats)) return VDL2HIP_E_INVAL;
	auto &q = c->toa.queue;
	size_t n = 0, used = 0;
	while(!q.empty() && n < cap_recs) {
		const vdl2hip_ctx::ToaItem &it = q.front();
		const size_t nfl = (it.r.flags & VDL2HIP_TOA_NO_CURVE) ? 0 : it.r.nlags;
		if(used + nfl > cap_floats || used + nfl > 0xffffffffull) break;
		recs[n] = it.r;
		recs[n].curve_off = (uint32_t)(nfl ? used : 0);
		if(nfl) memcpy(curves + used, it.curves->data() + it.r.curve_off, nfl * sizeof(float));
		used += nfl;
		n++;
		q.pop_front();
	}
	if(floats_used) *floats_used = used;
	return (int)n;
}

// ---- the second look (vdl2hip.h, "Second look"; kernels: relook.h) ----
// A tap on top of the preamble search, whose plan of the feed it reads and which switches it off (so it stands ahead of it here).  The
// ring behind an attempt: an anchor lies in the search's range, and every symbol an attempt reads lies at or before limit =
// last_sample + (H + 1) B, the last sample of the bin whose completion emits the record: inside the feed (the transmission capture's
// post window ends there too).
static_assert(sizeof(RlRec) == sizeof(vdl2hip_relook) && sizeof(vdl2hip_relook) == 256 && offsetof(RlRec, first_bin) == offsetof(vdl2hip_relook, first_bin)
              && offsetof(RlRec, anchor) == offsetof(vdl2hip_relook, anchor) && offsetof(RlRec, end_sample) == offsetof(vdl2hip_relook, end_sample)
              && offsetof(RlRec, pherr) == offsetof(vdl2hip_relook, pherr) && offsetof(vdl2hip_relook, pherr) == 32 && offsetof(RlRec, prev_phase) == offsetof(vdl2hip_relook, prev_phase)
              && offsetof(RlRec, tl_bits) == offsetof(vdl2hip_relook, tl_bits) && offsetof(RlRec, stop) == offsetof(vdl2hip_relook, stop) && offsetof(vdl2hip_relook, stop) == 60
              && offsetof(RlRec, frames) == offsetof(vdl2hip_relook, frames) && offsetof(RlRec, fec_corrections) == offsetof(vdl2hip_relook, fec_corrections)
              && offsetof(RlRec, frame_first) == offsetof(vdl2hip_relook, frame_first) && offsetof(RlRec, flags) == offsetof(vdl2hip_relook, flags) && offsetof(vdl2hip_relook, flags) == 84
              && offsetof(RlRec, counters) == offsetof(vdl2hip_relook, counters) && offsetof(vdl2hip_relook, counters) == 96, "the host copies the device's records as they are and fills in the rest");
static_assert(sizeof(vdl2hip_relook_cfg) == 32 && sizeof(vdl2hip_relook_info) == 96 && sizeof(RlHdr) == 32 && sizeof(RlPiece) == 128 && sizeof(RlPlan) == 32 && sizeof(RlAnchor) == 16, "vdl2hip.h states these sizes");
static_assert(VDL2HIP_RELOOK_PPM_REJECT == kRlPpmReject && VDL2HIP_RELOOK_TRUNCATED == kRlTruncated && VDL2HIP_RELOOK_NO_ROOM == kRlNoRoom
              && ((kRlPpmReject | kRlTruncated | kRlNoRoom) & kTxPartial) == 0, "the flags share a word");
constexpr unsigned kRlDecodeGrid = 256;       // wavefronts of k_relook_decode, an attempt each at a time
constexpr size_t kRlDecodeLds = ((sizeof(BurstShared) + 15) & ~(size_t)15) + sizeof(FrameShared);
static_assert(kRlDecodeLds + sizeof(OutCtl) + kNumCounters * 8 <= 65536, "k_relook_decode's wavefront has its BurstShared and FrameShared in LDS");
// FNV-1a, 64 bits: what the join compares beside the length
static uint64_t relook_hash(const uint8_t *p, uint32_t n) {
	uint64_t h = 0xcbf29ce484222325ull;
	for(uint32_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
	return h;
}
// Its share of a feed (launch_rest): directly behind the search's launches, whose plan it reads
static int relook_launch(vdl2hip_ctx *c, OutSlot &sl, hipStream_t st) {
	auto &m = c->rl;
	RlArgs a{};
	a.y = c->d_y; a.tab = c->d_tab; a.txhdr = sl.txl.mail.d_hdr(); a.txrec = sl.txl.mail.d_rec(); a.off = sl.txs.d_off; a.shdr = sl.txs.mail.d_hdr();
	a.piece = sl.rl.d_piece; a.rec = sl.rl.mail.d_rec(); a.plan = sl.rl.d_plan; a.hdr = sl.rl.mail.d_hdr(); a.frames = sl.rl.d_frames; a.pool = sl.rl.d_pool;
	a.acnt = sl.rl.d_acnt; a.nfring = c->d_nfring; a.frames_out = sl.rl.d_frames_out; a.pool_out = sl.rl.d_pool_out;
	a.thr = m.thr; a.max_ppm = m.max_ppm; a.max_anchors = m.max_anchors; a.pool_frames = m.pool_frames; a.pool_octets = m.pool_octets; a.rec_cap = m.rec_cap;
	a.piece_cap = c->txs.piece_cap; a.cap = c->cap; a.mask = c->cap - 1; a.chan_first = (uint32_t)c->chan_first; a.back = (c->act.H + 1) * c->act.B;
	KernelTimes &t = sl.rl.times;
	t.arm(c->profiling >= 2);
	// a workgroup per piece, grid-stride, sized as the search's
	const unsigned grid = (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(16, (uint64_t)sl.back_D * (uint64_t)c->C / (4 * kTxsPiece)));
	hipExtLaunchKernelGGL(k_relook_anchors, dim3(grid), dim3(kRlThreads), 0u, st, t.e(0), (hipEvent_t) nullptr, 0, a);
	hipLaunchKernelGGL(k_relook_select, dim3(1), dim3(kRlThreads), 0, st, a);
	hipLaunchKernelGGL(k_relook_decode, dim3(kRlDecodeGrid), dim3(64), (uint32_t)kRlDecodeLds, st, a);
	// what the attempts produced, packed: the host copies that, not the claims
	hipLaunchKernelGGL(k_relook_pack_plan, dim3(1), dim3(kRlThreads), 0, st, a);
	hipExtLaunchKernelGGL(k_relook_pack_copy, dim3(kRlDecodeGrid), dim3(64), 0u, st, (hipEvent_t) nullptr, t.e(1), 0, a);
	HIPCHK(hipGetLastError());
	HIPCHK(sl.rl.mail.post(st));
	t.launched(1);
	sl.rl.on = true;
	return VDL2HIP_OK;
}
// A collected feed's attempt records - in the order of the log's nrec records, a run of them per record - with the claimed part of
// its frame pool: one staging buffer, one wait
struct RlFeed { const RlRec *rec = nullptr; uint32_t natt = 0, cur = 0; std::shared_ptr<std::vector<OutFrame>> fr; std::shared_ptr<std::vector<uint8_t>> pool; };
static int relook_fetch(vdl2hip_ctx *c, OutSlot &sl, uint32_t nrec, RlFeed &f) {
	auto &m = c->rl;
	if(!m.on || !sl.rl.mail) return VDL2HIP_OK;
	const RlHdr h = sl.rl.mail.hdr();
	if(h.ntx != nrec) return VDL2HIP_E_DEVICE;                       // (never: both are the log's header of this feed)
	f.natt = std::min(h.nrec, m.rec_cap);
	const size_t nfr = std::min(h.frames_used, m.pool_frames), noct = std::min(h.octets_used, m.pool_octets);      // (what was produced, packed: not what was claimed)
	const size_t rec_bytes = sl.rl.mail.staged(f.natt), fr_bytes = nfr * sizeof(OutFrame);
	HIPCHK(sl.rl.mail.fetch(f.natt, m.stage, c->streams.out, f.rec, false, fr_bytes + noct));
	if(fr_bytes) HIPCHK(hipMemcpyAsync(m.stage + rec_bytes, sl.rl.d_frames_out, fr_bytes, hipMemcpyDeviceToHost, c->streams.out));
	if(noct) HIPCHK(hipMemcpyAsync(m.stage + rec_bytes + fr_bytes, sl.rl.d_pool_out, noct, hipMemcpyDeviceToHost, c->streams.out));
	if(rec_bytes + fr_bytes + noct) HIPCHK(hipStreamSynchronize(c->streams.out));
	const OutFrame *frp = reinterpret_cast<const OutFrame *>(m.stage + rec_bytes);
	f.fr = nfr ? std::make_shared<std::vector<OutFrame>>(frp, frp + nfr) : std::make_shared<std::vector<OutFrame>>();
	f.pool = noct ? std::make_shared<std::vector<uint8_t>>(m.stage + rec_bytes + fr_bytes, m.stage + rec_bytes + fr_bytes + noct) : std::make_shared<std::vector<uint8_t>>();
	m.records += nrec; m.anchors_found += h.anchors_found; m.dropped += h.dropped;
	return VDL2HIP_OK;
}
// ... the attempts of one log record, with what the log has joined to it: seen - (len, hash) of the main-path frames of the record
static void relook_take(vdl2hip_ctx *c, RlFeed &f, const vdl2hip_tx &tx, const std::vector<std::pair<uint32_t, uint64_t>> &seen) {
	auto &m = c->rl;
	for(; f.cur < f.natt && f.rec[f.cur].chan == tx.chan && f.rec[f.cur].first_bin == tx.first_bin; f.cur++) {
		vdl2hip_relook r;
		memcpy(&r, f.rec + f.cur, sizeof r);
		r.frames_new = 0; r.new_mask = 0; r.reserved = 0;
		if((size_t)r.frame_first + r.frames > f.fr->size()) { r.frames = r.frames_ok = 0; r.frame_first = 0; r.flags |= VDL2HIP_RELOOK_NO_ROOM; }      // (never)
		for(uint32_t k = 0; k < r.frames; k++) {
			const OutFrame &fr = (*f.fr)[r.frame_first + k];
			if((size_t)fr.pool_off + fr.len > f.pool->size() || fr.avlc_status != AVLC_OK) continue;
			const std::pair<uint32_t, uint64_t> key{ fr.len, relook_hash(f.pool->data() + fr.pool_off, fr.len) };
			if(std::find(seen.begin(), seen.end(), key) == seen.end()) { r.frames_new++; if(k < 32) r.new_mask |= 1u << k; }
		}
		m.attempts++; m.frames += r.frames; m.frames_ok += r.frames_ok; m.frames_new += r.frames_new; if(r.flags & VDL2HIP_RELOOK_NO_ROOM) m.dropped++;
		if((m.flags & VDL2HIP_RELOOK_NEW_ONLY) && r.frames_new == 0) continue;
		m.queue.push_back(vdl2hip_ctx::RlItem{ r, f.fr, f.pool });
	}
}
// give the second look's buffers back (nothing of it may be in flight: the callers have collected every feed)
static void relook_free(vdl2hip_ctx *c) {
	for(auto &sl : c->slot) sl.rl.reset();
	c->rl.queue.clear();
	c->rl.stage.reset();
	c->rl.on = false;
}
int vdl2hip_relook_enable(vdl2hip_ctx *c, const vdl2hip_relook_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_relook_cfg) || cfg->reserved != 0 || (cfg->flags & ~VDL2HIP_RELOOK_NEW_ONLY)) return VDL2HIP_E_INVAL;
	if(!c->txs.on || !c->txl.on || !c->act.on) return VDL2HIP_E_INVAL;
	if(!(cfg->threshold >= 0.f && cfg->threshold <= 30.f) || !(cfg->max_ppm >= 0.f) || std::isinf(cfg->max_ppm)) return VDL2HIP_E_INVAL;      // (a NaN fails both)
	if(cfg->max_anchors > kRlMaxAnchors || cfg->pool_frames > kRlMaxFrames || cfg->pool_octets > kRlMaxOctets) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }        // nothing of an earlier second look is in flight any more
	auto &m = c->rl;
	relook_free(c);
	const uint32_t K = cfg->max_anchors ? cfg->max_anchors : kRlDefAnchors;
	// (the defaults grow with the receiver: 256 records and 8192 octets a channel, at least 4096 and 2^20)
	const uint32_t pool_frames = cfg->pool_frames ? cfg->pool_frames : std::max<uint32_t>(kRlDefFrames, 256u * (uint32_t)c->C);
	const uint32_t pool_octets = cfg->pool_octets ? cfg->pool_octets : std::max<uint32_t>(kRlDefOctets, 8192u * (uint32_t)c->C);
	// the attempts one feed's records can have at the most: K a record, and - anchors lie 161 samples apart - what the pieces can hold
	const uint32_t rec_cap = (uint32_t)std::min<uint64_t>(kRlMaxRecs, std::min<uint64_t>((uint64_t)c->txl.pool * K, (uint64_t)c->txs.piece_cap * kRlPieceAnchors));
	for(auto &sl : c->slot) {
		auto &b = sl.rl;
		const bool ok = b.mail.alloc(rec_cap) == hipSuccess && b.d_piece.alloc(c->txs.piece_cap) == hipSuccess && b.d_plan.alloc(rec_cap) == hipSuccess
		                && b.d_frames.alloc(pool_frames) == hipSuccess && b.d_pool.alloc((size_t)pool_octets + 4) == hipSuccess
		                && b.d_frames_out.alloc(pool_frames) == hipSuccess && b.d_pool_out.alloc((size_t)pool_octets + 4) == hipSuccess && b.d_acnt.alloc((size_t)kRlDecodeGrid * kNumAvlcCounters, true) == hipSuccess;
		if(!ok) { relook_free(c); return VDL2HIP_E_NOMEM; }
	}
	if(hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); relook_free(c); return VDL2HIP_E_DEVICE; }
	m.flags = cfg->flags; m.thr = cfg->threshold != 0.f ? cfg->threshold : kSyncThr; m.max_ppm = cfg->max_ppm; m.max_anchors = K;
	m.pool_frames = pool_frames; m.pool_octets = pool_octets; m.rec_cap = rec_cap;
	m.records = m.anchors_found = m.attempts = m.frames = m.frames_ok = m.frames_new = m.dropped = 0; m.kernel_ms = 0.0;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_relook_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->rl.on && !c->failed) { int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	relook_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_relook_info_get(vdl2hip_ctx *c, vdl2hip_relook_info *info) {
	if(!c || !c->rl.on || !info || info->struct_size != sizeof(vdl2hip_relook_info)) return VDL2HIP_E_INVAL;
	const auto &m = c->rl;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info; info->flags = m.flags; info->threshold = m.thr; info->max_ppm = m.max_ppm;
	info->max_anchors = m.max_anchors; info->pool_frames = m.pool_frames; info->pool_octets = m.pool_octets;
	info->records = m.records; info->anchors_found = m.anchors_found; info->attempts = m.attempts;
	info->frames = m.frames; info->frames_ok = m.frames_ok; info->frames_new = m.frames_new; info->dropped = m.dropped; info->kernel_ms = (float)m.kernel_ms;
	return VDL2HIP_OK;
}
// (its own: a record goes out with its frames and their octets, each packed behind those of the records before it)
int vdl2hip_relook_read(vdl2hip_ctx *c, vdl2hip_relook *recs, size_t cap_recs, vdl2hip_packed_frame *frames, size_t cap_frames, uint8_t *octets, size_t cap_octets, size_t *octets_used) {
	if(!c || !c->rl.on || (!recs && cap_recs) || (!frames && cap_frames) || (!octets && cap_octets)) return VDL2HIP_E_INVAL;
	auto &q = c->rl.queue;
	size_t n = 0, nfr = 0, used = 0;
	while(!q.empty() && n < cap_recs) {
		const vdl2hip_ctx::RlItem &it = q.front();
		size_t need = 0;
		for(uint32_t k = 0; k < it.r.frames; k++) need += (*it.fr)[it.r.frame_first + k].len;
		if(nfr + it.r.frames > cap_frames || used + need > cap_octets || nfr + it.r.frames > 0xffffffffull) break;
		recs[n] = it.r;
		recs[n].frame_first = (uint32_t)(it.r.frames ? nfr : 0);
		for(uint32_t k = 0; k < it.r.frames; k++) {
			HostFrame h{ (*it.fr)[it.r.frame_first + k], nullptr };
			h.f.chan = (int32_t)(it.r.chan - (uint32_t)c->chan_first);
			vdl2hip_packed_frame &o = frames[nfr++];
			fill_frame(c, h, o.frame);
			o.frame.octets = nullptr; o.octets_off = used;
			const uint32_t len = h.f.len;
			if(len && (size_t)h.f.pool_off + len <= it.pool->size()) memcpy(octets + used, it.pool->data() + h.f.pool_off, len);
			else if(len) memset(octets + used, 0, len);                // (never)
			used += len;
		}
		n++;
		q.pop_front();
	}
	if(octets_used) *octets_used = used;
	return (int)n;
}

// ---- the preamble search (vdl2hip.h, "Preamble search"; kernels: txsearch.h) ----
// The ring behind the range.  The search of feed i reads y from search_first - 153 on (the taps of p(search_first - 3)), under the
// burst capture's conditions (above): what the ring keeps behind feed i's first sample k0 is kHistory + 1024 samples.  A record is
// emitted by the feed that completes bin last_bin + H + 1, so that bin ends at or after k0 and last_sample >= k0 - (H + 1) B
// >= k0 - kTxsMaxBack (vdl2hip_txsearch_enable refuses a monitor beyond that); search_first >= last_sample - (kTxsSpan - 1).
static_assert(kTxsMaxBack + (kTxsSpan - 1) + kTxsLead < kHistory + 1024, "a range and its taps begin inside what the ring keeps behind a feed");
static_assert(sizeof(TxsRec) == sizeof(vdl2hip_tx_search) && sizeof(vdl2hip_tx_search) == 96 && offsetof(TxsRec, first_bin) == offsetof(vdl2hip_tx_search, first_bin)
              && offsetof(TxsRec, first_lock) == offsetof(vdl2hip_tx_search, first_lock) && offsetof(TxsRec, best_pherr) == offsetof(vdl2hip_tx_search, best_pherr)
              && offsetof(TxsRec, best_ppm) == offsetof(vdl2hip_tx_search, best_ppm) && offsetof(TxsRec, lock_points) == offsetof(vdl2hip_tx_search, lock_points)
              && offsetof(TxsRec, flags) == offsetof(vdl2hip_tx_search, flags) && offsetof(vdl2hip_tx_search, flags) == 72 && offsetof(TxsRec, frames) == offsetof(vdl2hip_tx_search, frames)
              && offsetof(TxsRec, why) == offsetof(vdl2hip_tx_search, why) && offsetof(vdl2hip_tx_search, why) == 84, "the host copies the device's records as they are and fills in the rest");
static_assert(sizeof(vdl2hip_txsearch_cfg) == 16 && sizeof(vdl2hip_txsearch_info) == 40 && sizeof(TxsHdr) == 16 && sizeof(TxsPart) == 40, "vdl2hip.h states these sizes");
static_assert(VDL2HIP_TXS_CLIPPED == kTxsClipped && VDL2HIP_TX_PARTIAL == kTxPartial && (kTxsClipped & kTxPartial) == 0, "the two flags share a word");
// The pieces one feed's records can have at the most.  The transmissions of a channel are disjoint and the ranges of those a feed
// closes lie in [k0 - kTxsMaxBack - kTxsSpan, k0 + dmax): their lengths add up to less than dmax + kTxsMaxBack + kTxsSpan per channel,
// and a range of L samples has at most L / kTxsPiece + 1 pieces; the records are at most `pool`.
static uint64_t txsearch_piece_cap(const vdl2hip_ctx *c, uint32_t pool) {
	return (uint64_t)c->C * ((c->dmax + kTxsMaxBack + (uint64_t)kTxsSpan) / kTxsPiece + 1) + pool;
}
// Its share of a feed (launch_rest): behind the frame finisher and the copy of the log's records, which it reads, like the capture
static int txsearch_launch(vdl2hip_ctx *c, OutSlot &sl, hipStream_t st) {
	auto &m = c->txs;
	TxsArgs a{};
	a.y = c->d_y; a.tab = c->d_tab; a.txhdr = sl.txl.mail.d_hdr(); a.txrec = sl.txl.mail.d_rec();
	a.off = sl.txs.d_off; a.part = sl.txs.d_part; a.rec = sl.txs.mail.d_rec(); a.hdr = sl.txs.mail.d_hdr();
	a.pool = c->txl.pool; a.piece_cap = m.piece_cap; a.cap = c->cap; a.mask = c->cap - 1; a.chan_first = (uint32_t)c->chan_first;
	KernelTimes &t = sl.txs.times;
	t.arm(c->profiling >= 2);
	hipExtLaunchKernelGGL(k_txsearch_plan, dim3(1), dim3(kTxsThreads), 0u, st, t.e(0), (hipEvent_t) nullptr, 0, a);
	// a workgroup per piece, grid-stride: a piece per kTxsPiece channel-samples of the feed would be every sample busy - a quarter of that, 16 .. 2048
	const unsigned grid = (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(16, (uint64_t)sl.back_D * (uint64_t)c->C / (4 * kTxsPiece)));
	hipLaunchKernelGGL(k_txsearch_piece, dim3(grid), dim3(kTxsThreads), 0, st, a);
	hipExtLaunchKernelGGL(k_txsearch_reduce, dim3(std::min(256u, (c->txl.pool + 63) / 64)), dim3(64), 0u, st, (hipEvent_t) nullptr, t.e(1), 0, a);
	HIPCHK(hipGetLastError());
	HIPCHK(sl.txs.mail.post(st));
	t.launched(1);
	sl.txs.on = true;
	return VDL2HIP_OK;
}
// A collected feed's search records, index for index beside the log's nrec records
static int txsearch_fetch(vdl2hip_ctx *c, OutSlot &sl, uint32_t nrec, const TxsRec *&srec) {
	auto &m = c->txs;
	srec = nullptr;
	if(!m.on || !sl.txs.mail) return VDL2HIP_OK;
	if(sl.txs.mail.hdr().nrec != nrec) return VDL2HIP_E_DEVICE;      // (never: both are the log's header of this feed)
	HIPCHK(sl.txs.mail.fetch(nrec, m.stage, c->streams.out, srec));
	return VDL2HIP_OK;
}
// ... one of them, with the outcome the log has joined to its record
static void txsearch_take(vdl2hip_ctx *c, const TxsRec &s, const vdl2hip_tx &tx) {
	auto &m = c->txs;
	vdl2hip_tx_search r;
	memcpy(&r, &s, sizeof r);
	r.frames = tx.frames; r.frames_ok = tx.frames_ok; r.reserved = r.reserved2 = 0;
	r.why = tx.frames_ok ? VDL2HIP_TXS_DECODED : tx.frames ? VDL2HIP_TXS_FRAMES_BAD : r.lock_points ? VDL2HIP_TXS_LOCK_NO_FRAME : VDL2HIP_TXS_NO_PREAMBLE;
	m.records++; if(r.search_last >= r.search_first) m.samples += (uint64_t)(r.search_last - r.search_first + 1); if(r.flags & VDL2HIP_TXS_CLIPPED) m.clipped++;
	if((m.flags & VDL2HIP_TXSEARCH_UNDECODED_ONLY) && r.frames_ok != 0) return;
	m.queue.push_back(r);
}
// give the search's buffers back (nothing of it may be in flight: the callers have collected every feed)
static void txsearch_free(vdl2hip_ctx *c) {
	relook_free(c);                                                  // (a second look reads the search's plan: it goes first)
	for(auto &sl : c->slot) sl.txs.reset();
	c->txs.queue.clear();
	c->txs.on = false;
}
int vdl2hip_txsearch_enable(vdl2hip_ctx *c, const vdl2hip_txsearch_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_txsearch_cfg) || cfg->reserved[0] != 0 || cfg->reserved[1] != 0) return VDL2HIP_E_INVAL;
	if(!c->txl.on || !c->act.on || (cfg->flags & ~VDL2HIP_TXSEARCH_UNDECODED_ONLY)) return VDL2HIP_E_INVAL;
	if(((uint64_t)c->act.H + 1) * c->act.B > kTxsMaxBack) return VDL2HIP_E_INVAL;
	const uint64_t piece_cap = txsearch_piece_cap(c, c->txl.pool);
	if(piece_cap > 0x7fffffffull) return VDL2HIP_E_TOOBIG;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }        // nothing of an earlier search is in flight any more
	auto &m = c->txs;
	txsearch_free(c);
	const uint32_t pool = c->txl.pool;
	for(auto &sl : c->slot) {
		auto &b = sl.txs;
		const bool ok = b.mail.alloc(pool) == hipSuccess && b.d_off.alloc((size_t)pool + 1) == hipSuccess && b.d_part.alloc((size_t)piece_cap) == hipSuccess;
		if(!ok) { txsearch_free(c); return VDL2HIP_E_NOMEM; }
	}
	if(hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); txsearch_free(c); return VDL2HIP_E_DEVICE; }
	m.flags = cfg->flags; m.piece_cap = (uint32_t)piece_cap;
	m.records = m.samples = m.clipped = 0; m.kernel_ms = 0.0;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_txsearch_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->txs.on && !c->failed) { int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	txsearch_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_txsearch_info_get(vdl2hip_ctx *c, vdl2hip_txsearch_info *info) {
	if(!c || !c->txs.on || !info || info->struct_size != sizeof(vdl2hip_txsearch_info)) return VDL2HIP_E_INVAL;
	const auto &m = c->txs;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info; info->flags = m.flags;
	info->records = m.records; info->samples_searched = m.samples; info->clipped = m.clipped; info->kernel_ms = (float)m.kernel_ms;
	return VDL2HIP_OK;
}
int vdl2hip_txsearch_read(vdl2hip_ctx *c, vdl2hip_tx_search *recs, size_t cap_recs) {
	if(!c || !c->txs.on || (!recs && cap_recs)) return VDL2HIP_E_INVAL;
	return pop_records(c->txs.queue, recs, cap_recs);
}

// ---- the transmission capture (vdl2hip.h, "Transmission capture"; kernels: txcap.h) ----
// The ring behind the window and the extent.  Under the preamble search's conditions (above) a record's last_sample >= k0 - kTxsMaxBack;
// its window begins at or after last_sample - (kTxsSpan - 1) whatever pre is, and so does its extent: nothing is read further back than
// the search reads.  The window ends at last_sample + post <= last_sample + (H + 1) B, the last sample of the bin whose completion
// emits the record: inside the feed.  A window is at most kTxsSpan + kTxsMaxBack = 61 440 pairs long, less than the ring.
static_assert(kTxsMaxBack + (kTxsSpan - 1) < kHistory + 1024 && kTxsSpan + kTxsMaxBack < kHistory, "a window and an extent begin inside what the ring keeps behind a feed");
static_assert(sizeof(TxcRec) == sizeof(vdl2hip_tx_capture) && sizeof(vdl2hip_tx_capture) == 80 && offsetof(TxcRec, first_bin) == offsetof(vdl2hip_tx_capture, first_bin)
              && offsetof(TxcRec, win_first) == offsetof(vdl2hip_tx_capture, win_first) && offsetof(TxcRec, iq_off) == offsetof(vdl2hip_tx_capture, iq_off)
              && offsetof(TxcRec, spec_off) == offsetof(vdl2hip_tx_capture, spec_off) && offsetof(vdl2hip_tx_capture, spec_off) == 40
              && offsetof(TxcRec, iq_count) == offsetof(vdl2hip_tx_capture, iq_count) && offsetof(vdl2hip_tx_capture, iq_count) == 48
              && offsetof(TxcRec, flags) == offsetof(vdl2hip_tx_capture, flags) && offsetof(TxcRec, nfft) == offsetof(vdl2hip_tx_capture, nfft)
              && offsetof(TxcRec, frames) == offsetof(vdl2hip_tx_capture, frames) && offsetof(vdl2hip_tx_capture, frames) == 64, "the host copies the device's records as they are and fills in the rest");
static_assert(sizeof(vdl2hip_txcap_cfg) == 40 && sizeof(vdl2hip_txcap_info) == 88 && offsetof(vdl2hip_txcap_info, records) == 40 && sizeof(vdl2hip_tx_shape) == 48 && sizeof(TxcHdr) == 16, "vdl2hip.h states these sizes");
static_assert(VDL2HIP_TXCAP_IQ == kTxcapIq && VDL2HIP_TXCAP_SPECTRUM == kTxcapSpectrum && VDL2HIP_TXCAP_UNDECODED_ONLY == kTxcapUndecodedOnly && VDL2HIP_TXC_CLIPPED == kTxcClipped
              && VDL2HIP_TXC_TRUNCATED == kTxcTruncated && VDL2HIP_TXC_NO_ROOM == kTxcNoRoom && VDL2HIP_TXC_SHORT == kTxcShort && VDL2HIP_TXC_NO_SPECTRUM == kTxcNoSpectrum
              && ((kTxcClipped | kTxcTruncated | kTxcNoRoom | kTxcShort | kTxcNoSpectrum) & kTxPartial) == 0 && kTxcMaxPre == kCapMaxPre && kTxcMaxPool == kCapMaxPool, "the flags share a word; the burst capture's limits");
// The pieces one feed's spectra can have at the most.  A record of extent L has at most L / 4096 + 1 pieces (txc_pieces: S <= 2 L / N
// segments, 8192 / N to a piece) - 15, the extent being kTxsSpan at the most - and the first pool_spectra records have any; the extents
// of the transmissions a channel closes in one feed are disjoint and add up to less than dmax + kTxsMaxBack + kTxsSpan.
static uint64_t txcap_piece_cap(const vdl2hip_ctx *c, uint32_t txpool, uint32_t pool_spectra) {
	const uint64_t nspec = std::min(txpool, pool_spectra);
	return std::min<uint64_t>(nspec * (uint64_t)(kTxsSpan / 4096 + 1), (uint64_t)c->C * ((c->dmax + kTxsMaxBack + (uint64_t)kTxsSpan) / 4096 + 1) + nspec);
}
// Its share of a feed (launch_rest): behind the frame finisher and the copy of the log's records, which it reads, like the search
static int txcap_launch(vdl2hip_ctx *c, OutSlot &sl, hipStream_t st) {
	auto &m = c->txc;
	TxcArgs a{};
	a.y = c->d_y; a.txhdr = sl.txl.mail.d_hdr(); a.txrec = sl.txl.mail.d_rec(); a.w = m.buf.d_w; a.tw = m.buf.d_tw;
	a.poff = sl.txc.d_poff; a.part = sl.txc.d_part; a.rec = sl.txc.mail.d_rec(); a.hdr = sl.txc.mail.d_hdr(); a.pool = sl.txc.d_pool; a.spec = sl.txc.d_spec;
	a.k = m.k; a.norm = m.norm; a.txpool = c->txl.pool; a.piece_cap = m.piece_cap; a.cap = c->cap; a.mask = c->cap - 1; a.chan_first = (uint32_t)c->chan_first; a.log2n = m.log2n;
	const bool iq = (m.k.flags & kTxcapIq) != 0, spectrum = (m.k.flags & kTxcapSpectrum) != 0;
	KernelTimes &t = sl.txc.times;
	t.arm(c->profiling >= 2);
	hipExtLaunchKernelGGL(k_txcap_plan, dim3(1), dim3(kTxcThreads), 0u, st, t.e(0), iq ? (hipEvent_t) nullptr : t.e(1), 0, a);
	// a workgroup per record / per piece, grid-stride: a piece per 4096 channel-samples of the feed would be every sample busy - a quarter of that, 16 .. 2048
	const unsigned grid = (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(16, (uint64_t)sl.back_D * (uint64_t)c->C / (4 * 4096)));
	if(iq) hipExtLaunchKernelGGL(k_txcap_copy, dim3(std::min(512u, grid)), dim3(kTxcThreads), 0u, st, (hipEvent_t) nullptr, t.e(1), 0, a);
	if(spectrum) {
		hipExtLaunchKernelGGL(k_txcap_spectrum, dim3(grid), dim3(kTxcThreads), (uint32_t)m.lds, st, t.e(2), (hipEvent_t) nullptr, 0, a);
		hipExtLaunchKernelGGL(k_txcap_reduce, dim3(std::min(512u, grid)), dim3(kTxcThreads), 0u, st, (hipEvent_t) nullptr, t.e(3), 0, a);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(sl.txc.mail.post(st));
	t.launched(spectrum ? 2 : 1);
	sl.txc.on = true;
	return VDL2HIP_OK;
}
// A collected feed's capture records, index for index beside the log's nrec records, with the used part of its IQ pool and its
// spectra: one staging buffer, one wait
struct TxcFeed { const TxcRec *rec = nullptr; std::shared_ptr<std::vector<float>> iq, spec; uint64_t pairs = 0; };
static int txcap_fetch(vdl2hip_ctx *c, OutSlot &sl, uint32_t nrec, TxcFeed &f) {
	auto &m = c->txc;
	if(!m.on || !sl.txc.mail) return VDL2HIP_OK;
	const TxcHdr h = sl.txc.mail.hdr();
	if(h.nrec != nrec) return VDL2HIP_E_DEVICE;                      // (never: both are the log's header of this feed)
	f.pairs = std::min<uint64_t>(h.pairs, m.k.pool_samples);
	const size_t nspec = (m.k.flags & kTxcapSpectrum) ? std::min(nrec, m.k.pool_spectra) : 0u;
	const size_t rec_bytes = sl.txc.mail.staged(nrec), iq_bytes = (size_t)f.pairs * sizeof(cf32), sp_bytes = nspec * m.k.N * sizeof(float);
	HIPCHK(sl.txc.mail.fetch(nrec, m.stage, c->streams.out, f.rec, false, iq_bytes + sp_bytes));
	if(iq_bytes) HIPCHK(hipMemcpyAsync(m.stage + rec_bytes, sl.txc.d_pool, iq_bytes, hipMemcpyDeviceToHost, c->streams.out));
	if(sp_bytes) HIPCHK(hipMemcpyAsync(m.stage + rec_bytes + iq_bytes, sl.txc.d_spec, sp_bytes, hipMemcpyDeviceToHost, c->streams.out));
	if(rec_bytes + iq_bytes + sp_bytes) HIPCHK(hipStreamSynchronize(c->streams.out));
	const float *iqp = reinterpret_cast<const float *>(m.stage + rec_bytes), *spp = reinterpret_cast<const float *>(m.stage + rec_bytes + iq_bytes);
	f.iq = std::make_shared<std::vector<float>>(iqp, iqp + iq_bytes / sizeof(float));
	f.spec = std::make_shared<std::vector<float>>(spp, spp + sp_bytes / sizeof(float));
	return VDL2HIP_OK;
}
// ... one of them, with the outcome the log has joined to its record
static void txcap_take(vdl2hip_ctx *c, const TxcFeed &f, uint32_t i, const vdl2hip_tx &tx) {
	auto &m = c->txc;
	vdl2hip_tx_capture r;
	memcpy(&r, f.rec + i, sizeof r);
	if(r.iq_off + r.iq_count > f.pairs) { r.iq_count = 0; r.iq_off = 0; r.flags |= VDL2HIP_TXC_NO_ROOM; }      // (never)
	if(r.nfft && !(r.flags & VDL2HIP_TXC_NO_SPECTRUM) && r.spec_off + r.nfft > f.spec->size()) r.flags |= VDL2HIP_TXC_NO_SPECTRUM;      // (never)
	r.frames = tx.frames; r.frames_ok = tx.frames_ok; r.reserved[0] = r.reserved[1] = 0;
	m.records++; m.iq_samples += r.iq_count; if(r.flags & VDL2HIP_TXC_NO_ROOM) m.iq_dropped++;
	if(r.flags & VDL2HIP_TXC_NO_SPECTRUM) m.spectra_dropped++; else if(r.nfft) m.spectra++;
	if((m.k.flags & VDL2HIP_TXCAP_UNDECODED_ONLY) && r.frames_ok != 0) return;
	m.queue.push_back(vdl2hip_ctx::TxcItem{ r, f.iq, f.spec });
}
// give the capture's buffers back (nothing of it may be in flight: the callers have collected every feed)
static void txcap_free(vdl2hip_ctx *c) {
	for(auto &sl : c->slot) sl.txc.reset();
	c->txc.buf = {};
	c->txc.queue.clear();
	c->txc.on = false;
}
int vdl2hip_txcap_enable(vdl2hip_ctx *c, const vdl2hip_txcap_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_txcap_cfg) || cfg->reserved != 0) return VDL2HIP_E_INVAL;
	if(!c->txl.on || !c->act.on || !(cfg->flags & (VDL2HIP_TXCAP_IQ | VDL2HIP_TXCAP_SPECTRUM)) || (cfg->flags & ~(VDL2HIP_TXCAP_IQ | VDL2HIP_TXCAP_SPECTRUM | VDL2HIP_TXCAP_UNDECODED_ONLY))) return VDL2HIP_E_INVAL;
	const uint64_t back = ((uint64_t)c->act.H + 1) * c->act.B;
	if(back > kTxsMaxBack || cfg->pre_samples > kTxcMaxPre || cfg->post_samples > back || cfg->pool_samples > kTxcMaxPool) return VDL2HIP_E_INVAL;
	const uint32_t N = cfg->nfft ? cfg->nfft : kTxcDefN, pool_spectra = cfg->pool_spectra ? cfg->pool_spectra : kTxcDefSpectra;
	SpectrumDesign d;
	if(N < kTxcMinN || N > kTxcMaxN || !design_spectrum(N, cfg->window, d) || (uint64_t)pool_spectra * N > kTxcMaxSpecFloats) return VDL2HIP_E_INVAL;
	const uint64_t piece_cap = txcap_piece_cap(c, c->txl.pool, pool_spectra);
	if(piece_cap > 0x7fffffffull) return VDL2HIP_E_TOOBIG;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }        // nothing of an earlier capture is in flight any more
	auto &m = c->txc;
	txcap_free(c);
	const uint32_t txpool = c->txl.pool, pool = cfg->pool_samples ? cfg->pool_samples : kTxcDefPool;
	const bool iq = (cfg->flags & VDL2HIP_TXCAP_IQ) != 0, spectrum = (cfg->flags & VDL2HIP_TXCAP_SPECTRUM) != 0;
	bool ok = true;
	if(spectrum) ok = m.buf.d_w.alloc(N) == hipSuccess && m.buf.d_tw.alloc(N) == hipSuccess;
	for(auto &sl : c->slot) {
		auto &b = sl.txc;
		ok = ok && b.mail.alloc(txpool) == hipSuccess && b.d_poff.alloc((size_t)txpool + 1) == hipSuccess;
		if(iq) ok = ok && b.d_pool.alloc(pool) == hipSuccess;
		if(spectrum) ok = ok && b.d_part.alloc((size_t)std::max<uint64_t>(1, piece_cap) * N) == hipSuccess && b.d_spec.alloc((size_t)std::min(txpool, pool_spectra) * N) == hipSuccess;
	}
	if(!ok) { txcap_free(c); return VDL2HIP_E_NOMEM; }
	if((spectrum && (hipMemcpy(m.buf.d_w, d.w.data(), m.buf.d_w.bytes(), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(m.buf.d_tw, d.tw.data(), m.buf.d_tw.bytes(), hipMemcpyHostToDevice) != hipSuccess))
	   || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); txcap_free(c); return VDL2HIP_E_DEVICE; }
	m.k = TxcCfg{ pool, cfg->flags, cfg->pre_samples, cfg->post_samples, cfg->max_iq_samples, N, pool_spectra };
	m.window = cfg->window; m.log2n = d.log2n; m.norm = 1.0 / (d.sum_w * d.sum_w); m.lds = txc_lds_bytes(N); m.piece_cap = (uint32_t)piece_cap;
	m.records = m.iq_samples = m.iq_dropped = m.spectra = m.spectra_dropped = 0; m.kernel_ms = 0.0;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_txcap_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->txc.on && !c->failed) { int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	txcap_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_txcap_info_get(vdl2hip_ctx *c, vdl2hip_txcap_info *info) {
	if(!c || !c->txc.on || !info || info->struct_size != sizeof(vdl2hip_txcap_info)) return VDL2HIP_E_INVAL;
	const auto &m = c->txc;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info; info->flags = m.k.flags; info->pre_samples = m.k.pre; info->post_samples = m.k.post; info->max_iq_samples = m.k.max_iq;
	info->nfft = m.k.N; info->window = m.window; info->pool_samples = (uint32_t)m.k.pool_samples; info->pool_spectra = m.k.pool_spectra;
	info->records = m.records; info->iq_samples = m.iq_samples; info->iq_dropped = m.iq_dropped; info->spectra = m.spectra; info->spectra_dropped = m.spectra_dropped;
	info->kernel_ms = (float)m.kernel_ms;
	return VDL2HIP_OK;
}
// (its own: a record goes out with its IQ and its spectrum, each packed behind those of the records before it)
int vdl2hip_txcap_read(vdl2hip_ctx *c, vdl2hip_tx_capture *recs, size_t cap_recs, float *iq, size_t cap_pairs, size_t *pairs_used, float *spectra, size_t cap_floats, size_t *floats_used) {
	if(!c || !c->txc.on || (!recs && cap_recs) || (!iq && cap_pairs) || (!spectra && cap_floats)) return VDL2HIP_E_INVAL;
	auto &q = c->txc.queue;
	size_t n = 0, used = 0, fused = 0;
	while(!q.empty() && n < cap_recs) {
		const vdl2hip_ctx::TxcItem &it = q.front();
		const size_t nfl = it.r.nfft && !(it.r.flags & VDL2HIP_TXC_NO_SPECTRUM) ? it.r.nfft : 0;
		if(used + it.r.iq_count > cap_pairs || fused + nfl > cap_floats) break;
		recs[n] = it.r;
		recs[n].iq_off = used; recs[n].spec_off = fused;
		if(it.r.iq_count) memcpy(iq + 2 * used, it.iq->data() + 2 * it.r.iq_off, (size_t)it.r.iq_count * 2 * sizeof(float));
		if(nfl) memcpy(spectra + fused, it.spec->data() + it.r.spec_off, nfl * sizeof(float));
		used += it.r.iq_count; fused += nfl;
		n++;
		q.pop_front();
	}
	if(pairs_used) *pairs_used = used;
	if(floats_used) *floats_used = fused;
	return (int)n;
}
int vdl2hip_txcap_measure(const float *power, uint32_t nfft, vdl2hip_tx_shape *out) {
	if(!power || !out || nfft < kTxcMinN || nfft > kTxcMaxN || (nfft & (nfft - 1)) != 0) return VDL2HIP_E_INVAL;
	memset(out, 0, sizeof *out);
	const double step = 105000.0 / (double)nfft;
	double total = 0.0;
	for(uint32_t i = 0; i < nfft; i++) total += (double)power[i];
	if(!(total > 0.0)) return VDL2HIP_OK;
	uint32_t peak = 0, lo = nfft - 1, hi = nfft - 1; bool have_lo = false, have_hi = false;
	double moment = 0.0, run = 0.0;
	for(uint32_t i = 0; i < nfft; i++) {
		const double p = (double)power[i];
		if(p > (double)power[peak]) peak = i;
		moment += ((double)i - (double)(nfft / 2)) * step * p;
		run += p;
		if(!have_lo && run >= 0.005 * total) { lo = i; have_lo = true; }
		if(!have_hi && run >= 0.995 * total) { hi = i; have_hi = true; }
	}
	out->total = total; out->peak_bin = peak; out->peak_hz = ((double)peak - (double)(nfft / 2)) * step;
	out->centroid_hz = moment / total; out->obw_lo = lo; out->obw_hi = hi; out->obw_hz = (double)(hi - lo + 1) * step;
	return VDL2HIP_OK;
}

// ---- the transmission log (vdl2hip.h, "Transmission log"; kernels: txlog.h) ----
static_assert(sizeof(TxRec) == 64 && sizeof(vdl2hip_tx) == 80 && offsetof(vdl2hip_tx, frames) == sizeof(TxRec) && offsetof(vdl2hip_tx, first_burst_ord) == 72
              && offsetof(TxRec, first_bin) == offsetof(vdl2hip_tx, first_bin) && offsetof(TxRec, peak_bin) == offsetof(vdl2hip_tx, peak_bin)
              && offsetof(TxRec, first_sample) == offsetof(vdl2hip_tx, first_sample) && offsetof(TxRec, busy_bins) == offsetof(vdl2hip_tx, busy_bins)
              && offsetof(TxRec, mean_power) == offsetof(vdl2hip_tx, mean_power), "the host copies the device's records as they are and fills in the rest");
static_assert(sizeof(vdl2hip_txlog_cfg) == 16 && sizeof(vdl2hip_txlog_info) == 64 && sizeof(TxHdr) == 16 && sizeof(TxState) == 48, "vdl2hip.h states these sizes");
static_assert(kTxMaxChan == kK5MaxChan, "k_txlog_emit keeps every channel's offset in LDS");
constexpr uint32_t kTxMaxWait = 4096;      // frames per channel that may wait for their record (txlog_collect)
// Its share of a feed: behind k_activity_scan of the same feed, on the front stream (activity_feed): the bins m0 .. m0 + nb - 1 the feed
// completed are in the series ring (S >= the bins of the longest feed + 2) and stay there until the next feed's k_activity_power, which
// is queued behind.  (The copy of the header and the first records follows the feed's frame finisher: launch_rest.)
static int txlog_launch(vdl2hip_ctx *c, OutSlot &sl, uint64_t m0, uint32_t nb) {
	auto &m = c->txl; const auto &act = c->act;
	TxArgs a{};
	a.series = act.buf.d_series; a.freq = c->d_freq; a.st = m.buf.d_st; a.cnt = m.buf.d_cnt; a.rec = sl.txl.mail.d_rec(); a.hdr = sl.txl.mail.d_hdr();
	a.k_on = act.k_on; a.m0 = m0; a.thr = act.thr; a.nb = nb; a.H = act.H; a.B = act.B; a.S = act.S; a.smask = act.S - 1;
	a.nchan = (uint32_t)c->C; a.chan_first = (uint32_t)c->chan_first; a.pool = m.pool;
	KernelTimes &t = sl.txl.times;
	t.arm(c->profiling >= 2);
	hipExtLaunchKernelGGL(k_txlog_plan, dim3((unsigned)c->C), dim3(64), 0u, c->streams.front, t.e(0), t.e(1), 0, a);
	hipExtLaunchKernelGGL(k_txlog_emit, dim3((unsigned)c->C), dim3(64), 0u, c->streams.front, t.e(2), t.e(3), 0, a);
	HIPCHK(hipGetLastError());
	t.launched(2);
	sl.txl.on = true;
	return VDL2HIP_OK;
}
// A collected feed and the log.  The feed's frames first - all of them, whatever the AVLC filter lets through: they wait, per channel,
// for the record whose window holds their sync_sample.  Then the feed's records: each takes the waiting frames of its window; those
// before the window are counted as unmatched and dropped (vdl2hip.h, "Transmission log": Outcome).
static int txlog_collect(vdl2hip_ctx *c, OutSlot &sl, const OutFrame *fr, uint32_t nf, const uint8_t *po, uint32_t pool_n) {
	auto &m = c->txl;
	for(uint32_t i = 0; i < nf; i++) {
		if(fr[i].chan < 0 || fr[i].chan >= c->C) continue;
		auto &w = m.wait[(size_t)fr[i].chan];
		if(w.size() >= kTxMaxWait) { w.pop_front(); m.unmatched++; }
		// (the second look's join compares a frame's length and a hash of its octets: taken here, while the feed's octets are at hand, whether
		// that tap is on or not - a frame that waits for its record may see it enabled before the record comes)
		const bool hashed = po && (uint64_t)fr[i].pool_off + fr[i].len <= pool_n;
		w.push_back(vdl2hip_ctx::TxFrame{ fr[i].sync_sample, fr[i].burst_ord, fr[i].avlc_status == AVLC_OK, hashed ? fr[i].len : 0u, hashed ? relook_hash(po + fr[i].pool_off, fr[i].len) : 0ull });
	}
	if(!sl.txl.on) return VDL2HIP_OK;
	sl.txl.on = false;
	if(!sl.txl.mail) { sl.txs.on = sl.txc.on = sl.rl.on = false; return VDL2HIP_OK; }
	const TxHdr h = sl.txl.mail.hdr();
	const uint32_t nrec = std::min(h.nrec, m.pool);
	m.dropped += h.dropped;
	if(nrec == 0) { sl.txs.on = sl.txc.on = sl.rl.on = false; return VDL2HIP_OK; }
	const TxRec *rec = nullptr;
	HIPCHK(sl.txl.mail.fetch(nrec, m.stage, c->streams.out, rec));
	const TxsRec *srec = nullptr;
	if(sl.txs.on) { sl.txs.on = false; int r = txsearch_fetch(c, sl, nrec, srec); if(r != VDL2HIP_OK) return r; }
	TxcFeed capf;
	if(sl.txc.on) { sl.txc.on = false; int r = txcap_fetch(c, sl, nrec, capf); if(r != VDL2HIP_OK) return r; }
	RlFeed rlf; std::vector<std::pair<uint32_t, uint64_t>> seen;
	if(sl.rl.on) { sl.rl.on = false; int r = relook_fetch(c, sl, nrec, rlf); if(r != VDL2HIP_OK) return r; }
	const int64_t close_bins = (int64_t)c->act.H + 2, B = c->act.B;
	for(uint32_t i = 0; i < nrec; i++) {
		vdl2hip_tx r;
		memcpy(&r, rec + i, sizeof(TxRec));
		r.frames = r.frames_ok = 0; r.first_burst_ord = -1;
		const int64_t close_sample = c->act.k_on + ((int64_t)r.last_bin + close_bins) * B;
		int64_t first_sync = 0;
		if(r.chan >= (uint32_t)c->chan_first && r.chan < (uint32_t)(c->chan_first + c->C)) {
			auto &w = m.wait[r.chan - (uint32_t)c->chan_first];
			size_t keep = 0;
			for(const auto &f : w) {
				if(f.sync_sample < r.first_sample) m.unmatched++;
				else if(f.sync_sample < close_sample) {
					if(!r.frames || f.sync_sample < first_sync) { first_sync = f.sync_sample; r.first_burst_ord = f.burst_ord; }
					r.frames++; if(f.ok) r.frames_ok++;
					if(rlf.rec && f.len) seen.emplace_back(f.len, f.hash);
				} else w[keep++] = f;
			}
			w.resize(keep);
		}
		m.transmissions++; m.matched += r.frames; if(r.frames_ok) m.decoded++;
		if(srec) txsearch_take(c, srec[i], r);
		if(capf.rec) txcap_take(c, capf, i, r);
		if(rlf.rec) { relook_take(c, rlf, r, seen); seen.clear(); }
		if((m.flags & VDL2HIP_TXLOG_UNDECODED_ONLY) && r.frames_ok != 0) continue;
		m.queue.push_back(r);
	}
	return VDL2HIP_OK;
}
// give the log's buffers back (nothing of it may be in flight: the callers have collected every feed and the front stream has run dry
// of its launches)
static void txlog_free(vdl2hip_ctx *c) {
	for(auto &sl : c->slot) sl.txl.reset();
	auto &m = c->txl;
	m.buf = {}; m.queue.clear(); m.wait.clear();
	m.on = false;
}
// switch a running log off: the feeds under way are collected (their copies land in the slots' buffers), then everything goes
static int txlog_off(vdl2hip_ctx *c) {
	if(!c->txl.on) return VDL2HIP_OK;
	if(!c->failed) { int r = collect_all(c); if(r != VDL2HIP_OK) return r; }
	(void)hipStreamSynchronize(c->streams.front);
	txsearch_free(c);                                                // (a search and a capture read the log's records: they go first)
	txcap_free(c);
	txlog_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_txlog_enable(vdl2hip_ctx *c, const vdl2hip_txlog_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_txlog_cfg) || cfg->reserved != 0) return VDL2HIP_E_INVAL;
	if(!c->act.on || cfg->pool_records > kTxMaxPool || (cfg->flags & ~VDL2HIP_TXLOG_UNDECODED_ONLY)) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = collect_all(c); if(r != VDL2HIP_OK) return r; }        // nothing of an earlier log is in flight any more
	(void)hipStreamSynchronize(c->streams.front);
	auto &m = c->txl;
	txsearch_free(c);                                                // (a search and a capture that were running go with the log they read)
	txcap_free(c);
	txlog_free(c);
	const uint32_t pool = cfg->pool_records ? cfg->pool_records : kTxDefPool;
	const size_t C = (size_t)c->C;
	bool ok = m.buf.d_st.alloc(C) == hipSuccess && m.buf.d_cnt.alloc(C, true) == hipSuccess;
	for(auto &sl : c->slot) ok = ok && sl.txl.mail.alloc(pool) == hipSuccess;
	if(!ok) { txlog_free(c); return VDL2HIP_E_NOMEM; }
	// the log's state from the monitor's, on the front stream: behind every scan queued so far, ahead of the next feed's
	hipLaunchKernelGGL(k_txlog_init, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, c->streams.front, (const ActState *)c->act.buf.d_st.get(), m.buf.d_st.get(), (uint32_t)C);
	if(hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); txlog_free(c); return VDL2HIP_E_DEVICE; }
	m.wait.assign(C, {});
	m.pool = pool; m.flags = cfg->flags;
	m.transmissions = m.decoded = m.dropped = m.matched = m.unmatched = 0; m.kernel_ms = 0.0;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_txlog_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	return txlog_off(c);
}
int vdl2hip_txlog_info_get(vdl2hip_ctx *c, vdl2hip_txlog_info *info) {
	if(!c || !c->txl.on || !info || info->struct_size != sizeof(vdl2hip_txlog_info)) return VDL2HIP_E_INVAL;
	const auto &m = c->txl;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info; info->pool_records = m.pool; info->flags = m.flags;
	info->transmissions = m.transmissions; info->decoded = m.decoded; info->dropped = m.dropped;
	info->frames_matched = m.matched; info->frames_unmatched = m.unmatched; info->kernel_ms = (float)m.kernel_ms;
	return VDL2HIP_OK;
}
int vdl2hip_txlog_read(vdl2hip_ctx *c, vdl2hip_tx *recs, size_t cap_recs) {
	if(!c || !c->txl.on || (!recs && cap_recs)) return VDL2HIP_E_INVAL;
	return pop_records(c->txl.queue, recs, cap_recs);
}

// ---- the activity monitor (vdl2hip.h, "Activity monitor"; kernels: activity.h) ----
static_assert(sizeof(ActChan) == sizeof(vdl2hip_activity_chan) && offsetof(ActChan, hist) == offsetof(vdl2hip_activity_chan, hist), "the host copies the device's accumulators as they are");
// Its share of a feed: on the front stream directly behind the channeliser - k_chanfir, every piece of a cold-start feed, k_fixup
// where it is not fused - and ahead of the sync kernels.  Everything that rewrites y (the referee's scans, on the back streams)
// waits for an ev_front, which is recorded behind the sync kernels of its feed, and writes nothing at or beyond that feed's last
// sample (k_ref_scan_multi: n_hi <= in_end / os - 1): what the monitor reads of this feed, [k0, k0 + D), is the channeliser's.
// Host bookkeeping: the bin the stream stands in, the bins this feed completes, which carry is current.
static int activity_feed(vdl2hip_ctx *c, OutSlot &sl, int64_t k0, int64_t D) {
	auto &m = c->act;
	const uint64_t B = m.B, t0 = (uint64_t)(k0 - m.k_on), t1 = t0 + (uint64_t)D;
	const uint64_t m0 = t0 / B, m1 = t1 / B, nb = m1 - m0;
	ActArgs a{};
	a.y = (const float2 *)c->d_y.get(); a.series = m.buf.d_series; a.carry_in = m.buf.d_carry[m.carry_sel]; a.carry_out = m.buf.d_carry[m.carry_sel ^ 1];
	a.k0 = k0; a.m0 = m0; a.off = (int32_t)((int64_t)(m0 * B) - (int64_t)t0); a.D = (uint32_t)D; a.B = m.B; a.nbt = (uint32_t)nb + 1;
	a.cap = c->cap; a.mask = c->cap - 1; a.S = m.S; a.smask = m.S - 1;
	// bins per workgroup: some 4096 workgroups over the channels, each with one to eight chunks' worth of samples
	const uint64_t per = std::min<uint64_t>(8 * kActChunk, std::max<uint64_t>(kActChunk, (uint64_t)D * (uint64_t)c->C / 4096));
	a.run = (uint32_t)std::max<uint64_t>(1, per / B);
	const unsigned gx = (a.nbt + a.run - 1) / a.run;
	KernelTimes &t = sl.act_t;
	t.arm(c->profiling >= 2);
	hipExtLaunchKernelGGL(k_activity_power, dim3(gx, (unsigned)c->C), dim3(kActThreads), 0u, c->streams.front, t.e(0), t.e(1), 0, a);
	if(nb) {
		ActScanArgs sa{ m.buf.d_series, m.buf.d_acc, m.buf.d_st, m.buf.d_edges, m.thr, m0, (uint32_t)nb, m.H, m.S, m.S - 1 };
		hipExtLaunchKernelGGL(k_activity_scan, dim3((unsigned)c->C), dim3(64), 0u, c->streams.front, t.e(2), t.e(3), 0, sa);
	}
	HIPCHK(hipGetLastError());
	// the transmission log reads the series and the bins this feed completed directly behind the scan (ahead of the mark: whoever waits
	// for the monitor's last launch waits for the log's too)
	if(c->txl.on && nb) { int r = txlog_launch(c, sl, m0, (uint32_t)nb); if(r != VDL2HIP_OK) return r; }
	HIPCHK(m.tap.mark(c->streams.front));
	t.launched(nb ? 2 : 1);
	m.bins = m1; m.carry_sel ^= 1;
	return VDL2HIP_OK;
}
// wait for what the monitor has queued and give its buffers back (event, stream and landing place stay with the context: m.tap;
// what its launches took of the slots' feeds is not a later monitor's)
static void activity_free(vdl2hip_ctx *c) {
	auto &m = c->act;
	if(m.tap.queued) (void)hipEventSynchronize(m.tap.last);
	m.buf = {};
	for(auto &sl : c->slot) sl.act_t.n = 0;
	m.on = false; m.tap.queued = false;
}
static float activity_edge(int i) { return (float)std::pow(10.0, (double)(-120 + 2 * i) / 10.0); }

int vdl2hip_activity_edges(float *edges, size_t cap) {
	if(!edges || cap < (size_t)kActBuckets - 1) return VDL2HIP_E_TOOBIG;
	for(int i = 0; i < kActBuckets - 1; i++) edges[i] = activity_edge(i);
	return kActBuckets - 1;
}
int vdl2hip_activity_enable(vdl2hip_ctx *c, const vdl2hip_activity_cfg *cfg) {
	if(!c || !cfg || cfg->struct_size != sizeof(vdl2hip_activity_cfg) || cfg->reserved != 0) return VDL2HIP_E_INVAL;
	const uint32_t B = cfg->bin_samples ? cfg->bin_samples : 105u;
	if(B < kActMinBin || B > kActMaxBin || cfg->hang_bins > kActMaxHang) return VDL2HIP_E_INVAL;
	if(cfg->series_bins > kActMaxSeries || (cfg->series_bins & (cfg->series_bins - 1)) != 0) return VDL2HIP_E_INVAL;
	if(std::isnan(cfg->threshold_dbfs)) return VDL2HIP_E_INVAL;
	uint32_t S = 1; while(S < cfg->series_bins || S < c->dmax / B + 2) S <<= 1;           // a feed's bins never overwrite one another in the ring
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	{ int r = txlog_off(c); if(r != VDL2HIP_OK) return r; }          // (a transmission log's state would no longer mean anything)
	auto &m = c->act;
	activity_free(c);
	const size_t C = (size_t)c->C;
	HIPCHK(m.tap.last.ensure(hipEventDisableTiming));
	if(!m.tap.rd) HIPCHK(hipStreamCreateWithFlags(&m.tap.rd, hipStreamNonBlocking));
	if(!m.tap.land) HIPCHK(m.tap.land.alloc(C * (sizeof(ActChan) + sizeof(ActState))));
	auto &b = m.buf;
	for(hipError_t e : { b.d_series.alloc(C * S, true), b.d_carry[0].alloc(C, true), b.d_carry[1].alloc(C, true), b.d_edges.alloc(kActBuckets), b.d_acc.alloc(C, true), b.d_st.alloc(C, true) })
		if(e != hipSuccess) { activity_free(c); return e == hipErrorOutOfMemory ? VDL2HIP_E_NOMEM : VDL2HIP_E_DEVICE; }
	float edges[kActBuckets] = {};
	(void)vdl2hip_activity_edges(edges, kActBuckets);
	if(hipMemcpy(b.d_edges, edges, sizeof edges, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); activity_free(c); return VDL2HIP_E_DEVICE; }
	m.B = B; m.H = cfg->hang_bins; m.S = S; m.thr_dbfs = cfg->threshold_dbfs; m.thr = (float)std::pow(10.0, (double)cfg->threshold_dbfs / 10.0);
	m.k_on = c->k_total; m.bins = 0; m.carry_sel = 0; m.kernel_ms = 0.0; m.tap.queued = false;
	m.on = true;
	return VDL2HIP_OK;
}
int vdl2hip_activity_disable(vdl2hip_ctx *c) {
	if(!c) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	{ int r = txlog_off(c); if(r != VDL2HIP_OK) return r; }
	activity_free(c);
	return VDL2HIP_OK;
}
int vdl2hip_activity_read(vdl2hip_ctx *c, vdl2hip_activity_info *info, vdl2hip_activity_chan *chans, size_t cap_chans, int reset) {
	if(!c || !c->act.on || (info && info->struct_size != sizeof(vdl2hip_activity_info))) return VDL2HIP_E_INVAL;
	auto &m = c->act;
	const size_t C = (size_t)c->C;
	if(chans && cap_chans < C) return VDL2HIP_E_TOOBIG;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	if(chans) {
		uint8_t *land = m.tap.land;
		ActState *st = (ActState *)(land + C * sizeof(ActChan));
		if(m.tap.queued) {
			HIPCHK(m.tap.fetch(land, m.buf.d_acc, m.buf.d_acc.bytes()));
			HIPCHK(m.tap.fetch(st, m.buf.d_st, m.buf.d_st.bytes()));
		} else memset(land, 0, m.tap.land.bytes());      // nothing has touched them since they were zeroed
		memcpy(chans, land, C * sizeof(ActChan));
		for(size_t i = 0; i < C; i++) { chans[i].open = st[i].open; chans[i].reserved = 0; if(!chans[i].bins) chans[i].max_power = chans[i].min_power = 0.f; }
	}
	if(info) {
		memset(info, 0, sizeof *info);
		info->struct_size = sizeof *info; info->bin_samples = m.B; info->hang_bins = m.H; info->series_bins = m.S;
		info->threshold_dbfs = m.thr_dbfs; info->threshold_power = m.thr; info->first_sample = m.k_on; info->bins = m.bins;
		info->kernel_ms = (float)m.kernel_ms;
	}
	if(reset) {
		// (on the front stream: behind the launches that are queued, ahead of the next feed's; the transmission under way is kept)
		HIPCHK(hipMemsetAsync(m.buf.d_acc, 0, m.buf.d_acc.bytes(), c->streams.front));
		HIPCHK(m.tap.mark(c->streams.front));
	}
	return chans ? (int)C : 0;
}
int vdl2hip_activity_series(vdl2hip_ctx *c, uint32_t chan, int64_t first_bin, float *dst, size_t cap) {
	if(!c || !c->act.on || chan < (uint32_t)c->chan_first || chan >= (uint32_t)(c->chan_first + c->C)) return VDL2HIP_E_INVAL;
	auto &m = c->act;
	if(first_bin < 0 || (uint64_t)first_bin > m.bins || m.bins - (uint64_t)first_bin > m.S) return VDL2HIP_E_INVAL;
	const size_t n = std::min<size_t>(cap, (size_t)(m.bins - (uint64_t)first_bin));
	if(n == 0) return 0;
	if(!dst) return VDL2HIP_E_INVAL;
	OnDevice dev_guard(c);
	if(c->failed) return VDL2HIP_E_DEVICE;
	const float *base = m.buf.d_series + (size_t)(chan - (uint32_t)c->chan_first) * m.S;
	const size_t p0 = (size_t)((uint64_t)first_bin & (m.S - 1)), n0 = std::min<size_t>(n, m.S - p0);
	HIPCHK(m.tap.fetch(dst, base + p0, n0 * sizeof(float)));
	if(n0 < n) HIPCHK(m.tap.fetch(dst + n0, base, (n - n0) * sizeof(float)));
	return (int)n;
}
