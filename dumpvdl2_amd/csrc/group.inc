// group.inc - included at the end of vdl2hip.hip (uses its file-local helpers: collect_slot, feed_common, fill_frame ...).
// ======================================================================================================================
// vdl2hip_group: one receiver spread over several GPUs of THIS process, from plain C (include/vdl2hip.h).  The reference
// runs one worker per channel over a shared sample block (src/dumpvdl2.c:117-135, src/demod.c:300-301,356-365); here the
// workers are grouped by device: device k of n decodes the contiguous channel range k (the same rule as
// dist.shard_channels), and every block is put on every device in one of two ways:
//   all-gather (default)  the block is cut into n stripes; member k copies stripe k from host memory over ITS OWN PCIe link,
//                         then every member fetches the n-1 stripes it lacks from its peers over xGMI, all links at once
//   broadcast             the whole block crosses PCIe once, into the first device, and is sent from there to the others
//                         (north_star's literal form; bound by that one H2D copy)
// Both move data with hipMemcpyPeerAsync by default - the path that has run on hardware (also between "virtual shards" on
// one device: the path is testable with one GPU).  RCCL (ncclAllGather / ncclBroadcast, loaded at run time) is opt-in,
// VDL2HIP_USE_RCCL=1, until it has run on a multi-GPU node.
// ======================================================================================================================
#include <dlfcn.h>
// RCCL is dlopen()ed (no link-time dependency) and its header is optional too: without it the few ABI-stable names the
// broadcast needs are declared here, so that the single-GPU library and the peer-copy fan-out build on an installation
// that has no RCCL development files.
#if __has_include(<rccl/rccl.h>) && !defined(VDL2HIP_NO_RCCL_HEADER)
#include <rccl/rccl.h>
#else
typedef struct ncclComm *ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclChar = 0 } ncclDataType_t;
#endif
enum { GX_ALLGATHER = 0, GX_BROADCAST = 1 };

struct vdl2hip_group {
	int n = 0; size_t in_cap = 0; int fmt = 0; uint64_t feed_no = 0;
	std::vector<int> dev; std::vector<vdl2hip_ctx *> ctx;
	std::vector<uint8_t *> blk[kSlots];                 // [slot][device index] input block on that device
	std::vector<hipStream_t> xs;                         // per member: its H2D stream (own stripe, or the whole block on member 0 in the broadcast form)
	std::vector<std::vector<hipStream_t>> px;            // per member: streams its fetches from peers are spread over (n - 1 of them: every xGMI link at once)
	std::vector<hipEvent_t> own[kSlots];                 // member i's own stripe (broadcast: member 0's whole block) of slot k is in its memory
	std::vector<std::vector<hipEvent_t>> got[kSlots];    // member i's fetches on px[i][j] of slot k are complete
	std::vector<hipEvent_t> ready[kSlots];               // block of slot k complete on device i (RCCL paths)
	int exchange = GX_ALLGATHER; int last_form = -1;    // last_form: what the last feed really did (vdl2hip_group_exchange())
	// RCCL, loaded at run time (no link-time dependency)
	void *rccl = nullptr; std::vector<ncclComm_t> comms; bool use_rccl = false;
	ncclResult_t (*p_init_all)(ncclComm_t *, int, const int *) = nullptr;
	ncclResult_t (*p_bcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*p_allgather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*p_gstart)() = nullptr; ncclResult_t (*p_gend)() = nullptr; ncclResult_t (*p_destroy)(ncclComm_t) = nullptr;
	bool failed = false;                                // a feed went wrong part-way: the members are out of step, every later call fails
	std::vector<hipEvent_t> pinned_pending;             // H2D copies of the last vdl2hip_group_feed_pinned() whose source the caller may not touch yet
	struct QF { HostFrame h; int who; };
	std::vector<QF> merged;
};

namespace {
struct DeviceGuard {                                      // the calling thread's current device is left as it was found
	int prev = 0; DeviceGuard() { (void)hipGetDevice(&prev); } ~DeviceGuard() { (void)hipSetDevice(prev); }
};
void group_try_rccl(vdl2hip_group *g) {
	// opt-in: these calls have been built and reviewed but have not yet run on a multi-GPU node (the development boxes have one GPU)
	const char *use = getenv("VDL2HIP_USE_RCCL");
	if(!use || atoi(use) == 0 || getenv("VDL2HIP_NO_RCCL")) return;
	for(int i = 0; i < g->n; i++) for(int j = 0; j < i; j++) if(g->dev[i] == g->dev[j]) return;    // one communicator rank per GPU
	if(g->n < 2) return;
	g->rccl = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
	if(!g->rccl) g->rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
	if(!g->rccl) return;
	g->p_init_all = (decltype(g->p_init_all))dlsym(g->rccl, "ncclCommInitAll");
	g->p_bcast = (decltype(g->p_bcast))dlsym(g->rccl, "ncclBroadcast");
	g->p_allgather = (decltype(g->p_allgather))dlsym(g->rccl, "ncclAllGather");
	g->p_gstart = (decltype(g->p_gstart))dlsym(g->rccl, "ncclGroupStart");
	g->p_gend = (decltype(g->p_gend))dlsym(g->rccl, "ncclGroupEnd");
	g->p_destroy = (decltype(g->p_destroy))dlsym(g->rccl, "ncclCommDestroy");
	if(!g->p_init_all || !g->p_bcast || !g->p_allgather || !g->p_gstart || !g->p_gend || !g->p_destroy) return;
	g->comms.assign((size_t)g->n, nullptr);
	if(g->p_init_all(g->comms.data(), g->n, g->dev.data()) != ncclSuccess) { g->comms.clear(); return; }
	g->use_rccl = true;
}
}  // namespace

extern "C" {

void vdl2hip_group_destroy(vdl2hip_group *g) {
	if(!g) return;
	DeviceGuard guard;
	for(int i = 0; i < g->n; i++) {
		(void)hipSetDevice(g->dev[i]);
		if(i < (int)g->xs.size() && g->xs[i]) (void)hipStreamSynchronize(g->xs[i]);
		if(i < (int)g->px.size()) for(hipStream_t st : g->px[i]) if(st) (void)hipStreamSynchronize(st);
	}
	for(int i = 0; i < g->n; i++) {
		(void)hipSetDevice(g->dev[i]);
		if(i < (int)g->ctx.size() && g->ctx[i]) vdl2hip_destroy(g->ctx[i]);
		if(i < (int)g->xs.size() && g->xs[i]) (void)hipStreamDestroy(g->xs[i]);
		if(i < (int)g->px.size()) for(hipStream_t st : g->px[i]) if(st) (void)hipStreamDestroy(st);
		for(int k = 0; k < kSlots; k++) {
			if(i < (int)g->blk[k].size() && g->blk[k][i]) (void)hipFree(g->blk[k][i]);
			if(i < (int)g->ready[k].size() && g->ready[k][i]) (void)hipEventDestroy(g->ready[k][i]);
			if(i < (int)g->own[k].size() && g->own[k][i]) (void)hipEventDestroy(g->own[k][i]);
			if(i < (int)g->got[k].size()) for(hipEvent_t e : g->got[k][i]) if(e) (void)hipEventDestroy(e);
		}
		if(g->use_rccl && i < (int)g->comms.size() && g->comms[i]) (void)g->p_destroy(g->comms[i]);
	}
	if(g->rccl) dlclose(g->rccl);
	delete g;
}

int vdl2hip_group_create(const vdl2hip_cfg *cfg_in, const int32_t *devices, uint32_t ndev, vdl2hip_group **out) {
	vdl2hip_cfg cfg_v;
	if(cfg_read(cfg_in, cfg_v) != VDL2HIP_OK) return VDL2HIP_E_INVAL;      // (a 56-byte structure, from before input_rate, included)
	const vdl2hip_cfg *cfg = &cfg_v;
	if(!out || !devices || ndev == 0 || ndev > 64 || !cfg->freqs || cfg->nchan < ndev) return VDL2HIP_E_INVAL;
	if(cfg->chan_first != 0 || cfg->chan_count != 0) return VDL2HIP_E_INVAL;      // the group does the sharding
	*out = nullptr;
	DeviceGuard guard;
	vdl2hip_group *g = new(std::nothrow) vdl2hip_group();
	if(!g) return VDL2HIP_E_NOMEM;
	g->n = (int)ndev; g->dev.assign(devices, devices + ndev);
	g->in_cap = cfg->max_block_bytes ? cfg->max_block_bytes : 320000u; g->fmt = fmt_code(cfg->sample_fmt);
	g->ctx.assign(ndev, nullptr); g->xs.assign(ndev, nullptr); g->px.assign(ndev, std::vector<hipStream_t>());
	for(int k = 0; k < kSlots; k++) {
		g->blk[k].assign(ndev, nullptr); g->ready[k].assign(ndev, nullptr); g->own[k].assign(ndev, nullptr);
		g->got[k].assign(ndev, std::vector<hipEvent_t>());
	}
	if(const char *e = getenv("VDL2HIP_GROUP_EXCHANGE")) g->exchange = strcmp(e, "broadcast") == 0 ? GX_BROADCAST : GX_ALLGATHER;
	const uint32_t base = cfg->nchan / ndev, extra = cfg->nchan % ndev;
	for(uint32_t i = 0; i < ndev; i++) {
		vdl2hip_cfg c = *cfg;
		c.device = devices[i];
		c.chan_first = i * base + std::min(i, extra);                           // dist.shard_channels()
		c.chan_count = base + (i < extra ? 1u : 0u);
		int r = vdl2hip_create(&c, &g->ctx[i]);
		if(r != VDL2HIP_OK) { vdl2hip_group_destroy(g); return r; }
		bool ok = hipSetDevice(devices[i]) == hipSuccess && hipStreamCreateWithFlags(&g->xs[i], hipStreamNonBlocking) == hipSuccess;
		const uint32_t npx = ndev > 1 ? ndev - 1 : 1;                            // one fetch stream per peer: every xGMI link of the device at work at once
		g->px[i].assign(npx, nullptr);
		for(uint32_t j = 0; j < npx && ok; j++) ok = hipStreamCreateWithFlags(&g->px[i][j], hipStreamNonBlocking) == hipSuccess;
		for(int k = 0; k < kSlots && ok; k++) {
			ok = hipMalloc((void **)&g->blk[k][i], g->in_cap + 16) == hipSuccess && hipEventCreateWithFlags(&g->ready[k][i], hipEventDisableTiming) == hipSuccess
			     && hipEventCreateWithFlags(&g->own[k][i], hipEventDisableTiming) == hipSuccess;
			g->got[k][i].assign(npx, nullptr);
			for(uint32_t j = 0; j < npx && ok; j++) ok = hipEventCreateWithFlags(&g->got[k][i][j], hipEventDisableTiming) == hipSuccess;
		}
		if(!ok) { vdl2hip_group_destroy(g); return VDL2HIP_E_NOMEM; }
		for(uint32_t j = 0; j < ndev; j++)
			if(devices[j] != devices[i]) { int can = 0; (void)hipDeviceCanAccessPeer(&can, devices[i], devices[j]); if(can) (void)hipDeviceEnablePeerAccess(devices[j], 0); }
		(void)hipGetLastError();       // "peer access already enabled" (a second group, two members on one device) is not an error of the first feed
	}
	group_try_rccl(g);
	*out = g;
	return VDL2HIP_OK;
}

uint32_t vdl2hip_group_size(vdl2hip_group *g) { return g ? (uint32_t)g->n : 0u; }
vdl2hip_ctx *vdl2hip_group_ctx(vdl2hip_group *g, uint32_t i) { return g && i < (uint32_t)g->n ? g->ctx[i] : nullptr; }
int vdl2hip_group_uses_rccl(vdl2hip_group *g) { return g && g->use_rccl ? 1 : 0; }
int vdl2hip_group_set_exchange(vdl2hip_group *g, int form) {
	if(!g || (form != VDL2HIP_GROUP_ALLGATHER && form != VDL2HIP_GROUP_BROADCAST)) return VDL2HIP_E_INVAL;
	g->exchange = form == VDL2HIP_GROUP_BROADCAST ? GX_BROADCAST : GX_ALLGATHER;
	return VDL2HIP_OK;
}
int vdl2hip_group_exchange(vdl2hip_group *g) { return g ? g->last_form : VDL2HIP_E_INVAL; }

// One block to every member.  Any failure once the first member has been touched leaves the members out of step (some have
// queued the block, some have not; their slot counters no longer agree with the group's buffer index), so the group is marked
// failed and every later call returns VDL2HIP_E_DEVICE - the reference has no partial-failure mode either (src/util.c:37).
#define GRPCHK(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) { \
	fprintf(stderr, "vdl2hip: %s failed: %s (%s:%d) - group disabled\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); g->failed = true; return VDL2HIP_E_DEVICE; } } while(0)
static int group_wait_pinned(vdl2hip_group *g) {
	for(hipEvent_t e : g->pinned_pending) GRPCHK(hipEventSynchronize(e));
	g->pinned_pending.clear();
	return VDL2HIP_OK;
}

static int group_feed(vdl2hip_group *g, const void *buf, size_t nbytes, bool wait_copy) {
	if(!g || (!buf && nbytes)) return VDL2HIP_E_INVAL;
	if(g->failed) return VDL2HIP_E_DEVICE;
	if(nbytes == 0) return VDL2HIP_OK;
	if(nbytes > g->in_cap) return VDL2HIP_E_TOOBIG;
	nbytes -= nbytes % raw_bytes(g->fmt);
	DeviceGuard guard;
	{ int r = group_wait_pinned(g); if(r != VDL2HIP_OK) return r; }
	const int k = (int)(g->feed_no % kSlots), n = g->n;
	// the buffers of this slot were last read by the channelisers of feed i - kSlots: every member has to be past that
	// (members advance together, so ctx->feed_no == g->feed_no for all of them as long as the group has not failed)
	for(int i = 0; i < n; i++) {
		GRPCHK(hipSetDevice(g->dev[i]));
		vdl2hip_ctx *c = g->ctx[i];
		if(c->failed || c->feed_no != g->feed_no) { g->failed = true; return VDL2HIP_E_DEVICE; }
		int r = collect_slot(c, c->slot[c->feed_no % kSlots]);
		if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) { g->failed = true; return r; }
	}
	std::vector<hipEvent_t> host_done;                  // the H2D copies out of `buf`
	const bool gather = g->exchange == GX_ALLGATHER && n > 1;
	if(gather) {
		// ---- all-gather: stripe i crosses member i's own PCIe link, the rest comes from the peers ----
		const size_t unit = 256;                                        // stripe boundaries on 256 bytes: whole samples in every format (2, 4 or 8 bytes), and the broadcast sends the block whole
		const size_t per = ((nbytes + n - 1) / n + unit - 1) / unit * unit;
		static_assert(unit % 8 == 0, "a stripe ends on a sample boundary");
		std::vector<size_t> off(n + 1);
		for(int i = 0; i <= n; i++) off[i] = std::min(nbytes, per * (size_t)i);
		for(int i = 0; i < n; i++) {
			GRPCHK(hipSetDevice(g->dev[i]));
			if(off[i + 1] > off[i]) GRPCHK(hipMemcpyAsync(g->blk[k][i] + off[i], (const uint8_t *)buf + off[i], off[i + 1] - off[i], hipMemcpyHostToDevice, g->xs[i]));
			GRPCHK(hipEventRecord(g->own[k][i], g->xs[i]));
			host_done.push_back(g->own[k][i]);
		}
		bool sent = false;
		if(g->use_rccl && nbytes == per * (size_t)n) {
			// ncclAllGather in place (every member's stripe already sits at its place in that member's copy of the block), one rank per
			// device, all enqueued from this thread as one group
			bool ok = g->p_gstart() == ncclSuccess;
			for(int i = 0; i < n && ok; i++) ok = g->p_allgather(g->blk[k][i] + off[i], g->blk[k][i], per, ncclChar, g->comms[i], g->xs[i]) == ncclSuccess;
			ok = g->p_gend() == ncclSuccess && ok;
			if(ok) {
				sent = true; g->last_form = 3;
				for(int i = 0; i < n; i++) { GRPCHK(hipSetDevice(g->dev[i])); GRPCHK(hipEventRecord(g->ready[k][i], g->xs[i])); GRPCHK(hipStreamWaitEvent(g->ctx[i]->streams.front, g->ready[k][i], 0)); }
			} else {
				fprintf(stderr, "vdl2hip: RCCL all-gather failed - falling back to peer copies\n");
				g->use_rccl = false;
				for(int i = 0; i < n; i++) { GRPCHK(hipSetDevice(g->dev[i])); GRPCHK(hipStreamSynchronize(g->xs[i])); }
			}
		}
		if(!sent) {
			g->last_form = 2;
			for(int i = 0; i < n; i++) {
				GRPCHK(hipSetDevice(g->dev[i]));
				const int npx = (int)g->px[i].size();
				std::vector<char> used(npx, 0);
				for(int d = 1; d < n; d++) {
					const int j = (i + d) % n;                                  // member i starts with its right-hand neighbour: at any time the fetches in flight use distinct links
					if(off[j + 1] == off[j]) continue;
					hipStream_t st = g->px[i][(d - 1) % npx];
					GRPCHK(hipStreamWaitEvent(st, g->own[k][j], 0));
					GRPCHK(hipMemcpyPeerAsync(g->blk[k][i] + off[j], g->dev[i], g->blk[k][j] + off[j], g->dev[j], off[j + 1] - off[j], st));
					used[(d - 1) % npx] = 1;
				}
				GRPCHK(hipStreamWaitEvent(g->ctx[i]->streams.front, g->own[k][i], 0));
				for(int x = 0; x < npx; x++) if(used[x]) { GRPCHK(hipEventRecord(g->got[k][i][x], g->px[i][x])); GRPCHK(hipStreamWaitEvent(g->ctx[i]->streams.front, g->got[k][i][x], 0)); }
			}
		}
	} else if(n == 1 && wait_copy) {
		// ---- a group of one (the adapter's default) fed from caller-owned memory: the blocking copy, nothing to wait for afterwards
		//      (the same short cut as vdl2hip_feed(): feed_host) ----
		GRPCHK(hipSetDevice(g->dev[0]));
		// (relies on hipMemcpy() having landed in device memory when it returns: see feed_host() in vdl2hip.hip)
		GRPCHK(hipMemcpy(g->blk[k][0], buf, nbytes, hipMemcpyHostToDevice));
		g->last_form = 0;
	} else {
		// ---- broadcast: the block crosses PCIe once, into the first member, and goes from there to the others ----
		GRPCHK(hipSetDevice(g->dev[0]));
		GRPCHK(hipMemcpyAsync(g->blk[k][0], buf, nbytes, hipMemcpyHostToDevice, g->xs[0]));
		GRPCHK(hipEventRecord(g->own[k][0], g->xs[0]));
		host_done.push_back(g->own[k][0]);
		bool sent = false;
		if(g->use_rccl && n > 1) {
			bool ok = true;
			for(int i = 1; i < n && ok; i++) { ok = hipSetDevice(g->dev[i]) == hipSuccess && hipStreamWaitEvent(g->xs[i], g->own[k][0], 0) == hipSuccess; }
			ok = ok && g->p_gstart() == ncclSuccess;
			for(int i = 0; i < n && ok; i++)
				ok = g->p_bcast(g->blk[k][0], g->blk[k][i], nbytes, ncclChar, 0, g->comms[i], g->xs[i]) == ncclSuccess;
			ok = g->p_gend() == ncclSuccess && ok;
			if(ok) {
				sent = true; g->last_form = 1;
				for(int i = 0; i < n; i++) { GRPCHK(hipSetDevice(g->dev[i])); GRPCHK(hipEventRecord(g->ready[k][i], g->xs[i])); GRPCHK(hipStreamWaitEvent(g->ctx[i]->streams.front, g->ready[k][i], 0)); }
			} else {
				// nothing of this block has reached a member's receiver yet: the peer-copy fan-out below redoes the whole exchange
				fprintf(stderr, "vdl2hip: RCCL broadcast failed - falling back to peer copies\n");
				g->use_rccl = false;
				for(int i = 0; i < n; i++) { GRPCHK(hipSetDevice(g->dev[i])); GRPCHK(hipStreamSynchronize(g->xs[i])); }
			}
		}
		if(!sent) {
			g->last_form = 0;
			GRPCHK(hipSetDevice(g->dev[0]));
			GRPCHK(hipStreamWaitEvent(g->ctx[0]->streams.front, g->own[k][0], 0));
			for(int i = 1; i < n; i++) {
				GRPCHK(hipSetDevice(g->dev[i]));
				GRPCHK(hipStreamWaitEvent(g->xs[i], g->own[k][0], 0));
				GRPCHK(hipMemcpyPeerAsync(g->blk[k][i], g->dev[i], g->blk[k][0], g->dev[0], nbytes, g->xs[i]));
				GRPCHK(hipEventRecord(g->ready[k][i], g->xs[i]));
				GRPCHK(hipStreamWaitEvent(g->ctx[i]->streams.front, g->ready[k][i], 0));
			}
		}
	}
	if(wait_copy) { for(hipEvent_t e : host_done) GRPCHK(hipEventSynchronize(e)); }     // `buf` is only ours during the call
	else g->pinned_pending = host_done;
	int rc = VDL2HIP_OK;
	for(int i = 0; i < n; i++) {
		GRPCHK(hipSetDevice(g->dev[i]));
		int r = feed_block(g->ctx[i], g->blk[k][i], nbytes);      // (every member resamples the whole block itself, where the receiver resamples)
		if(r != VDL2HIP_OK) { g->failed = true; rc = r; break; }
	}
	g->feed_no++;
	return rc;
}

int vdl2hip_group_feed(vdl2hip_group *g, const void *buf, size_t nbytes) { return group_feed(g, buf, nbytes, true); }

int vdl2hip_group_feed_pinned(vdl2hip_group *g, const void *buf, size_t nbytes) { return group_feed(g, buf, nbytes, false); }

int vdl2hip_group_sync(vdl2hip_group *g) {
	if(!g) return VDL2HIP_E_INVAL;
	if(g->failed) return VDL2HIP_E_DEVICE;
	DeviceGuard guard;
	{ int r = group_wait_pinned(g); if(r != VDL2HIP_OK) return r; }
	int rc = VDL2HIP_OK;
	for(int i = 0; i < g->n; i++) { HIPCHK(hipSetDevice(g->dev[i])); int r = vdl2hip_sync(g->ctx[i]); if(r != VDL2HIP_OK) rc = r; }
	return rc;
}

// deliver every finished frame of every member, merged into the order vdl2hip_drain() uses: (end_sample, chan, idx)
int vdl2hip_group_drain(vdl2hip_group *g, vdl2hip_frame_cb cb, void *user) {
	if(!g) return VDL2HIP_E_INVAL;
	if(g->failed) return VDL2HIP_E_DEVICE;
	DeviceGuard guard;
	for(int i = 0; i < g->n; i++) {
		HIPCHK(hipSetDevice(g->dev[i]));
		vdl2hip_ctx *c = g->ctx[i];
		if(c->failed) return VDL2HIP_E_DEVICE;
		int r = collect_pending(c, c->drain_lag);
		if(r != VDL2HIP_OK && r != VDL2HIP_E_OVERFLOW) return r;
		for(auto &h : c->queue) g->merged.push_back(vdl2hip_group::QF{ std::move(h), i });
		c->queue.clear();
	}
	std::stable_sort(g->merged.begin(), g->merged.end(), [g](const vdl2hip_group::QF &a, const vdl2hip_group::QF &b) {
		if(a.h.f.end_sample != b.h.f.end_sample) return a.h.f.end_sample < b.h.f.end_sample;
		const int ca = a.h.f.chan + g->ctx[a.who]->chan_first, cb_ = b.h.f.chan + g->ctx[b.who]->chan_first;
		if(ca != cb_) return ca < cb_;
		return a.h.f.idx < b.h.f.idx;
	});
	int n = 0;
	for(const auto &q : g->merged) {
		if(cb) { vdl2hip_frame f{}; fill_frame(g->ctx[q.who], q.h, f); cb(&f, user); }
		n++;
	}
	g->merged.clear();
	return n;
}

int vdl2hip_group_set_drain_lag(vdl2hip_group *g, int lag) {
	if(!g) return VDL2HIP_E_INVAL;
	for(int i = 0; i < g->n; i++) { int r = vdl2hip_set_drain_lag(g->ctx[i], lag); if(r != VDL2HIP_OK) return r; }
	return VDL2HIP_OK;
}

static vdl2hip_ctx *group_owner(vdl2hip_group *g, uint32_t chan) {
	if(!g) return nullptr;
	for(int i = 0; i < g->n; i++) if(chan >= (uint32_t)g->ctx[i]->chan_first && chan < (uint32_t)(g->ctx[i]->chan_first + g->ctx[i]->C)) return g->ctx[i];
	return nullptr;
}

int vdl2hip_group_counters(vdl2hip_group *g, uint32_t chan, uint64_t out[VDL2HIP_NUM_COUNTERS]) {
	vdl2hip_ctx *c = group_owner(g, chan);
	if(!c) return VDL2HIP_E_INVAL;
	DeviceGuard guard;
	HIPCHK(hipSetDevice(c->cfg.device));
	return vdl2hip_counters(c, chan, out);
}

int vdl2hip_group_avlc_counters(vdl2hip_group *g, uint32_t chan, uint64_t out[VDL2HIP_NUM_AVLC_COUNTERS]) {
	vdl2hip_ctx *c = group_owner(g, chan);
	if(!c) return VDL2HIP_E_INVAL;
	DeviceGuard guard;
	HIPCHK(hipSetDevice(c->cfg.device));
	return vdl2hip_avlc_counters(c, chan, out);
}

}  // extern "C"
