// hostmem.h - host-only owners of what the HIP runtime hands out: one device allocation, one page-locked allocation, one event.
// The owner is the member and its destructor is the free: a struct that holds these needs no list of what to release, and cannot
// be copied by accident (all three are move-only and start empty).  Each kind counts its live objects (g_live: what the test hook
// vdl2hip_debug_live_resources reports) - the only state there is beside the handles themselves.
// Streams are not owned here: a receiver's streams outlive it in the pool (vdl2hip.hip, kSidePre).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>

namespace hostmem {

enum { LIVE_DEVICE = 0, LIVE_PINNED = 1, LIVE_EVENT = 2 };
inline std::atomic<long> g_live[3];

// one hipMalloc of `count` elements of T
template<typename T>
class DevBuf {
	T *p_ = nullptr; size_t bytes_ = 0;
public:
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
	DevBuf &operator=(DevBuf &&o) noexcept { if(this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); } return *this; }
	~DevBuf() { reset(); }
	// (a failed call leaves the owner empty and the runtime's error state clear: the caller reports, the next HIP call is not blamed)
	hipError_t alloc_bytes(size_t bytes, bool zero = false) {
		reset();
		hipError_t e = hipMalloc((void **)&p_, bytes);
		if(e != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return e; }
		bytes_ = bytes; g_live[LIVE_DEVICE]++;
		if(zero && (e = hipMemset(p_, 0, bytes)) != hipSuccess) { (void)hipGetLastError(); reset(); }
		return e;
	}
	hipError_t alloc(size_t count, bool zero = false) { return alloc_bytes(count * sizeof(T), zero); }
	void reset() { if(p_) { (void)hipFree(p_); g_live[LIVE_DEVICE]--; } p_ = nullptr; bytes_ = 0; }
	size_t bytes() const { return bytes_; }
	T *get() const { return p_; }
	operator T *() const { return p_; }      // kernel argument structs are filled as they were with raw pointers
};

// one hipHostMalloc (page-locked), in bytes
class PinnedBuf {
	uint8_t *p_ = nullptr; size_t bytes_ = 0;
public:
	PinnedBuf() = default;
	PinnedBuf(PinnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
	PinnedBuf &operator=(PinnedBuf &&o) noexcept { if(this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); } return *this; }
	~PinnedBuf() { reset(); }
	hipError_t alloc(size_t bytes, bool zero = false) {
		reset();
		const hipError_t e = hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault);
		if(e != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return e; }
		bytes_ = bytes; g_live[LIVE_PINNED]++;
		if(zero) memset(p_, 0, bytes);
		return e;
	}
	// staging that grows on demand - the one policy: half as much again as is needed now, at least 1 MiB, the old block freed first
	hipError_t reserve(size_t need) { return need <= bytes_ ? hipSuccess : alloc(std::max<size_t>(need + need / 2, 1u << 20)); }
	void reset() { if(p_) { (void)hipHostFree(p_); g_live[LIVE_PINNED]--; } p_ = nullptr; bytes_ = 0; }
	size_t bytes() const { return bytes_; }
	template<typename T> T *as() const { return reinterpret_cast<T *>(p_); }
	operator uint8_t *() const { return p_; }
};

// one hipEvent_t, created on first use
class Event {
	hipEvent_t e_ = nullptr;
public:
	Event() = default;
	Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
	Event &operator=(Event &&o) noexcept { if(this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); } return *this; }
	~Event() { reset(); }
	hipError_t ensure(unsigned flags = 0) {
		if(e_) return hipSuccess;
		const hipError_t e = hipEventCreateWithFlags(&e_, flags);
		if(e != hipSuccess) { e_ = nullptr; (void)hipGetLastError(); return e; }
		g_live[LIVE_EVENT]++;
		return e;
	}
	void reset() { if(e_) { (void)hipEventDestroy(e_); g_live[LIVE_EVENT]--; } e_ = nullptr; }
	operator hipEvent_t() const { return e_; }
};

// The mailbox of a tap that delivers records, one per feed in flight.  The device side is one allocation: a header, the records behind
// it.  The host side is a page-locked landing place for the header and the first kMailRecs records: post() brings them in one small
// copy queued behind the tap's kernels, which is all most feeds of a live receiver need.  A feed with more records has all of them
// fetched into a staging buffer of the caller's, who may have more to copy into it (the burst capture: its IQ) before the one wait.
constexpr uint32_t kMailRecs = 32;
template<typename Hdr, typename Rec>
class RecordMail {
	DevBuf<Hdr> d_; PinnedBuf h_;
public:
	static constexpr size_t kMailBytes = sizeof(Hdr) + kMailRecs * sizeof(Rec);
	// room for `cap` records; the mail's share of the device side and the landing place start zeroed (an error with the mail
	// standing - operator bool - is the clearing's, any other an allocation's)
	hipError_t alloc(size_t cap) {
		hipError_t e = d_.alloc_bytes(sizeof(Hdr) + std::max<size_t>(cap, kMailRecs) * sizeof(Rec));
		if(e == hipSuccess) e = h_.alloc(kMailBytes, true);
		if(e == hipSuccess && (e = hipMemset(d_, 0, kMailBytes)) != hipSuccess) (void)hipGetLastError();
		return e;
	}
	explicit operator bool() const { return h_.bytes() != 0; }
	Hdr *d_hdr() const { return d_; }
	Rec *d_rec() const { return reinterpret_cast<Rec *>(d_.get() + 1); }
	hipError_t post(hipStream_t st) const { return hipMemcpyAsync(h_, d_, kMailBytes, hipMemcpyDeviceToHost, st); }
	// once the feed is done: the header as post() brought it ...
	const Hdr &hdr() const { return *h_.template as<Hdr>(); }
	// ... and its `nrec` records: in the landing place, or - staged(nrec) bytes - at the start of `stage`, copied there on `out` and
	// waited for.  extra: the caller copies as many bytes behind them on `out` and then waits itself, if there is anything to wait for
	static size_t staged(uint32_t nrec) { return nrec > kMailRecs ? sizeof(Rec) * (size_t)nrec : 0; }
	hipError_t fetch(uint32_t nrec, PinnedBuf &stage, hipStream_t out, const Rec *&rec, bool wait = true, size_t extra = 0) const {
		const size_t bytes = staged(nrec);
		hipError_t e = stage.reserve(bytes + extra);
		rec = bytes ? stage.as<Rec>() : reinterpret_cast<const Rec *>(h_ + sizeof(Hdr));
		if(e == hipSuccess && bytes) e = hipMemcpyAsync(stage, d_rec(), bytes, hipMemcpyDeviceToHost, out);
		return e == hipSuccess && bytes && wait ? hipStreamSynchronize(out) : e;
	}
};

}  // namespace hostmem
