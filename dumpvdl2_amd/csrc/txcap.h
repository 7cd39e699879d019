// txcap.h - the transmission capture: for every transmission the transmission log closes, the channel's decimated samples around it
// and a Welch-averaged power spectrum of the channel during it - what a foreign carrier, a collision or a burst too weak to
// synchronise looked like.  Not in the reference.  Definition: vdl2hip.h, "Transmission capture".  A read-only pass behind
// k_frame_finish of the feed that closes the transmission (the preamble search's placement): it reads the log's records of the feed
// and y, writes buffers of its own, and touches nothing the decoder, the activity monitor, the log or the search read or write.
//
// k_txcap_plan: one workgroup over the feed's records, 256 at a time.  Each lane works out the IQ window of one record, its extent,
// its segments and its number of pieces of kTxcPieceFloats / N segments (txc_plan_rec); two inclusive scans - per wavefront by
// __shfl_up, the four wavefronts' totals through LDS - carried from one round of 256 to the next give every record the place of its
// window in the IQ pool and the offset of its pieces among the feed's.  The lane writes the whole record: every integer field is
// known here.  A window that ends beyond the pool is refused; offsets only grow, so every record behind it is refused too and the
// pairs in use are those up to the last window that fitted (an integer maximum over the lanes).
//
// k_txcap_copy: 256 lanes, a workgroup per record, grid-stride: the burst capture's cap_copy().
//
// k_txcap_spectrum: 256 lanes, a workgroup per piece, grid-stride over the feed's pieces.  A piece's record is found by a search in
// poff[].  The piece's (ns + 1) N / 2 samples are loaded from the ring ONCE into LDS (lane l takes samples l, l + 256, ...: coalesced,
// the ring index masked per element); its ns overlapping segments are then taken from there.  A transform of N points has N / 4
// butterflies a pass: the workgroup is G = 1024 / N groups of N / 4 lanes - 64 lanes, a full wavefront, at N = 256; four groups to a
// wavefront at N = 64 - and group g takes segments g, g + G, ... of the piece, a round of G segments at a time, each group in a pair
// of padded buffers of its own (spec_pad: spectrum.h says why).  The transform is the input monitor's: spec_pass4 / spec_pass2 and
// the host's twiddle table, no device sin / cos.  A lane keeps its four bins of its group's sum in float64 registers and stores them
// to LDS, where a lane per bin adds the groups' sums in group order into row `piece` of part[]: plain stores, no atomics.
//
// k_txcap_reduce: a lane per bin adds a record's rows in index order, narrows once and stores.  Pieces ascending, within a piece the
// groups ascending, within a group the rounds ascending: an order that is a function of the record's segment count and N alone.
// The per-record and per-piece steps are functions that also compile for the host: vdl2hip_debug_txcap_* run them lane by lane (tests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vdl2_core.h"
#include "txlog.h"
#include "txsearch.h"
#include "capture.h"
#include "spectrum.h"

namespace vdl2 {

constexpr int kTxcThreads = 256;
constexpr uint32_t kTxcMinN = 64, kTxcMaxN = 1024, kTxcDefN = 256;
constexpr uint32_t kTxcPieceFloats = 8192;           // segments of a piece times N: a piece covers 4096 + N / 2 samples
constexpr uint32_t kTxcGroupFloats = 1024;           // groups of a workgroup times N: N / 4 lanes a group
constexpr uint32_t kTxcRounds = kTxcPieceFloats / kTxcGroupFloats;
constexpr uint32_t kTxcMaxPre = 4096, kTxcMaxPool = 1u << 24, kTxcDefPool = 1u << 20, kTxcDefSpectra = 1024, kTxcMaxSpecFloats = 1u << 24;
// cfg.flags (VDL2HIP_TXCAP_*) and record flags (VDL2HIP_TXC_*; bit 0 is VDL2HIP_TX_PARTIAL, passed on)
constexpr uint32_t kTxcapIq = 1u, kTxcapSpectrum = 2u, kTxcapUndecodedOnly = 4u;
constexpr uint32_t kTxcClipped = 2u, kTxcTruncated = 4u, kTxcNoRoom = 8u, kTxcShort = 16u, kTxcNoSpectrum = 32u;
static_assert(kTxcMaxN <= kTxcGroupFloats && kTxcGroupFloats / 4 == kTxcThreads && kTxcPieceFloats % kTxcGroupFloats == 0, "N / 4 lanes a group, 256 lanes, whole rounds");

// the record as the device writes it; the layout is vdl2hip_tx_capture's (vdl2hip.hip asserts size and offsets): the host copies it
// as it is, turns iq_off and spec_off into offsets of the caller's buffers and fills in frames and frames_ok
struct TxcRec {
	uint32_t chan, freq; uint64_t first_bin; int64_t win_first, win_last; uint64_t iq_off, spec_off;
	uint32_t iq_count, flags, segments, nfft, frames, frames_ok, reserved[2];
};
struct TxcHdr { uint32_t nrec, npieces; uint64_t pairs; };     // records and pieces of the feed; pairs of the IQ pool in use
struct TxcCfg { uint64_t pool_samples; uint32_t flags, pre, post, max_iq, N, pool_spectra; };

struct TxcArgs {
	const cf32 *y; const TxHdr *txhdr; const TxRec *txrec;         // txhdr, txrec: the log's, of the same feed
	const float *w; const float2 *tw;                              // [N] each: the window, exp(-2 pi i k / N)
	uint32_t *poff; double *part; TxcRec *rec; TxcHdr *hdr;        // poff: [txpool + 1]; part: [piece_cap][N]
	cf32 *pool; float *spec;                                       // pool: [pool_samples]; spec: [pool_spectra][N]
	TxcCfg k; double norm;                                         // norm: 1 / (sum w)^2
	uint32_t txpool, piece_cap, cap, mask, chan_first, log2n;
};

__host__ __device__ __forceinline__ uint32_t txc_groups(uint32_t N) { return kTxcGroupFloats / N; }
__host__ __device__ __forceinline__ uint32_t txc_piece_segments(uint32_t N) { return kTxcPieceFloats / N; }
// the IQ window of a record: [max(0, first - pre, last - (kTxsSpan - 1)), last + post]
__host__ __device__ __forceinline__ void txc_window(int64_t first, int64_t last, uint32_t pre, uint32_t post, int64_t &wfirst, int64_t &wlast, uint32_t &flags) {
	int64_t lo = first - (int64_t)pre; if(lo < 0) lo = 0;
	const int64_t back = last - (kTxsSpan - 1);
	wfirst = back > lo ? back : lo; wlast = last + (int64_t)post; flags = back > lo ? kTxcClipped : 0u;
}
// segments of N samples, N / 2 apart, in an extent of len samples
__host__ __device__ __forceinline__ uint32_t txc_segments(int64_t len, uint32_t N) { return len >= (int64_t)N ? (uint32_t)((len - (int64_t)N) / (int64_t)(N / 2)) + 1u : 0u; }
__host__ __device__ __forceinline__ uint32_t txc_pieces(uint32_t S, uint32_t N) { const uint32_t q = txc_piece_segments(N); return (S + q - 1) / q; }
// record i of the feed from the log's record: everything but its place in the IQ pool; count: its window's pairs BEFORE room,
// pieces: of its spectrum
__host__ __device__ __forceinline__ void txc_plan_rec(const TxRec &t, uint32_t i, const TxcCfg &k, TxcRec &r, uint32_t &count, uint32_t &pieces) {
	uint32_t fl;
	txc_window(t.first_sample, t.last_sample, k.pre, k.post, r.win_first, r.win_last, fl);
	r.chan = t.chan; r.freq = t.freq; r.first_bin = t.first_bin; r.iq_off = 0; r.spec_off = 0;
	count = 0; pieces = 0; r.segments = 0; r.nfft = 0;
	if(k.flags & kTxcapIq) {
		const int64_t len = r.win_last - r.win_first + 1;                // (at most kTxsSpan + post; a partial record nothing was seen of may have none)
		count = len > 0 ? (uint32_t)len : 0u;
		if(k.max_iq && count > k.max_iq) { count = k.max_iq; fl |= kTxcTruncated; }
	}
	if(k.flags & kTxcapSpectrum) {
		r.nfft = k.N;
		if(i < k.pool_spectra) {
			int64_t ef; uint32_t efl;
			txs_range(t.first_sample, t.last_sample, ef, efl);
			r.segments = txc_segments(t.last_sample - ef + 1, k.N);
			r.spec_off = (uint64_t)i * k.N;
			pieces = txc_pieces(r.segments, k.N);
			if(!r.segments) fl |= kTxcShort;
		} else fl |= kTxcNoSpectrum;
	}
	r.iq_count = count; r.flags = fl | (t.flags & kTxPartial);
	r.frames = 0; r.frames_ok = 0; r.reserved[0] = 0; r.reserved[1] = 0;
}
// ... and its place: pair `off` of the pool, if its window ends inside it
__host__ __device__ __forceinline__ bool txc_place(TxcRec &r, uint64_t off, const TxcCfg &k) {
	if(!(k.flags & kTxcapIq)) return true;
	if(off + r.iq_count > k.pool_samples) { r.iq_count = 0; r.flags |= kTxcNoRoom; return false; }
	r.iq_off = off;
	return true;
}
// piece p of a record with S segments: its first segment, how many it has
__host__ __device__ __forceinline__ void txc_piece(uint32_t S, uint32_t N, uint32_t p, uint32_t &s0, uint32_t &ns) {
	const uint32_t q = txc_piece_segments(N);
	s0 = p * q; ns = S - s0 < q ? S - s0 : q;
}
// one lane's share of the piece's samples: smp[spec_pad(j)] = y[base + j], j < count = (ns + 1) N / 2; the ring index is masked per
// element (padded: the groups of a wavefront read N / 2 samples apart, which at N = 64 would be the same banks)
__host__ __device__ __forceinline__ void txc_load_step(const cf32 *yc, uint32_t mask, int64_t base, uint32_t count, uint32_t lane, uint32_t nl, float2 *smp) {
	for(uint32_t j = lane; j < count; j += nl) { const cf32 v = yc[(uint32_t)((base + (int64_t)j) & (int64_t)mask)]; smp[spec_pad(j)] = make_float2(v.re, v.im); }
}
// lane l (of N / 4) of a group: segment s of the piece, times the window, into the group's first buffer
__host__ __device__ __forceinline__ void txc_fill_step(const float2 *smp, const float *w, uint32_t N, uint32_t s, uint32_t l, float2 *x) {
	#pragma unroll
	for(uint32_t r = 0; r < 4; r++) {
		const uint32_t n = l + r * (N >> 2);
		const float2 v = smp[spec_pad(s * (N >> 1) + n)]; const float wn = w[n];
		x[spec_pad(n)] = make_float2(v.x * wn, v.y * wn);
	}
}
// ... its butterflies of pass `pass` (radix 4 while 4 divides what is left, one radix-2 pass at the end where log2 N is odd); a
// barrier behind every pass, the buffers change places.  false: there is no such pass
__host__ __device__ __forceinline__ bool txc_pass_step(const float2 *x, float2 *y, const float2 *tw, uint32_t N, uint32_t log2n, uint32_t pass, uint32_t l) {
	const uint32_t log2s = 2 * pass;
	if(log2s + 2 <= log2n) { spec_pass4(x, y, tw, N, log2s, l); return true; }
	if(log2s < log2n) { spec_pass2(x, y, N, l); spec_pass2(x, y, N, l + (N >> 2)); return true; }
	return false;
}
__host__ __device__ __forceinline__ uint32_t txc_passes(uint32_t log2n) { return (log2n + 1) / 2; }
// ... and its four bins of |X|^2 (two products and a sum in float32), bin i of the ascending-frequency order being X[(i + N / 2) mod N]
__host__ __device__ __forceinline__ void txc_power_step(const float2 *x, uint32_t N, uint32_t l, double acc[4]) {
	#pragma unroll
	for(uint32_t r = 0; r < 4; r++) {
		const uint32_t i = l + r * (N >> 2);
		const float2 X = x[spec_pad((i + (N >> 1)) & (N - 1))];
		const float q = X.x * X.x + X.y * X.y;
		acc[r] += (double)q;
	}
}
// bin i of a piece from its groups' sums gacc[G][N]: added in group order
__host__ __device__ __forceinline__ double txc_group_sum(const double *gacc, uint32_t G, uint32_t N, uint32_t i) {
	double s = 0.0;
	for(uint32_t g = 0; g < G; g++) s += gacc[(size_t)g * N + i];
	return s;
}
// bin i of a record with S segments from its pieces' rows [first_row .. first_row + rows) of part[]: added in index order, narrowed once
__host__ __device__ __forceinline__ float txc_reduce_bin(const double *part, uint32_t first_row, uint32_t rows, uint32_t N, uint32_t i, double norm, uint32_t S) {
	double s = 0.0;
	for(uint32_t r = 0; r < rows; r++) s += part[(size_t)(first_row + r) * N + i];
	return (float)(s * norm / (double)S);
}
// LDS of k_txcap_spectrum in float2: the piece's samples (padded), then a pair of padded buffers per group - over which the groups'
// float64 sums [G][N] go once the transforms are done: G N doubles, less than the G 2 N float2 they replace
__host__ __device__ __forceinline__ uint32_t txc_span(uint32_t N) { return spec_pad((txc_piece_segments(N) + 1) * (N >> 1)) + 1; }
__host__ __device__ __forceinline__ uint32_t txc_half(uint32_t N) { return spec_pad(N) + 1; }
inline size_t txc_lds_bytes(uint32_t N) { return ((size_t)txc_span(N) + (size_t)txc_groups(N) * 2 * txc_half(N)) * sizeof(float2); }

#ifdef __HIPCC__
// an inclusive scan of v over the workgroup's 256 lanes (wsum: [4] in LDS; a barrier behind it before wsum is written again) -> the
// lane's inclusive value; total: the workgroup's
template<typename T>
__device__ __forceinline__ T txc_scan(T v, uint32_t lane, uint32_t wave, T *wsum, T &total) {
	T inc = v;
	#pragma unroll
	for(int d = 1; d < 64; d <<= 1) { const T o = __shfl_up(inc, d); if(lane >= (uint32_t)d) inc += o; }
	if(lane == 63) wsum[wave] = inc;
	__syncthreads();
	T before = 0; total = 0;
	#pragma unroll
	for(uint32_t k = 0; k < (uint32_t)kTxcThreads / 64; k++) { const T s = wsum[k]; if(k < wave) before += s; total += s; }
	return before + inc;
}

__global__ __launch_bounds__(kTxcThreads) void k_txcap_plan(const TxcArgs a) {
	__shared__ uint64_t wsum_iq[kTxcThreads / 64];
	__shared__ uint32_t wsum_p[kTxcThreads / 64];
	__shared__ unsigned long long used;
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t nlog = a.txhdr->nrec, nrec = nlog < a.txpool ? nlog : a.txpool;
	if(t == 0) used = 0;
	uint64_t carry_iq = 0; uint32_t carry_p = 0;
	for(uint32_t w = 0; w < nrec; w += kTxcThreads) {                      // (uniform)
		const uint32_t i = w + t;
		TxcRec r; uint32_t cnt = 0, pieces = 0;
		if(i < nrec) txc_plan_rec(a.txrec[i], i, a.k, r, cnt, pieces);
		uint64_t tot_iq; uint32_t tot_p;
		const uint64_t inc_iq = txc_scan<uint64_t>(cnt, lane, wave, wsum_iq, tot_iq);
		const uint32_t inc_p = txc_scan<uint32_t>(pieces, lane, wave, wsum_p, tot_p);
		if(i < nrec) {
			const uint64_t off = carry_iq + inc_iq - cnt;
			const bool fits = txc_place(r, off, a.k);
			a.rec[i] = r;
			a.poff[i] = carry_p + inc_p - pieces;
			if(fits && cnt) atomicMax(&used, (unsigned long long)(off + cnt));      // (an integer maximum in LDS: whatever the order, the same)
		}
		carry_iq += tot_iq; carry_p += tot_p;
		__syncthreads();                                                // (the scans' totals are written again by the next round)
	}
	__syncthreads();
	if(t == 0) { a.poff[nrec] = carry_p; TxcHdr h; h.nrec = nrec; h.npieces = carry_p < a.piece_cap ? carry_p : a.piece_cap; h.pairs = used; *a.hdr = h; }
}

__global__ __launch_bounds__(kTxcThreads) void k_txcap_copy(const TxcArgs a) {
	const uint32_t nrec = a.hdr->nrec;
	for(uint32_t i = blockIdx.x; i < nrec; i += gridDim.x) {                // (uniform)
		const TxcRec r = a.rec[i];
		if(!r.iq_count) continue;
		cap_copy(a.y + (size_t)(r.chan - a.chan_first) * a.cap, a.mask, r.win_first, r.iq_count, a.pool + r.iq_off, r.iq_off, threadIdx.x, kTxcThreads);
	}
}

__global__ __launch_bounds__(kTxcThreads) void k_txcap_spectrum(const TxcArgs a) {
	extern __shared__ float2 txc_lds[];
	const uint32_t N = a.k.N, G = txc_groups(N), lane = threadIdx.x, g = lane / (N >> 2), l = lane & ((N >> 2) - 1);
	const uint32_t nrec = a.hdr->nrec, total = a.hdr->npieces, npass = txc_passes(a.log2n);
	float2 *smp = txc_lds, *bufa = txc_lds + txc_span(N) + (size_t)g * 2 * txc_half(N), *bufb = bufa + txc_half(N);
	for(uint32_t pc = blockIdx.x; pc < total; pc += gridDim.x) {            // (uniform)
		const uint32_t i = txs_find_rec(a.poff, nrec, pc);
		const TxRec t = a.txrec[i];
		int64_t ef; uint32_t efl;
		txs_range(t.first_sample, t.last_sample, ef, efl);
		const uint32_t S = txc_segments(t.last_sample - ef + 1, N);
		uint32_t s0, ns;
		txc_piece(S, N, pc - a.poff[i], s0, ns);
		txc_load_step(a.y + (size_t)(t.chan - a.chan_first) * a.cap, a.mask, ef + (int64_t)s0 * (int64_t)(N >> 1), (ns + 1) * (N >> 1), lane, kTxcThreads, smp);
		__syncthreads();
		double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
		for(uint32_t rd = 0; rd < kTxcRounds; rd++) {                       // (uniform)
			const uint32_t s = rd * G + g;
			const bool mine = s < ns;
			if(mine) txc_fill_step(smp, a.w, N, s, l, bufa);
			__syncthreads();
			float2 *x = bufa, *y = bufb;
			for(uint32_t p = 0; p < npass; p++) {
				if(mine) txc_pass_step(x, y, a.tw, N, a.log2n, p, l);
				__syncthreads();
				float2 *sw = x; x = y; y = sw;
			}
			if(mine) txc_power_step(x, N, l, acc);
			__syncthreads();                                            // (the next round overwrites both buffers)
		}
		double *gacc = (double *)(txc_lds + txc_span(N));
		#pragma unroll
		for(uint32_t r = 0; r < 4; r++) gacc[(size_t)g * N + l + r * (N >> 2)] = acc[r];
		__syncthreads();
		for(uint32_t b = lane; b < N; b += kTxcThreads) a.part[(size_t)pc * N + b] = txc_group_sum(gacc, G, N, b);
		__syncthreads();                                                // (smp and the buffers are written again by the next piece)
	}
}

__global__ __launch_bounds__(kTxcThreads) void k_txcap_reduce(const TxcArgs a) {
	const uint32_t nrec = a.hdr->nrec, N = a.k.N;
	for(uint32_t i = blockIdx.x; i < nrec; i += gridDim.x) {                // (uniform)
		const TxcRec r = a.rec[i];
		if(r.nfft == 0 || (r.flags & kTxcNoSpectrum)) continue;
		const uint32_t p0 = a.poff[i], p1 = a.poff[i + 1] < a.piece_cap ? a.poff[i + 1] : a.piece_cap;      // (p1 <= piece_cap: always - txcap_piece_cap())
		for(uint32_t b = threadIdx.x; b < N; b += kTxcThreads)
			a.spec[r.spec_off + b] = r.segments && p1 > p0 ? txc_reduce_bin(a.part, p0, p1 - p0, N, b, a.norm, r.segments) : 0.f;
	}
}
#endif  // __HIPCC__

}  // namespace vdl2
