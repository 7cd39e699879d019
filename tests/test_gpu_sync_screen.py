"""k_sync_screen (kernels.h: the screening tier of the sync kernel) and the exact tier against an exhaustive evaluation and against
plain references, at EVERY decimated sample of small captures built to cross the kernel's structures: the tile of 2 560 samples and
its 150 of history, the lane map (10 and 80 samples), the eight windows a lane shares, the fast path and the edge path, the early
exit, the 64-bit words, the NaN rule, the row offset per channel, the ring.

Every case feeds the same input to two receivers with the referee off (so that no scan overwrites y): S with the product's screen, X
with the test hook "screen_all" = 1 (every sample evaluated); both with the dense form of the exact tier.  What is asserted:

  1  X's pf (pherr, slope) is BIT-equal at every sample to tests/core_reference.py's numpy sync_metric on the device's exact phases
     of y (probed with vdl2hip_debug_core_probe, which tests/test_gpu_core_probe.py holds to libm), taps n-150 .. n step 10, phase 0
     before the stream;
  2  X's cand is pf[n-3].p < 4 and pf[n].p > pf[n-3].p of that reference (none for n < 3);
  3  the screen is sound: every sample whose reference pherr is under 4 is flagged in S; S's cand equals X's everywhere; S's pf is
     bit-equal to X's where the exact tier has work - a flagged sample, the samples 3 before and 3 after one, and the last 3 of a
     feed (whose right neighbour has not arrived) - and all-zero bits elsewhere (captures fed whole that do not wrap the ring);
  4  the flags are the screen's own: phase_fast of y from the device (probed), the 16-tap and the 12-tap screening value of every
     window with the host build's screen arithmetic, flag = !(value >= 5.5), a NaN flagged.  The module measures on the capture's own
     windows whether the device's screen arithmetic is bit-identical to the host build's; if it is, every flag must equal the
     prediction, otherwise exceptions are allowed only where the value lies within the measured difference of 5.5.  One licence the
     kernel has: a window whose 12-tap value is already 5.8 or more stops there unless another lane of its wavefront goes on, so
     where the 12-tap value is >= 5.8 and the 16-tap one is under 5.5 (an unwrap guard that trips in the last four taps) the flag
     may be either - nowhere else.  The bits past the last sample of the last word are zero;
  5  feed boundaries move nothing: the same input in pieces (odd lengths, some under 64 decimated samples, some ending inside a tile
     and inside a word, one single sample) passes 1-4 at every sample, with S's pf on exactly the samples with work - the last 3 of
     every piece included - and zero elsewhere.  (Not "the same bits as the whole feed": the channeliser's y itself moves in the
     last place under another cut of the stream, at most of its samples.)

Wall time of the module on an MI355X: see profiles/core_probe_device.txt."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import core_reference as cr
import pyhostsim
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
F32 = np.float32
CF = 136975000
OS = 10
TILE, HIST = 2560, 150
N_DEC = 13 * TILE - 37                    # 13 tiles, ending inside a tile and inside a word
N_IN = N_DEC * OS + 7
GRID = [0, 1, 9, 10, 63, 64, 79, 80, 2559, 2560 - 150, 2560 - 149]
FREQS = {1: [CF + 25000], 3: [CF - 50000, CF + 25000, CF + 87500]}
AMP = (0.15, 0.4)                         # weak bursts: amplitude over the noise's sigma per component of the input
SEED = {1: 3, 3: 4}                       # picked on the CPU (oracle trace + numpy sync_metric) so that the region 3 < pherr < 6 is populated


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


@pytest.fixture(scope="module")
def hs():
    H = C.CDLL(pyhostsim.build())
    H.hostsim_screen_turns.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return H


_captures = {}


def capture(nchan, start_at_zero=False):
    """complex64 [N_IN]: short bursts on noise, most of them around the sync threshold, different content on every channel.  Built once and shared"""
    key = (nchan, start_at_zero)
    if key in _captures:
        return _captures[key]
    from dumpvdl2_amd import synth
    rng = np.random.default_rng(SEED[nchan] + (100 if start_at_zero else 0))
    sps = synth.SPS * OS
    fs = synth.SYMBOL_RATE * sps
    acc = np.zeros(N_IN, dtype=np.complex128)
    for k, f in enumerate(FREQS[nchan]):
        at = 0 if start_at_zero else int(rng.integers(2000, 9000))
        nb = 0
        while True:
            # one burst in eight carries a frame and is loud enough to decode; the others are a weak unique word and two symbols
            loud = nb % 8 == 0
            nb += 1
            if loud:
                steps = synth.build_burst([synth.make_avlc_frame(rng.integers(0, 256, size=int(rng.integers(9, 14)), dtype=np.uint8).tobytes())]).symbols
            else:
                steps = rng.integers(0, 8, size=2)
            wave = synth.modulate(steps, sps, ramp_symbols=0 if at == 0 else (5 if loud else 2), start_phase=float(rng.uniform(0, 2 * np.pi)))
            if at == 0:
                wave = wave[4 * sps:]         # the pulse-shaping lead-in cut off: the unique word starts with the stream
            if at + wave.size >= N_IN:
                break
            amp = 0.03 if loud else 0.02 * float(rng.uniform(*AMP))
            w = 2.0 * np.pi * ((f - CF) + float(rng.uniform(-2, 2)) * 1e-6 * f) / fs
            acc[at:at + wave.size] += amp * wave * np.exp(1j * w * np.arange(at, at + wave.size))
            at += wave.size + int(rng.integers(100, 900))
    acc += 0.02 * (rng.standard_normal(N_IN) + 1j * rng.standard_normal(N_IN))
    out = acc.astype(np.complex64)
    out.setflags(write=False)
    _captures[key] = out
    return out


def as_s16(x):
    iq = np.empty(2 * len(x), dtype=np.float32)
    iq[0::2] = x.real; iq[1::2] = x.imag
    return np.clip(np.rint(iq * 32768.0), -32768, 32767).astype(np.int16)


def pieces_of(n_items, seed):
    """feed lengths in input samples: odd ones, some under 64 decimated samples, one single sample, ends inside tiles and words"""
    rng = np.random.default_rng(seed)
    out, k = [], 0
    while k < n_items:
        u = rng.random()
        m = 1 if len(out) == 3 else int(rng.integers(1, 64 * OS)) if u < 0.3 else int(rng.integers(1000, 6000)) * 2 + 1 if u < 0.6 else int(rng.integers(20000, 60000)) * 2 + 1
        m = min(m, n_items - k)
        out.append(m); k += m
    return out


@dataclasses.dataclass
class Run:
    y: list
    pf: list
    cand: list
    flags: list
    frames: list
    ndec: int


def run(vh, freqs, raw, fmt, screen_all, pieces=None, max_block=None, referee=0, oversample=OS, max_ppm=0.0, tail=None):
    """raw: int16 (interleaved) or complex64; pieces: feed lengths in input samples; tail: read only the last `tail` decimated samples"""
    item = 4 if fmt == vh.FMT_S16LE else 8
    b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    pieces = pieces or [b.size // item]
    rx = vh.Receiver(CF, list(freqs), oversample, fmt, max_ppm, max_block_bytes=max_block or max(pieces) * item)
    try:
        rx.debug_option("exact_tier", 1)
        rx.debug_option("screen_all", screen_all)
        if not referee:
            rx.debug_option("referee", 0)
        k = 0
        for m in pieces:
            rx.feed(b[k * item:(k + m) * item]); k += m
        assert k * item == b.size
        fr = rx.drain()
        D = k // oversample
        first = 0 if tail is None else max(0, D - tail)
        nword = ((D + 63) & ~63) - first
        r = Run([], [], [], [], fr, D)
        for c in range(len(freqs)):
            r.y.append(rx.read_decimated(c, first, D - first))
            pf, cand = rx.read_sync(c, first, D - first)
            r.pf.append(pf); r.cand.append(cand)
            r.flags.append(rx.read_flags(c, first, nword))
            assert len(r.y[-1]) == len(pf) == len(cand) == D - first and len(r.flags[-1]) == nword
        return r
    finally:
        rx.close()


def u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def windows_of(ph):
    """[n, 16]: ph[n - 150 + 10 i], 0 before the stream"""
    p = np.concatenate([np.zeros(HIST, dtype=F32), np.asarray(ph, dtype=F32)])
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(p, HIST + 1)[:, ::10])


def reference_metric(L, y):
    ph = cr.device_probe(L, "phase", y)[:, 0]
    return cr.sync_metric(windows_of(ph))


def predicted_flags(L, hs, y, stats):
    """-> (flag predicted from the 16-tap value, may stop after 12 taps, |16-tap value - 5.5|, the 16-tap value)"""
    pfast = cr.device_probe(L, "phase_fast", y)[:, 0]
    w = windows_of(pfast)
    n = len(w)
    v16 = np.zeros(n, dtype=F32); v12 = np.zeros(n, dtype=F32)
    hs.hostsim_screen_turns(w.ctypes.data, n, v16.ctypes.data, v12.ctypes.data)
    # is the device's screen arithmetic the host build's, on these very windows?  (NaN for NaN counts as the same)
    dev = cr.device_probe(L, "screen", w)
    for d, h in ((dev[:, 0], v16), (dev[:, 1], v12)):
        ne = (u32(d) != u32(h)) & ~(np.isnan(d) & np.isnan(h))
        stats["differ"] += int(ne.sum()); stats["windows"] += n
        both = np.isfinite(d) & np.isfinite(h)
        if (ne & both).any():
            stats["far"] = max(stats["far"], float(np.abs(d[ne & both].astype(np.float64) - h[ne & both]).max()))
        assert not (ne & ~both).any(), "the device's and the host build's screening values differ in being finite"
    with np.errstate(invalid="ignore"):
        return ~(v16 >= cr.SCREEN_THR), v12 >= cr.SCREEN_EARLY_THR, np.abs(v16.astype(np.float64) - 5.5), v16


def check_pair(vh, hs, S, X, label, whole_feed=True, wrapped=False, stats=None, populated=True, ends=None):
    """assertions 1-4 on one case; returns the flagged share"""
    L = vh.load_library()
    stats = stats if stats is not None else {"differ": 0, "windows": 0, "far": 0.0}
    under4 = between = 0
    nflag = nsamp = 0
    for c in range(len(S.y)):
        lab = f"{label}: channel {c}"
        assert np.array_equal(u32(S.y[c]), u32(X.y[c])), lab
        D = len(S.y[c])
        skip = HIST + 3 if wrapped else 0                      # (a tail of a wrapped ring: the first windows reach before what was read)
        p, s = reference_metric(L, S.y[c])
        # 1
        d = np.flatnonzero((u32(X.pf[c][:, 0]) != u32(p)) | (u32(X.pf[c][:, 1]) != u32(s)))
        d = d[d >= skip]
        assert d.size == 0, f"{lab}: X's pf differs from the numpy reference at {d.size} samples, first {d[:5]}: {X.pf[c][d[:3]]} / {p[d[:3]]} {s[d[:3]]}"
        # 2
        want = np.zeros(D, dtype=np.uint8)
        want[3:] = (p[:-3] < cr.SYNC_THR) & (p[3:] > p[:-3])
        d = np.flatnonzero(X.cand[c] != want); d = d[d >= skip]
        assert d.size == 0, f"{lab}: X's cand differs from the reference at {d.size} samples, first {d[:5]}"
        # 3
        fl = S.flags[c][:D].astype(bool)
        miss = np.flatnonzero((p < cr.SYNC_THR) & ~fl); miss = miss[miss >= skip]
        assert miss.size == 0, f"{lab}: {miss.size} samples under the threshold are not flagged, first {miss[:5]}: pherr {p[miss[:5]]}"
        d = np.flatnonzero(S.cand[c] != X.cand[c])
        assert d.size == 0, f"{lab}: cand of S and X differ at {d.size} samples, first {d[:5]}"
        need = fl.copy()
        need[3:] |= fl[:-3]; need[:-3] |= fl[3:]
        if whole_feed:
            for e in ends or [D]:                                # the last 3 of every feed
                need[max(0, e - 3):e] = True
        sp, xp = u32(S.pf[c]), u32(X.pf[c])
        d = np.flatnonzero(need & (sp != xp).any(axis=1))
        assert d.size == 0, f"{lab}: pf of S and X differ at {d.size} samples with work, first {d[:5]}: {S.pf[c][d[:3]]} / {X.pf[c][d[:3]]}"
        if whole_feed and not wrapped:
            d = np.flatnonzero(~need & (sp != 0).any(axis=1))
            assert d.size == 0, f"{lab}: S wrote pf at {d.size} samples without work, first {d[:5]}"
        # 4
        pred, stop, dist, v16 = predicted_flags(L, hs, S.y[c], stats)
        free = stop & pred                                   # stopped after 12 taps unless a wavefront-mate went on: either verdict
        bad = (fl != pred) & ~free
        bad[:skip] = False
        if stats["differ"]:
            bad &= dist > stats["far"]
        d = np.flatnonzero(bad)
        assert d.size == 0, (f"{lab}: {d.size} flags are not the screen's (device/host screen arithmetic: {stats['differ']} values differ, by at most {stats['far']:.3e}), "
                             f"first {d[:5]}: flag {fl[d[:5]]} value {v16[d[:5]]}")
        assert not S.flags[c][D:].any(), f"{lab}: bits set past the last sample"
        under4 += int((p[skip:] < 4).sum()); between += int(((p[skip:] >= 4) & (p[skip:] < 5.5)).sum())
        nflag += int(fl.sum()); nsamp += D
    print(f"{label}: {under4} samples under 4, {between} between 4 and 5.5, flagged share {nflag / nsamp:.3e}")
    if populated:
        assert under4 >= 50 and between >= 50, f"{label}: the region around the threshold is not populated: {under4} / {between}"
    return nflag / nsamp


def both(vh, freqs, raw, fmt, **kw):
    return run(vh, freqs, raw, fmt, 0, **kw), run(vh, freqs, raw, fmt, 1, **kw)


@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("k", GRID)
def test_grid(vh, hs, nchan, k):
    """the capture behind k decimated samples of zeros (the filter state stays zero): every preamble crosses the lane boundaries (10 and
    80 samples), the word boundary and the tile boundary"""
    raw = np.concatenate([np.zeros(2 * k * OS, dtype=np.int16), as_s16(capture(nchan))])
    S, X = both(vh, FREQS[nchan], raw, vh.FMT_S16LE)
    stats = {"differ": 0, "windows": 0, "far": 0.0}
    check_pair(vh, hs, S, X, f"grid {k} x{nchan}", stats=stats)
    print(f"grid {k} x{nchan}: device screen bit-identical to the host build on the capture's windows: {'yes' if not stats['differ'] else 'no'} ({stats['differ']} of {stats['windows']})")


@pytest.mark.parametrize("nchan", [1, 3])
def test_stream_start(vh, hs, nchan):
    """a burst whose unique word starts with the stream: windows that reach before it (the edge path, the phase 0 of t < 0)"""
    raw = as_s16(capture(nchan, start_at_zero=True))
    S, X = both(vh, FREQS[nchan], raw, vh.FMT_S16LE)
    check_pair(vh, hs, S, X, f"stream start x{nchan}")


def test_silence(vh, hs):
    """exact zeros: phase 0 everywhere, on both tiers"""
    raw = np.zeros(2 * (3 * TILE * OS + 130), dtype=np.int16)
    S, X = both(vh, FREQS[3], raw, vh.FMT_S16LE)
    check_pair(vh, hs, S, X, "silence", populated=False)
    assert all(not y.any() for y in S.y)
    assert_frames_equal(S.frames, X.frames, label="silence")


def test_noise_only(vh, hs):
    """no signal at all: the share of samples the screen sends to the exact tier (printed; profiles/core_probe_device.txt)"""
    rng = np.random.default_rng(31)
    raw = as_s16((0.02 * (rng.standard_normal(N_IN) + 1j * rng.standard_normal(N_IN))).astype(np.complex64))
    S, X = both(vh, FREQS[3], raw, vh.FMT_S16LE)
    check_pair(vh, hs, S, X, "noise only", populated=False)
    # (without the stream's first 150 samples, whose windows reach before it: taps of phase 0 - silence - are flagged)
    nflag = sum(int(f[HIST:S.ndec].sum()) for f in S.flags)
    share = nflag / (3 * (S.ndec - HIST))
    print(f"noise only: flagged share {share:.3e} ({nflag} of {3 * (S.ndec - HIST)} samples)")
    assert share < 0.01                                            # (a screen that flags everything is sound too - and useless)


def test_subnormal_samples(vh, hs):
    """cf32 input so small that y is subnormal: phase_fast's reciprocal overflows, the screening value is a NaN, and the NaN rule
    sends every such window to the exact tier - whose phases are as exact as ever"""
    raw = (capture(1).astype(np.complex128) * 2.0e-37).astype(np.complex64)
    S, X = both(vh, FREQS[1], raw, vh.FMT_CF32)
    y = np.abs(S.y[0]).max(axis=1)
    tiny = (y > 0) & (y < F32(2.0 ** -126))
    print(f"subnormal: {tiny.sum()} of {len(y)} samples have a subnormal larger component, {S.flags[0].sum()} flagged")
    assert tiny.mean() > 0.5
    L = vh.load_library()
    pfast = cr.device_probe(L, "phase_fast", S.y[0])[:, 0]
    assert (~np.isfinite(pfast)).sum() > 1000, "the case does not reach the NaN rule"
    check_pair(vh, hs, S, X, "subnormal")
    assert len(X.frames) > 0
    # (a frame's power is -inf dBFS here, and -inf minus -inf is no number: the levels are compared as equal values)
    level = lambda fr: [(f["frame_pwr_dbfs"], f["nf_pwr_dbfs"]) for f in sorted(fr, key=lambda f: f["sync_sample"])]
    flat = lambda fr: [dict(f, frame_pwr_dbfs=0.0, nf_pwr_dbfs=0.0) for f in fr]
    assert_frames_equal(flat(S.frames), flat(X.frames), label="subnormal")
    assert repr(level(S.frames)) == repr(level(X.frames))


@pytest.mark.parametrize("nchan", [1, 3])
def test_feed_boundaries_move_nothing(vh, hs, nchan):
    raw = as_s16(capture(nchan))
    pcs = pieces_of(N_IN, 21 + nchan)
    dec = np.cumsum(pcs) // OS
    assert 1 in pcs and any(m < 64 * OS for m in pcs) and any(m % 2 for m in pcs) and any(d % 64 and d % TILE for d in dec[:-1])
    S, X = both(vh, FREQS[nchan], raw, vh.FMT_S16LE, pieces=pcs, max_block=raw.size * 2)
    # the channeliser's own y is not the same bits under another cut of the stream (its block recurrence tiles the feed: 28 844 of
    # the 33 243 samples of the one-channel capture move in the last place, profiles/core_probe_device.txt), so "the same as the whole feed, bit for bit" is not there to be asked of what is computed FROM y.
    # What is asked instead is more: the pieces' own run against the references at every sample (1-4) - every flag predicted from
    # this run's y, X's pf the numpy metric of this run's y, S's pf on exactly the samples with work (the ends of the pieces
    # included) and zero elsewhere - so wherever a feed ends, the tier's outputs are the same function of y
    check_pair(vh, hs, S, X, f"pieces x{nchan}", ends=[int(d) for d in dec])
    assert_frames_equal(S.frames, X.frames, label=f"pieces x{nchan}")


def test_ring_wrap(vh, hs):
    """a ring of a few feeds: the capture goes round it several times; compared over the last block's worth"""
    raw = as_s16(capture(3))
    blk = 20000                                                   # input samples per feed at most: 2 000 decimated
    rng = np.random.default_rng(5)
    pcs, k = [], 0
    while k < N_IN:
        m = min(N_IN - k, int(rng.integers(6000, blk)) | 1); pcs.append(m); k += m
    S, X = both(vh, FREQS[3], raw, vh.FMT_S16LE, pieces=pcs, max_block=blk * 4, tail=blk // OS)
    check_pair(vh, hs, S, X, "ring wrap", whole_feed=False, wrapped=True, populated=False)
    assert_frames_equal(S.frames, X.frames, label="ring wrap")


def test_referee_on_leaves_room_for_the_margins(vh):
    """the library's default (referee on): pf's sign is the referee's mark and a candidate "may fire" includes its margin, so cand of
    S == cand of X says that the screen's 5.5 leaves room for the margins too.  Weak bursts by the dozen: config4 without its ppm
    gate, 8 of its channels (8 kHz apart: idle channels lock on to what leaks over from their neighbours)"""
    from dumpvdl2_amd import workloads, synth
    cfg = workloads.config4(0.3)
    cfg = dataclasses.replace(cfg, freqs=list(cfg.freqs)[:8], rx_max_ppm=0.0)
    iq, _ = synth.synthesize(cfg)
    runs = []
    for screen_all in (0, 1):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, 0.0, max_block_bytes=iq.size * 2)
        rx.debug_option("exact_tier", 1); rx.debug_option("screen_all", screen_all)
        rx.feed(iq)
        fr = rx.drain()
        D = iq.size // 2 // cfg.oversample
        runs.append((fr, [rx.read_sync(c, 0, D)[1] for c in range(8)]))
        rx.close()
    (fs_, cs), (fx, cx) = runs
    ncand = sum(int(c.sum()) for c in cx)
    print(f"referee on: {ncand} candidates, {len(fx)} frames")
    assert ncand >= 50 and len(fx) > 0
    for c in range(8):
        d = np.flatnonzero(cs[c] != cx[c])
        assert d.size == 0, f"referee on: channel {c}: cand differs at {d.size} samples, first {d[:5]}"
    assert_frames_equal(fs_, fx, label="referee on")
