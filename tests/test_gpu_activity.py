"""The activity monitor on the GPU (include/vdl2hip.h, "Activity monitor"; kernels: dumpvdl2_amd/csrc/activity.h): per-channel power
in fixed time bins of the decimated stream, busy / idle decisions, transmissions, a level histogram and a short series.

The model is numpy float64 (tests/activity_model.py).  Powers are held to the header's bound against the receiver's own decimated
stream, read back with read_decimated() and summed in float64:  |p - p_ref| <= (B + 4) 2^-24 p_ref.  Flags are compared exactly, but
only after the model has asserted, on the float64 reference, that no bin lies within 1 dB of the threshold.  The scan is held, exactly,
to the model applied to the device's own float32 series.

The test signal: noise at about -60 dBFS and, per channel, a tone at the channel frequency of about -20 dBFS keyed on and off; the
keying changes in the middle of a 105-sample bin, so the bin of an edge holds half a tone (-23 dBFS) and the next one the noise.  The
threshold is -40 dBFS.  Oversample 10, s16 input, the referee off unless stated.  Every test prints the worst ratio it reaches."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import activity_model as am
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAV = os.path.join(ROOT, "tests", "golden", "vdl2_model_16b_1050kHz.wav")
E_INVAL, E_TOOBIG = -1, -4
THR = -40.0
ACC_KEYS = ("chan_bins", "busy_bins", "transmissions", "longest_bins", "open")      # (the model calls the first one bins)


def mk(k):
    return "bins" if k == "chan_bins" else k


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


# ---------------------------------------------------------------- streams
def plan(nchan, step=50000):
    return [CF + step * (i - nchan // 2) for i in range(nchan)]


def keying(nbins, seed, first=3):
    """[(first busy bin, last busy bin)] of 105-sample bins: lengths 2 .. 40 and one of 70 (it crosses a 64-bin word), gaps of 1, 2
    and 4 idle bins among others"""
    rng = np.random.default_rng(seed)
    gaps = [1, 2, 4, 1, 2, 4, 7, 20, 3]
    out, m, i = [], first, 0
    while True:
        length = 70 if i == 2 else int(rng.integers(2, 41))
        if m + length + 2 >= nbins:
            break
        out.append((m, m + length - 1))
        m += length + gaps[i % len(gaps)]
        i += 1
    return out


@functools.lru_cache(maxsize=8)
def make_stream(nchan, n_in, seed, step=50000, rate=1050000, os_=10):
    """-> (int16 (n_in, 2), freqs, keying per channel).  The tone of channel c is on from the middle of bin s to the middle of bin e
    of every (s, e) of its keying; bins are 105 decimated samples = 105 * rate / 105000 input samples."""
    rng = np.random.default_rng(seed)
    freqs = plan(nchan, step)
    t = np.arange(n_in, dtype=np.float64)
    x = np.sqrt(0.5e-6) * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    per_bin = 105 * rate // 105000
    nbins = n_in // per_bin
    keys = []
    for c, f in enumerate(freqs):
        k = keying(nbins, seed * 100 + c, first=3 + 2 * c)
        keys.append(k)
        gate = np.zeros(n_in)
        for s, e in k:
            gate[s * per_bin + per_bin // 2:e * per_bin + per_bin // 2] = 1.0
        amp = 0.1 * (1.0 + 0.02 * c)                           # about -20 dBFS, a little different per channel
        x += amp * gate * np.exp(2j * np.pi * ((f - CF) / rate) * t + 1j * c)
    iq = np.stack([x.real, x.imag], axis=1)
    return np.clip(np.rint(32768.0 * iq), -32768, 32767).astype("<i2"), freqs, keys


def cut_sizes(n, sizes):
    out, k, i = [], 0, 0
    while k < n:
        d = min(sizes[i % len(sizes)], n - k)
        out.append(d)
        k += d
        i += 1
    return out


def receiver(vh, freqs, referee=0, **kw):
    rx = vh.Receiver(CF, freqs, kw.pop("oversample", 10), vh.FMT_S16LE, **kw)
    rx.debug_option("referee", referee)
    return rx


def feed_and_read(rx, raw, sizes, chans=None, on_feed=None):
    """feed raw in pieces of `sizes` samples; after every feed read the decimated samples it made, of every channel -> y [C][k, 2]"""
    chans = list(range(rx.chan_first, rx.chan_first + rx.chan_count)) if chans is None else chans
    ys = {c: [] for c in chans}
    k = kdec = 0
    for i, d in enumerate(sizes):
        rx.feed(raw[k:k + d])
        k += d
        got = 0
        for c in chans:
            y = rx.read_decimated(c, kdec, 1 << 20)
            ys[c].append(y.copy())
            got = y.shape[0]
        kdec += got
        if on_feed:
            on_feed(i, kdec)
    return {c: np.concatenate(v) if v else np.zeros((0, 2), np.float32) for c, v in ys.items()}, kdec


def series_of(rx, chan, info=None):
    info = info or rx.activity()
    return rx.activity_series(chan, 0, int(info["bins"]))


def worst_ratio(p, ref, B):
    return float(np.max(np.abs(p.astype(np.float64) - ref) / (am.bound(B) * ref))) if ref.size else 0.0


# ---------------------------------------------------------------- 1. power against y
N1 = 262147                                                     # 26 214 decimated samples: no multiple of 64, nor of any B below


@pytest.mark.parametrize("B", [10, 64, 105, 1000, 10500])
@pytest.mark.parametrize("nchan", [1, 9, 17])
def test_power_against_y(vh, nchan, B):
    raw, freqs, _ = make_stream(nchan, N1, 11)
    rx = receiver(vh, freqs)
    rx.activity_enable(B, THR, series_bins=4096)                # (the whole stream's bins stay readable)
    ys, kdec = feed_and_read(rx, raw, cut_sizes(N1, [80000]))
    assert kdec == N1 // 10 and kdec % 64 != 0 and kdec % B != 0
    a = rx.activity()
    assert a["bins"] == kdec // B and a["first_sample"] == 0 and a["bin_samples"] == B
    assert a["threshold_power"] == am.threshold(THR) and a["busy_bins"].shape == (nchan,) and np.all(a["chan_bins"] == kdec // B)
    worst = 0.0
    for c in range(nchan):
        ref = am.bin_powers(ys[c], B)
        p = series_of(rx, c, a)
        assert p.shape == ref.shape
        worst = max(worst, worst_ratio(p, ref, B))
    print(f"nchan={nchan} B={B}: worst |p - p_ref| / bound = {worst:.3f}")
    rx.close()
    assert worst <= 1.0


# ---------------------------------------------------------------- 2. cuts
N2 = 210007


def run_cut(vh, raw, freqs, sizes, B=105, H=0):
    rx = receiver(vh, freqs, max_block_bytes=1 << 20)
    rx.activity_enable(B, THR, H)
    ys, kdec = feed_and_read(rx, raw, sizes)
    a = rx.activity()
    ser = [series_of(rx, c, a) for c in range(len(freqs))]
    rx.close()
    return a, ser, ys, kdec


def test_cuts(vh):
    raw, freqs, keys = make_stream(3, N2, 22, step=200000)
    B = 105
    whole, sw, ys, kdec = run_cut(vh, raw, freqs, [N2])
    again, sa, _, _ = run_cut(vh, raw, freqs, [N2])
    nb = kdec // B
    assert whole["bins"] == nb
    # a cut inside a transmission and one inside a gap of channel 0, feeds shorter than a bin, one input sample
    s, e = keys[0][1]
    gap_bin = e + 1
    assert keys[0][2][0] > gap_bin
    marks = sorted({10 * (B * (s + 1) + 40), 10 * (B * gap_bin + 50)})
    sizes = [1, 300, 7, marks[0] - 308, 1049, 1, marks[1] - marks[0] - 1050]
    sizes += cut_sizes(N2 - sum(sizes), [50000, 333, 20011])
    assert sum(sizes) == N2 and min(sizes) > 0
    ragged, sr, _, kdec2 = run_cut(vh, raw, freqs, sizes)
    assert kdec2 == kdec
    worst = 0.0
    for c in range(3):
        ref = am.bin_powers(ys[c], B)
        am.assert_clear_of_threshold(ref, THR, label=f"channel {c}")
        want = am.scan(ref.astype(np.float32), am.threshold(THR), 0)
        assert want["transmissions"] == len(keys[c])
        for name, a, ser in (("whole", whole, sw), ("ragged", ragged, sr)):
            assert np.array_equal(ser[c] > am.threshold(THR), want["flags"]), (name, c)
            for k in ACC_KEYS:
                assert int(a[k][c]) == want[mk(k)], (name, c, k)
            worst = max(worst, worst_ratio(ser[c], ref, B))
        assert np.all(np.abs(sw[c].astype(np.float64) - sr[c]) <= 2 * am.bound(B) * ref)
        # the same calls, the same bits
        assert np.array_equal(sw[c].view(np.uint32), sa[c].view(np.uint32))
    for k in whole:
        assert np.array_equal(np.asarray(whole[k]), np.asarray(again[k])) or k == "kernel_ms", k
    assert np.array_equal(whole["sum_power"].view(np.uint64), again["sum_power"].view(np.uint64))
    print(f"cuts: worst |p - p_ref| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- 3. the scan, exactly
@pytest.mark.parametrize("H", [0, 1, 3])
def test_scan_exact(vh, H):
    n = 525013                                                  # 500 bins
    raw, freqs, keys = make_stream(3, n, 33, step=200000)
    gaps = {b[0] - a[1] - 1 for a, b in zip(keys[0], keys[0][1:])}
    assert {1, 2, 4} <= gaps and any(e // 64 > s // 64 for s, e in keys[0])
    rx = receiver(vh, freqs, max_block_bytes=4 * 320000)
    rx.activity_enable(105, THR, H)
    per_feed = []
    # 304, 66 and 142 bins in a feed: more than 64, more than 128, several words
    ys, kdec = feed_and_read(rx, raw, cut_sizes(n, [320000, 70000, 150000]), on_feed=lambda i, k: per_feed.append(k))
    bins_per_feed = np.diff([0] + [k // 105 for k in per_feed])
    assert bins_per_feed.max() > 128 and np.any((bins_per_feed > 64) & (bins_per_feed <= 128))
    a = rx.activity()
    E = vh.activity_edges()
    assert np.array_equal(E, am.edges())
    for c in range(3):
        am.assert_clear_of_threshold(am.bin_powers(ys[c], 105), THR, label=f"channel {c}")
        p = series_of(rx, c, a)
        want = am.scan(p, am.threshold(THR), H)
        for k in ACC_KEYS:
            assert int(a[k][c]) == want[mk(k)], (c, k, int(a[k][c]), want[k])
        assert np.array_equal(a["hist"][c], want["hist"]), c
        assert a["max_power"][c] == want["max_power"] and a["min_power"][c] == want["min_power"]
        assert abs(a["sum_power"][c] - want["sum_power"]) <= 1e-12 * want["sum_power"]
        # the keying as the monitor saw it: with H = 0 every keyed stretch is one transmission
        if H == 0:
            assert want["transmissions"] == len(keys[c]) and want["longest_bins"] == max(e - s + 1 for s, e in keys[c])
    # a transmission that crossed a word of 64 bins inside a feed
    first_feed_bins = bins_per_feed[0]
    assert any(s // 64 != e // 64 and e < first_feed_bins for s, e in keys[0])
    rx.close()


# ---------------------------------------------------------------- 4. the ring of y
def test_decimated_ring_wrap(vh):
    """default block size at oversample 10: the decimated ring holds 131 072 samples (vdl2hip_create: 6 feeds of 8 002 + 65 536 +
    1 024, to the next power of two); the stream runs past it and the feed that straddles the wrap is held to the bound"""
    B = 105
    per = 79990
    n = 18 * per
    raw, freqs, _ = make_stream(1, n, 44)
    rx = receiver(vh, freqs)
    rx.activity_enable(B, THR, series_bins=2048)
    ys, kdec = feed_and_read(rx, raw, cut_sizes(n, [per]))
    assert kdec == n // 10 > 131072 + 7999
    straddle = 131072 // 7999                                   # the feed that holds sample 131 072
    assert straddle * 7999 < 131072 < (straddle + 1) * 7999
    a = rx.activity()
    assert a["bins"] == kdec // B and a["series_bins"] == 2048
    ref = am.bin_powers(ys[0], B)
    p = series_of(rx, 0, a)
    lo, hi = straddle * 7999 // B - 1, (straddle + 1) * 7999 // B + 1
    w_all, w_wrap = worst_ratio(p, ref, B), worst_ratio(p[lo:hi], ref[lo:hi], B)
    print(f"ring wrap: worst ratio {w_all:.3f} over the stream, {w_wrap:.3f} over bins {lo}..{hi} of the straddling feed")
    rx.close()
    assert w_all <= 1.0


# ---------------------------------------------------------------- 5. series ring, reset, enabling mid-stream
def test_series_ring_and_reset(vh):
    B = 105
    n = 4 * 80000
    raw, freqs, keys = make_stream(1, n, 55)
    rx = receiver(vh, freqs)
    rx.activity_enable(B, THR)                                  # series_bins 0: the minimum - 8 002 / 105 + 2 bins, to a power of two
    thr = am.threshold(THR)
    # stop in the middle of a transmission: feed up to 20 samples into a bin in its middle
    s, e = next(k for k in keys[0] if k[1] - k[0] >= 6 and k[0] > 80)
    n1 = 10 * (B * (s + 3) + 20)
    sizes = cut_sizes(n1, [80000]) + cut_sizes(n - n1, [80000])
    state = am.new_state()
    seen = {}

    def on_feed(i, kdec):
        if sum(sizes[:i + 1]) == n1:
            before = rx.activity(reset=True)
            seen["before"] = before
            seen["p1"] = rx.activity_series(0, int(before["bins"]) - 100, 100)
    ys, kdec = feed_and_read(rx, raw, sizes, on_feed=on_feed)
    a = rx.activity()
    assert a["series_bins"] == 128 and a["bins"] == kdec // B
    ref = am.bin_powers(ys[0], B)
    am.assert_clear_of_threshold(ref, THR)
    nb1 = int(seen["before"]["bins"])
    assert nb1 == (n1 // 10) // B and seen["before"]["open"][0] == 1
    # the model, applied to the reference rounded to float32 (flags are clear of the threshold, so they are the device's)
    w1 = am.scan(ref[:nb1].astype(np.float32), thr, 0, state)
    for k in ACC_KEYS:
        assert int(seen["before"][k][0]) == w1[mk(k)], k
    w2 = am.scan(ref[nb1:].astype(np.float32), thr, 0, state)   # the open transmission is carried, not counted again
    assert w1["open"] == 1 and w2["transmissions"] == len(keys[0]) - w1["transmissions"]
    for k in ACC_KEYS:
        assert int(a[k][0]) == w2[mk(k)], k
    assert a["chan_bins"][0] == kdec // B - nb1 and int(a["hist"][0].sum()) == w2["bins"]
    assert a["longest_bins"][0] >= e - s + 1                    # the transmission the reset fell into counts with its whole length
    # the series ring: the newest 128 bins are there and right, older ones are refused
    nb = kdec // B
    p = rx.activity_series(0, nb - 128, 128)
    assert p.shape == (128,) and worst_ratio(p, ref[nb - 128:nb], B) <= 1.0
    assert worst_ratio(seen["p1"], ref[nb1 - 100:nb1], B) <= 1.0
    assert rx.activity_series(0, nb, 10).size == 0
    assert rx.activity_series(0, nb - 5, 100).size == 5
    for bad in (0, nb - 129, nb + 1, -1):
        with pytest.raises(vh.Vdl2HipError):
            rx.activity_series(0, bad, 1)
    rx.close()


def test_enable_mid_stream(vh):
    B = 64
    n = 200000
    raw, freqs, _ = make_stream(1, n, 56)
    rx = receiver(vh, freqs)
    rx.feed(raw[:12345])
    rx.activity_enable(B, THR, series_bins=512)
    ys, kdec = feed_and_read(rx, raw[12345:], cut_sizes(n - 12345, [70001]))
    # read_decimated counted from 0: what the first feed made comes first
    a = rx.activity()
    assert a["first_sample"] == 1234 and kdec == n // 10
    ref = am.bin_powers(ys[0][1234:], B)
    assert a["bins"] == ref.size == (kdec - 1234) // B
    w = worst_ratio(series_of(rx, 0, a), ref, B)
    print(f"enabled mid-stream: worst ratio {w:.3f}")
    assert w <= 1.0
    # enabling again starts afresh where the stream stands
    rx.activity_enable(B, THR, series_bins=512)
    a = rx.activity()
    assert a["first_sample"] == kdec and a["bins"] == 0 and a["busy_bins"][0] == 0 and a["hist"].sum() == 0
    rx.close()


# ---------------------------------------------------------------- 6. arguments
def test_arguments(vh):
    raw, freqs, _ = make_stream(3, N2, 22, step=200000)
    rx = receiver(vh, freqs)
    L = rx.L
    info = vh.ActivityInfo(C.sizeof(vh.ActivityInfo))
    one = np.zeros(1, dtype=np.float32)
    chans = np.zeros(3, dtype=vh.ACTIVITY_CHAN_DTYPE)
    # off: nothing to read
    assert L.vdl2hip_activity_read(rx.h, C.byref(info), chans.ctypes.data, 3, 0) == E_INVAL
    assert L.vdl2hip_activity_series(rx.h, 0, 0, one.ctypes.data, 1) == E_INVAL
    rx.activity_enable(105, THR, 2, 256)
    rx.feed(raw[:80000])

    def state():
        a = rx.activity()
        return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in a.items() if k != "kernel_ms"}
    s0 = state()
    good = dict(struct_size=C.sizeof(vh.ActivityCfg), bin_samples=105, hang_bins=0, series_bins=0, threshold_dbfs=THR, reserved=0)
    for bad in (dict(struct_size=20), dict(struct_size=28), dict(bin_samples=9), dict(bin_samples=10501), dict(hang_bins=256),
                dict(series_bins=100), dict(series_bins=(1 << 20) + 1), dict(series_bins=1 << 21), dict(threshold_dbfs=float("nan")), dict(reserved=1)):
        cfg = vh.ActivityCfg(**{**good, **bad})
        assert L.vdl2hip_activity_enable(rx.h, C.byref(cfg)) == E_INVAL, bad
        assert state() == s0, bad
    assert L.vdl2hip_activity_enable(rx.h, None) == E_INVAL and L.vdl2hip_activity_enable(None, C.byref(vh.ActivityCfg(**good))) == E_INVAL
    assert s0["bin_samples"] == 105 and s0["hang_bins"] == 2 and s0["series_bins"] == 256 and s0["bins"] == 8000 // 105
    # capacities and structure sizes of the read
    assert L.vdl2hip_activity_read(rx.h, C.byref(info), chans.ctypes.data, 2, 0) == E_TOOBIG
    assert L.vdl2hip_activity_read(rx.h, C.byref(info), chans.ctypes.data, 3, 0) == 3
    assert L.vdl2hip_activity_read(rx.h, C.byref(info), None, 0, 0) == 0 and info.bins == 8000 // 105
    assert L.vdl2hip_activity_read(rx.h, None, chans.ctypes.data, 3, 0) == 3
    assert L.vdl2hip_activity_read(rx.h, C.byref(vh.ActivityInfo(40)), None, 0, 0) == E_INVAL
    assert L.vdl2hip_activity_series(rx.h, 3, 0, one.ctypes.data, 1) == E_INVAL
    # the extremes that are taken
    for ok in (dict(bin_samples=10, hang_bins=255, series_bins=1 << 20), dict(bin_samples=10500), dict(bin_samples=0, threshold_dbfs=-200.0)):
        cfg = vh.ActivityCfg(**{**good, **ok})
        assert L.vdl2hip_activity_enable(rx.h, C.byref(cfg)) == 0, ok
    assert rx.activity()["bin_samples"] == 105
    rx.activity_disable()
    assert L.vdl2hip_activity_read(rx.h, C.byref(info), chans.ctypes.data, 3, 0) == E_INVAL
    rx.feed(raw[80000:160000])
    rx.sync()
    rx.close()


# ---------------------------------------------------------------- 7. shards and groups
def test_shards_and_group(vh):
    n = 160000
    raw, freqs, _ = make_stream(6, n, 77, step=100000)
    B = 105

    def run(rx):
        rx.activity_enable(B, THR, series_bins=256)
        for k in range(0, n, 80000):
            rx.feed(raw[k:k + 80000])

    full = receiver(vh, freqs)
    run(full)
    af = full.activity()
    nb = int(af["bins"])
    assert nb == (n // 10) // B
    sf = [full.activity_series(c, 0, nb) for c in range(6)]
    yf = [full.read_decimated(c, 0, n // 10) for c in range(6)]
    for c in range(6):
        assert worst_ratio(sf[c], am.bin_powers(yf[c], B), B) <= 1.0
    shard = receiver(vh, freqs, chan_first=2, chan_count=3)
    run(shard)
    a = shard.activity()
    assert a["busy_bins"].shape == (3,) and a["hist"].shape == (3, 64) and a["bins"] == nb
    for c in (2, 3, 4):
        ref = am.bin_powers(yf[c], B)
        p = shard.activity_series(c, 0, nb)
        assert np.all(np.abs(p.astype(np.float64) - sf[c]) <= 2 * am.bound(B) * ref), c
        for k in ACC_KEYS:
            assert a[k][c - 2] == af[k][c], (c, k)
    one = np.zeros(1, dtype=np.float32)
    for c in (0, 1, 5, 6):
        assert shard.L.vdl2hip_activity_series(shard.h, c, 0, one.ctypes.data, 1) == E_INVAL
    shard.close()
    # a group of two virtual shards on one device: vdl2hip_group_ctx(g, k) is the handle of member k's channels
    g = vh.ReceiverGroup(CF, freqs, [0, 0], 10, vh.FMT_S16LE)
    for i in range(g.size()):
        assert g.L.vdl2hip_debug_option(g.member(i), b"referee", 0) == 0
    g.activity_enable(B, THR, series_bins=256)
    for k in range(0, n, 80000):
        g.feed(raw[k:k + 80000])
    g.sync()
    seen = 0
    for i in range(2):
        am_i = g.activity(i)
        cnt = am_i["busy_bins"].size
        assert cnt == 3 and am_i["bins"] == nb
        for j in range(cnt):
            c = seen + j
            p = g.activity_series(c, 0, nb)
            assert np.all(np.abs(p.astype(np.float64) - sf[c]) <= 2 * am.bound(B) * am.bin_powers(yf[c], B)), c
            for k in ACC_KEYS:
                assert am_i[k][j] == af[k][c], (c, k)
        seen += cnt
    assert seen == 6
    g.close()
    full.close()


# ---------------------------------------------------------------- 8. nothing else moves, and the real thing
def all_counters(rx):
    return [list(rx.counters(0).values()), list(rx.avlc_counters(0).values())]


def test_reference_wav(vh, golden_wav):
    B = 105

    def run(monitor, referee):
        rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE)
        rx.debug_option("referee", referee)
        if monitor:
            rx.activity_enable(B, -30.0, 0, series_bins=512)
        frames = []
        for k in range(0, golden_wav.size, 320000):
            rx.feed(golden_wav[k:k + 320000])
            frames += rx.drain()
        nd = rx.stats()["input_samples"] // 10
        y = rx.read_decimated(0, 0, nd)
        a = rx.activity() if monitor else None
        p = rx.activity_series(0, 0, int(a["bins"])) if monitor else None
        out = (frames, all_counters(rx), y.copy(), a, p)
        rx.close()
        return out
    f0, c0, _, _, _ = run(False, 1)
    f1, c1, _, a, p = run(True, 1)
    _, _, y_raw, a_off, p_off = run(True, 0)
    assert len(f0) == 2 and sum(len(c) for c in c0) >= 20
    assert_frames_equal(f0, f1, label="activity monitor on")
    assert c0 == c1
    ref = am.bin_powers(y_raw, B)
    db = 10 * np.log10(ref)
    assert a["bins"] == ref.size == 376
    # the burst as the receiver (and the CPU oracle) place it: sync_sample 11 975, end_sample 25 871 - bins 114 .. 245
    sync, end = min(f["sync_sample"] for f in f1), max(f["end_sample"] for f in f1)
    assert sync // B == 11972 // B == 114 and end // B == 25870 // B == 246
    # Bin 0 is not noise: the file is fed as it is, and its 44 header bytes are eleven samples of up to 0.04 that ring the channel
    # filter (the CPU oracle's stream has the same bin: -38.68 dBFS, 8.68 dB under the threshold).  It is idle, and clear of the
    # threshold by the rule every flag comparison here goes by; the figures below are those of the bins after it, to the 0.1 dB
    # they are stated with (the oracle's stream: noise -56.79 .. -51.02, burst -11.94 .. -9.59, no bin within 18.06 dB).
    am.assert_clear_of_threshold(ref[:1], -30.0, margin_db=1.0, label="reference file, the header's bin")
    assert -39.0 < db[0] < -38.4
    am.assert_clear_of_threshold(ref[1:], -30.0, margin_db=18.0, label="reference file")
    want = am.scan(ref.astype(np.float32), am.threshold(-30.0), 0)
    flags = p > am.threshold(-30.0)
    first = int(np.argmax(flags))
    assert first == 112 and np.all(flags[sync // B:end // B])
    assert not flags[0] and np.array_equal(flags, want["flags"])
    idle = ~flags
    idle[0] = False
    assert np.all((db[flags] >= -12.05) & (db[flags] <= -9.55)) and np.all((db[idle] >= -57.05) & (db[idle] <= -50.95))
    assert a["transmissions"][0] == 1 and a["open"][0] == 0
    assert a["busy_bins"][0] == want["busy_bins"] == a_off["busy_bins"][0]
    # the monitor reads what the channeliser wrote, whether the referee rewrites stretches of it later or not
    assert np.array_equal(p.view(np.uint32), p_off.view(np.uint32))
    w = worst_ratio(p, ref, B)
    print(f"reference file: worst ratio {w:.3f}")
    assert w <= 1.0


# ---------------------------------------------------------------- 9. a receiver that resamples monitors the stream it decodes
def test_resampled_receiver(vh):
    B = 105
    n = 600811                                                  # 0.25 s at 2.4 MS/s: 26 285 decimated samples, give or take the filter's run-in
    raw, freqs, _ = make_stream(1, n, 99, rate=2400000)
    rx = vh.Receiver(CF, freqs, 20, vh.FMT_S16LE, input_rate=2400000)
    rx.debug_option("referee", 0)
    rx.activity_enable(B, THR, series_bins=512)
    ys, kdec = feed_and_read(rx, raw, cut_sizes(n, [80000]))
    assert abs(kdec - n * 105000 // 2400000) <= 4 and kdec % 64 != 0 and kdec % B != 0
    a = rx.activity()
    ref = am.bin_powers(ys[0], B)
    assert a["bins"] == ref.size == kdec // B
    am.assert_clear_of_threshold(ref, THR, label="resampled")
    p = series_of(rx, 0, a)
    w = worst_ratio(p, ref, B)
    print(f"resampled receiver: worst ratio {w:.3f}")
    want = am.scan(ref.astype(np.float32), am.threshold(THR), 0)
    assert np.array_equal(p > am.threshold(THR), want["flags"]) and a["transmissions"][0] == want["transmissions"] > 3
    rx.close()
    assert w <= 1.0


# ---------------------------------------------------------------- 10. the tool
def test_tool(vh, tmp_path):
    from dumpvdl2_amd import build
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    out = str(tmp_path / "activity.txt")
    base = [exe, "--iq-file", WAV, "--sample-format", "S16_LE"]
    p0 = subprocess.run(base, check=True, capture_output=True, text=True, timeout=120)
    p1 = subprocess.run(base + ["--activity-out", out, "--activity-threshold", "-30"], check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stdout.count("[S:") == 2
    assert " busy=" not in p0.stderr and [l.split(" busy=")[0] for l in p1.stderr.splitlines()] == p0.stderr.splitlines()
    lines = open(out).read().splitlines()
    head = dict(l[2:].split(" ", 1) for l in lines if l.startswith("# "))
    rows = [l.split() for l in lines if not l.startswith("#")]
    assert set(head) == {k for k, _ in vh.ActivityInfo._fields_ if k not in ("struct_size", "reserved")}
    assert int(head["bin_samples"]) == 105 and int(head["hang_bins"]) == 0 and float(head["threshold_dbfs"]) == -30.0
    assert int(head["bins"]) == 376 and int(head["first_sample"]) == 0
    assert len(rows) == 1 and len(rows[0]) == 10
    freq, bins, busy, occ, tx, longest_ms, mean_db, max_db, p10, p50 = rows[0]
    assert int(freq) == CF and int(bins) == 376 and int(tx) == 1
    assert abs(float(occ) - int(busy) / int(bins)) < 1e-6 and int(busy) >= 25870 // 105 - 11972 // 105
    assert abs(float(longest_ms) - int(busy)) < 1e-3             # one transmission without a gap, bins of 1 ms
    assert -12.05 <= float(max_db) <= -9.55 and -57.0 <= float(p10) <= -51.0 and -57.0 <= float(p50) <= -51.0
    assert f" busy={100.0 * int(busy) / int(bins):.2f}% tx=1" in p1.stderr
