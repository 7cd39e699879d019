"""The spectrogram on the GPU (include/vdl2hip.h, "Spectrogram"; kernels: dumpvdl2_amd/csrc/spectrum.h, the plan of a feed:
specgram_plan.h): max-hold, floor and time lines on top of the input monitor.

The model is tests/specgram_model.py: numpy float64 by the definition, with the bounds a value is held to (the monitor's per-segment
bound, averaged over a line for line_mean, its maximum over the segments covered for line_max and max_hold, plus one float32
rounding).  Every test that compares against the model prints the worst ratio it reaches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import specgram_model as M
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAV = os.path.join(ROOT, "tests", "golden", "vdl2_model_16b_1050kHz.wav")
E_INVAL, E_TOOBIG = -1, -4
COUNTS = ("lines", "hold_segments", "hold_lines", "first_segment", "first_sample", "line_segments")


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def receiver(vh, fmt, **kw):
    return vh.Receiver(CF, [CF], 10, M.FMTS[fmt], **kw)


def read_all(rx):
    """the holds and every line the tap has completed (the tests keep them inside the ring) -> dict"""
    sg = rx.specgram()
    sg["line_mean"], sg["line_max"] = rx.specgram_lines(0, sg["lines"])
    assert sg["line_mean"].shape == (sg["lines"], sg["nfft"]) == sg["line_max"].shape
    return sg


def feed_cut(rx, raw, pieces):
    """the stream in the given pieces (sample counts; what is left goes last)"""
    k = 0
    for p in list(pieces) + [raw.shape[0]]:
        if k < raw.shape[0] and p > 0:
            rx.feed(raw[k:k + p])
            k += p


def run_cut(vh, fmt, raw, pieces, n, R, window=1, stride=1, **kw):
    rx = receiver(vh, fmt, **kw)
    rx.spectrum_enable(n, window, stride)
    rx.specgram_enable(R)
    feed_cut(rx, raw, pieces)
    sg = read_all(rx)
    sg["spectrum"] = rx.spectrum()
    rx.close()
    return sg


def check_against_model(sg, q, b, R, label, **hold):
    """lines, holds and counts against the definition within the bounds -> the worst ratio"""
    m = M.model(q, b, R, **hold)
    for k in ("lines", "hold_segments", "hold_lines"):
        assert sg[k] == m[k], (label, k, sg[k], m[k])
    assert sg["line_mean"].dtype == np.float32 and sg["max_hold"].dtype == np.float32
    ratios = dict(mean=M.worst_ratio(sg["line_mean"], m["line_mean"], m["mean_bound"]), max=M.worst_ratio(sg["line_max"], m["line_max"], m["max_bound"]),
                  hold=M.worst_ratio(sg["max_hold"], m["max_hold"], m["hold_bound"]), floor=M.worst_ratio(sg["floor_hold"], m["floor_hold"], m["floor_bound"]))
    print(f"specgram bound ratios {label}: " + " ".join(f"{k}={v:.4f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, (label, ratios)
    assert_floor_is_min_of_lines(sg, label, hold.get("hold_from_line", 0))
    return max(ratios.values())


def assert_floor_is_min_of_lines(sg, label="", first=0):
    if sg["line_mean"].shape[0] > first:
        assert np.array_equal(sg["floor_hold"].view(np.uint32), sg["line_mean"][first:].min(axis=0).view(np.uint32)), label
    else:
        assert not sg["floor_hold"].any(), label


def assert_same_stream(a, b, label=""):
    """two cuts of one stream: line_max, max_hold and the counts exactly, line_mean and floor_hold equal or adjacent float32"""
    for k in COUNTS:
        assert a[k] == b[k], (label, k, a[k], b[k])
    assert np.array_equal(a["line_max"].view(np.uint32), b["line_max"].view(np.uint32)), label
    assert np.array_equal(a["max_hold"].view(np.uint32), b["max_hold"].view(np.uint32)), label
    for k in ("line_mean", "floor_hold"):
        # (non-negative floats: adjacent values have adjacent bit patterns)
        assert np.all(np.abs(a[k].view(np.int32).astype(np.int64) - b[k].view(np.int32).astype(np.int64)) <= 1), (label, k)


def assert_same_bytes(a, b, label=""):
    for k in COUNTS:
        assert a[k] == b[k], (label, k)
    for k in ("line_mean", "line_max", "max_hold", "floor_hold"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (label, k)


def assert_monitor_clause(a, b, label=""):
    """the monitor's own determinism clause: counts and the peak exactly, the float64 sums within 1e-12 relative"""
    for k in ("segments", "samples", "clipped", "peak"):
        assert a[k] == b[k], (label, k, a[k], b[k])
    assert np.all(np.abs(a["power"] - b["power"]) <= 1e-12 * np.abs(a["power"])), label
    assert abs(a["mean_power"] - b["mean_power"]) <= 1e-12 * abs(a["mean_power"])
    for k in ("dc_i", "dc_q"):
        assert abs(a[k] - b[k]) <= 1e-12 * max(abs(a[k]), np.sqrt(a["mean_power"])), (label, k)


# ---------------------------------------------------------------- 1. the definition
R3 = 3
DEFINITION_CASES = [("s16", 64), ("cf32", 64), ("u8", 64), ("s16", 1024), ("s16", 4096), ("s8", 64)]


@pytest.mark.parametrize("fmt,n", DEFINITION_CASES)
def test_definition(vh, fmt, n):
    nseg = 7 * R3 + 2                                        # the last line stays incomplete
    raw = M.make_stream(fmt, nseg * n + 37)
    w = vh.spectrum_window(n, 1)
    sg = run_cut(vh, fmt, raw, [], n, R3, max_block_bytes=max(320000, raw.nbytes))
    assert sg["nfft"] == n and sg["window"] == 1 and sg["stride"] == 1 and sg["line_segments"] == R3
    assert sg["sample_rate"] == 1050000 and sg["centerfreq"] == CF and sg["first_segment"] == 0 and sg["first_sample"] == 0
    assert sg["ring_lines"] & (sg["ring_lines"] - 1) == 0 and sg["ring_lines"] >= 8
    assert sg["freq_hz"][n // 2] == CF
    assert sg["lines"] == 7 and sg["hold_segments"] == nseg and sg["hold_lines"] == 7
    q, b = M.segments(M.to_float(raw, fmt), n, w)
    check_against_model(sg, q, b, R3, f"definition {fmt} nfft={n}")


# ---------------------------------------------------------------- 2. how the stream is cut does not matter
@pytest.mark.parametrize("n", [64, 1024])
def test_cuts(vh, n):
    raw = M.make_stream("s16", (7 * R3 + 2) * n + 37)
    pieces = [1, 7, n - 1, n, n + 1, 3 * n]
    kw = dict(max_block_bytes=max(320000, raw.nbytes))
    one = run_cut(vh, "s16", raw, [], n, R3, **kw)
    cut = run_cut(vh, "s16", raw, pieces, n, R3, **kw)
    assert one["lines"] == 7
    assert_same_stream(one, cut, f"cuts nfft {n}")
    assert_floor_is_min_of_lines(cut, "cut")
    assert_monitor_clause(one["spectrum"], cut["spectrum"], f"cuts nfft {n}")
    assert_same_bytes(cut, run_cut(vh, "s16", raw, pieces, n, R3, **kw), "the same calls again")
    assert_same_bytes(one, run_cut(vh, "s16", raw, [], n, R3, **kw), "the same call again")
    if n == 64:
        short = raw[:(2 * R3 + 1) * n + 3]
        a = run_cut(vh, "s16", short, [], n, R3)
        b = run_cut(vh, "s16", short, [1] * short.shape[0], n, R3)
        assert a["lines"] == 2 and a["hold_segments"] == 2 * R3 + 1
        assert_same_stream(a, b, "one sample per feed")
        assert_floor_is_min_of_lines(b, "one sample per feed")


# ---------------------------------------------------------------- 3. stride
def test_stride_3_lines_of_2(vh):
    n, R = 64, 2
    raw = M.make_stream("s16", 13 * n + 5)                   # segments 0, 3, 6, 9, 12 count: lines {0, 3}, {6, 9}, and 12 carried
    w = vh.spectrum_window(n, 1)
    # cuts inside a segment that is skipped (1), inside one that counts (3) and where line 0 ends (the end of segment 3)
    sg = run_cut(vh, "s16", raw, [n + 10, 2 * n + 7, n - 17], n, R, 1, 3)
    assert sg["stride"] == 3 and sg["lines"] == 2 and sg["hold_segments"] == 5
    q, b = M.segments(M.to_float(raw, "s16"), n, w, stride=3)
    check_against_model(sg, q, b, R, "stride 3")
    assert_same_stream(run_cut(vh, "s16", raw, [], n, R, 1, 3), sg, "stride 3 in one block")


# ---------------------------------------------------------------- 4. more lines than workgroups
@pytest.fixture(scope="module")
def long_stream(vh):
    n = 64
    raw = M.make_stream("s16", 1100 * n, seed=4)             # 1100 segments in one feed: 550 workgroups of two segments
    q, b = M.segments(M.to_float(raw, "s16"), n, vh.spectrum_window(n, 1))
    return raw, q, b


@pytest.mark.parametrize("R", [1, 3, 1000])
def test_more_lines_than_workgroups(vh, long_stream, R):
    raw, q, b = long_stream
    n = 64
    assert raw.nbytes <= 320000
    one = run_cut(vh, "s16", raw, [], n, R)
    assert one["lines"] == 1100 // R and one["hold_segments"] == 1100
    check_against_model(one, q, b, R, f"1100 segments, R={R}")
    three = run_cut(vh, "s16", raw, [400 * n + 13, 300 * n + 5], n, R)
    check_against_model(three, q, b, R, f"1100 segments in three feeds, R={R}")
    assert_same_stream(one, three, f"R={R}")
    assert_monitor_clause(one["spectrum"], three["spectrum"], f"R={R}")


# ---------------------------------------------------------------- 5. the point of it
def test_a_burst_the_average_hides(vh):
    n, R, seg, k = 64, 16, 600, 20
    raw = M.to_raw(M.burst_stream(n, 1000, seg, k, 0.03, 0.01), "s16")
    sg = run_cut(vh, "s16", raw, [], n, R)
    i = (k + n // 2) % n
    avg = sg["spectrum"]["power"]
    over_median = 10 * np.log10(avg[i] / np.median(avg))
    hold_db = 10 * np.log10(sg["max_hold"][i] / 0.03 ** 2)
    far = np.abs(np.arange(n) - i) > 2
    over_others = 10 * np.log10(sg["max_hold"][i] / sg["max_hold"][far].max())
    print(f"burst: average {over_median:.2f} dB over the median bin, max_hold {hold_db:.2f} dB from the tone, {over_others:.2f} dB over the other bins")
    assert over_median < 2.0
    assert abs(hold_db) <= 1.0
    assert over_others >= 10.0
    assert sg["lines"] == 62 and int(np.argmax(sg["line_max"][:, i])) == seg // R


# ---------------------------------------------------------------- 6. the ring
def test_ring(vh):
    n, R = 64, 16
    rx = receiver(vh, "s16", max_block_bytes=4 * 4096)       # 4096 samples a feed: 64 segments, 4 lines -> the smallest ring is 8
    rx.spectrum_enable(n)
    rx.specgram_enable(R)
    ring = rx.specgram()["ring_lines"]
    assert ring == 8
    raw = M.make_stream("s16", 19 * 1000, seed=6)
    feed_cut(rx, raw, [1000] * 18)
    sg = rx.specgram()
    lines = sg["lines"]
    assert lines == 19000 // (n * R) and lines > 2 * ring
    q, b = M.segments(M.to_float(raw, "s16"), n, vh.spectrum_window(n, 1))
    m = M.model(q, b, R)
    mean, mx = rx.specgram_lines(lines - ring, ring)
    assert mean.shape == (ring, n)
    r = max(M.worst_ratio(mean, m["line_mean"][lines - ring:], m["mean_bound"][lines - ring:]), M.worst_ratio(mx, m["line_max"][lines - ring:], m["max_bound"][lines - ring:]))
    print(f"specgram bound ratio ring: {r:.4f}")
    assert r <= 1.0
    part, _ = rx.specgram_lines(lines - 3, 100)              # fewer than asked for: what there is
    assert part.shape == (3, n) and np.array_equal(part, mean[-3:])
    buf = np.zeros((ring + 1, n), dtype=np.float32)
    L = rx.L
    assert L.vdl2hip_specgram_lines(rx.h, lines - ring - 1, buf.ctypes.data, None, ring + 1) == E_INVAL
    assert L.vdl2hip_specgram_lines(rx.h, lines + 1, buf.ctypes.data, None, 1) == E_INVAL
    assert L.vdl2hip_specgram_lines(rx.h, -1, buf.ctypes.data, None, 1) == E_INVAL
    assert L.vdl2hip_specgram_lines(rx.h, lines, buf.ctypes.data, None, 1) == 0
    assert L.vdl2hip_specgram_lines(rx.h, lines - 1, None, buf.ctypes.data, 1) == 1 and np.array_equal(buf[0], mx[-1])
    # the holds cover everything, whatever the ring still has
    assert sg["hold_lines"] == lines and sg["hold_segments"] == 19000 // n
    assert M.worst_ratio(sg["max_hold"], m["max_hold"], m["hold_bound"]) <= 1.0 and M.worst_ratio(sg["floor_hold"], m["floor_hold"], m["floor_bound"]) <= 1.0
    rx.close()


# ---------------------------------------------------------------- 7. lifecycle and refusals
def test_refusals(vh):
    n = 64
    rx = receiver(vh, "s16")
    L = rx.L
    good = vh.SpecgramCfg(C.sizeof(vh.SpecgramCfg), 3, 0, 0)
    assert L.vdl2hip_specgram_enable(rx.h, C.byref(good)) == E_INVAL          # the monitor is off
    with pytest.raises(vh.Vdl2HipError):
        rx.specgram()
    rx.spectrum_enable(n)
    with pytest.raises(vh.Vdl2HipError):
        rx.specgram()                                                        # the tap is off
    before = vh.live_resources()
    for bad in (vh.SpecgramCfg(C.sizeof(vh.SpecgramCfg) - 4, 3, 0, 0),        # struct_size
                vh.SpecgramCfg(C.sizeof(vh.SpecgramCfg), 3, 0, 1),            # reserved
                vh.SpecgramCfg(C.sizeof(vh.SpecgramCfg), (1 << 20) + 1, 0, 0),
                vh.SpecgramCfg(C.sizeof(vh.SpecgramCfg), 3, (1 << 25) // n * 2, 0),   # a ring over the limit
                vh.SpecgramCfg(C.sizeof(vh.SpecgramCfg), 3, 24, 0)):          # not a power of two
        assert L.vdl2hip_specgram_enable(rx.h, C.byref(bad)) == E_INVAL
        assert vh.live_resources() == before
    assert L.vdl2hip_specgram_enable(rx.h, C.byref(vh.SpecgramCfg(C.sizeof(vh.SpecgramCfg), 1 << 20, (1 << 25) // n, 0))) == 0      # both limits themselves
    sg = rx.specgram()
    assert sg["line_segments"] == 1 << 20 and sg["ring_lines"] == (1 << 25) // n
    rx.specgram_enable(0, 0)
    sg = rx.specgram()
    assert sg["line_segments"] == 16 and sg["lines"] == 0 and not sg["max_hold"].any() and not sg["floor_hold"].any()
    info = vh.SpecgramInfo(C.sizeof(vh.SpecgramInfo))
    buf = np.zeros(n, dtype=np.float32)
    assert L.vdl2hip_specgram_read(rx.h, C.byref(info), buf.ctypes.data, None, n - 1, 0) == E_TOOBIG
    assert L.vdl2hip_specgram_read(rx.h, C.byref(info), None, buf.ctypes.data, n - 1, 0) == E_TOOBIG
    assert L.vdl2hip_specgram_read(rx.h, C.byref(info), None, None, 0, 0) == n
    assert L.vdl2hip_specgram_read(rx.h, None, buf.ctypes.data, buf.ctypes.data, n, 0) == n
    info.struct_size -= 8
    assert L.vdl2hip_specgram_read(rx.h, C.byref(info), None, None, 0, 0) == E_INVAL
    one = np.zeros(1, dtype=np.float32)
    assert L.vdl2hip_specgram_channels(rx.h, one.ctypes.data, None, 0) == E_TOOBIG
    assert L.vdl2hip_specgram_channels(rx.h, None, None, 0) == 1
    rx.close()


def test_lifecycle(vh):
    n, R = 64, 2
    raw = M.make_stream("s16", 11 * n + 10, seed=7)
    x = M.to_float(raw, "s16")
    w = vh.spectrum_window(n, 1)
    q, b = M.segments(x, n, w)
    start = vh.live_resources()
    rx = receiver(vh, "s16")
    rx.spectrum_enable(n)
    rx.feed(raw[:2 * n + 30])                                # two segments complete, a third half carried
    rx.specgram_enable(R)
    sg = rx.specgram()
    assert sg["first_segment"] == 2 and sg["first_sample"] == 2 * n and sg["lines"] == 0 and sg["hold_segments"] == 0
    rx.feed(raw[2 * n + 30:5 * n + 1])                       # segments 2, 3, 4: line 0 and one carried
    sg = read_all(rx)
    check_against_model(sg, q[2:5], b[2:5], R, "enabled with a segment half carried")
    # reset: the holds and their counts go, the line numbers and the ring stay
    assert rx.specgram(reset=True)["hold_segments"] == 3
    sg = rx.specgram()
    assert sg["hold_segments"] == 0 and sg["hold_lines"] == 0 and sg["lines"] == 1 and not sg["max_hold"].any() and not sg["floor_hold"].any()
    rx.feed(raw[5 * n + 1:9 * n + 3])                        # segments 5 .. 8: lines 1 and 2 (line 1 began before the reset)
    sp = rx.spectrum(reset=True)                             # (the monitor's reset is not the tap's)
    assert sp["segments"] == 9
    sg = read_all(rx)
    assert sg["lines"] == 3 and sg["first_segment"] == 2
    check_against_model(sg, q[2:9], b[2:9], R, "after the reset", hold_from_line=1, hold_from_segment=3)
    # enabling again restarts at the then-current ordinal with zeroed state (ordinals do not restart with the monitor's reset)
    rx.specgram_enable(R)
    sg = rx.specgram()
    assert sg["first_segment"] == 9 and sg["first_sample"] == 9 * n and sg["lines"] == 0 and not sg["max_hold"].any()
    rx.feed(raw[9 * n + 3:])
    sg = read_all(rx)
    check_against_model(sg, q[9:11], b[9:11], R, "enabled again")
    # the monitor's enable switches the tap off, also with nfft 0
    rx.spectrum_enable(n)
    with pytest.raises(vh.Vdl2HipError):
        rx.specgram()
    rx.specgram_enable(R)
    rx.spectrum_disable()
    with pytest.raises(vh.Vdl2HipError):
        rx.specgram()
    with pytest.raises(vh.Vdl2HipError):
        rx.specgram_enable(R)
    # nothing stays behind
    rx.spectrum_enable(n)
    rx.feed(raw[:n])
    rx.specgram_enable(R)
    held = vh.live_resources()["device"]
    rx.specgram_disable()
    own = held - vh.live_resources()["device"]               # the tap's device buffers; it has no page-locked buffer or event of its own
    assert own > 0
    for k in range(20):
        before = vh.live_resources()
        rx.specgram_enable(1 + k % 3)                        # (every other time over a tap that is still on)
        assert vh.live_resources()["device"] == before["device"] + (own if k % 2 == 0 else 0)
        rx.feed(raw[:4 * n + k])                             # (a feed may bring a slot's input buffer into being: counted afresh)
        assert rx.specgram()["hold_segments"] >= 3
        before = vh.live_resources()
        if k % 2:
            rx.specgram_disable()
            assert vh.live_resources() == dict(before, device=before["device"] - own)
    rx.specgram_disable()                                    # (off already: fine)
    rx.specgram_enable(R)                                    # ... and one that is on when the receiver goes
    rx.close()
    assert vh.live_resources() == start


# ---------------------------------------------------------------- 8. it leaves the receiver alone
def all_counters(rx):
    return [list(rx.counters(0).values()), list(rx.avlc_counters(0).values())]


@pytest.fixture(scope="module")
def golden_runs(vh, golden_wav):
    def run(lag, tap):
        rx = receiver(vh, "s16")
        rx.set_drain_lag(lag)
        rx.spectrum_enable(1024)
        if tap:
            rx.specgram_enable(16, 32)                       # (24 lines: the ring keeps the whole file)
        frames = []
        for k in range(0, golden_wav.size, 320000):
            rx.feed(golden_wav[k:k + 320000])
            frames += rx.drain()
        rx.set_drain_lag(0)
        frames += rx.drain()
        nd = rx.stats()["input_samples"] // 10
        y = rx.read_decimated(0, nd - 2000, 2000)
        out = dict(frames=frames, counters=all_counters(rx), y=y.copy(), spectrum=rx.spectrum(), specgram=read_all(rx) if tap else None)
        rx.close()
        return out
    return {(lag, tap): run(lag, tap) for lag in (0, 2) for tap in (False, True)}


@pytest.mark.parametrize("lag", [0, 2])
def test_leaves_the_receiver_alone(vh, golden_wav, golden_runs, lag):
    off, on = golden_runs[(lag, False)], golden_runs[(lag, True)]
    assert len(off["frames"]) == 2 and sorted(len(f["octets"]) for f in off["frames"]) == [186, 314]
    assert_frames_equal(off["frames"], on["frames"], label=f"specgram on, lag {lag}")
    assert off["counters"] == on["counters"]
    assert off["y"].shape == (2000, 2) and np.array_equal(off["y"].view(np.uint32), on["y"].view(np.uint32))
    assert_monitor_clause(off["spectrum"], on["spectrum"], f"lag {lag}")
    sg = on["specgram"]
    nseg = golden_wav.size // 4 // 1024
    assert sg["lines"] == nseg // 16 and sg["hold_segments"] == nseg
    assert_floor_is_min_of_lines(sg, f"lag {lag}")
    assert_same_bytes(sg, golden_runs[(2 - lag, True)]["specgram"], "the drain lag does not matter")


def test_resampling_receiver_and_other_feed_paths(vh, golden_wav, golden_runs):
    import torch
    n, R = 1024, 16
    # a receiver that resamples: the tap sees what was fed, as its monitor does
    rng = np.random.default_rng(8)
    raw = np.clip(np.rint(3000 * rng.standard_normal((40000, 2))), -32768, 32767).astype("<i2")
    q, b = M.segments(M.to_float(raw, "s16"), n, vh.spectrum_window(n, 1))
    res = []
    for kw in (dict(input_rate=1000000), dict()):
        rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, **kw)
        rx.spectrum_enable(n)
        rx.specgram_enable(R)
        rx.feed(raw[:12345])
        rx.feed(raw[12345:])
        res.append(read_all(rx))
        rx.close()
    assert res[0]["sample_rate"] == 1000000 and res[1]["sample_rate"] == 1050000
    check_against_model(res[0], q, b, R, "resampling receiver")
    assert_same_bytes(res[0], res[1], "resampling receiver against a plain one")
    # the other ways in: the same lines as vdl2hip_feed
    nbytes = 1 << 20
    blk = golden_wav[:nbytes].copy()
    out, keep = [], []
    for how in ("feed", "device", "pinned"):
        rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=nbytes)
        rx.spectrum_enable(n)
        rx.specgram_enable(R)
        if how == "feed":
            rx.feed(blk)
        elif how == "device":
            t = torch.from_numpy(blk).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(t)
            rx.feed_tensor(t)
        else:
            t = torch.from_numpy(blk).pin_memory()
            keep.append(t)
            rx.feed_pinned_tensor(t)
        out.append(read_all(rx))
        rx.drain()
        rx.close()
    assert out[0]["lines"] == nbytes // 4 // n // R == 16
    for sg, how in zip(out[1:], ("device", "pinned")):
        assert_same_bytes(out[0], sg, how)
    # ... and they are the first lines of the same file fed in blocks of 320 000 bytes, up to the order of the additions
    whole = golden_runs[(0, True)]["specgram"]
    assert np.array_equal(out[0]["line_max"], whole["line_max"][:16])


# ---------------------------------------------------------------- 9. channels
def test_channels(vh):
    n, R = 1024, 2
    rng = np.random.default_rng(9)
    t = np.arange(8 * n + 3, dtype=np.float64)
    x = 0.1 * np.exp(2j * np.pi * 25000.0 / 1050000.0 * t) * (t >= 5 * n) * (t < 6 * n)
    x += 1e-3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    raw = M.to_raw(x, "cf32")
    freqs = [CF - 25000, CF, CF + 25000, CF + 524900]
    rx = vh.Receiver(CF, freqs, 10, vh.FMT_CF32)
    rx.spectrum_enable(n, vh.WIN_BH4)
    rx.specgram_enable(R)
    peak, floor = rx.specgram_channels()
    assert peak.shape == (4,) and np.all(np.isneginf(peak)) and np.all(np.isneginf(floor))     # nothing seen yet
    rx.feed(raw)
    peak, floor = rx.specgram_channels()
    sg, sp = rx.specgram(), rx.spectrum()
    rx.close()
    print("specgram channels: peak", peak, "floor", floor)
    want_peak, want_floor = M.channel_rule(sg["max_hold"], sg["floor_hold"], sg["freq_hz"], sp["enbw_bins"], freqs)
    assert np.all(np.abs(peak - want_peak) <= 1e-4) and np.all(np.abs(floor - want_floor) <= 1e-4)
    # one segment of tone, at its level as the strongest BIN shows it: 25 kHz is 24.38 bins from the centre, 0.38 bins off a bin
    # centre, where the 4-term Blackman-Harris window reads 0.48 dB low (0.83 dB half way between two bins, its worst)
    assert -20.0 - 0.83 - 0.05 <= peak[2] <= -20.0 + 0.05 and peak[0] < -40.0 and peak[1] < -40.0
    assert np.all(floor < -40.0)                                                  # ... and no floor lifted by it
    # a shard reports every channel of the list, not only its own
    rx = vh.Receiver(CF, freqs, 10, vh.FMT_CF32, chan_first=1, chan_count=1)
    rx.spectrum_enable(n, vh.WIN_BH4)
    rx.specgram_enable(R)
    rx.feed(raw)
    p2, f2 = rx.specgram_channels()
    rx.close()
    assert np.array_equal(p2, peak) and np.array_equal(f2, floor)


# ---------------------------------------------------------------- 10. the tool
def test_tool(vh, golden_wav, tmp_path):
    from dumpvdl2_amd import build
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    out, mx_path, mean_path = str(tmp_path / "waterfall.txt"), str(tmp_path / "max.f32"), str(tmp_path / "mean.f32")
    base = [exe, "--iq-file", WAV, "--sample-format", "S16_LE"]
    p0 = subprocess.run(base, check=True, capture_output=True, text=True, timeout=120)
    p1 = subprocess.run(base + ["--waterfall-out", out, "--waterfall-max", mx_path, "--waterfall-mean", mean_path, "--waterfall-segments", "8"],
                        check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stdout.count("[S:") == 2
    assert " peak=" not in p0.stderr
    assert [l.split(" peak=")[0] for l in p1.stderr.splitlines()] == p0.stderr.splitlines()
    # the binding on the same file, cut as the tool cuts it (8 blocks of 320 000 bytes per feed at this format and rate)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=8 * 320000)
    rx.spectrum_enable(1024)
    rx.specgram_enable(8)
    for k in range(0, golden_wav.size, 8 * 320000):
        rx.feed(golden_wav[k:k + 8 * 320000])
    sg = rx.specgram()
    lines = sg["lines"]
    got_mean, got_max = rx.specgram_lines(0, lines)          # (the file is one feed of that size: the ring holds all its lines)
    peak, floor = rx.specgram_channels()
    rx.close()
    text = open(out).read().splitlines()
    head = dict(l[2:].split(" ", 1) for l in text if l.startswith("# "))
    bins = np.array([[float(v) for v in l.split()] for l in text if not l.startswith("#")])
    assert set(head) == {k for k, _ in vh.SpecgramInfo._fields_ if k != "struct_size"}
    for k in head:
        assert int(head[k]) == sg[k], k
    assert bins.shape == (1024, 3)
    with np.errstate(divide="ignore"):
        assert np.all(np.abs(bins[:, 0] - sg["freq_hz"]) <= 0.00051)
        assert np.all(np.abs(bins[:, 1] - 10 * np.log10(sg["max_hold"].astype(np.float64))) <= 0.000051)
        assert np.all(np.abs(bins[:, 2] - 10 * np.log10(sg["floor_hold"].astype(np.float64))) <= 0.000051)
    assert f" peak={peak[0]:.2f} dBFS floor={floor[0]:.2f} dBFS" in p1.stderr
    file_max, file_mean = np.fromfile(mx_path, dtype=np.float32), np.fromfile(mean_path, dtype=np.float32)
    assert file_max.size == lines * 1024 == file_mean.size and lines > 0
    assert lines == golden_wav.size // 4 // 1024 // 8 and got_max.shape == (lines, 1024)
    file_max, file_mean = file_max.reshape(lines, 1024), file_mean.reshape(lines, 1024)
    assert np.array_equal(file_max.view(np.uint32), got_max.view(np.uint32)) and np.array_equal(file_mean.view(np.uint32), got_mean.view(np.uint32))
    assert np.array_equal(file_max.max(axis=0), sg["max_hold"]) and np.array_equal(file_mean.min(axis=0).view(np.uint32), sg["floor_hold"].view(np.uint32))
