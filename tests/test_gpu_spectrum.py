"""The input monitor on the GPU (include/vdl2hip.h, "Input monitor"; kernels: dumpvdl2_amd/csrc/spectrum.h): a Welch-averaged
windowed-FFT power spectrum and level statistics of the stream as fed.

The model is numpy float64 in this file: the format conversion in numpy float32 arithmetic (what the header defines), the library's
own window, np.fft.fft.  The bound a bin is held to is measured against that float64 definition, never against the kernel: with
eps = log2(N) 2^-24, per segment  2 eps |X[k]| ||X||_2 + eps^2 ||X||_2^2 + 4 2^-24 |X[k]|^2,  over (sum w)^2, averaged over the
segments - a float32 transform's error is eps ||X||_2 per bin at the worst, and |X|^2 itself is rounded a few times.  A plain float32
radix-2 Stockham FFT uses at most 0.18 of it on one segment and 0.03 averaged over six; a lost bit of twiddle accuracy shows as ten
times the bound.  Every test prints the worst ratio it reaches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAV = os.path.join(ROOT, "tests", "golden", "vdl2_model_16b_1050kHz.wav")
FMTS = {"u8": 0, "s16": 1, "cf32": 2}
LEVEL_KEYS = ("segments", "samples", "clipped", "peak")


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


# ---------------------------------------------------------------- streams and the model (numpy)
def make_stream(fmt, n, seed=1):
    """noise, a strong off-bin tone and a tone 80 dB under it -> the stream in the caller's format (u8 / int16 pairs, complex64)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.5 * np.exp(2j * np.pi * 0.12345 * t) + 0.5e-4 * np.exp(-2j * np.pi * 0.31 * t)
    x += 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack([x.real, x.imag], axis=1)
    if fmt == "u8":
        return np.clip(np.rint(127.5 + 127.5 * iq), 0, 255).astype(np.uint8)
    if fmt == "s16":
        return np.clip(np.rint(32768.0 * iq), -32768, 32767).astype("<i2")
    return iq.astype(np.float32)


def to_float(raw, fmt):
    """x[i] as the header defines it, computed in float32 -> complex128"""
    if fmt == "u8":
        v = (raw.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    elif fmt == "s16":
        v = raw.astype(np.float32) / np.float32(32768.0)
    else:
        v = raw.astype(np.float32)
    assert v.dtype == np.float32
    v = v.astype(np.float64).reshape(-1, 2)
    return v[:, 0] + 1j * v[:, 1]


def model(x, n, w, stride=1, first=0):
    """(power, bound, levels) of the stream x by the definition: segments first, first + stride, ... of n samples"""
    nseg = x.size // n
    segs = x[:nseg * n].reshape(nseg, n)[first::stride]
    wd = w.astype(np.float64)
    X = np.fft.fft(segs * wd, axis=1)
    sw2 = wd.sum() ** 2
    mag = np.abs(X)
    nrm = np.sqrt((mag ** 2).sum(axis=1, keepdims=True))
    eps = np.log2(n) * 2.0 ** -24
    bound = (2 * eps * mag * nrm + eps ** 2 * nrm ** 2 + 4 * 2.0 ** -24 * mag ** 2).mean(axis=0) / sw2
    power = (mag ** 2).mean(axis=0) / sw2
    flat = segs.reshape(-1)
    levels = dict(segments=segs.shape[0], samples=flat.size, mean_power=float(np.mean(np.abs(flat) ** 2)), dc_i=float(flat.real.mean()),
                  dc_q=float(flat.imag.mean()), peak=float(np.float32(max(np.abs(flat.real).max(), np.abs(flat.imag).max()))),
                  mean_abs=float(np.mean(np.abs(flat))))
    return np.fft.fftshift(power), np.fft.fftshift(bound), levels


def check_against_model(got, x, n, w, stride=1, first=0, label=""):
    power, bound, lv = model(x, n, w, stride, first)
    assert got["segments"] == lv["segments"] and got["samples"] == lv["samples"], (label, got["segments"], lv["segments"])
    ratio = float(np.max(np.abs(got["power"] - power) / bound))
    print(f"spectrum bound ratio {label} nfft={n}: {ratio:.4f}")
    assert ratio <= 1.0, (label, ratio)
    assert got["peak"] == lv["peak"], (label, got["peak"], lv["peak"])
    assert abs(got["mean_power"] - lv["mean_power"]) <= 1e-6 * lv["mean_power"]
    assert abs(got["dc_i"] - lv["dc_i"]) <= 1e-9 * lv["mean_abs"] and abs(got["dc_q"] - lv["dc_q"]) <= 1e-9 * lv["mean_abs"]
    return ratio


def receiver(vh, fmt, **kw):
    return vh.Receiver(CF, [CF], 10, FMTS[fmt], **kw)


def run_cut(vh, fmt, raw, pieces, n, window=1, stride=1):
    """the stream fed in the given pieces (sample counts; what is left goes last) -> spectrum dict"""
    rx = receiver(vh, fmt)
    rx.spectrum_enable(n, window, stride)
    k = 0
    for p in list(pieces) + [raw.shape[0]]:
        if k < raw.shape[0] and p > 0:
            rx.feed(raw[k:k + p])
            k += p
    sp = rx.spectrum()
    rx.close()
    return sp


def assert_same_bits(a, b, label=""):
    for k in LEVEL_KEYS + ("mean_power", "dc_i", "dc_q"):
        assert a[k] == b[k], (label, k, a[k], b[k])
    assert np.array_equal(a["power"], b["power"]), label


def assert_same_stream(a, b, label=""):
    """two cuts of one stream: counts and the peak exactly, the float64 sums within 1e-12 relative"""
    for k in LEVEL_KEYS:
        assert a[k] == b[k], (label, k, a[k], b[k])
    assert np.all(np.abs(a["power"] - b["power"]) <= 1e-12 * np.abs(a["power"])), label
    assert abs(a["mean_power"] - b["mean_power"]) <= 1e-12 * abs(a["mean_power"])
    for k in ("dc_i", "dc_q"):
        # (a mean of signed values: relative to the mean magnitude of what was summed)
        assert abs(a[k] - b[k]) <= 1e-12 * max(abs(a[k]), np.sqrt(a["mean_power"])), (label, k)


# ---------------------------------------------------------------- 1. the definition
DEFINITION_CASES = [(f, n, 1) for f in ("u8", "s16", "cf32") for n in (64, 1024, 4096)] + [("s16", 1024, 0), ("s16", 1024, 2)]


@pytest.mark.parametrize("fmt,n,window", DEFINITION_CASES)
def test_definition(vh, fmt, n, window):
    raw = make_stream(fmt, 6 * n + 37)
    w = vh.spectrum_window(n, window)
    sp = run_cut(vh, fmt, raw, [], n, window)
    assert sp["segments"] == 6 and sp["samples"] == 6 * n
    assert sp["nfft"] == n and sp["window"] == window and sp["stride"] == 1
    assert sp["sample_rate"] == 1050000 and sp["centerfreq"] == CF
    wd = w.astype(np.float64)
    assert abs(sp["enbw_bins"] - n * (wd ** 2).sum() / wd.sum() ** 2) < 1e-12
    assert sp["freq_hz"][n // 2] == CF and abs(sp["freq_hz"][0] - (CF - 525000)) < 1e-6
    check_against_model(sp, to_float(raw, fmt), n, w, label=f"definition {fmt} window {window}")


# ---------------------------------------------------------------- 2. how the stream is cut does not matter
@pytest.mark.parametrize("n", [64, 1024])
def test_cuts(vh, n):
    raw = make_stream("s16", 6 * n + 37)
    one = run_cut(vh, "s16", raw, [], n)
    cut = run_cut(vh, "s16", raw, [1, 7, n - 1, n, n + 1], n)
    assert_same_stream(one, cut, f"cuts nfft {n}")
    assert_same_bits(cut, run_cut(vh, "s16", raw, [1, 7, n - 1, n, n + 1], n), "the same calls again")
    assert_same_bits(one, run_cut(vh, "s16", raw, [], n), "the same call again")
    if n == 64:
        short = raw[:2 * n + 3]
        a = run_cut(vh, "s16", short, [], n)
        b = run_cut(vh, "s16", short, [1] * (2 * n + 3), n)
        assert a["segments"] == 2
        assert_same_stream(a, b, "one sample per feed")


# ---------------------------------------------------------------- 3. stride
def test_stride_3(vh):
    n = 64
    raw = make_stream("s16", 7 * n + 5)                      # segments 0 .. 6 are complete: 0, 3 and 6 count
    w = vh.spectrum_window(n, 1)
    # cuts inside a segment that is skipped (1), inside one that counts (3) and inside the last one that counts (6)
    sp = run_cut(vh, "s16", raw, [n + 10, 2 * n + 7, 3 * n + 3], n, 1, 3)
    assert sp["segments"] == 3 and sp["stride"] == 3
    check_against_model(sp, to_float(raw, "s16"), n, w, stride=3, label="stride 3")
    assert_same_stream(run_cut(vh, "s16", raw, [], n, 1, 3), sp, "stride 3 in one block")


# ---------------------------------------------------------------- 4. a tone: scale and orientation
def test_tone_and_orientation(vh):
    n = 1024
    t = np.arange(4 * n, dtype=np.float64)
    x = 0.5 * np.exp(2j * np.pi * 5 * t / n)                 # 5 bins ABOVE the centre
    raw = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    w = vh.spectrum_window(n, 1)
    sp = run_cut(vh, "cf32", raw, [], n)
    power, bound, _ = model(to_float(raw, "cf32"), n, w)
    i = n // 2 + 5
    assert abs(sp["power"][i] - 0.25) <= bound[i]
    for j in (i - 1, i + 1):
        assert abs(sp["power"][j] - 0.0625) <= bound[j]
    assert sp["power"][n // 2 - 5] < 1e-10
    assert sp["freq_hz"][i] == CF + 5 * 1050000 / n
    check_against_model(sp, to_float(raw, "cf32"), n, w, label="tone")


# ---------------------------------------------------------------- 5. levels
def test_levels(vh):
    n = 256
    rng = np.random.default_rng(5)
    total = 8 * n + 11
    inside = 16 + rng.choice(8 * n - 16, 23, replace=False)  # samples of the analysed part that sit at a rail
    # s16
    raw = rng.integers(-20000, 20000, size=(total, 2)).astype("<i2")
    raw[:, 0] += 300
    raw[:, 1] -= 150
    raw[inside[:10], 0] = -32768
    raw[inside[10:18], 1] = 32767
    raw[inside[18:], 0] = 32767
    raw[inside[18:], 1] = -32768
    raw[8 * n + 3, 0] = -32768                               # behind the last complete segment: not counted
    raw[5, 0] = -32767                                       # one short of the rail
    sp = run_cut(vh, "s16", raw, [3 * n + 5], n)
    assert sp["clipped"] == 23 and sp["peak"] == 1.0
    check_against_model(sp, to_float(raw, "s16"), n, vh.spectrum_window(n, 1), label="levels s16")
    # u8
    raw = rng.integers(40, 200, size=(total, 2)).astype(np.uint8)
    raw[inside[:12], 0] = 0
    raw[inside[12:], 1] = 255
    raw[8 * n + 3, 1] = 255
    raw[7, 0] = 1
    raw[8, 1] = 254
    sp = run_cut(vh, "u8", raw, [n - 1], n)
    assert sp["clipped"] == 23 and sp["peak"] == 1.0
    check_against_model(sp, to_float(raw, "u8"), n, vh.spectrum_window(n, 1), label="levels u8")
    # cf32: at or beyond full scale
    raw = (0.3 * rng.standard_normal((total, 2)) + np.array([0.02, -0.01])).astype(np.float32)
    raw = np.clip(raw, -0.99, 0.99)
    raw[inside[:8], 0] = 1.0
    raw[inside[8:16], 1] = -1.0
    raw[inside[16:22], 0] = 1.25
    raw[inside[22], 1] = -3.5
    raw[8 * n + 3, 0] = 7.0
    raw[9, 0] = np.float32(1.0) - np.float32(2.0 ** -24)
    sp = run_cut(vh, "cf32", raw, [n + 1], n)
    assert sp["clipped"] == 23 and sp["peak"] == 3.5
    check_against_model(sp, to_float(raw, "cf32"), n, vh.spectrum_window(n, 1), label="levels cf32")
    # a NaN is not at the rail (and is no peak)
    raw[11, 0] = np.nan
    sp = run_cut(vh, "cf32", raw, [], n)
    assert sp["clipped"] == 23 and sp["peak"] == 3.5


# ---------------------------------------------------------------- 6. lifecycle
def test_lifecycle(vh):
    n = 64
    raw = make_stream("s16", 5 * n + 10)
    x = to_float(raw, "s16")
    w = vh.spectrum_window(n, 1)
    rx = receiver(vh, "s16")
    with pytest.raises(vh.Vdl2HipError):
        rx.spectrum()                                        # never enabled
    rx.spectrum_enable(n)
    sp = rx.spectrum()
    assert sp["segments"] == 0 and sp["samples"] == 0 and not sp["power"].any() and sp["mean_power"] == 0 and sp["peak"] == 0
    rx.feed(raw[:40])
    sp = rx.spectrum()
    assert sp["segments"] == 0 and not sp["power"].any() and sp["clipped"] == 0
    rx.feed(raw[40:3 * n + 10])
    sp = rx.spectrum(reset=True)
    check_against_model(sp, x[:3 * n], n, w, label="before the reset")
    sp = rx.spectrum()
    assert sp["segments"] == 0 and not sp["power"].any() and sp["mean_power"] == 0 and sp["peak"] == 0
    rx.feed(raw[3 * n + 10:])                                # segments 3 and 4 of the stream: still aligned to the original i
    sp = rx.spectrum()
    assert sp["segments"] == 2
    check_against_model(sp, x[3 * n:5 * n], n, w, label="after the reset")
    assert rx.spectrum(power=False)["segments"] == 2 and "power" not in rx.spectrum(power=False)
    # cap < nfft, bad struct_size
    info = vh.SpectrumInfo(C.sizeof(vh.SpectrumInfo))
    buf = np.zeros(n, dtype=np.float64)
    assert rx.L.vdl2hip_spectrum_read(rx.h, C.byref(info), buf.ctypes.data, n - 1, 0) == -4
    assert rx.L.vdl2hip_spectrum_read(rx.h, C.byref(info), buf.ctypes.data, n, 0) == n
    bad = vh.SpectrumCfg(C.sizeof(vh.SpectrumCfg) - 4, 128, 1, 1)
    assert rx.L.vdl2hip_spectrum_enable(rx.h, C.byref(bad)) == -1
    for nfft, window in ((96, 1), (8192, 1), (128, 3)):
        cfg = vh.SpectrumCfg(C.sizeof(vh.SpectrumCfg), nfft, window, 1)
        assert rx.L.vdl2hip_spectrum_enable(rx.h, C.byref(cfg)) == -1
    assert rx.spectrum()["segments"] == 2                    # a refused call changed nothing
    rx.spectrum_disable()
    with pytest.raises(vh.Vdl2HipError):
        rx.spectrum()
    with pytest.raises(vh.Vdl2HipError):
        rx.channel_levels()
    rx.feed(raw[:17])                                        # unseen
    rx.spectrum_enable(128, vh.WIN_BH4)
    rx.feed(raw[100:100 + 128 + 5])                          # i restarts at 0 with the first sample fed after the call
    sp = rx.spectrum()
    assert sp["nfft"] == 128 and sp["segments"] == 1
    check_against_model(sp, x[100:100 + 128], 128, vh.spectrum_window(128, vh.WIN_BH4), label="enabled again")
    rx.close()


# ---------------------------------------------------------------- 7. the receiver does not notice
def all_counters(rx):
    return [list(rx.counters(0).values()), list(rx.avlc_counters(0).values())]


@pytest.mark.parametrize("lag", [0, 2])
def test_leaves_the_receiver_alone(vh, golden_wav, lag):
    def run(monitor):
        rx = receiver(vh, "s16")
        rx.set_drain_lag(lag)
        if monitor:
            rx.spectrum_enable(1024)
        frames, seen = [], []
        for k in range(0, golden_wav.size, 320000):
            rx.feed(golden_wav[k:k + 320000])
            if monitor:
                seen.append(rx.spectrum()["segments"])
            frames += rx.drain()
        rx.set_drain_lag(0)
        frames += rx.drain()
        nd = rx.stats()["input_samples"] // 10
        y = rx.read_decimated(0, nd - 2000, 2000)
        out = (frames, all_counters(rx), y.copy(), seen, rx.spectrum() if monitor else None)
        rx.close()
        return out
    f0, c0, y0, _, _ = run(False)
    f1, c1, y1, seen, sp = run(True)
    assert len(f0) == 2 and sorted(len(f["octets"]) for f in f0) == [186, 314]
    assert_frames_equal(f0, f1, label=f"monitor on, lag {lag}")
    assert c0 == c1
    assert y0.shape == (2000, 2) and np.array_equal(y0.view(np.uint32), y1.view(np.uint32))
    nsamp = (golden_wav.size // 4)
    assert seen == [min((k + 320000) // 4, nsamp) // 1024 for k in range(0, golden_wav.size, 320000)]
    assert sp["segments"] == nsamp // 1024


# ---------------------------------------------------------------- 8. a receiver that resamples: the monitor sees what was fed
def test_resampling_receiver(vh):
    n = 1024
    rng = np.random.default_rng(8)
    raw = np.clip(np.rint(3000 * rng.standard_normal((30000, 2))), -32768, 32767).astype("<i2")
    out = []
    for monitor in (False, True):
        rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, input_rate=1000000)
        if monitor:
            rx.spectrum_enable(n)
        rx.feed(raw[:12345])
        rx.feed(raw[12345:])
        rx.sync()
        nout = rx.stats()["resampled_samples"]
        out.append(rx.read_resampled(nout - 20000, 20000).copy())
        if monitor:
            sp = rx.spectrum()
            assert sp["sample_rate"] == 1000000
            assert abs(sp["freq_hz"][0] - (CF - 500000)) < 1e-6
            check_against_model(sp, to_float(raw, "s16"), n, vh.spectrum_window(n, 1), label="resampling receiver")
        rx.close()
    assert out[0].shape == (20000, 2) and np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


# ---------------------------------------------------------------- 9. the other ways in
def test_other_feed_paths(vh, golden_wav):
    import torch
    nbytes = 8 << 20
    blk = np.tile(golden_wav[:golden_wav.size & ~3], 6)[:nbytes].copy()
    res = []
    keep = []
    for how in ("feed", "device", "pinned"):
        rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=nbytes)
        rx.spectrum_enable(1024)
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
            rx.feed_pinned_tensor(t)                         # 8 MiB, page-locked, idle receiver: the cold-start path's conditions
        sp = rx.spectrum()
        fr = rx.drain()
        # with the monitor on a block is not copied in pieces, whichever way it comes
        assert rx.stats()["cold_start_feeds"] == 0, how
        res.append((sp, fr))
        rx.close()
    # ... and the pinned block above does meet the cold-start path's conditions: with the monitor off it goes in pieces
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=nbytes)
    rx.feed_pinned_tensor(keep[-1])
    fr = rx.drain()
    assert rx.stats()["cold_start_feeds"] == 1
    assert_frames_equal(res[0][1], fr, label="pinned, monitor off")
    rx.close()
    assert res[0][0]["segments"] == nbytes // 4 // 1024 and len(res[0][1]) >= 8
    for (sp, fr), how in zip(res[1:], ("device", "pinned")):
        assert_same_bits(res[0][0], sp, how)
        assert_frames_equal(res[0][1], fr, label=how)


# ---------------------------------------------------------------- 10. channel levels
def channel_rule(sp, freqs):
    out = []
    for f in freqs:
        d = np.abs(sp["freq_hz"] - f)
        sel = d <= 12500.0
        s = sp["power"][sel].sum() if sel.any() else sp["power"][np.argmin(d)]
        out.append(10 * np.log10(s / sp["enbw_bins"]) if s > 0 else -np.inf)
    return np.array(out)


def test_channel_levels(vh):
    n = 1024
    t = np.arange(8 * n, dtype=np.float64)
    x = 0.1 * np.exp(2j * np.pi * 25000.0 / 1050000.0 * t)
    raw = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    freqs = [CF - 25000, CF, CF + 25000]
    rx = vh.Receiver(CF, freqs, 10, vh.FMT_CF32)
    rx.spectrum_enable(n, vh.WIN_BH4)
    rx.feed(raw)
    lv = rx.channel_levels()
    sp = rx.spectrum()
    rx.close()
    print("channel levels:", lv)
    assert lv.shape == (3,) and abs(lv[2] + 20.0) <= 0.05
    assert lv[0] < -100.0 and lv[1] < -100.0
    assert np.all(np.abs(lv - channel_rule(sp, freqs)) <= 1e-4)
    # a shard reports every channel of the list, not only its own
    rx = vh.Receiver(CF, freqs, 10, vh.FMT_CF32, chan_first=1, chan_count=1)
    rx.spectrum_enable(n, vh.WIN_BH4)
    rx.feed(raw)
    assert np.array_equal(rx.channel_levels(), lv)
    rx.close()


# ---------------------------------------------------------------- 11. a group: member 0's context is the handle
def test_group(vh, golden_wav):
    freqs = [CF, CF + 50000]
    blocks = [golden_wav[k:k + 320000] for k in range(0, golden_wav.size, 320000)]

    def run_group(monitor):
        g = vh.ReceiverGroup(CF, freqs, [0, 0], 10, vh.FMT_S16LE)
        ctx = C.c_void_p(g.L.vdl2hip_group_ctx(g.h, 0))
        if monitor:
            cfg = vh.SpectrumCfg(C.sizeof(vh.SpectrumCfg), 1024, vh.WIN_HANN, 1)
            assert g.L.vdl2hip_spectrum_enable(ctx, C.byref(cfg)) == 0
        frames = []
        for b in blocks:
            g.feed(b)
            frames += g.drain()
        sp = vh._spectrum_read(g.L, ctx, False, True) if monitor else None
        g.close()
        return frames, sp
    f0, _ = run_group(False)
    f1, sp = run_group(True)
    assert len(f0) == 2
    assert_frames_equal(f0, f1, label="group with a monitor")
    rx = vh.Receiver(CF, freqs, 10, vh.FMT_S16LE)
    rx.spectrum_enable(1024)
    for b in blocks:
        rx.feed(b)
    assert_same_bits(rx.spectrum(), sp, "member 0 against a single receiver")
    rx.close()


# ---------------------------------------------------------------- 12. the tool
def test_tool(vh, golden_wav, tmp_path):
    from dumpvdl2_amd import build
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    out = str(tmp_path / "spectrum.txt")
    base = [exe, "--iq-file", WAV, "--sample-format", "S16_LE"]
    p0 = subprocess.run(base, check=True, capture_output=True, text=True, timeout=120)
    p1 = subprocess.run(base + ["--spectrum-out", out], check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stdout.count("[S:") == 2
    assert " level=" not in p0.stderr and f"{CF} Hz: sync.good=1" in p1.stderr and " dBFS\n" in p1.stderr
    assert [l.split(" level=")[0] for l in p1.stderr.splitlines()] == p0.stderr.splitlines()
    # the binding on the same file, cut as the tool cuts it (8 blocks of 320 000 bytes per feed at this format and rate)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=8 * 320000)
    rx.spectrum_enable(1024)
    for k in range(0, golden_wav.size, 8 * 320000):
        rx.feed(golden_wav[k:k + 8 * 320000])
    sp = rx.spectrum()
    lv = rx.channel_levels()
    rx.close()
    lines = open(out).read().splitlines()
    head = dict(l[2:].split(" ", 1) for l in lines if l.startswith("# "))
    bins = np.array([[float(v) for v in l.split()] for l in lines if not l.startswith("#")])
    assert set(head) == {k for k, _ in vh.SpectrumInfo._fields_ if k != "struct_size"}
    for k in ("nfft", "window", "stride", "sample_rate", "centerfreq", "segments", "samples", "clipped"):
        assert int(head[k]) == sp[k], k
    for k in ("enbw_bins", "mean_power", "dc_i", "dc_q", "peak"):
        assert abs(float(head[k]) - sp[k]) <= 1e-8 * abs(sp[k]), k                  # (nine significant digits are printed)
    assert bins.shape == (1024, 2)
    # to the printed precision: three decimals of the frequency, four of the level
    assert np.all(np.abs(bins[:, 0] - sp["freq_hz"]) <= 0.00051)
    assert np.all(np.abs(bins[:, 1] - 10 * np.log10(sp["power"])) <= 0.000051)
    assert f" level={lv[0]:.2f} dBFS" in p1.stderr
