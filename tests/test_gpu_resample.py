"""IQ at any rational sample rate: the resampler in front of the channeliser (vdl2hip_cfg.input_rate, K0 = k_resample).

The contract (include/vdl2hip.h, "Resampling"): with fout = 105000 * oversample, L / M = fout / input_rate reduced and h[] the taps
vdl2hip_resampler_design() returns,
    r[n] = sum_{j < T} h[j L + p_n] x[b_n - j],   p_n = (n M) mod L,   b_n = floor(n M / L),   x[i < 0] = 0
in float32 in one fixed order, ceil(N L / M) outputs after N inputs, and the receiver IS a VDL2HIP_FMT_CF32 receiver fed r[].

Captures at odd rates are rendered here with numpy only, by a float64 windowed-sinc interpolator of this file (64 taps per output,
Kaiser beta 10.06: 100 dB - longer and deeper than the library's 29-34 taps at 86 dB, and not the code under test); the float64 model
of r[] is a dozen lines over the library's own taps.  What a receiver must decode is held by the oracle on the ORIGINAL capture."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))
HOT_DELTA, HOT_POS = 25000, 6


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


# ---------------------------------------------------------------- rendering and the model (numpy, float64)
def complex_of_s16(raw):
    v = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    v = v[:v.size & ~3].view("<i2").astype(np.float64) / 32768.0
    return v[0::2] + 1j * v[1::2]


def render(x, fs_in, fs_out, half=32, beta=10.06):
    """x (complex128 at fs_in) on the grid of fs_out: y[m] = sum_k x[k] g(m fs_in / fs_out - k), g a Kaiser-windowed sinc of
    2 * half taps (in samples of the lower rate), cutoff 0.45 of the lower rate: flat to 0.40, 100 dB down from 0.50.
    -> complex64, floor(len(x) fs_out / fs_in) samples"""
    g = math.gcd(fs_in, fs_out)
    P, Q = fs_out // g, fs_in // g                        # output m sits at input time m Q / P
    r = min(1.0, P / Q)                                   # (rendering to a lower rate: the kernel is stretched, the cutoff lowered)
    W = int(math.ceil(half / r))
    nout = x.size * P // Q
    m = np.arange(nout, dtype=np.int64)
    k0, ph = (m * Q) // P, (m * Q) % P
    xp = np.concatenate([np.zeros(W, dtype=np.complex128), x, np.zeros(W + 1, dtype=np.complex128)])
    y = np.zeros(nout, dtype=np.complex128)
    frac = np.arange(P, dtype=np.float64) / P
    for i in range(-W + 1, W + 1):                        # tap at input sample k0 + i: distance (frac - i) input samples
        d = frac - i
        u = d / W
        w = np.where(np.abs(u) < 1.0, np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(beta), 0.0)
        tap = 0.9 * r * np.sinc(0.9 * r * d) * w          # per phase
        y += xp[k0 + (i + W)] * tap[ph]
    return y.astype(np.complex64)


def model(vh, x, fin, fout):
    """-> (L, M, T, r float64 complex [ceil(N L / M)], bound float64 [n, 2]): the definition, and per output and component the
    worst-case rounding of a T-term float32 dot product, (T + 2) 2^-24 sum_j |h_j| |x_j|"""
    L, M, T, taps = vh.resampler_design(fin, fout)
    h = taps.astype(np.float64)                           # [T, L]: h[j L + p]
    N = x.size
    nout = -((-N * L) // M)
    n = np.arange(nout, dtype=np.int64)
    b, p = (n * M) // L, (n * M) % L
    assert nout == 0 or (b[-1] <= N - 1 and ((nout * M) // L) > N - 1)
    xp = np.concatenate([np.zeros(T - 1, dtype=np.complex128), x.astype(np.complex128)])
    r = np.zeros(nout, dtype=np.complex128)
    bound = np.zeros((nout, 2), dtype=np.float64)
    for j in range(T):
        xj, hj = xp[b - j + (T - 1)], h[j, p]
        r += hj * xj
        bound[:, 0] += np.abs(hj) * np.abs(xj.real)
        bound[:, 1] += np.abs(hj) * np.abs(xj.imag)
    return L, M, T, r, bound * ((T + 2) * 2.0 ** -24)


def n_out(N, L, M):
    return -((-N * L) // M)


def all_counters(x, nch):
    return [list(x.counters(c).values()) for c in range(nch)]


def as_pairs(z):
    return np.ascontiguousarray(z, dtype=np.complex64).view(np.float32).reshape(-1, 2)


def feed_cut(rx, z, cuts=None, read=False):
    """z: complex64 (or any array of whole samples, with `unit` = samples per row); cuts: None (one block) or the piece lengths.
    read: -> the resampled stream, read back after every feed and concatenated"""
    b = np.ascontiguousarray(z)
    out, k, got = [], 0, 0
    for m in ([b.shape[0]] if cuts is None else cuts):
        rx.feed(b[k:k + m]); k += m
        if read:
            st = rx.stats()
            new = st["resampled_samples"] - got
            out.append(rx.read_resampled(got, new).copy())
            assert out[-1].shape == (new, 2)
            got += new
    assert k >= b.shape[0]
    return np.concatenate(out) if read else None


@pytest.fixture(scope="module")
def wav(golden_wav):
    return complex_of_s16(golden_wav)


@pytest.fixture(scope="module")
def rendered(wav):
    """the reference's WAV (1.05 MS/s) at other rates, each rendered once"""
    cache = {}

    def at(rate):
        if rate not in cache:
            cache[rate] = render(wav, 1050000, rate)
            cache[rate].setflags(write=False)
        return cache[rate]
    return at


@pytest.fixture(scope="module")
def wav_answer(oracle_mod, golden_wav):
    o = oracle_mod.Oracle(CF, [CF], oversample=10)
    o.process(golden_wav)
    fo, co = o.frames(), all_counters(o, 1)
    o.close()
    assert [len(f["octets"]) for f in fo] == [314, 186]
    return fo, co


@pytest.fixture(scope="module")
def hot(oracle_mod):
    """resample_wav.upsampled2x(25000) on hot_plan(25000, 6) - 16 channels at oversample 20, four channels per wavefront - and the
    capture rendered at 2.5 MS/s"""
    import resample_wav as rw
    from test_oracle_golden import hot_plan
    raw = rw.upsampled2x(HOT_DELTA)
    cf, freqs = hot_plan(HOT_DELTA, HOT_POS)
    o = oracle_mod.Oracle(cf, freqs, oversample=20)
    o.process(raw)
    fo = o.frames()
    o.close()
    z = render(complex_of_s16(raw), 2100000, 2500000)
    z.setflags(write=False)
    return dict(cf=cf, freqs=freqs, frames=fo, z=z)


@pytest.fixture(scope="module")
def seed12(oracle_mod):
    """the two-channel synthetic capture of test_gpu_cf32.py::test_full_mantissa_values (seed 12), as int16"""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(centerfreq=CF, freqs=[CF, CF + 40000], oversample=10, duration_s=0.6, seed=12, amplitude=0.3, noise_sigma=0.01)
    iq, _ = synth.synthesize(cfg)
    raw = iq.view(np.uint8)
    o = oracle_mod.Oracle(CF, list(cfg.freqs), oversample=10, max_ppm=cfg.rx_max_ppm)
    o.process(raw)
    fo = o.frames()
    o.close()
    assert len(fo) == 9
    return dict(cfg=cfg, x=complex_of_s16(raw), frames=fo)


# ---------------------------------------------------------------- a. the stream against the float64 model
@pytest.mark.parametrize("rate", [1250000, 1000000, 1024000, 6000000], ids=["21/25", "21/20 up", "525/512 large table", "7/40 long T"])
def test_stream_is_the_definition(vh, rendered, rate):
    z = rendered(rate)
    L, M, T, r, bound = model(vh, z, rate, 1050000)
    g = math.gcd(rate, 1050000)
    assert (L, M) == (1050000 // g, rate // g)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_CF32, max_block_bytes=z.nbytes, input_rate=rate)
    rx.feed(z)
    rx.sync()
    assert rx.stats()["resampled_samples"] == n_out(z.size, L, M) == r.size
    got = rx.read_resampled(0, r.size + 10)
    rx.close()
    assert got.shape == (r.size, 2)
    peak = float(np.abs(got).max())
    err = np.abs(got.astype(np.float64) - np.stack([r.real, r.imag], axis=1))
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{rate} -> 1050000: L {L} M {M} T {T}, {r.size} outputs, peak {peak:.3f}, max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert peak > 0.05
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"{len(bad)} values beyond the rounding bound, first at output {bad[0][0]}: {err[tuple(bad[0])]:.3e} > {bound[tuple(bad[0])]:.3e}"


# ---------------------------------------------------------------- b. cutting does not change a bit
def test_cutting_does_not_change_a_bit(vh, rendered):
    rate = 1250000
    z = rendered(rate)
    L, M, T, _ = vh.resampler_design(rate, 1050000)
    assert T > 7
    rng = np.random.default_rng(21)
    pieces = [1, 7, 1, 5000]
    while sum(pieces) < z.size:
        pieces.append(int(rng.integers(1, 5001)))
    assert 1 in pieces and 7 in pieces and max(pieces) <= 5000
    res = {}
    for name, cuts in (("whole", None), ("4001", [4001] * (z.size // 4001 + 1)), ("random", pieces)):
        rx = vh.Receiver(CF, [CF], 10, vh.FMT_CF32, max_block_bytes=z.nbytes if cuts is None else 8 * 5000, input_rate=rate)
        r = feed_cut(rx, z, cuts, read=True)
        fr = rx.drain()
        st = rx.stats()
        assert st["resampled_samples"] == n_out(z.size, L, M) == r.shape[0] and st["input_samples"] == z.size, st
        assert st["cold_start_feeds"] == 0
        res[name] = (r, fr, all_counters(rx, 1))
        rx.close()
    r0, f0, c0 = res["whole"]
    assert len(f0) == 2 and float(np.abs(r0).max()) > 0.05
    for name in ("4001", "random"):
        r, fr, cn = res[name]
        assert r.tobytes() == r0.tobytes(), f"{name}: {int((r != r0).sum())} values of the resampled stream differ from the whole block's"
        assert_frames_equal(f0, fr, exact_samples=True, label=name)
        assert cn == c0


def test_pinned_block_is_not_cut(vh, rendered):
    import torch
    rate = 1250000
    z3 = np.concatenate([rendered(rate)] * 3)
    assert z3.nbytes >= (8 << 20)
    L, M, T, _ = vh.resampler_design(rate, 1050000)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_CF32, max_block_bytes=z3.nbytes, input_rate=rate)
    rx.feed(z3)
    rx.sync()
    want = rx.read_resampled(0, n_out(z3.size, L, M)).copy()
    f0 = rx.drain()
    rx.close()
    pin = torch.from_numpy(z3.view(np.float32).copy()).pin_memory()
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_CF32, max_block_bytes=z3.nbytes, input_rate=rate)
    rx.feed_pinned(pin.data_ptr(), z3.nbytes)
    rx.sync()
    got = rx.read_resampled(0, want.shape[0] + 1)
    fr = rx.drain()
    assert rx.stats()["cold_start_feeds"] == 0
    rx.close()
    assert want.shape[0] == n_out(z3.size, L, M) and got.tobytes() == want.tobytes()
    assert_frames_equal(f0, fr, exact_samples=True, label="pinned")
    assert len(fr) == 6


# ---------------------------------------------------------------- c. formats
def test_integer_formats_resample_their_float_values(vh, rendered):
    rate = 1250000
    z = as_pairs(rendered(rate)).reshape(-1)
    k16 = np.clip(np.rint(z.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")
    b8 = np.clip(np.rint(z.astype(np.float64) * 127.5 + 127.5), 0, 255).astype(np.uint8)
    f16 = k16.astype(np.float32) / np.float32(32768.0)
    f8 = (b8.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    L, M, T, _ = vh.resampler_design(rate, 1050000)
    n = n_out(z.size // 2, L, M)
    for fmt, data, f32 in ((vh.FMT_S16LE, k16, f16), (vh.FMT_U8, b8, f8)):
        out = []
        for f, d in ((fmt, data), (vh.FMT_CF32, f32)):
            rx = vh.Receiver(CF, [CF], 10, f, max_block_bytes=d.nbytes, input_rate=rate)
            rx.feed(d)
            rx.sync()
            assert rx.stats()["input_samples"] == z.size // 2
            out.append(rx.read_resampled(0, n).copy())
            rx.close()
        assert out[0].shape == (n, 2) and float(np.abs(out[0]).max()) > 0.05
        assert out[0].tobytes() == out[1].tobytes(), f"format {fmt}: {int((out[0] != out[1]).sum())} values differ from the CF32 receiver's"


# ---------------------------------------------------------------- d. it is a CF32 receiver fed r[]
def _pair(vh, cf, freqs, os_, z, rate, max_ppm, referee):
    nch = len(freqs)
    rx = vh.Receiver(cf, freqs, os_, vh.FMT_CF32, max_ppm, max_block_bytes=z.nbytes, input_rate=rate)
    if not referee:
        rx.debug_option("referee", 0)
    rx.feed(z)
    fa = rx.drain()
    st = rx.stats()
    n = st["resampled_samples"]
    r = rx.read_resampled(0, n).copy()
    assert r.shape == (n, 2)
    D = n // os_
    ya = [rx.read_decimated(c, 0, D).copy() for c in range(nch)]
    ca = all_counters(rx, nch)
    assert st["front_sync_timeouts"] == 0
    rx.close()
    rx = vh.Receiver(cf, freqs, os_, vh.FMT_CF32, max_ppm, max_block_bytes=r.nbytes)
    if not referee:
        rx.debug_option("referee", 0)
    rx.feed(r)
    fb = rx.drain()
    assert rx.stats()["input_samples"] == n and rx.stats()["resampled_samples"] == 0
    yb = [rx.read_decimated(c, 0, D).copy() for c in range(nch)]
    cb = all_counters(rx, nch)
    rx.close()
    return fa, ca, ya, fb, cb, yb


@pytest.mark.parametrize("which", ["hot at 2.5 MS/s", "seed 12 at 1.2 MS/s"])
def test_it_is_a_cf32_receiver_fed_the_resampled_stream(vh, hot, seed12, which):
    if which.startswith("hot"):
        cf, freqs, os_, z, rate, ppm = hot["cf"], hot["freqs"], 20, hot["z"], 2500000, 0.0
    else:
        cfg = seed12["cfg"]
        cf, freqs, os_, rate, ppm = CF, list(cfg.freqs), 10, 1200000, cfg.rx_max_ppm
        z = render(seed12["x"], 1050000, rate)
    fa, ca, _, fb, cb, _ = _pair(vh, cf, freqs, os_, z, rate, ppm, referee=True)
    assert len(fa) >= 2
    assert_frames_equal(fb, fa, exact_samples=True, label=which)
    assert ca == cb
    _, _, ya, _, _, yb = _pair(vh, cf, freqs, os_, z, rate, ppm, referee=False)
    assert max(float(np.abs(y).max()) for y in ya) > 0.05
    for c in range(len(freqs)):
        assert ya[c].shape == yb[c].shape and ya[c].tobytes() == yb[c].tobytes(), f"{which}: channel {c}: {int((ya[c] != yb[c]).sum())} decimated values differ"


# ---------------------------------------------------------------- e. it still decodes what was sent
def _delay_bound(vh, rate, os_):
    L, M, T, _ = vh.resampler_design(rate, 105000 * os_)
    return 3 + -((-(L * T - 1)) // (2 * M * os_))


@pytest.mark.parametrize("rate", [1250000, 1200000, 1000000])
def test_wav_at_other_rates_decodes_the_oracles_frames(vh, rendered, wav_answer, rate):
    fo, _ = wav_answer
    z = rendered(rate)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_CF32, max_block_bytes=z.nbytes, input_rate=rate)
    rx.feed(z)
    fr = rx.drain()
    rx.close()
    assert [len(f["octets"]) for f in fr] == [314, 186]
    assert [f["octets"] for f in fr] == [f["octets"] for f in fo]
    lim = _delay_bound(vh, rate, 10)
    d = [b["sync_sample"] - a["sync_sample"] for a, b in zip(fo, fr)]
    print(f"{rate}: sync_sample moved by {d} (bound {lim})")
    assert all(abs(v) <= lim for v in d), (d, lim)


def test_hot_capture_at_2500k_decodes_the_oracles_frames(vh, hot):
    z = hot["z"]
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_CF32, max_block_bytes=z.nbytes, input_rate=2500000)
    rx.feed(z)
    fr = [f for f in rx.drain() if f["chan"] == HOT_POS]
    rx.close()
    fo = [f for f in hot["frames"] if f["chan"] == HOT_POS]
    assert len(fo) == 2 and [f["octets"] for f in fr] == [f["octets"] for f in fo]
    assert [(f["idx"], f["datalen_octets"], f["num_fec_corrections"]) for f in fr] == [(f["idx"], f["datalen_octets"], f["num_fec_corrections"]) for f in fo]


@pytest.mark.parametrize("rate", [1200000, 1250000])
def test_seed12_at_other_rates_decodes_the_oracles_frames(vh, seed12, rate):
    cfg, fo = seed12["cfg"], seed12["frames"]
    z = render(seed12["x"], 1050000, rate)
    rx = vh.Receiver(CF, list(cfg.freqs), 10, vh.FMT_CF32, cfg.rx_max_ppm, max_block_bytes=z.nbytes, input_rate=rate)
    rx.feed(z)
    fr = rx.drain()
    rx.close()
    key = lambda f: (f["chan"], f["sync_sample"], f["idx"])
    fo, fr = sorted(fo, key=key), sorted(fr, key=key)
    assert sorted((f["chan"], f["octets"]) for f in fr) == sorted((f["chan"], f["octets"]) for f in fo) and len(fo) == 9
    assert [(f["chan"], f["octets"]) for f in fr] == [(f["chan"], f["octets"]) for f in fo]
    d = [b["sync_sample"] - a["sync_sample"] for a, b in zip(fo, fr)]
    print(f"seed 12 at {rate}: sync_sample moved by {d}")
    assert all(abs(v) <= 3 for v in d), d


# ---------------------------------------------------------------- f. nothing changed for plain receivers
class Cfg56(C.Structure):
    """vdl2hip_cfg as it was before input_rate: 56 bytes, the last four of them padding"""
    _fields_ = [("struct_size", C.c_uint32), ("centerfreq", C.c_uint32), ("oversample", C.c_uint32),
                ("sample_fmt", C.c_uint32), ("nchan", C.c_uint32), ("freqs", C.POINTER(C.c_uint32)),
                ("max_ppm", C.c_float), ("device", C.c_int32), ("max_block_bytes", C.c_uint32),
                ("chan_first", C.c_uint32), ("chan_count", C.c_uint32)]


def _legacy_receiver(vh):
    assert C.sizeof(Cfg56) == 56
    lib = vh.load_library()
    freqs = (C.c_uint32 * 1)(CF)
    buf = (C.c_uint8 * 64)(*([0xA5] * 64))                 # what follows the structure, and its padding, is not the library's to read
    cfg = Cfg56.from_buffer(buf)
    cfg.struct_size, cfg.centerfreq, cfg.oversample, cfg.sample_fmt, cfg.nchan = 56, CF, 10, vh.FMT_S16LE, 1
    cfg.freqs = C.cast(freqs, C.POINTER(C.c_uint32))
    cfg.max_ppm, cfg.device, cfg.max_block_bytes, cfg.chan_first, cfg.chan_count = 0.0, 0, 320000, 0, 0
    assert bytes(buf[52:64]) == b"\xa5" * 12
    h = C.c_void_p()
    r = lib.vdl2hip_create(C.cast(buf, C.POINTER(vh.Cfg)), C.byref(h))
    assert r == 0, r
    rx = vh.Receiver.__new__(vh.Receiver)
    rx.L, rx.h, rx.freqs, rx._freq_arr, rx.chan_first, rx.chan_count = lib, h, [CF], freqs, 0, 1
    return rx


def test_plain_receivers_are_what_they_were(vh, golden_wav, wav_answer):
    fo, co = wav_answer
    res = []
    for how in ("input_rate 0", "input_rate 1050000", "56-byte cfg"):
        rx = _legacy_receiver(vh) if how == "56-byte cfg" else vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, input_rate=0 if how.endswith(" 0") else 1050000)
        for k in range(0, golden_wav.size, 320000):
            rx.feed(golden_wav[k:k + 320000])
        fr = rx.drain()
        st = rx.stats()
        assert st["resampled_samples"] == 0 and st["resample_ms"] == 0.0 and st["input_samples"] == golden_wav.size // 4
        buf = np.zeros(16, dtype=np.float32)
        assert rx.L.vdl2hip_read_resampled(rx.h, 0, buf.ctypes.data, 8) == -1
        y = rx.read_decimated(0, 0, st["input_samples"] // 10).copy()
        res.append((fr, all_counters(rx, 1), y))
        rx.close()
        assert_frames_equal(fo, fr, exact_samples=True, label=how)
        assert res[-1][1] == co
    for fr, cn, y in res[1:]:
        assert fr == res[0][0] and cn == res[0][1] and y.tobytes() == res[0][2].tobytes()


# ---------------------------------------------------------------- g. group
@pytest.mark.parametrize("form", ["allgather", "broadcast"])
def test_group_of_two(vh, hot, form):
    z = hot["z"]
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_CF32, max_block_bytes=z.nbytes, input_rate=2500000)
    rx.feed(z)
    single, cs = rx.drain(), all_counters(rx, 16)
    rx.close()
    assert len([f for f in single if f["chan"] == HOT_POS]) == 2
    g = vh.ReceiverGroup(hot["cf"], hot["freqs"], [0, 0], 20, vh.FMT_CF32, 0.0, max_block_bytes=1 << 20, input_rate=2500000)
    g.set_exchange(form)
    step = (1 << 20) // 8
    for k in range(0, z.size, step):
        g.feed(z[k:k + step])
    got = g.drain()
    assert g.exchange().startswith(form)
    assert_frames_equal(single, got, exact_samples=True, label=f"group of two, {form}")
    assert all_counters(g, 16) == cs
    st = g.stats()
    assert st["input_samples"] == 2 * z.size and st["resampled_samples"] == 2 * n_out(z.size, 21, 25)
    g.close()


# ---------------------------------------------------------------- h. the command-line tool
def test_cli_reads_a_file_at_another_rate(vh, rendered, wav_answer, tmp_path):
    import subprocess
    from dumpvdl2_amd import build
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    path = str(tmp_path / "wav_1250k.cf32")
    rendered(1250000).tofile(path)
    statsd = str(tmp_path / "statsd.txt")
    p = subprocess.run([exe, "--iq-file", path, "--sample-format", "CF32", "--sample-rate", "1250000", "--station-id", "TEST", "--avlc-filter",
                        "--statsd-out", statsd], check=True, capture_output=True, text=True, timeout=120)
    table = dict(l.rsplit(":", 1) for l in open(statsd).read().splitlines())
    assert table[f"dumpvdl2.TEST.{CF}.decoder.msg.good"] == "2|c" and table[f"dumpvdl2.TEST.{CF}.demod.sync.good"] == "1|c"
    lines = [l for l in p.stdout.splitlines() if "[S:" in l]
    assert len(lines) == 2 and all("[S:0] [L:504] [F:0]" in l for l in lines)
    hexes = [bytes.fromhex(l.rsplit(" ", 1)[1]) for l in lines]
    assert b" -RA BR OVC005\n" in hexes[0] and b" SLP135\n" in hexes[1]
    assert [f["octets"] for f in wav_answer[0]] == hexes
