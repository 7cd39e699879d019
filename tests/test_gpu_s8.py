"""Signed 8-bit input (VDL2HIP_FMT_S8) through the whole receiver.

A byte b counts (float)b / 128.0f, which is bit for bit the float process_buf_short() makes of the int16 256 b (include/vdl2hip.h).  So
an S8 receiver is an FMT_S16LE receiver fed b << 8, and the reference for every test here is the oracle fed those int16 bytes: the
oracle's frames, integer metadata, timing and counters exactly, the floats within tests/util.py's tolerances; and where the arithmetic
is the same source on the same values (everything after the staging), the same bits as an FMT_S16LE receiver fed b << 8.
Pieces are always whole samples (2 bytes); the feeder is tests/util.py's, the conversions tests/rawfmt_cases.py's, and the referee's
scans of an S8 capture are rows of tests/test_gpu_referee.py's scan tests."""
import os
import sys

import numpy as np
import pytest

import cases
import rawfmt_cases
from rawfmt_cases import s8_of_s16, s16_of_s8
from util import assert_frames_equal, feed_pieces, all_counters

pytestmark = pytest.mark.gpu
CF = 136975000
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def feed_s8(rx, b, samples=None, rng=None):
    assert b.dtype == np.int8
    feed_pieces(rx, b, 2, samples, rng)


def oracle_answer(oracle_mod, cf, freqs, os_, b, max_ppm=0.0):
    """frames and counters of the oracle fed b << 8"""
    o = oracle_mod.Oracle(cf, list(freqs), oversample=os_, max_ppm=max_ppm)
    o.process(s16_of_s8(b), block_bytes=1 << 24, nthreads=8)
    fo, co = o.frames(), all_counters(o, len(freqs))
    o.close()
    assert len(fo) > 0
    return fo, co


# ---------------------------------------------------------------- 1. accepted and rejected values
def test_accepted_and_rejected_values(vh):
    import torch
    assert vh.FMT_S8 == 4
    rx = vh.Receiver(CF, [CF], 10, sample_fmt=4)                       # (rejected before this format existed)
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):
        vh.Receiver(CF, [CF], 10, sample_fmt=5)
    t = torch.zeros(4096, dtype=torch.int8, device="cuda")
    assert t.data_ptr() % 2 == 0
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):    # (an odd address)
        rx.feed_device(t.data_ptr() + 1, 2 * 1000)
    rx.feed_device(t.data_ptr() + 2, 2 * 1000)                         # (an even one that a 4-byte format would refuse)
    rx.feed(np.zeros(15, dtype=np.int8))                               # 15 bytes: truncated to 7 whole samples
    rx.drain()
    assert rx.stats()["input_samples"] == 1000 + 7
    assert rx.L.vdl2hip_abi_version() == 6
    rx.close()


# ---------------------------------------------------------------- 2. the conversion
def test_conversion_is_exact(vh):
    """s8_level() on the device, all 256 byte patterns (even ones through the low byte of the word, odd ones through the high byte),
    against the plain conversion on the device and against numpy - as bits"""
    import ctypes as C
    L = vh.load_library()
    L.vdl2hip_debug_s8_levels.argtypes = [C.POINTER(C.c_float)]
    out = (C.c_float * 512)()
    assert L.vdl2hip_debug_s8_levels(out) == 0
    got = np.frombuffer(out, dtype=np.float32)
    want = np.arange(256, dtype=np.uint8).view(np.int8).astype(np.float32) / np.float32(128.0)
    assert want[128] == -1.0 and want[127] == np.float32(127 / 128) and want[0] == 0.0
    assert got[:256].tobytes() == want.tobytes(), np.flatnonzero(got[:256].view(np.uint32) != want.view(np.uint32))
    assert got[256:].tobytes() == want.tobytes(), np.flatnonzero(got[256:].view(np.uint32) != want.view(np.uint32))


# ---------------------------------------------------------------- 3. generic build, unmixed channel
@pytest.fixture(scope="module")
def wav(oracle_mod, golden_wav):
    b = s8_of_s16(golden_wav)
    fo, co = oracle_answer(oracle_mod, CF, [CF], 10, b)
    assert [len(f["octets"]) for f in fo] == [314, 186]
    return b, fo, co


@pytest.mark.parametrize("samples", [None, 40000, 4001], ids=["whole", "40000-sample blocks", "4001-sample blocks"])
def test_generic_build_unmixed_channel(vh, wav, samples):
    """The reference's WAV (oversample 10, one channel on the centre: one channel per wavefront, the generic staging path) as S8:
    load_sample, k_carry with every remainder 1..9 (4001 samples a block), the scan's shortcut for channels that are not mixed."""
    b, fo, co = wav
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S8, max_block_bytes=b.nbytes if samples is None else 320000)
    feed_s8(rx, b, samples)
    fr = rx.drain()
    assert [len(f["octets"]) for f in fr] == [314, 186]
    assert_frames_equal(fo, fr, label=f"wav as s8, {samples}")
    assert all_counters(rx, 1) == co
    rx.close()


# ---------------------------------------------------------------- 4. the hot build, oversample 20
HOT_DELTA, HOT_POS = 25000, 6


@pytest.fixture(scope="module")
def hot(oracle_mod):
    """resample_wav.upsampled2x(25000) on hot_plan(25000, 6) as S8: 16 channels at oversample 20 - the smallest shape that selects four
    channels per wavefront, i.e. the signed-byte build of k_chanfir that fetches its tiles ahead"""
    import resample_wav as rw
    from test_oracle_golden import hot_plan
    b = s8_of_s16(rw.upsampled2x(HOT_DELTA))
    cf, freqs = hot_plan(HOT_DELTA, HOT_POS)
    fo, co = oracle_answer(oracle_mod, cf, freqs, 20, b)
    assert len(fo) == 4 and len([f for f in fo if f["chan"] == HOT_POS]) == 2
    return dict(b=b, cf=cf, freqs=freqs, frames=fo, counters=co)


@pytest.mark.parametrize("samples", [None, 40001], ids=["one block", "40001-sample blocks"])
def test_hot_build_oversample_20(vh, hot, samples):
    """(a) one block: every tile on the look-ahead path; (b) blocks of 40001 samples: the carry walks through 1..19, the tiles that
    straddle blocks take the generic path"""
    b = hot["b"]
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_S8, max_block_bytes=b.nbytes if samples is None else 80002)
    assert rx.chan_count == 16
    feed_s8(rx, b, samples)
    fr = rx.drain()
    assert len(fr) > 0
    assert_frames_equal(hot["frames"], fr, label=f"hot capture as s8, {samples}")
    assert all_counters(rx, 16) == hot["counters"]
    rx.close()


# ---------------------------------------------------------------- 5. the hot build, oversample 10
@pytest.fixture(scope="module")
def os10(oracle_mod):
    """16 channels at oversample 10, loud enough to saturate a few bytes"""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(centerfreq=CF, freqs=synth.channel_plan(16, CF, 12000), oversample=10, duration_s=0.5, seed=87, amplitude=0.2,
                            noise_sigma=0.01, tdm_slots=4, tdm_slot_s=0.1, rx_max_ppm=5.0)
    iq, _ = synth.synthesize(cfg)
    b = s8_of_s16(iq)
    fo, co = oracle_answer(oracle_mod, CF, cfg.freqs, 10, b, cfg.rx_max_ppm)
    return dict(cfg=cfg, b=b, frames=fo, counters=co)


def test_hot_build_oversample_10(vh, os10):
    cfg, b = os10["cfg"], os10["b"]
    pairs = b.reshape(-1, 2)
    assert int(((pairs == -128) | (pairs == 127)).any(axis=1).sum()) == 3         # saturation is in
    assert len(os10["frames"]) == 11 and len({f["chan"] for f in os10["frames"]}) == 6
    rx = vh.Receiver(CF, list(cfg.freqs), 10, vh.FMT_S8, cfg.rx_max_ppm, max_block_bytes=2 * 200000)
    assert rx.chan_count == 16
    feed_s8(rx, b, (11, 200001), np.random.default_rng(3))
    fr = rx.drain()
    assert len(fr) > 0
    assert_frames_equal(os10["frames"], fr, label="16 channels at oversample 10 as s8")
    assert all_counters(rx, 16) == os10["counters"]
    rx.close()


# ---------------------------------------------------------------- 6. the stream is the s16 build's
def _stream(vh, hot, fmt, data, step_bytes):
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, fmt, max_block_bytes=data.size if step_bytes is None else step_bytes)
    rx.debug_option("referee", 0)                    # the stream as the channeliser leaves it
    for k in range(0, data.size, step_bytes or data.size):
        rx.feed(data[k:k + (step_bytes or data.size)])
    rx.drain()
    D = rx.stats()["input_samples"] // 20
    y = [rx.read_decimated(c, 0, D).copy() for c in range(16)]
    assert rx.stats()["front_sync_timeouts"] == 0
    rx.close()
    return D, y


@pytest.mark.parametrize("samples", [None, 40001], ids=["one block", "40001-sample blocks"])
def test_hot_build_stream_is_the_s16_builds_bit_for_bit(vh, hot, samples):
    """After the staging the two builds are the same source on the same values: the decimated stream of all 16 channels is
    bit-identical to an FMT_S16LE receiver's fed b << 8 the same way."""
    s8 = hot["b"].view(np.uint8)
    s16 = s16_of_s8(hot["b"])
    Da, ya = _stream(vh, hot, vh.FMT_S16LE, s16, None if samples is None else 4 * samples)
    Db, yb = _stream(vh, hot, vh.FMT_S8, s8, None if samples is None else 2 * samples)
    assert Da == Db == s8.size // 2 // 20
    assert max(float(np.abs(y).max()) for y in ya) > 0.05
    for c in range(16):
        assert ya[c].shape == yb[c].shape == (Da, 2)
        assert ya[c].tobytes() == yb[c].tobytes(), f"channel {c}: {int((ya[c] != yb[c]).sum())} values differ, max {np.abs(ya[c] - yb[c]).max():.3e}"


# ---------------------------------------------------------------- 7. cold start
def test_hot_build_cold_start(vh, oracle_mod, hot):
    """Page-locked, in one call to an idle receiver: the capture six times over (9.5 MB of S8, above the 8 MiB from which a block goes
    in pieces - stats.cold_start_feeds says so), against the oracle fed the same bytes as b << 8."""
    import torch
    b6 = np.concatenate([hot["b"]] * 6)
    fo, co = oracle_answer(oracle_mod, hot["cf"], hot["freqs"], 20, b6)
    pin = torch.from_numpy(b6).pin_memory()
    nbytes = pin.numel()
    assert nbytes >= (8 << 20) and nbytes % 2 == 0
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_S8, max_block_bytes=nbytes)
    rx.feed_pinned(pin.data_ptr(), nbytes)
    fr = rx.drain()
    assert rx.stats()["cold_start_feeds"] == 1
    assert len(fr) > 0
    assert_frames_equal(fo, fr, label="hot capture six times as s8, cold start")
    assert all_counters(rx, 16) == co
    rx.close()


# ---------------------------------------------------------------- 8. the capture of the scan tests
@pytest.fixture(scope="module")
def config2(oracle_mod):
    """(the scans on this capture: tests/test_gpu_referee.py, the s8 rows)"""
    case = rawfmt_cases.config2(oracle_mod, "s8")
    return dict(cfg=case["cfg"], b=case["raw"].view(np.int8), frames=case["frames"], counters18=case["counters18"])


# ---------------------------------------------------------------- 9. referee on
def test_referee_on(vh, config2):
    """config2 as S8 in 1 MiB feeds with the referee at work: strictly the oracle's frames, to the sample"""
    cfg, b = config2["cfg"], config2["b"]
    nch = len(cfg.freqs)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S8, cfg.rx_max_ppm, max_block_bytes=1 << 20)
    feed_s8(rx, b, 1 << 19)
    fr = rx.drain()
    assert len(fr) > 0
    assert_frames_equal(config2["frames"], fr, exact_samples=True, label="config2 as s8")
    assert [list(rx.counters(c).values())[:18] for c in range(nch)] == config2["counters18"]
    assert rx.stats()["referee_refused"] == 0
    rx.close()


# ---------------------------------------------------------------- 10. the resampler
def test_resampler_reads_s8(vh):
    """2 channels at oversample 20, the bytes taken as 2.5 MS/s (L / M = 21 / 25): r[] is byte-identical to an FMT_S16LE receiver's with
    the same input_rate fed b << 8 in the same pieces - single samples among them - and so is everything after it"""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(centerfreq=CF, freqs=[CF - 25000, CF + 50000], oversample=20, duration_s=0.3, seed=12, amplitude=0.3, noise_sigma=0.01)
    iq, _ = synth.synthesize(cfg)
    b = s8_of_s16(iq)
    N = b.size // 2
    rng = np.random.default_rng(7)
    pieces = [1, 1, 30000, 1, 7] + [int(x) for x in rng.integers(1, 30001, 64)] + [1, 29999]
    out = []
    for fmt, data, sb in ((vh.FMT_S16LE, s16_of_s8(b), 4), (vh.FMT_S8, b, 2)):
        rx = vh.Receiver(CF, list(cfg.freqs), 20, fmt, cfg.rx_max_ppm, max_block_bytes=sb * 30000, input_rate=2500000)
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        r, k, i, have = [], 0, 0, 0
        while k < raw.size:                          # (r[] is read back after every feed: the device keeps the last feeds' blocks only)
            m = sb * pieces[i % len(pieces)]
            rx.feed(raw[k:k + m]); k += m; i += 1
            new = rx.stats()["resampled_samples"] - have
            r.append(rx.read_resampled(have, new).copy())
            assert r[-1].shape == (new, 2)
            have += new
        assert i > len(pieces) // 2
        fr = rx.drain()
        st = rx.stats()
        assert st["input_samples"] == N and st["resampled_samples"] == (N * 21 + 24) // 25 == have, st
        out.append((fr, all_counters(rx, 2), np.concatenate(r)))
        rx.close()
    (fa, ca, ra), (fb, cb, rb) = out
    assert ra.shape == rb.shape and float(np.abs(ra).max()) > 0.05
    assert ra.tobytes() == rb.tobytes(), f"{int((ra != rb).sum())} values of r[] differ"
    assert_frames_equal(fa, fb, exact_samples=True, label="resampled s8 against resampled s16")
    assert ca == cb


# ---------------------------------------------------------------- 11. the input monitor
def test_input_monitor(vh, os10):
    """nfft 256, Hann, stride 1 over a hand-made block with known rail bytes followed by the oversample-10 capture: every figure but
    `clipped` is an FMT_S16LE receiver's fed b << 8 to the bit; `clipped` counts bytes -128 and 127, where the s16 rail is -32768 and 32767"""
    head = np.zeros((256, 2), dtype=np.int8)
    head[:64] = np.random.default_rng(2).integers(-100, 100, (64, 2))
    head[3] = (-128, 5)              # I only
    head[10] = (7, 127)              # Q only
    head[20] = (-128, 127)           # both, one sample
    head[30] = (127, -128)
    head[40] = (-127, 126)           # near misses
    head[41] = (126, -127)
    b = np.concatenate([head.reshape(-1), os10["b"]])
    n = 256
    got = []
    for fmt, data, sb in ((vh.FMT_S16LE, s16_of_s8(b), 4), (vh.FMT_S8, b, 2)):
        rx = vh.Receiver(CF, list(os10["cfg"].freqs), 10, fmt, max_block_bytes=sb * 100000)
        rx.spectrum_enable(n, vh.WIN_HANN, 1)
        feed_pieces(rx, data, sb, 100000)
        rx.drain()
        got.append(rx.spectrum())
        rx.close()
    a, s = got
    segs = b.size // 2 // n
    assert s["segments"] == a["segments"] == segs and s["samples"] == a["samples"] == segs * n
    for k in ("peak", "mean_power", "dc_i", "dc_q"):
        assert np.float64(s[k]).tobytes() == np.float64(a[k]).tobytes(), (k, s[k], a[k])
    assert s["power"].shape == (n,) and s["power"].tobytes() == a["power"].tobytes()
    pairs = b[:2 * segs * n].reshape(-1, 2)
    want = int(((pairs == -128) | (pairs == 127)).any(axis=1).sum())
    want_s16 = int((pairs == -128).any(axis=1).sum())                           # (127 << 8 is 32512: no rail)
    assert want >= 4 and s["clipped"] == want
    assert a["clipped"] == want_s16 != want


# ---------------------------------------------------------------- 12. group
@pytest.mark.parametrize("form", ["allgather", "broadcast"])
def test_group_of_two(vh, hot, form):
    """vdl2hip_group over [0, 0] on the hot capture in 1 MiB feeds: stripes cut on sample boundaries deliver the single receiver's frames"""
    b = hot["b"]
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_S8, max_block_bytes=b.nbytes)
    feed_s8(rx, b)
    single, cs = rx.drain(), all_counters(rx, 16)
    rx.close()
    assert len(single) == len(hot["frames"]) >= 2
    g = vh.ReceiverGroup(hot["cf"], hot["freqs"], [0, 0], 20, vh.FMT_S8, 0.0, max_block_bytes=1 << 20)
    g.set_exchange(form)
    feed_s8(g, b, (1 << 20) // 2)
    got = g.drain()
    assert g.exchange().startswith(form)
    assert_frames_equal(single, got, label=f"group of two, {form}")
    assert all_counters(g, 16) == cs
    g.close()


# ---------------------------------------------------------------- 13. the command-line tool
def test_cli_reads_an_s8_file(vh, wav, tmp_path):
    """tools/vdl2hip_iqfile --sample-format S8 on the reference's WAV written out as signed bytes, with the reference CI's arguments
    otherwise (tests/test_gpu_parity.py::test_cli_runner_and_raw_frame_archive): the same two frames"""
    import subprocess
    from dumpvdl2_amd import build
    b, fo, _ = wav
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    path = str(tmp_path / "wav.cs8")
    b.tofile(path)
    statsd = str(tmp_path / "statsd.txt")
    p = subprocess.run([exe, "--iq-file", path, "--sample-format", "S8", "--station-id", "TEST", "--avlc-filter", "--statsd-out", statsd],
                       check=True, capture_output=True, text=True, timeout=120)
    table = dict(l.rsplit(":", 1) for l in open(statsd).read().splitlines())
    assert table[f"dumpvdl2.TEST.{CF}.decoder.msg.good"] == "2|c" and table[f"dumpvdl2.TEST.{CF}.demod.sync.good"] == "1|c"
    lines = [l for l in p.stdout.splitlines() if "[S:" in l]
    assert len(lines) == 2
    hexes = [bytes.fromhex(l.rsplit(" ", 1)[1]) for l in lines]
    assert [f["octets"] for f in fo] == hexes
