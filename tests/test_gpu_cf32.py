"""Complex float32 input (VDL2HIP_FMT_CF32) through the whole receiver.

A CF32 sample is the reference's sbuf[] value taken as it is (include/vdl2hip.h).  So the reference for every test here is the oracle
fed INTEGER bytes: a float32 that equals k / 32768 exactly goes through the same sbuf[] value as the int16 k, and (b - 127.5f) / 127.5f
computed in float32 (src/demod.c:352) through the same value as the byte b.  A CF32 rendering of an S16 or U8 capture must therefore
give the oracle's frames, integer metadata, timing and counters exactly, the floats within tests/util.py's tolerances; and where the
arithmetic is the same source (everything after the channeliser's staging), the same bits as an FMT_S16LE receiver.
Pieces are always whole samples (multiples of 8 bytes); this file brings its own feeder; the conversions shared with other tests are in
tests/rawfmt_cases.py, and the referee's scans of a CF32 capture are rows of tests/test_gpu_referee.py's scan tests."""
import os
import sys

import numpy as np
import pytest

import cases
from rawfmt_cases import cf32_of_s16
from util import assert_frames_equal, all_counters

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


def cf32_of_u8(raw):
    """unsigned bytes -> float32 levels: (b - 127.5f) / 127.5f in float32 (process_buf_uchar(), src/demod.c:349-354)"""
    b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1).astype(np.float32)
    return (b - np.float32(127.5)) / np.float32(127.5)


def feed_cf32(rx, f32, samples=None, rng=None):
    """samples: None - one block; an int - blocks of that many complex samples; (lo, hi) - random pieces of lo..hi-1 samples"""
    b = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint8)
    assert b.size % 8 == 0
    if samples is None:
        rx.feed(b)
        return
    k = 0
    while k < b.size:
        m = 8 * (samples if isinstance(samples, int) else int(rng.integers(*samples)))
        rx.feed(b[k:k + m]); k += m


# ---------------------------------------------------------------- 1. accepted and rejected values
def test_accepted_and_rejected_values(vh):
    import torch
    assert vh.FMT_CF32 == 2
    rx = vh.Receiver(CF, [CF], 10, sample_fmt=2)                       # (rejected before this format existed)
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):
        vh.Receiver(CF, [CF], 10, sample_fmt=3)
    t = torch.zeros(4096, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 8 == 0
    rx.feed_device(t.data_ptr(), 8 * 1000)
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):    # (4 bytes off a sample boundary: accepted by a 4-byte format, not by this one)
        rx.feed_device(t.data_ptr() + 4, 8 * 1000)
    rx.feed(np.zeros(2 * 7 + 1, dtype=np.float32))                     # 60 bytes: truncated to 7 whole samples
    rx.drain()
    assert rx.stats()["input_samples"] == 1000 + 7
    assert rx.L.vdl2hip_abi_version() == 6
    rx.close()


# ---------------------------------------------------------------- 2. generic build, unmixed channel
@pytest.fixture(scope="module")
def wav_answer(oracle_mod, golden_wav):
    o = oracle_mod.Oracle(CF, [CF], oversample=10)
    o.process(golden_wav)
    return o.frames(), all_counters(o, 1)


@pytest.mark.parametrize("samples", [None, 40000, 4001], ids=["whole", "320000-byte blocks", "4001-sample blocks"])
def test_generic_build_unmixed_channel(vh, golden_wav, wav_answer, samples):
    """The reference's WAV (oversample 10, one channel on the centre: one channel per wavefront, the generic staging path) as CF32:
    load_sample, k_carry with every remainder 1..9 (4001 samples a block), the scan's shortcut for channels that are not mixed."""
    fo, co = wav_answer
    f32 = cf32_of_s16(golden_wav)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_CF32, max_block_bytes=f32.nbytes if samples is None else 320000)
    feed_cf32(rx, f32, samples)
    fr = rx.drain()
    assert [len(f["octets"]) for f in fr] == [314, 186]
    assert_frames_equal(fo, fr, label=f"wav as cf32, {samples}")
    assert all_counters(rx, 1) == co
    rx.close()


# ---------------------------------------------------------------- 3. the hot build
HOT_DELTA, HOT_POS = 25000, 6


@pytest.fixture(scope="module")
def hot(oracle_mod):
    """resample_wav.upsampled2x(25000) on hot_plan(25000, 6): 16 channels at oversample 20 - the smallest shape that selects four
    channels per wavefront, i.e. the float32 build of k_chanfir that fetches its tiles ahead"""
    import resample_wav as rw
    from test_oracle_golden import hot_plan
    raw = rw.upsampled2x(HOT_DELTA)
    cf, freqs = hot_plan(HOT_DELTA, HOT_POS)
    o = oracle_mod.Oracle(cf, freqs, oversample=20)
    o.process(raw)
    fo, co = o.frames(), all_counters(o, 16)
    o.close()
    assert len([f for f in fo if f["chan"] == HOT_POS]) == 2
    return dict(raw=raw, f32=cf32_of_s16(raw), cf=cf, freqs=freqs, frames=fo, counters=co)


@pytest.mark.parametrize("samples", [None, 40001], ids=["one block", "320008-byte blocks"])
def test_hot_build(vh, hot, samples):
    """(a) one block: every tile on the look-ahead path; (b) blocks of 40001 samples: the carry walks through 1..19, the tiles that
    straddle blocks take the generic path"""
    f32 = hot["f32"]
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_CF32, max_block_bytes=f32.nbytes if samples is None else 320008)
    assert rx.chan_count == 16
    feed_cf32(rx, f32, samples)
    fr = rx.drain()
    assert_frames_equal(hot["frames"], fr, label=f"hot capture as cf32, {samples}")
    assert all_counters(rx, 16) == hot["counters"]
    rx.close()


def test_hot_build_cold_start(vh, oracle_mod, hot):
    """(c) page-locked, in one call to an idle receiver.  The rendering of the capture is 6.3 MB - under the 8 MiB from which a block
    goes in pieces - so the capture is fed twice over in one block (12.7 MB: four pieces, stats.cold_start_feeds says so), against the
    oracle fed the int16 bytes twice over."""
    import torch
    raw2 = np.concatenate([hot["raw"], hot["raw"]])
    o = oracle_mod.Oracle(hot["cf"], hot["freqs"], oversample=20)
    o.process(raw2)
    fo, co = o.frames(), all_counters(o, 16)
    o.close()
    pin = torch.from_numpy(cf32_of_s16(raw2)).pin_memory()
    nbytes = pin.numel() * 4
    assert nbytes >= (8 << 20) and nbytes % 8 == 0
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_CF32, max_block_bytes=nbytes)
    rx.feed_pinned(pin.data_ptr(), nbytes)
    fr = rx.drain()
    assert rx.stats()["cold_start_feeds"] == 1
    assert_frames_equal(fo, fr, label="hot capture twice as cf32, cold start")
    assert all_counters(rx, 16) == co
    rx.close()


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
    bit-identical to an FMT_S16LE receiver's fed the int16 bytes the same way."""
    s16 = np.ascontiguousarray(hot["raw"]).view(np.uint8)
    f32 = hot["f32"].view(np.uint8)
    Da, ya = _stream(vh, hot, vh.FMT_S16LE, s16, None if samples is None else 4 * samples)
    Db, yb = _stream(vh, hot, vh.FMT_CF32, f32, None if samples is None else 8 * samples)
    assert Da == Db == s16.size // 4 // 20
    assert max(float(np.abs(y).max()) for y in ya) > 0.05
    for c in range(16):
        assert ya[c].shape == yb[c].shape == (Da, 2)
        assert ya[c].tobytes() == yb[c].tobytes(), f"channel {c}: {int((ya[c] != yb[c]).sum())} values differ, max {np.abs(ya[c] - yb[c]).max():.3e}"


# ---------------------------------------------------------------- 4. full-mantissa values
def test_full_mantissa_values(vh, oracle_mod):
    """The shape of test_gpu_parity.py::test_uint8_input (2 channels, oversample 10, 0.6 s, random pieces of 11..50000 samples), the
    u8 capture rendered as the 256 float32 levels (b - 127.5f) / 127.5f - values with full mantissas - against the oracle fed the bytes."""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(centerfreq=CF, freqs=[CF, CF + 40000], oversample=10, duration_s=0.6, seed=12, amplitude=0.3, noise_sigma=0.01)
    iq8, _ = synth.synthesize(cfg, dtype=np.uint8)
    o = oracle_mod.Oracle(CF, list(cfg.freqs), oversample=10, sample_fmt=oracle_mod.FMT_U8)
    o.process(iq8)
    fo = o.frames()
    assert len(fo) >= 2
    rx = vh.Receiver(CF, list(cfg.freqs), 10, vh.FMT_CF32, cfg.rx_max_ppm, max_block_bytes=8 * 50000)
    feed_cf32(rx, cf32_of_u8(iq8), (11, 50000), np.random.default_rng(3))
    fr = rx.drain()
    assert_frames_equal(fo, fr, label="u8 levels as cf32")
    assert all_counters(rx, 2) == all_counters(o, 2)
    rx.close(); o.close()


# ---------------------------------------------------------------- 5. exact power-of-two scaling
def test_power_of_two_scaling_is_exact(vh, hot):
    """Values no integer format can express: the hot capture times 2^-6.  Every operation of the channeliser is a rounded product or
    sum, so the decimated stream must be 2^-6 times the FMT_S16LE receiver's, bit for bit, wherever the latter's magnitude is >= 2^-60
    (below that denormals end the exactness)."""
    s16 = np.ascontiguousarray(hot["raw"]).view(np.uint8)
    scaled = hot["f32"] * np.float32(2.0 ** -6)
    assert np.array_equal(scaled * np.float32(64.0), hot["f32"])
    D, ya = _stream(vh, hot, vh.FMT_S16LE, s16, None)
    Db, yb = _stream(vh, hot, vh.FMT_CF32, scaled.view(np.uint8), None)
    assert D == Db
    held = 0
    for c in range(16):
        big = np.hypot(ya[c][:, 0].astype(np.float64), ya[c][:, 1].astype(np.float64)) >= 2.0 ** -60
        want = ya[c] * np.float32(2.0 ** -6)
        assert want[big].tobytes() == yb[c][big].tobytes(), f"channel {c}: {int((want[big] != yb[c][big]).sum())} values are not 2^-6 times the s16 stream's"
        held += int(big.sum())
    assert held >= D, held                              # (the tuned channel alone carries signal or its filter's tail all along)


# ---------------------------------------------------------------- 6. the referee reads CF32 (the scans: tests/test_gpu_referee.py, the cf32 rows)
@pytest.mark.parametrize("seed,profile", [(175, "plain"), (274, "plain"), (1014, "extreme")])
def test_decisions_that_hang_on_the_references_rounding(vh, oracle_mod, seed, profile):
    """The captures that differ from the oracle without the referee (tests/test_gpu_referee.py), as CF32: strictly the oracle's with it"""
    import fuzz_gpu
    from dumpvdl2_amd import synth
    cfg, _ = fuzz_gpu.make_cfg(seed, profile)
    iq, _ = synth.synthesize(cfg)
    raw = iq.view(np.uint8)
    nch = len(cfg.freqs)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
    o.process(raw, block_bytes=1 << 24, nthreads=8)
    fo = o.frames()
    co = [list(o.counters(c).values())[:18] for c in range(nch)]
    o.close()
    f32 = cf32_of_s16(raw)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_CF32, cfg.rx_max_ppm, max_block_bytes=f32.nbytes)
    feed_cf32(rx, f32, 1 << 18)                       # (the S16 test's 1 MiB feeds, in samples)
    fr = rx.drain()
    assert_frames_equal(fo, fr, exact_samples=True, label=f"seed {seed} as cf32")
    assert [list(rx.counters(c).values())[:18] for c in range(nch)] == co
    s = rx.stats()
    assert s["referee_scans"] > 0 and s["referee_refused"] == 0, s
    rx.close()


# ---------------------------------------------------------------- 7. group
@pytest.mark.parametrize("form", ["allgather", "broadcast"])
def test_group_of_two(vh, hot, form):
    """vdl2hip_group over [0, 0] on the hot capture in 1 MiB feeds: stripes cut on sample boundaries deliver the single receiver's frames"""
    f32 = hot["f32"]
    rx = vh.Receiver(hot["cf"], hot["freqs"], 20, vh.FMT_CF32, max_block_bytes=f32.nbytes)
    feed_cf32(rx, f32)
    single, cs = rx.drain(), all_counters(rx, 16)
    rx.close()
    assert len(single) == len(hot["frames"]) >= 2
    g = vh.ReceiverGroup(hot["cf"], hot["freqs"], [0, 0], 20, vh.FMT_CF32, 0.0, max_block_bytes=1 << 20)
    g.set_exchange(form)
    feed_cf32(g, f32, (1 << 20) // 8)
    got = g.drain()
    assert g.exchange().startswith(form)
    assert_frames_equal(single, got, label=f"group of two, {form}")
    assert all_counters(g, 16) == cs
    g.close()


# ---------------------------------------------------------------- 8. the command-line tool
def test_cli_reads_a_cf32_file(vh, golden_wav, wav_answer, tmp_path):
    """tools/vdl2hip_iqfile --sample-format CF32 on the reference's WAV written out as float32, with the reference CI's arguments
    otherwise (tests/test_gpu_parity.py::test_cli_runner_and_raw_frame_archive): the same two frames"""
    import subprocess
    from dumpvdl2_amd import build
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    path = str(tmp_path / "wav.cf32")
    cf32_of_s16(golden_wav).tofile(path)
    statsd = str(tmp_path / "statsd.txt")
    p = subprocess.run([exe, "--iq-file", path, "--sample-format", "CF32", "--station-id", "TEST", "--avlc-filter", "--statsd-out", statsd],
                       check=True, capture_output=True, text=True, timeout=120)
    table = dict(l.rsplit(":", 1) for l in open(statsd).read().splitlines())
    assert table[f"dumpvdl2.TEST.{CF}.decoder.msg.good"] == "2|c" and table[f"dumpvdl2.TEST.{CF}.demod.sync.good"] == "1|c"
    lines = [l for l in p.stdout.splitlines() if "[S:" in l]
    assert len(lines) == 2 and all("[S:0] [L:504] [F:0]" in l for l in lines)
    hexes = [bytes.fromhex(l.rsplit(" ", 1)[1]) for l in lines]
    assert b" -RA BR OVC005\n" in hexes[0] and b" SLP135\n" in hexes[1]
    assert [f["octets"] for f in wav_answer[0]] == hexes
