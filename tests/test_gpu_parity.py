"""Parity of the HIP path (through the C ABI of libvdl2hip.so) with the CPU oracle and with the
committed golden answers.  Frame octets, integer metadata, burst timing and per-channel counters
must be identical; float metadata within SURVEY.md 8.5's tolerances (0.05 dB, 0.01 ppm) because a
time-parallel IIR cannot reproduce the reference's rounding sequence."""
import numpy as np
import pytest

import cases
from util import assert_frames_equal, truth_is_subset

pytestmark = pytest.mark.gpu
CF = 136975000


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()          # raises if the HIP library is missing: no fallback
    return vdl2hip


def gpu_decode(vh, cfg, raw, fmt=1, chunks=None, max_block=None, seed=3, debug=None, **kw):
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, fmt, cfg.rx_max_ppm,
                     max_block_bytes=max_block or raw.size, **kw)
    for k, v in (debug or {}).items():
        rx.debug_option(k, v)
    sb = 4 if fmt == 1 else 2
    if chunks is None:
        rx.feed(raw)
    else:
        rng = np.random.default_rng(seed); k = 0
        while k < raw.size:
            m = min(raw.size - k, int(rng.integers(*chunks)) * sb)
            rx.feed(raw[k:k + m]); k += m
    fr = rx.drain()
    first = kw.get("chan_first", 0)
    cnt = [list(rx.counters(c).values()) for c in range(first, first + rx.chan_count)]
    return rx, fr, cnt


def test_reference_wav_is_a_drop_in(vh, oracle_mod, golden_wav):
    """BASELINE configs[0]: the reference's own test vector, file blocks of FILE_BUFSIZE bytes."""
    import types
    cfg = types.SimpleNamespace(centerfreq=CF, freqs=[CF], oversample=10, rx_max_ppm=0.0)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE)
    for k in range(0, golden_wav.size, 320000):        # process_iq_file(), dumpvdl2.c:353-356
        rx.feed(golden_wav[k:k + 320000])
    fr = rx.drain()
    assert [len(f["octets"]) for f in fr] == [314, 186]
    assert b" -RA BR OVC005\n" in fr[0]["octets"] and b" SLP135\n" in fr[1]["octets"]
    o = oracle_mod.Oracle(CF, [CF], oversample=10)
    o.process(golden_wav)
    assert_frames_equal(o.frames(), fr, label="wav")
    assert list(o.counters(0).values()) == list(rx.counters(0).values())
    A, B = rx.lpf(); Ao, Bo = o.lpf()
    assert A.tobytes() == Ao.tobytes() and B.tobytes() == Bo.tobytes()


@pytest.mark.parametrize("delta", [25000, -250000, 100008, -412500])
def test_reference_wav_offset_tuned(vh, oracle_mod, delta):
    """The NCO / mix branch of K1 (demod.c:58-72,200-203,312-317,385) against reference-held data: the reference's capture moved
    off-centre (tests/golden/shift_wav.py), the same expectations as tests/test_oracle_golden.py::test_reference_wav_offset_tuned,
    and the oracle beside it."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import shift_wav as sw
    from test_oracle_golden import _expect_offset_tuned
    raw = sw.shifted(delta)
    cf = sw.CHANNEL - delta
    rx = vh.Receiver(cf, [sw.CHANNEL], 10, vh.FMT_S16LE)
    for k in range(0, raw.size, 320000):
        rx.feed(raw[k:k + 320000])
    fr = rx.drain()
    step = _expect_offset_tuned(fr, delta, oracle_mod.crc16_x25)
    assert rx.nco_step(0) & 0xFFFFFFFF == step & 0xFFFFFFFF
    o = oracle_mod.Oracle(cf, [sw.CHANNEL], oversample=10)
    o.process(raw)
    assert_frames_equal(o.frames(), fr, label=f"wav shifted by {delta} Hz")
    assert list(o.counters(0).values()) == list(rx.counters(0).values())


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_golden_cases_single_feed(vh, name):
    cfg, iq, bursts, gold = cases.load(name)
    rx, fr, cnt = gpu_decode(vh, cfg, iq)
    cases.check_against_golden(fr, cnt, gold, label=name, exact_diagnostics=False)
    rx.close()


@pytest.mark.parametrize("name,chunks", [("config2_1s", (1, 3000)), ("config2_1s", (100000, 900000)),
                                         ("config4_0p4s", (20000, 200000)), ("os10_noisy_1s", (7, 20000))])
def test_chunking_does_not_change_the_answer(vh, name, chunks):
    cfg, iq, bursts, gold = cases.load(name)
    rx, fr, cnt = gpu_decode(vh, cfg, iq, chunks=chunks, max_block=4 * chunks[1])
    cases.check_against_golden(fr, cnt, gold, label=f"{name} chunks {chunks}", exact_diagnostics=False)
    rx.close()


def test_decimated_stream_close_to_reference(vh, oracle_mod):
    """K1 against the reference's sequential IIR: not bit-equal by construction (no time-parallel evaluation can repeat the
    rounding history of a sequential fp32 scan), but as close as EXACT arithmetic is - what is left is the reference's own rounding
    noise (3.2e-5 of the channel's peak, 4.4e-6 rms on this capture; dev/k1_state_basis.py).  The bounds below fail for the block
    form carried in the recursion's own basis (v[n], v[n-1]) (7.1e-5 / 7.0e-6): they guard design.h's normal-form state."""
    cfg, iq, _, _ = cases.load("config2_1s")
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample)
    D = iq.size // 2 // cfg.oversample
    tr = o.trace_all(D)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=4)
    rx, _, _ = gpu_decode(vh, cfg, iq)
    for c in range(len(cfg.freqs)):
        y = rx.read_decimated(c, 0, D)
        ref = tr[c, :len(y)]
        d = (np.asarray(y, dtype=np.float64).reshape(-1, 2) - np.asarray(ref, dtype=np.float64).reshape(-1, 2))
        peak = float(np.abs(ref).max())
        assert np.abs(d).max() <= 5e-5 * peak, f"channel {c}: {np.abs(d).max() / peak:.2e} of the peak"
        assert np.sqrt((d * d).sum(axis=1).mean()) <= 6.5e-6 * peak, f"channel {c}: rms {np.sqrt((d * d).sum(axis=1).mean()) / peak:.2e} of the peak"
        assert o.dphi(c) & 0xFFFFFF == rx.nco_step(c) & 0xFFFFFF
    rx.close()


def test_shards_reproduce_the_whole(vh):
    """chan_first/chan_count (the multi-GPU split) decode exactly the frames of the full receiver."""
    cfg, iq, _, gold = cases.load("config3_0p6s")
    parts = []
    for first, count in ((0, 20), (20, 20), (40, 24)):
        rx, fr, _ = gpu_decode(vh, cfg, iq, chan_first=first, chan_count=count)
        parts += fr
        rx.close()
    cases.check_against_golden(parts, None, gold, label="3 shards")


def test_feed_device_matches_feed_host(vh):
    import torch
    cfg, iq, _, gold = cases.load("config2_1s")
    t = torch.from_numpy(iq.copy()).cuda()
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=iq.nbytes)
    half = (iq.size // 4) * 2
    rx.feed_device(t.data_ptr(), half * 2)
    rx.feed_device(t.data_ptr() + half * 2, (iq.size - half) * 2)
    fr = rx.drain()
    cases.check_against_golden(fr, [list(rx.counters(c).values()) for c in range(len(cfg.freqs))], gold, label="device feed", exact_diagnostics=False)
    rx.close()


def test_drain_packed_equals_drain(vh):
    cfg, iq, _, gold = cases.load("config2_1s")
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=iq.nbytes)
    rx.feed(iq)
    n, recs, octs = rx.drain_packed()
    cases.check_against_golden(vh.Receiver.unpack(n, recs, octs), None, gold, label="packed")
    assert rx.drain() == []
    rx.close()


@pytest.mark.parametrize("lag", [1, 2, 3, 5])
def test_pipelined_feeds_with_drain_lag(vh, lag):
    """Streaming mode (drain lag L): L+1 blocks in flight, frames arrive L blocks late, nothing is lost or reordered."""
    cfg, iq, _, gold = cases.load("config2_1s")
    raw = iq.view(np.uint8)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=1 << 20)
    rx.set_drain_lag(lag)
    with pytest.raises(vh.Vdl2HipError):
        rx.set_drain_lag(vh.MAX_DRAIN_LAG + 1)
    got = []
    for k in range(0, raw.size, 1 << 20):
        rx.feed(raw[k:k + (1 << 20)])
        got += rx.drain()
    rx.set_drain_lag(0)
    got += rx.drain()
    cases.check_against_golden(got, [list(rx.counters(c).values()) for c in range(len(cfg.freqs))], gold, label=f"lag-{lag} streaming",
                               exact_diagnostics=False)
    ends = [f["end_sample"] for f in got]
    assert ends == sorted(ends)
    rx.close()


def test_front_stream_handle_is_usable_from_torch(vh):
    """bench.py orders the RCCL broadcast behind the channeliser through this handle."""
    import torch
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE)
    ext = torch.cuda.ExternalStream(rx.stream())
    ev = ext.record_event()
    torch.cuda.current_stream().wait_event(ev)
    torch.cuda.synchronize()
    rx.close()


def _counters_of_a_noiseless_capture(o, rx, pos, n=16):
    """All 20 counters of the tuned channel identical to the oracle's.  The other channels of these tests see the burst only as
    leakage 50 kHz and more away on a capture WITHOUT noise: they lock on it 40-60 dB down, in the quantisation noise, where which
    RS block or stuffing rule ends a doomed burst hinges on the 1e-5 by which the time-parallel filter differs from the sequential
    one - for those, what was delivered must agree (frames: compared by the caller; locks and messages: here)."""
    co = [list(o.counters(c).values()) for c in range(n)]
    cg = [list(rx.counters(c).values()) for c in range(n)]
    assert co[pos] == cg[pos]
    for c in range(n):
        assert (co[c][0], co[c][16], co[c][17]) == (cg[c][0], cg[c][16], cg[c][17]), (c, co[c], cg[c])   # demod.sync.good, decoder.msg.good, .good_loud


@pytest.mark.parametrize("delta,pos", [(0, 0), (25000, 5), (-250000, 10), (100008, 15)])
def test_reference_wav_at_2100kHz_hot_instantiation(vh, oracle_mod, delta, pos):
    """k_chanfir<20, 2, 4> - oversample 20, four channels per wavefront: the instantiation the headline number and the roofline are
    quoted on - against reference-held data: the reference's capture interpolated to 2.1 MS/s (tests/golden/resample_wav.py), as
    one of 16 channels (>= 16 channels select four per wavefront; `pos` walks the tuned channel through the wavefront's four
    slots and the workgroup's four waves).  Same expectations as tests/test_oracle_golden.py::test_reference_wav_at_2100kHz, and
    the oracle beside it on all 16 channels."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import resample_wav as rw
    from test_oracle_golden import _expect_resampled, hot_plan
    raw = rw.upsampled2x(delta)
    cf, freqs = hot_plan(delta, pos)
    rx = vh.Receiver(cf, freqs, 20, vh.FMT_S16LE, max_block_bytes=raw.size)
    assert rx.chan_count == 16
    rx.feed(raw)                                        # one block: the tile-prefetching fast path of the specialised build
    fr = rx.drain()
    step = _expect_resampled([f for f in fr if f["chan"] == pos], delta, rw.FS2, oracle_mod.crc16_x25)
    assert rx.nco_step(pos) & 0xFFFFFFFF == step & 0xFFFFFFFF
    o = oracle_mod.Oracle(cf, freqs, oversample=20)
    o.process(raw)
    assert_frames_equal(o.frames(), fr, label=f"wav at 2.1 MS/s, moved by {delta} Hz")
    _counters_of_a_noiseless_capture(o, rx, pos)
    # ... and in the reference's own block size (dumpvdl2.h:48), which takes the tiles that straddle blocks through the carry path
    rx2 = vh.Receiver(cf, freqs, 20, vh.FMT_S16LE)
    for k in range(0, raw.size, 320000):
        rx2.feed(raw[k:k + 320000])
    _expect_resampled([f for f in rx2.drain() if f["chan"] == pos], delta, rw.FS2, oracle_mod.crc16_x25)
    rx.close(); rx2.close()


def test_reference_wav_as_u8(vh, oracle_mod):
    """process_buf_uchar()'s path (demod.c:339-354) against reference-held data: the reference's capture re-quantised to u8
    (tests/golden/resample_wav.py) at 1.05 MS/s on the centre, and interpolated to 2.1 MS/s off the centre as one of 16 channels
    (k_chanfir<20, 2, 4> reading u8)."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import resample_wav as rw
    from test_oracle_golden import _expect_resampled, hot_plan
    pw = -9.841 + rw.U8_GAIN_DB
    raw = rw.as_u8()
    rx = vh.Receiver(rw.CHANNEL, [rw.CHANNEL], 10, vh.FMT_U8)
    for k in range(0, raw.size, 160000):
        rx.feed(raw[k:k + 160000])
    fr = rx.drain()
    _expect_resampled(fr, 0, rw.FS, oracle_mod.crc16_x25, pwr_db=pw)
    o = oracle_mod.Oracle(rw.CHANNEL, [rw.CHANNEL], oversample=10, sample_fmt=oracle_mod.FMT_U8)
    o.process(raw)
    assert_frames_equal(o.frames(), fr, label="wav as u8")
    assert list(o.counters(0).values()) == list(rx.counters(0).values())
    d, pos = 25000, 6
    raw = rw.as_u8(rw.upsampled2x(d))
    cf, freqs = hot_plan(d, pos)
    rx2 = vh.Receiver(cf, freqs, 20, vh.FMT_U8, max_block_bytes=raw.size)
    rx2.feed(raw)
    fr = rx2.drain()
    _expect_resampled([f for f in fr if f["chan"] == pos], d, rw.FS2, oracle_mod.crc16_x25, pwr_db=pw)
    o = oracle_mod.Oracle(cf, freqs, oversample=20, sample_fmt=oracle_mod.FMT_U8)
    o.process(raw)
    assert_frames_equal(o.frames(), fr, label="wav as u8 at 2.1 MS/s")
    _counters_of_a_noiseless_capture(o, rx2, pos)
    rx.close(); rx2.close()


def test_uint8_input(vh, oracle_mod):
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(centerfreq=CF, freqs=[CF, CF + 40000], oversample=10, duration_s=0.6, seed=12, amplitude=0.3, noise_sigma=0.01)
    iq8, _ = synth.synthesize(cfg, dtype=np.uint8)
    o = oracle_mod.Oracle(CF, list(cfg.freqs), oversample=10, sample_fmt=oracle_mod.FMT_U8)
    o.process(iq8)
    rx, fr, cnt = gpu_decode(vh, cfg, iq8, fmt=0, chunks=(11, 50000), max_block=200000)
    assert_frames_equal(o.frames(), fr, label="u8")
    assert cnt == [list(o.counters(c).values()) for c in range(2)]


@pytest.mark.parametrize("os_", [20, 10])
def test_uint8_input_many_channels(vh, oracle_mod, os_):
    """The channeliser's unsigned-byte build (four channels per wavefront, tiles fetched a tile ahead, conversion without the division:
    oversampling 20 and 10, the reference's --iq-file default): 64 channels of a u8 capture, 1.5 s in pieces from a few samples to
    1.5 M, against the oracle fed the same bytes (process_buf_uchar, src/demod.c:339-354)."""
    from dumpvdl2_amd import synth
    import os
    cfg = synth.SynthConfig(centerfreq=CF, freqs=synth.channel_plan(64, CF, 25000 if os_ == 20 else 12000), oversample=os_, duration_s=1.5, seed=77 + os_,
                            amplitude=0.2, noise_sigma=0.01, tdm_slots=4, tdm_slot_s=0.2, rx_max_ppm=5.0)
    iq8, bursts = synth.synthesize(cfg, dtype=np.uint8)
    o = oracle_mod.Oracle(CF, list(cfg.freqs), oversample=os_, sample_fmt=oracle_mod.FMT_U8, max_ppm=cfg.rx_max_ppm)
    o.process(iq8, block_bytes=1 << 22, nthreads=min(64, os.cpu_count() or 8))
    fo = o.frames()
    rx, fr, cnt = gpu_decode(vh, cfg, iq8, fmt=0, chunks=(11, 1_500_000), max_block=4_000_000)
    assert len(fo) > 40
    assert_frames_equal(fo, fr, label=f"u8 x 64, os {os_}")
    cases.assert_counters_equal(cnt, [list(o.counters(c).values()) for c in range(64)], f"u8 x 64, os {os_}", exact_diagnostics=False)
    rx.close()


@pytest.mark.parametrize("os_", [13, 16, 7])
def test_other_oversampling_factors(vh, oracle_mod, os_):
    """13 = Mirics rate (specialised build), 16 and 7 go through the generic-oversample build."""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(centerfreq=CF, freqs=[CF + 30000, CF - 60000], oversample=os_, duration_s=0.7, seed=40 + os_)
    iq, bursts = synth.synthesize(cfg)
    o = oracle_mod.Oracle(CF, list(cfg.freqs), oversample=os_)
    o.process(iq.view(np.uint8))
    want = o.frames()
    rx, fr, cnt = gpu_decode(vh, cfg, iq, chunks=(1000, 100000), max_block=400000)
    assert len(fr) > 0
    assert_frames_equal(want, fr, label=f"os{os_}")
    assert cnt == [list(o.counters(c).values()) for c in range(2)]
    rx.close()


def test_full_size_config2_properties(vh, oracle_mod):
    """BASELINE configs[1] at full size (16 s, 8 channels): properties that need no oracle run -
    every transmitted frame comes back on its channel, decoding is deterministic, and feeding the
    stream in 7 pieces gives the same frames as feeding it at once - plus the oracle on the whole
    16 s of the very same bytes."""
    from dumpvdl2_amd import workloads, synth
    cfg = workloads.config2(16.0)
    iq, bursts = synth.synthesize(cfg)
    rx, fr, cnt = gpu_decode(vh, cfg, iq)
    assert truth_is_subset(bursts, fr) == 0
    assert len(fr) == sum(len(b.frames) for b in bursts if b.decodable)
    rx2, fr2, cnt2 = gpu_decode(vh, cfg, iq, chunks=(3_000_000, 6_000_000), max_block=24_000_000)
    key = lambda f: (f["chan"], f["burst_ord"], f["idx"])
    assert [(key(f), f["octets"], f["sync_sample"], f["num_fec_corrections"]) for f in sorted(fr, key=key)] == \
           [(key(f), f["octets"], f["sync_sample"], f["num_fec_corrections"]) for f in sorted(fr2, key=key)]
    assert cnt == cnt2
    # the oracle over the whole 16 s of the very same bytes: frames, timing and every counter
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=20)
    o.process(iq.view(np.uint8), block_bytes=320000, nthreads=8)
    assert_frames_equal(o.frames(), fr, label="16 s vs oracle")
    assert [list(o.counters(c).values()) for c in range(len(cfg.freqs))] == cnt


def test_dropin_adapter_with_reference_main_sequence(vh, oracle_mod, golden_wav, tmp_path):
    """The reference-named entry points (include/vdl2hip_dropin.h) driven by a stand-in for the
    unmodified dumpvdl2 main(): same call sequence, barriers and thread-per-channel as src/dumpvdl2.c;
    the frames arriving at avlc_decoder_queue_push() must be the oracle's."""
    import os, subprocess
    from dumpvdl2_amd import build
    exe = build.build_harness(str(tmp_path / "dropin_harness"))
    wav = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "vdl2_model_16b_1050kHz.wav")
    out = subprocess.run([exe, wav, "10", str(CF), str(CF)], check=True, capture_output=True, text=True, timeout=120).stdout
    lines = [l for l in out.splitlines() if l.startswith("FRAME")]
    o = oracle_mod.Oracle(CF, [CF], oversample=10)
    o.process(golden_wav)
    ref = o.frames()
    assert len(lines) == len(ref) == 2
    for l, f in zip(lines, ref):
        kv = dict(t.split("=", 1) for t in l.split()[1:])
        assert bytes.fromhex(kv["octets"]) == f["octets"]
        assert (int(kv["idx"]), int(kv["S"]), int(kv["L"]), int(kv["F"]), int(kv["freq"])) == (f["idx"], f["synd_weight"], f["datalen_octets"], f["num_fec_corrections"], CF)
        assert abs(float(kv["pwr"]) - f["frame_pwr_dbfs"]) < 0.05 and abs(float(kv["nf"]) - f["nf_pwr_dbfs"]) < 0.05
        assert kv["station"] == "HARNESS" and kv["flags"] == "0"


@pytest.mark.parametrize("which,secs", [("config3", 4.0), ("config4", 3.0), ("config5", 3.0)])
def test_many_channel_configs_vs_oracle(vh, oracle_mod, which, secs):
    """BASELINE configs[2..4] (64 / 256 channels, cross-talk + --max-ppm gate, injected RS errors) at a few
    seconds each: the oracle runs on the same bytes on the box's host cores; frames, timing, integer metadata and
    the reference's counters must be identical, and every decodable transmitted frame must be present."""
    import os
    from dumpvdl2_amd import workloads, synth
    cfg = getattr(workloads, which)(secs)
    iq, bursts = synth.synthesize(cfg)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=20, max_ppm=cfg.rx_max_ppm)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=min(len(cfg.freqs), os.cpu_count() or 8))
    fo = o.frames()
    rx, fg, cnt = gpu_decode(vh, cfg, iq, chunks=(2_000_000, 4_000_000), max_block=16_000_000)
    assert len(fo) > 100
    assert_frames_equal(fo, fg, label=which)
    cases.assert_counters_equal(cnt, [list(o.counters(c).values()) for c in range(len(cfg.freqs))], which, exact_diagnostics=False)
    assert truth_is_subset(bursts, fg) == 0
    if which == "config5":
        assert sum(f["num_fec_corrections"] for f in fg) > 100          # the FEC-heavy path really ran
        tot = [sum(c[i] for c in cnt) for i in range(20)]
        assert tot[10] > 5                                               # decoder.errors.fec_bad: over-capacity blocks dropped by both
    rx.close()


@pytest.mark.parametrize("pieces", ["blocks", "collected", "long"])
def test_weak_bursts_without_the_ppm_gate(vh, oracle_mod, pieces):
    """config4 WITHOUT its --max-ppm gate (the reference's default, demod.c:190-192): idle channels lock on to what leaks over from
    neighbours 8 kHz away and decode it - hundreds of weak bursts a second, a symbol in a few hundred within the referee's margin:
    40 listed stretches per 320 000-byte block where the gated workload has one.  The burst decoder lists such bursts, the
    stretches are scanned side by side and a second pass decodes them (vdl2hip.hip: launch_rest) - in short feeds too since round
    6c (`blocks`: the reference's own block size, every block a short feed), in the adapter's collected blocks (16 per feed) and in
    long pieces.  Frames, timing and the 18 counters identical to the oracle's; and the lists hold: almost nothing is scanned by a
    burst's own wavefront (a stretch costs 4.4 ms there)."""
    import dataclasses, os
    from dumpvdl2_amd import workloads, synth
    cfg = dataclasses.replace(workloads.config4(1.5), rx_max_ppm=0.0)
    iq, bursts = synth.synthesize(cfg)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=20, max_ppm=0.0)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=min(len(cfg.freqs), os.cpu_count() or 8))
    fo = o.frames()
    chunks = {"blocks": (80_000, 80_001), "collected": (1_280_000, 1_280_001), "long": (2_000_000, 4_000_000)}[pieces]
    rx, fg, cnt = gpu_decode(vh, cfg, iq, chunks=chunks, max_block=16_000_000)
    assert len(fo) > 300
    assert_frames_equal(fo, fg, label=f"no gate, {pieces}")
    cases.assert_counters_equal(cnt, [list(o.counters(c).values()) for c in range(len(cfg.freqs))], f"no gate, {pieces}", exact_diagnostics=False)
    st = rx.stats()
    assert st["referee_refused"] == 0 and st["referee_symbol_scans"] > 200, st
    rx.close()


@pytest.mark.parametrize("mode", ["plain", "again", "straddle_again", "straddle_mismatch"])
@pytest.mark.parametrize("which,secs,chunks", [("config4", 3.0, (1_100_000, 1_500_000)), ("config3", 4.0, (700_000, 4_000_000)), ("config3", 3.0, (30_000, 1_500_000))])
def test_walk_ahead_chosen_feed_by_feed(vh, oracle_mod, which, secs, chunks, mode):
    """Whether the next feed's walk goes ahead of a feed's check is decided per feed from its channel-samples (vdl2hip.hip:
    walk_ahead_of): a 256-channel receiver fed a second or so at a time - the drop-in adapter's collected blocks - walks ahead
    like a rank-sized one does on 16 s blocks.  `plain`: the library's own choice on pieces of 1.1-1.5 M samples (256 channels) /
    0.7-4 M (64), and 30 000-1.5 M (64: short feeds - unsegmented, everything on the front stream - between the long ones);
    `again`: the hook that flags every channel of every feed, so every second walk runs and is compared with what
    the next feed started from; `straddle_*`: the threshold moved into the range of the pieces (debug option walk_ahead_below), so
    feeds that let the next walk go ahead and feeds that do not alternate in one stream - with every channel walked again, and
    with every comparison forced to fail (every channel of the following feed stitched once more).  Frames, burst timing and the
    reference's 18 counters identical to the oracle's (src/demod.c:173-286, src/decode.c:204-373)."""
    import os
    from dumpvdl2_amd import workloads, synth
    cfg = getattr(workloads, which)(secs)
    iq, bursts = synth.synthesize(cfg)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=20, max_ppm=cfg.rx_max_ppm)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=min(len(cfg.freqs), os.cpu_count() or 8))
    fo = o.frames()
    dbg = {}
    if mode != "plain": dbg["force_again"] = 1
    if mode.startswith("straddle"): dbg["walk_ahead_below"] = len(cfg.freqs) * ((chunks[0] + chunks[1]) // 2 // 20)
    if mode.endswith("mismatch"): dbg["force_mismatch"] = 1
    rx, fg, cnt = gpu_decode(vh, cfg, iq, chunks=chunks, max_block=16_000_000, debug=dbg)
    assert len(fo) > 100
    assert_frames_equal(fo, fg, label=f"{which} {mode}")
    cases.assert_counters_equal(cnt, [list(o.counters(c).values()) for c in range(len(cfg.freqs))], f"{which} {mode}", exact_diagnostics=False)
    st = rx.stats()
    assert st["referee_refused"] == 0
    if mode != "plain": assert st["referee_rewalks"] >= len(cfg.freqs)
    rx.close()


@pytest.mark.parametrize("mode", ["ahead", "ahead_mismatch", "serial"])
@pytest.mark.parametrize("which,secs,chunks", [("config3", 4.0, (2_000_000, 4_000_000)), ("config4", 3.0, (2_000_000, 4_000_000)),
                                               ("config3", 2.0, (700_000, 1_500_000))])
def test_every_channel_walked_again_beside_the_previous_feeds_burst_decoder(vh, oracle_mod, which, secs, chunks, mode):
    """Round 5's red test, made certain instead of likely: the test hook `force_again` makes the referee's check flag EVERY channel of
    every long feed, so every channel's walker state and counters go back to the feed's snapshot and the feed is stitched a second
    time - while the burst decoder of the feed before still adds its own counters (decoder.blocks.*, decoder.msg.*, decoder.errors.*)
    on its burst stream.  Several long feeds in flight, drained once at the end.  The walker may only put back what it owns
    (demod.sync.good, the header outcomes, ppm_reject): frames AND the reference's 18 counters identical to the oracle's on every
    channel (src/decode.c:204-373).  (0.7-1.5 M-sample pieces: two to four walk segments per feed and a front of a fraction of a
    millisecond, so the walks run as far ahead of the burst decoders as the slots allow.)

    Round 6: a feed's walk no longer waits for the check of the feed before (vdl2hip.hip: launch_back / launch_rest).  `ahead`: the
    product - every second walk runs after the next feed's first walk and must find that it ended where that walk started;
    `ahead_mismatch`: the hook `force_mismatch` makes every such comparison fail, so every channel of every following feed is stitched
    once more from the "corrected" snapshot - the path a real misprediction takes; `serial`: round 5's schedule (walk, check, walk
    again, then the next feed's walk)."""
    import os
    from dumpvdl2_amd import workloads, synth
    cfg = getattr(workloads, which)(secs)
    iq, bursts = synth.synthesize(cfg)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=20, max_ppm=cfg.rx_max_ppm)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=min(len(cfg.freqs), os.cpu_count() or 8))
    fo = o.frames()
    dbg = {"force_again": 1, "walk_ahead": 0 if mode == "serial" else 1, "force_mismatch": 1 if mode.endswith("_mismatch") else 0}
    rx, fg, cnt = gpu_decode(vh, cfg, iq, chunks=chunks, max_block=16_000_000, debug=dbg)
    s = rx.stats()
    assert s["feeds"] >= 2 and s["referee_rewalks"] >= (s["feeds"] - 1) * len(cfg.freqs), s      # every channel, every long feed
    if mode.endswith("_mismatch"):
        assert s["referee_redone_next"] >= (s["feeds"] - 3) * len(cfg.freqs), s
    elif mode.startswith("ahead"):
        # (a second walk ends where the first did unless a decision really fell, or the burst in progress at the feed's end carries a
        # slope that the second walk knows to be the reference's own and the first did not: a few channels, not all of them)
        assert s["referee_redone_next"] <= s["referee_rewalks"] // 8, s
    assert len(fo) > 100
    assert_frames_equal(fo, fg, label=which)
    cases.assert_counters_equal(cnt, [list(o.counters(c).values()) for c in range(len(cfg.freqs))], which, exact_diagnostics=False)
    rx.close()


def test_burst_dense_block_vs_oracle(vh, oracle_mod):
    """The lock-dense secondary workload of bench.py (config4_bursty: 4x the bursts and ~4.6x the gate-dropped locks of config4) at 3 s
    against the oracle on all 256 channels: frames, timing and integer metadata identical, the reference's 18 counters identical on
    every channel (the referee, DESIGN 5: no tie allowances, no bookkeeping exception)."""
    import os
    from dumpvdl2_amd import workloads, synth
    from util import compare_reference_counters, compare_at_full_size
    cfg = workloads.config4_bursty(3.0)
    iq, bursts = synth.synthesize(cfg)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=20, max_ppm=cfg.rx_max_ppm)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=min(len(cfg.freqs), os.cpu_count() or 8))
    fo = o.frames()
    rx, fg, cnt = gpu_decode(vh, cfg, iq, chunks=(2_000_000, 4_000_000), max_block=16_000_000)
    assert len(fo) > 1500 and truth_is_subset(bursts, fg) == 0
    cmp = compare_at_full_size(fo, fg, label="config4_bursty 3 s")
    names = list(o.counters(0).keys())
    co = [list(o.counters(c).values()) for c in range(len(cfg.freqs))]
    which, nbad = compare_reference_counters(names, co, cnt, label="config4_bursty 3 s", strict=True)
    assert cmp["timing_ties"] == 0 and cmp["nf_update_ties"] == 0 and nbad == 0
    assert sum(c[18] for c in co) > 10000                                # demod.ppm_reject: the gate really is busy
    s = rx.stats()
    assert s["referee_scans"] > 0 and s["referee_refused"] == 0, s
    print("config4_bursty 3 s:", cmp, "referee:", {k: v for k, v in s.items() if k.startswith("referee_")})
    rx.close()


def test_cli_runner_and_raw_frame_archive(vh, oracle_mod, golden_wav, tmp_path):
    """tools/vdl2hip_iqfile with the reference CI's own arguments (.github/workflows/build.yml:16-18):
    --iq-file test/vdl2_model_16b_1050kHz.wav --sample-format S16_LE.  The two messages must appear, and the
    raw-frame archive it writes must parse back (2-byte BE length + proto3 raw_avlc_frame) to the same octets."""
    import os, struct, subprocess
    from dumpvdl2_amd import build
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    wav = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "vdl2_model_16b_1050kHz.wav")
    raw = str(tmp_path / "frames.bin"); statsd = str(tmp_path / "statsd.txt")
    p = subprocess.run([exe, "--iq-file", wav, "--sample-format", "S16_LE", "--station-id", "TEST", "--raw-frames-out", raw,
                        "--avlc-filter", "--statsd-out", statsd], check=True, capture_output=True, text=True, timeout=120)
    table = dict(l.rsplit(":", 1) for l in open(statsd).read().splitlines())
    assert table[f"dumpvdl2.TEST.{CF}.decoder.msg.good"] == "2|c" and table[f"dumpvdl2.TEST.{CF}.avlc.frames.good"] == "2|c"
    assert table[f"dumpvdl2.TEST.{CF}.demod.sync.good"] == "1|c" and table[f"dumpvdl2.TEST.{CF}.avlc.errors.bad_fcs"] == "0|c"
    lines = [l for l in p.stdout.splitlines() if "[S:" in l]
    assert len(lines) == 2 and all("[S:0] [L:504] [F:0]" in l for l in lines)
    hexes = [bytes.fromhex(l.rsplit(" ", 1)[1]) for l in lines]
    assert b" -RA BR OVC005\n" in hexes[0] and b" SLP135\n" in hexes[1]
    o = oracle_mod.Oracle(CF, [CF], oversample=10)
    o.process(golden_wav)
    assert [f["octets"] for f in o.frames()] == hexes
    import test_rawframe_format as trf
    RawFrame = trf.build_schema()
    blob = open(raw, "rb").read()
    off, got = 0, []
    while off < len(blob):
        (ln,) = struct.unpack(">H", blob[off:off + 2])
        m = RawFrame(); m.ParseFromString(blob[off + 2:off + ln]); got.append(m); off += ln
    assert [m.data for m in got] == hexes
    assert all(m.metadata.station_id == "TEST" and m.metadata.frequency == CF and m.metadata.datalen_octets == 504 for m in got)


def test_degenerate_feeds_and_errors(vh, golden_wav):
    """Empty, sub-sample and tiny feeds; oversized blocks; bad channel numbers: same answers, clean errors."""
    import ctypes as C
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=400000)
    ref = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=golden_wav.size)
    ref.feed(golden_wav[:golden_wav.size - golden_wav.size % 4])
    want = ref.drain()
    rng = np.random.default_rng(0)
    k = 0
    wav = golden_wav[:golden_wav.size - golden_wav.size % 4]
    rx.feed(wav[:0])                                            # len == 0 is a no-op (demod.c:341,358)
    while k < wav.size:
        m = int(rng.choice([4, 8, 36, 40, 44, 4000, 200000, 399996]))
        m = min(m, wav.size - k)
        rx.feed(wav[k:k + m]); k += m
        if rng.random() < 0.3:
            rx.sync()
    got = rx.drain()
    assert_frames_equal(want, got, label="tiny feeds")
    assert list(ref.counters(0).values()) == list(rx.counters(0).values())
    with pytest.raises(vh.Vdl2HipError, match="max_block_bytes"):
        rx.feed(np.zeros(400004, dtype=np.uint8))
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):
        rx.counters(1)
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):
        vh.Receiver(CF, [CF, CF + 25000], 10, vh.FMT_S16LE, chan_first=1, chan_count=2)
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):
        vh.Receiver(CF, [CF], 33, vh.FMT_S16LE)
    rx.close(); ref.close()


def test_silence_and_decaying_tails(vh, oracle_mod):
    """Exact zeros in the input: the filter output decays through the denormal range to exact zero, where the screening
    tier's phase (v_rcp of a denormal, 0 * inf) has to stay harmless - a zero sample has phase 0, a sample too small for
    v_rcp flags its windows for the exact tier.  A capture with stretches of silence cut into it, one that ends in silence,
    and pure silence: same frames, counters and timing as the oracle."""
    cfg, iq, bursts, _ = cases.load("config2_1s")
    x = cases.with_silence(cfg, iq, bursts)
    for raw, label in ((x.reshape(-1), "silence cut in"), (np.zeros(600000, dtype=np.int16), "pure silence")):
        o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
        o.process(raw.view(np.uint8), block_bytes=1 << 22, nthreads=4)
        rx, fr, cnt = gpu_decode(vh, cfg, raw, chunks=(30000, 400000), max_block=1600000)
        assert_frames_equal(o.frames(), fr, label=label)
        assert cnt == [list(o.counters(c).values()) for c in range(len(cfg.freqs))]
        rx.close()
    assert len(fr) == 0                                    # pure silence decodes to nothing


def test_two_receivers_in_one_process(vh, oracle_mod, golden_wav):
    """Contexts are independent (different oversampling, formats, channel counts) and can interleave their feeds."""
    cfg, iq, _, gold = cases.load("config2_1s")
    a = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=320000)
    b = vh.Receiver(cfg.centerfreq, list(cfg.freqs), 20, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=1 << 21)
    raw_b = iq.view(np.uint8)
    ka = kb = 0
    while ka < golden_wav.size or kb < raw_b.size:
        if ka < golden_wav.size:
            a.feed(golden_wav[ka:ka + 320000]); ka += 320000
        if kb < raw_b.size:
            b.feed(raw_b[kb:kb + (1 << 21)]); kb += 1 << 21
    fa, fb = a.drain(), b.drain()
    assert [len(f["octets"]) for f in fa] == [314, 186]
    cases.check_against_golden(fb, [list(b.counters(c).values()) for c in range(8)], gold, label="interleaved", exact_diagnostics=False)
    a.close(); b.close()


@pytest.mark.parametrize("name,seg_min,seg_max", [("config2_1s", 700, 32), ("config2_1s", 3000, 32), ("dirty25k_1s", 1000, 32),
                                                  ("config4_0p4s", 2000, 7), ("config5_0p4s", 400, 32), ("os10_noisy_1s", 500, 32),
                                                  ("config2_1s", 16384, 1)])
def test_segmented_walk_is_exact(vh, monkeypatch, name, seg_min, seg_max):
    """K4 in speculative segments (k_walk_spec / k_walk_stitch): whatever the segment length - down to a fraction of a
    burst, so that most boundaries fall inside one - the frames, counters and metadata are those of the sequential walk
    (the golden fixtures); seg_max = 1 is the sequential kernel itself."""
    monkeypatch.setenv("VDL2HIP_SEG_MIN", str(seg_min)); monkeypatch.setenv("VDL2HIP_SEG_MAX", str(seg_max))
    cfg, iq, bursts, gold = cases.load(name)
    rx, fr, cnt = gpu_decode(vh, cfg, iq)
    st = rx.stats()
    cases.check_against_golden(fr, cnt, gold, label=f"{name} seg {seg_min}x{seg_max}", exact_diagnostics=False)
    if seg_max > 1:
        assert st["seg_adopted"] > 0
        assert st["seg_adopted"] + st["seg_walked"] >= len(cfg.freqs)
    else:
        assert st["seg_adopted"] == st["seg_walked"] == 0
    rx.close()


def test_avlc_front_door_on_device(vh, oracle_mod, golden_wav):
    """SURVEY 8.7 rows 3+4: FCS / minimum length / link addresses per frame and the avlc.* counters, computed on the
    device (k_frame_finish), against the oracle's restatement of src/avlc.c:163-236; the optional filter; the statsd lines."""
    cfg, iq, _, gold = cases.load("config5_0p4s")
    nch = len(cfg.freqs)
    rx, fr, cnt = gpu_decode(vh, cfg, iq)
    assert len(fr) > 50
    for f in fr:
        st, dst, src, _ = oracle_mod.avlc_screen(f["octets"])
        assert (f["avlc_status"], f["dst_addr"], f["src_addr"]) == (st, dst, src)
    want = oracle_mod.avlc_counters(fr, nch)
    got = [list(rx.avlc_counters(c).values()) for c in range(nch)]
    assert got == want
    # statsd: first call announces every counter (statsd_initialize_counters_per_channel), deltas afterwards
    lines = rx.statsd_lines("dumpvdl2.TEST")
    assert len(lines) == nch * (vh.NUM_COUNTERS + vh.NUM_AVLC_COUNTERS)
    table = dict(l.rsplit(":", 1) for l in lines)
    for c in range(nch):
        for k, v in {**rx.counters(c), **rx.avlc_counters(c)}.items():
            assert table[f"dumpvdl2.TEST.{cfg.freqs[c]}.{k}"] == f"{v}|c"
    assert rx.statsd_lines("dumpvdl2.TEST") == []               # nothing changed since
    rx.close()

    # the reference's own vector: both frames pass; with the filter on, a corrupted frame would not be delivered
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=golden_wav.size)
    rx.set_avlc_filter(True)
    rx.feed(golden_wav[:golden_wav.size - golden_wav.size % 4])
    fr = rx.drain()
    assert [f["avlc_status"] for f in fr] == [0, 0] and [len(f["octets"]) for f in fr] == [314, 186]
    assert list(rx.avlc_counters(0).values())[:4] == [2, 0, 2, 0]
    assert sum(list(rx.avlc_counters(0).values())[4:]) == 2
    rx.close()


def test_avlc_filter_drops_what_avlc_parse_drops(vh, oracle_mod):
    """Bursts whose payload is not a valid AVLC frame (no FCS, short frames) still decode (decoder.msg.good), but
    avlc_parse() returns NULL for them: with the filter on they are counted and not delivered."""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(freqs=synth.channel_plan(2, spacing=100000), duration_s=1.5, mean_gap_s=0.05, max_payload=300,
                            invalid_frame_rate=0.4, seed=77)
    iq, bursts = synth.synthesize(cfg)
    rx_all, fr_all, _ = gpu_decode(vh, cfg, iq)
    status = [oracle_mod.avlc_screen(f["octets"])[0] for f in fr_all]
    assert status.count(1) >= 3 and status.count(2) >= 3 and status.count(0) >= 3
    assert [f["avlc_status"] for f in fr_all] == status
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=iq.nbytes)
    rx.set_avlc_filter(True)
    rx.feed(iq.view(np.uint8))
    fr = rx.drain()
    assert len(fr) == status.count(0) and all(f["avlc_status"] == 0 for f in fr)
    key = lambda f: (f["chan"], f["burst_ord"], f["idx"])
    assert sorted(map(key, fr)) == sorted(key(f) for f, st in zip(fr_all, status) if st == 0)
    tot = [sum(rx.avlc_counters(c)[k] for c in range(len(cfg.freqs))) for k in ("avlc.frames.processed", "avlc.errors.too_short", "avlc.errors.bad_fcs", "avlc.frames.good")]
    assert tot == [len(fr_all), status.count(1), status.count(2), status.count(0)]
    rx.close(); rx_all.close()


def test_ring_wraps_many_times(vh, oracle_mod):
    """Small blocks make the per-channel history ring small (2^17 samples here): over 5 s of signal it wraps 4 times, with
    bursts, speculative segments and noise-floor look-backs straddling the wrap.  Same frames as the oracle."""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(freqs=synth.channel_plan(3, spacing=100000), duration_s=5.0, mean_gap_s=0.08, max_payload=600, seed=4242)
    iq, bursts = synth.synthesize(cfg)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=3)
    raw = iq.view(np.uint8)
    blk = 1600000                                                   # 400 000 samples = 20 000 decimated per feed
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, max_block_bytes=blk)
    rx.set_drain_lag(2)
    got = []
    for k in range(0, raw.size, blk):
        rx.feed(raw[k:k + blk])
        got += rx.drain()
    rx.set_drain_lag(0)
    got += rx.drain()
    assert 5 * 105000 > 4 * (1 << 17)
    assert_frames_equal(o.frames(), got, label="ring wrap")
    cases.assert_counters_equal([list(rx.counters(c).values()) for c in range(3)], [list(o.counters(c).values()) for c in range(3)],
                                label="ring wrap", exact_diagnostics=False)
    assert len(got) >= 60
    rx.close()


@pytest.mark.parametrize("name", ["config2_1s", "os10_noisy_1s", "config4_0p4s"])
def test_separate_fixup_kernel_gives_the_same_answer(vh, name):
    """By default K1 applies the segment-start fix-up itself (one-step look-back between workgroup segments); the test hook
    "no_fuse" runs the separate kernel k_fixup instead.  Same arithmetic, so the decimated samples are bit-identical
    and so is everything after them; and no look-back wait ever times out."""
    cfg, iq, bursts, gold = cases.load(name)
    rx, fr, cnt = gpu_decode(vh, cfg, iq, chunks=(50000, 400000), max_block=1600000)
    assert rx.stats()["front_sync_timeouts"] == 0
    D = iq.size // 2 // cfg.oversample
    y_fused = [rx.read_decimated(c, max(0, D - 60000), 60000) for c in range(len(cfg.freqs))]
    rx2, fr2, cnt2 = gpu_decode(vh, cfg, iq, chunks=(50000, 400000), max_block=1600000, debug={"no_fuse": 1})
    y_sep = [rx2.read_decimated(c, max(0, D - 60000), 60000) for c in range(len(cfg.freqs))]
    for a, b in zip(y_fused, y_sep):
        assert a.tobytes() == b.tobytes()
    key = lambda f: (f["chan"], f["burst_ord"], f["idx"])
    assert [(key(f), f["octets"], f["sync_sample"], f["ppm_error"], f["frame_pwr_dbfs"], f["nf_pwr_dbfs"]) for f in sorted(fr, key=key)] == \
           [(key(f), f["octets"], f["sync_sample"], f["ppm_error"], f["frame_pwr_dbfs"], f["nf_pwr_dbfs"]) for f in sorted(fr2, key=key)]
    assert cnt == cnt2
    cases.check_against_golden(fr2, cnt2, gold, label=f"{name} separate K2", exact_diagnostics=False)
    rx.close(); rx2.close()


@pytest.mark.parametrize("name", ["config2_1s", "os10_noisy_1s", "config4_0p4s", "config5_0p4s"])
def test_with_and_without_the_referee_on_the_golden_captures(vh, name):
    """The golden captures hold no decision within the margin of the channeliser's distance from the reference's scan that comes out
    differently (they are compared with the committed oracle answers elsewhere): with the referee (the default) and without it
    (test hook "referee" = 0) frames, timing, integer metadata and counters are the same, for whole and for chunked feeds; the floats
    within SURVEY 8.5 (a stretch the referee has made exact carries the reference's own samples, the rest the channeliser's)."""
    cfg, iq, bursts, gold = cases.load(name)
    key = lambda f: (f["chan"], f["burst_ord"], f["idx"])
    out, flt = [], []
    for dbg in ({"referee": 0}, {"referee": 1}):
        for kw in ({}, dict(chunks=(3000, 200000), max_block=800000)):
            rx, fr, cnt = gpu_decode(vh, cfg, iq, debug=dbg, **kw)
            out.append(([(key(f), f["octets"], f["sync_sample"], f["end_sample"], f["synd_weight"], f["num_fec_corrections"]) for f in sorted(fr, key=key)], [c[:18] for c in cnt]))
            flt.append([(f["ppm_error"], f["frame_pwr_dbfs"], f["nf_pwr_dbfs"]) for f in sorted(fr, key=key)])
            cases.check_against_golden(fr, cnt, gold, label=f"{name} {dbg} {kw}", exact_diagnostics=False)
            rx.close()
    assert out[0] == out[1] == out[2] == out[3]
    for a, b in zip(flt[0], flt[2]):
        assert abs(a[0] - b[0]) <= 0.01 and abs(a[1] - b[1]) <= 0.05 and abs(a[2] - b[2]) <= 0.05


@pytest.mark.parametrize("name,prescan", [("config2_1s", 0), ("config2_1s", 1), ("dirty25k_1s", 0), ("config4_0p4s", 1), ("config5_0p4s", 1), ("config3_0p6s", 0)])
def test_referee_scans_ahead_of_or_behind_the_walk(vh, monkeypatch, name, prescan):
    """The library puts the referee's scans ahead of the walk for receivers of <= 64 channels and behind it (note, scan, check, walk
    again) for larger ones (vdl2hip_create).  Here each golden capture runs in the mode that is NOT its default
    (VDL2HIP_REF_PRESCAN): golden frames, timing, integer metadata and counters, whole and in pieces long enough for segmented walks
    with several feeds in flight."""
    monkeypatch.setenv("VDL2HIP_REF_PRESCAN", str(prescan))
    cfg, iq, bursts, gold = cases.load(name)
    for kw in ({}, dict(chunks=(700_000, 1_200_000), max_block=4_800_000)):
        rx, fr, cnt = gpu_decode(vh, cfg, iq, **kw)
        cases.check_against_golden(fr, cnt, gold, label=f"{name} prescan={prescan} {kw}", exact_diagnostics=False)
        s = rx.stats()
        assert s["referee_refused"] == 0, s
        rx.close()


@pytest.mark.parametrize("name", ["config2_1s", "config4_0p4s"])
def test_deferred_back_end_gives_the_same_answer(vh, name):
    """Golden frames, timing and counters on 1 MiB feeds drained after every feed, with three blocks in flight and with one.  (The name
    is from when this ran a second placement of the back end, behind the next feed's channeliser - DESIGN 8: measured, lost, removed;
    what it checks besides is kept under the same id: every feed's back end is queued with the feed, and whoever collects a feed first
    flushes what still waits for a successor's walk.)"""
    cfg, iq, _, gold = cases.load(name)
    raw = iq.view(np.uint8)
    for lag in (2, 0):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=1 << 20)
        rx.set_drain_lag(lag)
        got = []
        for k in range(0, raw.size, 1 << 20):
            rx.feed(raw[k:k + (1 << 20)])
            got += rx.drain()
        rx.set_drain_lag(0)
        got += rx.drain()
        cases.check_against_golden(got, [list(rx.counters(c).values()) for c in range(len(cfg.freqs))], gold, label=f"1 MiB feeds, lag {lag}",
                                   exact_diagnostics=False)
        rx.close()


def test_pinned_feed_overlaps_and_matches(vh):
    """vdl2hip_feed_pinned(): blocks queued from two alternating page-locked buffers without waiting for the copies give
    the golden answers; so does the blocking vdl2hip_feed() from pageable memory with three blocks in flight (the copy of
    block i+1 runs on the copy stream beside the kernels of block i)."""
    import torch
    cfg, iq, _, gold = cases.load("config2_1s")
    raw = torch.from_numpy(iq.copy()).view(torch.uint8)
    blk = 1 << 20
    pins = [torch.empty(blk, dtype=torch.uint8).pin_memory() for _ in range(2)]
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=blk)
    rx.set_drain_lag(2)
    got = []
    for j, k in enumerate(range(0, raw.numel(), blk)):
        n = min(blk, raw.numel() - k)
        pins[j % 2][:n].copy_(raw[k:k + n])            # the other buffer's copy may still be in flight: allowed by the contract
        rx.feed_pinned(pins[j % 2].data_ptr(), n)
        got += rx.drain()
    rx.set_drain_lag(0)
    got += rx.drain()
    cases.check_against_golden(got, [list(rx.counters(c).values()) for c in range(len(cfg.freqs))], gold, label="pinned feed",
                               exact_diagnostics=False)
    st = rx.stats()
    assert st["front_sync_timeouts"] == 0 and st["overflow_feeds"] == 0
    rx.close()


@pytest.mark.parametrize("name,chunks", [("config2_1s", None), ("config4_0p4s", None), ("os10_noisy_1s", (3000, 200000)), ("config5_0p4s", (50000, 400000))])
def test_lookback_fallback_recovers(vh, name, chunks):
    """A channeliser workgroup that gives up waiting for its predecessor's filter state works that state out itself from the
    previous segment's last tile (kernels.h).  With the hand-off forced to fail for EVERY workgroup (the producers publish under
    a wrong epoch, the consumers poll 16 times) the whole decimated stream goes through the fall-back: golden frames, timing and
    counters all the same, a stream within rounding of the normal one, nothing refused - and the statistics say it happened."""
    cfg, iq, _, gold = cases.load(name)
    kw = dict(chunks=chunks, max_block=1600000) if chunks else {}
    rx, fr, cnt = gpu_decode(vh, cfg, iq, **kw)
    rx2, fr2, cnt2 = gpu_decode(vh, cfg, iq, debug={"force_timeout": 1}, **kw)
    assert rx.stats()["front_sync_timeouts"] == 0 and rx2.stats()["front_sync_timeouts"] > 0
    cases.check_against_golden(fr2, cnt2, gold, label=f"{name} through the look-back fall-back", exact_diagnostics=False)
    D = iq.size // 2 // cfg.oversample
    peak = float(np.abs(np.asarray(iq).astype(np.float32)).max()) / 32768.0
    for c in range(min(len(cfg.freqs), 16)):
        a, b = rx.read_decimated(c, max(0, D - 30000), 30000), rx2.read_decimated(c, max(0, D - 30000), 30000)
        # a sum of the lanes' states instead of a scan: the state differs in its last bit, and so - with the state in the normal form
        # of the recursion matrix (design.h) - do the first 128 outputs of a segment: 1.6e-7 of the stream's peak measured
        # (dev/gpu_fallback_diff.py); in the recursion's own basis the same last bit was ~1e-5 of the signal
        assert np.abs(a - b).max() <= 1e-6 * peak
    rx.close(); rx2.close()


def test_handoff_under_uneven_load(vh):
    """The fused look-back (kernels.h) is a cross-workgroup hand-off; MI355X_MICROARCH.md asks for such hand-offs to be
    tested under UNEVEN load.  Another stream keeps a varying part of the chip busy (matrix products of changing size,
    and a kernel that parks long-running workgroups on some CUs) while blocks are fed; every block must give the golden
    answers, with no look-back timeouts."""
    import torch
    cfg, iq, _, gold = cases.load("config2_1s")
    t = torch.from_numpy(iq.copy()).cuda()
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=iq.nbytes)
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda"); b = torch.randn(4096, 4096, device="cuda")
    big = torch.randn(64 << 20, device="cuda")
    ref = None
    for rep in range(12):
        with torch.cuda.stream(side):
            for j in range(6):
                n = 256 << ((rep + j) % 5)              # 256 .. 4096: from a handful of workgroups to the whole chip
                torch.mm(a[:n, :n], b[:n, :n])
                big[: (1 << 20) << ((rep + j) % 6)].sin_()
        rx2 = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=iq.nbytes)
        rx2.feed_device(t.data_ptr(), iq.nbytes)
        fr = rx2.drain()
        assert rx2.stats()["front_sync_timeouts"] == 0
        cases.check_against_golden(fr, None, gold, label=f"under load, rep {rep}")
        key = [(f["chan"], f["burst_ord"], f["idx"], f["octets"], f["sync_sample"], f["ppm_error"], f["frame_pwr_dbfs"]) for f in fr]
        assert ref is None or key == ref               # bit-identical floats too: a stale hand-off would move them
        ref = key
        rx2.close()
    torch.cuda.synchronize()
    rx.close()


@pytest.mark.parametrize("devices", [[0], [0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]])
def test_group_of_virtual_shards_from_c(vh, devices):
    """vdl2hip_group_* (multi-GPU from plain C): the channels spread over n members - here all on device 0, "virtual shards",
    SURVEY 8.6 - fed with host blocks (one H2D, then the fan-out to the other members), frames merged in drain order."""
    cfg, iq, _, gold = cases.load("config2_1s")
    raw = iq.view(np.uint8)
    g = vh.ReceiverGroup(cfg.centerfreq, list(cfg.freqs), devices, cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=1 << 20)
    assert g.size() == len(devices) and not g.uses_rccl()          # peer copies (RCCL is opt-in)
    g.set_drain_lag(1)
    got = []
    for k in range(0, raw.size, 1 << 20):
        g.feed(raw[k:k + (1 << 20)])
        got += g.drain()
    g.set_drain_lag(0)
    got += g.drain()
    cases.check_against_golden(got, [list(g.counters(c).values()) for c in range(len(cfg.freqs))], gold, label=f"group of {len(devices)}",
                               exact_diagnostics=False)
    ends = [(f["end_sample"], f["chan"], f["idx"]) for f in got]
    assert ends == sorted(ends)
    g.close()


@pytest.mark.parametrize("name", ["config3", "config4"])
def test_group_of_eight_on_the_bench_configs_vs_oracle(vh, oracle_mod, name):
    """BASELINE.json's configs[3] (32 channels) and configs[4] (256 channels) at 3 s through an 8-member vdl2hip_group - the channels
    sharded 8 ways, here on one GPU - in both exchange forms, against the oracle: frames, burst timing and the reference's 18 counters
    identical on every channel."""
    import os
    from dumpvdl2_amd import workloads, synth
    from util import compare_reference_counters, compare_at_full_size
    cfg = getattr(workloads, name)(3.0)
    iq, bursts = synth.synthesize(cfg)
    raw = iq.view(np.uint8)
    nch = len(cfg.freqs)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
    o.process(raw, block_bytes=1 << 24, nthreads=min(nch, os.cpu_count() or 8))
    fo = o.frames(); names = list(o.counters(0).keys()); co = [list(o.counters(c).values()) for c in range(nch)]
    assert len(fo) > 100
    for form in ("allgather", "broadcast"):
        g = vh.ReceiverGroup(cfg.centerfreq, list(cfg.freqs), [0] * 8, cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=8_000_000)
        g.set_exchange(form); g.set_drain_lag(vh.MAX_DRAIN_LAG)
        got = []
        for k in range(0, raw.size, 8_000_000):
            g.feed(raw[k:k + 8_000_000]); got += g.drain()
        g.set_drain_lag(0); got += g.drain()
        assert g.exchange().startswith(form)
        cnt = [list(g.counters(c).values()) for c in range(nch)]
        assert truth_is_subset(bursts, got) == 0
        cmp = compare_at_full_size(fo, got, label=f"{name} 3 s, group of 8, {form}")
        which, nbad = compare_reference_counters(names, co, cnt, label=f"{name} 3 s, group of 8, {form}", strict=True)
        assert cmp["timing_ties"] == 0 and cmp["nf_update_ties"] == 0 and nbad == 0
        g.close()
    o.close()


@pytest.mark.parametrize("devices", [[0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]])
def test_group_exchange_forms_agree(vh, devices):
    """The two ways vdl2hip_group_feed() puts a block on every member - stripes over each member's own host link + all-gather
    (default), and one host copy + broadcast - deliver the same bytes: frames (floats included), counters and the decimated
    stream itself are bit-identical, with block sizes that do and do not divide into whole stripes."""
    cfg, iq, _, gold = cases.load("config2_1s")
    raw = iq.view(np.uint8)
    D = iq.size // 2 // cfg.oversample
    res = {}
    for form in ("allgather", "broadcast"):
        g = vh.ReceiverGroup(cfg.centerfreq, list(cfg.freqs), devices, cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=1 << 20)
        g.set_exchange(form)
        assert g.exchange() == "none yet"
        g.set_drain_lag(2)
        got = []
        k, j = 0, 0
        sizes = [1 << 20, 999996, 4, 700000, 1 << 20]              # 4 bytes: fewer samples than members
        while k < raw.size:
            m = min(sizes[j % len(sizes)], raw.size - k); j += 1
            g.feed(raw[k:k + m]); k += m
            got += g.drain()
        g.set_drain_lag(0)
        got += g.drain()
        assert g.exchange() == form + "/peer-copy" and not g.uses_rccl()
        cnt = [list(g.counters(c).values()) for c in range(len(cfg.freqs))]
        cases.check_against_golden(got, cnt, gold, label=f"group {form}", exact_diagnostics=False)
        y = [g.read_decimated(c, D - 20000, 20000).copy() for c in range(len(cfg.freqs))]
        res[form] = (got, cnt, y, g.stats()["front_sync_timeouts"])
        g.close()
    a, b = res["allgather"], res["broadcast"]
    assert a[1] == b[1]
    key = lambda f: (f["chan"], f["burst_ord"], f["idx"])
    fa, fb = sorted(a[0], key=key), sorted(b[0], key=key)
    if a[3] == 0 and b[3] == 0:
        assert [tuple(sorted(f.items())) for f in fa] == [tuple(sorted(f.items())) for f in fb]
    else:
        assert_frames_equal(fa, fb, label="group exchange forms (with look-back fall-backs)")
    for ya, yb in zip(a[2], b[2]):
        if a[3] == 0 and b[3] == 0:
            assert ya.tobytes() == yb.tobytes()
        else:       # a channeliser look-back fell back (a GPU shared with another process): equal up to fp32 rounding of the segment-start state
            assert np.abs(ya - yb).max() <= 1e-4 * float(np.abs(ya).max())


def test_cold_start_block_goes_in_pieces_and_gives_the_same_stream(vh):
    """A large block from page-locked memory fed to an idle receiver is copied and channelised in four pieces (feed_host's cold
    start).  The decimated stream must be the very floats one copy + one channeliser launch give (the pageable vdl2hip_feed() of
    the same bytes never takes that path), frames and counters the golden ones; a second block, fed while the first is still
    pending, goes in one piece and must agree as well."""
    import torch
    cfg, iq, _, gold = cases.load("config2_1s")
    raw = torch.from_numpy(iq.copy()).view(torch.uint8)
    reps = 5                                              # 1 s = 8.4 MB is the case; 5 x the same second makes the block 42 MB
    big = raw.repeat(reps).contiguous()
    assert big.numel() >= (8 << 20)
    pin = big.pin_memory()
    D = big.numel() // 4 // cfg.oversample
    streams, frames = [], []
    for how in ("pinned", "pageable"):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=big.numel())
        if how == "pinned":
            rx.set_drain_lag(2)
            rx.feed_pinned(pin.data_ptr(), pin.numel())   # idle receiver: four pieces
            rx.feed_pinned(pin.data_ptr(), pin.numel())   # the first still pending: one piece
            rx.set_drain_lag(0)
        else:
            rx.feed(big.numpy()); rx.feed(big.numpy())
        fr = rx.drain()
        streams.append([rx.read_decimated(c, max(0, 2 * D - 40000), 40000) for c in range(len(cfg.freqs))])
        frames.append([(f["chan"], f["idx"], bytes(f["octets"]), f["sync_sample"], f["frame_pwr_dbfs"], f["ppm_error"]) for f in fr])
        st = rx.stats()
        assert st["front_sync_timeouts"] == 0 and st["overflow_feeds"] == 0
        rx.close()
    assert len(frames[0]) >= len(gold["frames"]) and frames[0] == frames[1]
    for a, b in zip(*streams):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_group_feed_pinned(vh):
    """vdl2hip_group_feed_pinned(): blocks from two alternating page-locked buffers, queued without waiting for the copy."""
    import torch
    cfg, iq, _, gold = cases.load("config2_1s")
    raw = torch.from_numpy(iq.view(np.uint8).copy())
    blk = 1 << 20
    pins = [torch.empty(blk, dtype=torch.uint8).pin_memory() for _ in range(2)]
    g = vh.ReceiverGroup(cfg.centerfreq, list(cfg.freqs), [0, 0], cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=blk)
    g.set_drain_lag(2)
    got = []
    for j, k in enumerate(range(0, raw.numel(), blk)):
        n = min(blk, raw.numel() - k)
        if j >= 2:
            pass            # buffer j % 2 was handed over two feeds ago: the feed in between has returned, so it is ours again
        pins[j % 2][:n].copy_(raw[k:k + n])
        g.feed_pinned(pins[j % 2].data_ptr(), n)
        got += g.drain()
    g.sync()
    g.set_drain_lag(0)
    got += g.drain()
    cases.check_against_golden(got, [list(g.counters(c).values()) for c in range(len(cfg.freqs))], gold, label="group, pinned feeds",
                               exact_diagnostics=False)
    g.close()


_TWO_GPU_SNIPPET = r"""
import os, sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import cases
from dumpvdl2_amd import vdl2hip as vh
want_rccl = os.environ.get("VDL2HIP_USE_RCCL") == "1"
cfg, iq, _, gold = cases.load("config2_1s")
raw = iq.view(np.uint8)
for form in ("allgather", "broadcast"):
    g = vh.ReceiverGroup(cfg.centerfreq, list(cfg.freqs), [0, 1], cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=1 << 20)
    assert g.uses_rccl() == want_rccl, "librccl.so did not load or ncclCommInitAll failed" if want_rccl else "RCCL in use without having been asked for"
    g.set_exchange(form)
    got = []
    for k in range(0, raw.size, 1 << 20):
        g.feed(raw[k:k + (1 << 20)])
        got += g.drain()
    assert g.exchange() == form + ("/rccl" if want_rccl else "/peer-copy"), g.exchange()
    cases.check_against_golden(got, [list(g.counters(c).values()) for c in range(len(cfg.freqs))], gold, label="two GPUs, " + g.exchange(), exact_diagnostics=False)
    g.close()
print("TWO_GPU_OK")
"""


def _two_gpus(env_extra):
    import os, subprocess, sys, torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _TWO_GPU_SNIPPET, root], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env_extra))
    assert r.returncode == 0 and "TWO_GPU_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_group_over_two_real_gpus(vh):
    """vdl2hip_group_* over two physical GPUs, both exchange forms, with the default transport (hipMemcpyPeerAsync): only where two
    GPUs are visible.  In a process of its own with a time limit."""
    _two_gpus({"VDL2HIP_USE_RCCL": "0"})


def test_group_over_two_real_gpus_rccl(vh):
    """The opt-in RCCL transport of vdl2hip_group_feed (ncclCommInitAll + grouped ncclAllGather / ncclBroadcast from one thread).  Run in
    a process of its own with a time limit, so that a hang or a crash inside RCCL cannot take the suite with it.  Skipped with one GPU;
    wherever two are visible it must pass - these calls have not run on hardware yet, and a failure is to be seen, not expected."""
    _two_gpus({"VDL2HIP_USE_RCCL": "1"})


def test_dropin_adapter_over_several_devices(vh, tmp_path):
    """The reference-named adapter with VDL2HIP_DEVICES=0,0,0: an unmodified dumpvdl2 main() linking it spreads its channels over
    the listed GPUs (here three virtual shards of device 0); 8 channels of the golden 1 s capture."""
    import os, subprocess, hashlib
    from dumpvdl2_amd import build
    cfg, iq, _, gold = cases.load("config2_1s")
    exe = build.build_harness(str(tmp_path / "dropin_harness"))
    path = tmp_path / "cap.cs16"
    iq.tofile(path)
    env = dict(os.environ, VDL2HIP_DEVICES="0,0,0")
    out = subprocess.run([exe, str(path), str(cfg.oversample), str(cfg.centerfreq)] + [str(f) for f in cfg.freqs], check=True,
                         capture_output=True, text=True, timeout=180, env=env).stdout
    got = []
    for l in out.splitlines():
        if l.startswith("FRAME"):
            kv = dict(t.split("=", 1) for t in l.split()[1:])
            got.append((int(kv["freq"]), int(kv["idx"]), hashlib.sha1(bytes.fromhex(kv["octets"])).hexdigest(), int(kv["S"]), int(kv["L"]), int(kv["F"])))
    want = [(cfg.freqs[f["chan"]], f["idx"], f["sha1"], f["synd_weight"], f["datalen_octets"], f["num_fec_corrections"]) for f in gold["frames"]]
    assert sorted(got) == sorted(want) and len(got) > 20


@pytest.mark.parametrize("blocks", [None, 10])
def test_dropin_adapter_collects_blocks(vh, tmp_path, blocks):
    """The adapter hands a fast producer's 320 000-byte blocks to the GPU several at a time (csrc/dropin.c, "Blocks per feed"):
    the frames pushed to avlc_decoder_queue_push() must be the golden capture's whatever the collecting - the default (16 blocks of
    this size), 5 (the last batch of the stream is a partial one), 1 (every block on its own: the old behaviour) - per channel in the
    same order, none lost at the end of the stream: neither when the file ends in a short block (`blocks` None: 26.25 blocks) nor
    when it ends on a block boundary and process_iq_file()'s last fread() returns nothing (10 blocks exactly; there the runs are
    compared with each other)."""
    import os, subprocess, hashlib
    from dumpvdl2_amd import build
    cfg, iq, _, gold = cases.load("config2_1s")
    exe = build.build_harness(str(tmp_path / "dropin_harness"))
    raw = iq.view(np.uint8)
    if blocks: raw = raw[: blocks * 320000]
    path = tmp_path / "cap.cs16"
    raw.tofile(path)
    runs = {}
    for batch in (None, "5", "1"):
        env = dict(os.environ)
        env.pop("VDL2HIP_DROPIN_BATCH", None)
        if batch: env["VDL2HIP_DROPIN_BATCH"] = batch
        out = subprocess.run([exe, str(path), str(cfg.oversample), str(cfg.centerfreq)] + [str(f) for f in cfg.freqs], check=True,
                             capture_output=True, text=True, timeout=180, env=env).stdout
        got = {}
        for l in out.splitlines():
            if l.startswith("FRAME"):
                kv = dict(t.split("=", 1) for t in l.split()[1:])
                got.setdefault(int(kv["freq"]), []).append((int(kv["idx"]), hashlib.sha1(bytes.fromhex(kv["octets"])).hexdigest(), int(kv["S"]), int(kv["L"]), int(kv["F"]),
                                                            float(kv["pwr"]), float(kv["nf"]), float(kv["ppm"])))
        runs[batch] = got
    for other in ("5", "1"):        # octets and integer metadata identical and in the same order per channel; the floats (printed to 0.001) within SURVEY 8.5
        assert runs[None].keys() == runs[other].keys()
        for k in runs[None]:
            assert [t[:5] for t in runs[None][k]] == [t[:5] for t in runs[other][k]]
            assert all(abs(p - q) <= 0.0011 for a, b in zip(runs[None][k], runs[other][k]) for p, q in zip(a[5:], b[5:]))
    assert sum(len(v) for v in runs["1"].values()) > (5 if blocks else 20)
    if not blocks:
        want = {}
        for f in gold["frames"]:
            want.setdefault(cfg.freqs[f["chan"]], []).append((f["idx"], f["sha1"], f["synd_weight"], f["datalen_octets"], f["num_fec_corrections"]))
        assert {k: sorted(t[:5] for t in v) for k, v in runs[None].items()} == {k: sorted(v) for k, v in want.items()}


def test_uint8_conversion_without_the_division(vh):
    """The channeliser's unsigned-byte build converts (i - 127.5f) / 127.5f (src/demod.c:349-354) with a multiplication and one Newton
    step instead of the division: the same float for every one of the 256 byte values, on the device and against numpy."""
    import ctypes as C
    L = vh.load_library()
    L.vdl2hip_debug_u8_levels.argtypes = [C.POINTER(C.c_float)]
    out = (C.c_float * 512)()
    assert L.vdl2hip_debug_u8_levels(out) == 0
    o = np.array(out[:], dtype=np.float32)
    want = ((np.arange(256, dtype=np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32)
    assert o[:256].tobytes() == o[256:].tobytes() == want.tobytes()


def test_dropin_adapter_unsigned_bytes(vh, oracle_mod, tmp_path):
    """process_buf_uchar() (src/demod.c:339-347: the --iq-file default format) through the adapter, blocks collected (4 u8 blocks of
    320 000 bytes at oversample 10 hold 64 000 decimated samples) and one by one: the oracle's frames."""
    import os, subprocess
    from dumpvdl2_amd import build, synth
    cfg = synth.SynthConfig(centerfreq=CF, freqs=[CF, CF + 40000], oversample=10, duration_s=1.9, seed=12, amplitude=0.3, noise_sigma=0.01)
    iq8, _ = synth.synthesize(cfg, dtype=np.uint8)
    o = oracle_mod.Oracle(CF, list(cfg.freqs), oversample=10, sample_fmt=oracle_mod.FMT_U8)
    o.process(iq8)
    want = sorted((cfg.freqs[f["chan"]], f["idx"], f["octets"], f["synd_weight"], f["datalen_octets"], f["num_fec_corrections"]) for f in o.frames())
    exe = build.build_harness(str(tmp_path / "dropin_harness"))
    path = tmp_path / "cap.cu8"
    iq8.tofile(path)
    for batch in (None, "1"):
        env = dict(os.environ, HARNESS_U8="1")
        env.pop("VDL2HIP_DROPIN_BATCH", None)
        if batch: env["VDL2HIP_DROPIN_BATCH"] = batch
        out = subprocess.run([exe, str(path), "10", str(CF)] + [str(f) for f in cfg.freqs], check=True, capture_output=True, text=True, timeout=180, env=env).stdout
        got = []
        for l in out.splitlines():
            if l.startswith("FRAME"):
                kv = dict(t.split("=", 1) for t in l.split()[1:])
                got.append((int(kv["freq"]), int(kv["idx"]), bytes.fromhex(kv["octets"]), int(kv["S"]), int(kv["L"]), int(kv["F"])))
        assert sorted(got) == want and len(got) > 5, (batch, len(got), len(want))


def test_dpp_primitives_behave_as_the_scan_assumes(vh):
    """The channeliser's wave scan (kernels.h) moves filter states between lanes with DPP controls: row_shr inside rows of 16 lanes
    (out-of-row sources read 0), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3, wave_shr:1 across the wavefront."""
    import ctypes as C
    L = vh.load_library()
    L.vdl2hip_debug_dpp_probe.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    a = (C.c_float * 64)(*[float(l + 1) for l in range(64)])
    out = (C.c_float * 256)()
    assert L.vdl2hip_debug_dpp_probe(a, out) == 0
    o = np.array(out[:]).reshape(4, 64)
    lanes = np.arange(64)
    assert np.array_equal(o[0], np.where((lanes & 15) >= 4, lanes - 4 + 1, 0))
    assert np.array_equal(o[1], np.where((lanes // 16) % 2 == 1, (lanes // 16) * 16 - 1 + 1, 0))
    assert np.array_equal(o[2], np.where(lanes >= 32, 32, 0))
    assert np.array_equal(o[3], np.where(lanes >= 1, lanes, 0))


@pytest.mark.parametrize("seed,profile", [(55, "plain"), (145, "plain"), (104, "extreme"), (4, "plain"), (8, "extreme"), (12, "rejects"),
                                          (17, "extreme"), (20, "extreme"), (31, "plain"), (41, "extreme"), (9, "rejects"),
                                          (175, "plain"), (274, "plain"), (1014, "extreme"), (2274, "plain"), (1738, "plain")])
def test_random_capture_in_random_pieces(vh, seed, profile):
    """tests/fuzz_gpu.py's seeds as a test: a random capture fed in random pieces (long feeds with the speculative walk and the back
    end on its own streams, short ones with everything on the front stream, in one stream; random drain lag).  The answer is the
    oracle's - frames, burst timing, the reference's 18 counters on every channel, strictly.  (Seeds 55, 145, 104 differed in
    profiles/r04_gpu_fuzz.txt, 175, 274, 1014 in round 4's CPU prediction over 2000 captures: decisions that hang on the reference's
    own rounding - the referee takes them on the reference's own samples now.)  The host build of the device logic, run on the
    decimated stream read back from the GPU, must give the GPU's answer as well."""
    import fuzz_gpu
    r = fuzz_gpu.run_seed(seed, profile, always_check=True, strict=True)
    assert r["host_build_check"] is True and r["frames"] > 0 and r["ties"] == 0 and r["nf_ties"] == 0 and r["bookkeeping_channels"] == 0, r
    assert r["referee_refused"] == 0, r


@pytest.mark.xfail(strict=True, reason="without the referee a symbol at a slicer boundary is decided on the channeliser's samples: num_fec_corrections 1, the reference's 2 (DESIGN 5)")
def test_random_capture_without_the_referee(vh, monkeypatch):
    """what the referee is for: seed 175 with VDL2HIP_REFEREE=0 is NOT the oracle's answer (if this ever passes, the channeliser has
    become the reference's scan bit for bit and the referee can go)"""
    import fuzz_gpu
    monkeypatch.setenv("VDL2HIP_REFEREE", "0")
    fuzz_gpu.run_seed(175, "plain", always_check=False, strict=True)
