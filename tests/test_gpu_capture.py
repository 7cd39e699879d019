"""The burst capture on the GPU (include/vdl2hip.h, "Burst capture"; kernels: dumpvdl2_amd/csrc/capture.h): of every burst handed
to the burst decoder the decimated IQ around it, its timing and a phase-error quality figure, joined on the host with the frames
it produced.

The IQ is held, bit for bit, to the receiver's own decimated stream read back with read_decimated() right after the feed that
delivered the record; the quality to the numpy model of tests/capture_model.py applied to the captured IQ and the record's own dphi
and prev_phase, within the bounds derived there.  The referee is off unless a test says otherwise (with it on, a later feed under
way may rewrite a stretch of y while a window is copied; one feed has no later feed).  IQ is compared within a run only, never
across cuts: the channeliser's stream is not bit-identical across cuts."""
import ctypes as C

import numpy as np
import pytest

import capture_model as cm
import cases
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
E_INVAL = -1
INT_FIELDS = ("chan", "freq", "burst_ord", "sync_sample", "end_sample", "first_symbol", "nsym", "tl_bits", "flags", "iq_first", "iq_count",
              "frames", "frames_ok", "fec_corrections", "weak_symbols")       # (iq_off depends on how the reads were grouped)


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_iq(rx, recs, wins, label=""):
    """every window against the decimated stream as it stands now"""
    for r, w in zip(recs, wins):
        assert w.size == r["iq_count"]
        if r["iq_count"]:
            y = rx.read_decimated(r["chan"], r["iq_first"], r["iq_count"])
            assert y.shape[0] == r["iq_count"], (label, r)
            assert np.array_equal(bits(w.view(np.float32)), bits(y).reshape(-1)), f"{label}: IQ of burst {r['chan']}/{r['burst_ord']} differs from read_decimated"


def check_quality(r, w, label=""):
    assert r["end_sample"] == r["first_symbol"] + 10 * (r["nsym"] - 1) and r["iq_first"] <= r["first_symbol"]
    at = r["first_symbol"] - r["iq_first"] + 10 * np.arange(r["nsym"])
    sym = w.view(np.float32).reshape(-1, 2)[at]
    return cm.check_quality(r, cm.quality(sym, r["prev_phase"], r["dphi"]), label=label)


def feed_pieces(rx, raw, sizes, per_feed=None):
    """raw: int16 [n, 2]; sizes: samples per feed, cycling -> (frames, records, windows); every record's IQ is checked after its feed"""
    frames, recs, wins = [], [], []
    k = i = 0
    while k < raw.shape[0]:
        d = min(sizes[i % len(sizes)], raw.shape[0] - k)
        rx.feed(raw[k:k + d])
        k += d; i += 1
        rx.sync()
        r, w = rx.capture_read()
        check_iq(rx, r, w, label=f"feed {i}")
        frames += rx.drain()
        recs += r; wins += w
        if per_feed:
            per_feed(i, r)
    return frames, recs, wins


def by_key(recs):
    return {(r["chan"], r["burst_ord"]): r for r in recs}


# ---------------------------------------------------------------- 1. the reference's test vector
def run_wav(vh, wav, capture, referee, one_feed=False):
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=wav.size if one_feed else 320000)
    rx.debug_option("referee", referee)
    if capture:
        rx.capture_enable()
    frames, recs, wins = [], [], []
    step = wav.size if one_feed else 320000
    for k in range(0, wav.size, step):
        rx.feed(wav[k:k + step])
        rx.sync()
        if capture:
            r, w = rx.capture_read()
            check_iq(rx, r, w, label="wav")
            recs += r; wins += w
        frames += rx.drain()
    info = rx.capture_info() if capture else None
    cnt = [list(rx.counters(0).values()), list(rx.avlc_counters(0).values())]
    rx.close()
    return frames, recs, wins, info, cnt


@pytest.mark.parametrize("referee,one_feed", [(0, False), (1, True)])
def test_reference_wav(vh, golden_wav, referee, one_feed):
    frames, recs, wins, info, cnt = run_wav(vh, golden_wav, True, referee, one_feed)
    assert len(frames) == 2 and len(recs) == 1
    r, w = recs[0], wins[0]
    for f in frames:
        assert (f["sync_sample"], f["end_sample"], f["burst_ord"], f["chan"]) == (r["sync_sample"], r["end_sample"], r["burst_ord"], r["chan"])
    assert r["frames"] == 2 and r["frames_ok"] == sum(f["avlc_status"] == vh.AVLC_OK for f in frames) and r["freq"] == CF and r["flags"] == 0
    assert r["fec_corrections"] == max(frames, key=lambda f: f["idx"])["num_fec_corrections"]
    assert r["iq_first"] == r["sync_sample"] - 256 and r["iq_count"] == r["end_sample"] + 32 - r["iq_first"] + 1
    assert abs(r["ppm_error"] - frames[0]["ppm_error"]) < 1e-6
    check_quality(r, w, label=f"wav referee={referee}")
    db = 10 * np.log10(r["mean_power"])
    for f in frames:
        print(f"10 log10(mean_power) = {db:.5f}, frame_pwr_dbfs = {f['frame_pwr_dbfs']:.5f}")
        assert abs(db - f["frame_pwr_dbfs"]) <= 0.001
    assert (info["bursts"], info["iq_samples"], info["iq_dropped"], info["pre_samples"], info["post_samples"], info["pool_samples"]) == (1, r["iq_count"], 0, 256, 32, 1 << 20)
    # nothing else moves: the frames and counters of a run without the capture
    f0, _, _, _, c0 = run_wav(vh, golden_wav, False, referee, one_feed)
    assert_frames_equal(f0, frames, label="capture on")
    assert c0 == cnt


# ---------------------------------------------------------------- 2. bursts that straddle feeds, and the cut does not matter
def run_config2(vh, sizes, post, **kw):
    cfg, iq, _, _ = cases.load("config2_1s")
    raw = np.asarray(iq).reshape(-1, 2)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=4 * max(sizes), **kw)
    rx.debug_option("referee", 0)
    rx.capture_enable(256, post)
    straddle = []

    def per_feed(i, recs):
        k0 = rx.stats()["input_samples"] // cfg.oversample
        straddle.extend(r for r in recs if r["sync_sample"] < k0 - (sizes[(i - 1) % len(sizes)] // cfg.oversample))
    frames, recs, wins = feed_pieces(rx, raw, sizes, per_feed)
    st = rx.stats()
    info = rx.capture_info()
    rx.close()
    return frames, recs, wins, st, info, straddle


@pytest.fixture(scope="module")
def config2_whole(vh):
    cfg, iq, _, _ = cases.load("config2_1s")
    return run_config2(vh, [np.asarray(iq).size // 2], 0)


@pytest.fixture(scope="module")
def config2_halves(vh):
    """the stream in two feeds: what the tests below, which feed it the same way, compare their records with field by field"""
    cfg, iq, _, _ = cases.load("config2_1s")
    return run_config2(vh, [np.asarray(iq).size // 4], 0)


def test_config2_in_pieces(vh, config2_whole):
    frames, recs, wins, st, info, straddle = run_config2(vh, [100000, 333333, 7], 0)
    assert len(recs) == st["bursts"] == info["bursts"] > 8 and info["iq_dropped"] == 0
    assert len(straddle) >= 1, "no burst began in an earlier feed than the one that decoded it"
    keys = by_key(recs)
    assert len(keys) == len(recs) and {(f["chan"], f["burst_ord"]) for f in frames} <= set(keys)
    for f in frames:
        r = keys[(f["chan"], f["burst_ord"])]
        assert (r["sync_sample"], r["end_sample"]) == (f["sync_sample"], f["end_sample"])
    worst = max(check_quality(r, w, label=f"{r['chan']}/{r['burst_ord']}") for r, w in zip(recs, wins))
    print(f"config2 in pieces: {len(recs)} bursts, {len(straddle)} across feeds, worst phase figure at {worst:.3f} of its bound")
    # cut invariance (post = 0): the same stream fed whole
    _, recs_w, _, st_w, _, _ = config2_whole
    assert st_w["bursts"] == st["bursts"]
    kw = by_key(recs_w)
    assert set(kw) == set(keys)
    for k, r in keys.items():
        for name in INT_FIELDS:
            assert r[name] == kw[k][name], (k, name, r[name], kw[k][name])


def test_order_is_channel_then_position(config2_whole):
    _, recs, _, _, _, _ = config2_whole
    order = [(r["chan"], r["burst_ord"]) for r in recs]
    assert order == sorted(order) and len({c for c, _ in order}) > 1


# ---------------------------------------------------------------- 3. failed bursts
def run_config5(vh, referee, failed_only):
    cfg, iq, _, gold = cases.load("config5_0p4s")
    raw = np.asarray(iq).reshape(-1, 2)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=raw.nbytes)
    rx.debug_option("referee", referee)
    rx.capture_enable(failed_only=failed_only)
    frames, recs, wins = feed_pieces(rx, raw, [raw.shape[0]])
    cnt = [list(rx.counters(c).values()) for c in range(len(cfg.freqs))]
    st, info = rx.stats(), rx.capture_info()
    rx.close()
    return frames, recs, wins, cnt, st, info, gold


def test_config5_failed_bursts(vh):
    frames, recs, wins, cnt, st, info, gold = run_config5(vh, 0, False)
    assert sum(c[10] for c in gold["counters"]) == 4            # decoder.errors.fec_bad of the golden answers: failed bursts exist
    assert len(recs) == st["bursts"] == info["bursts"]
    with_frames = {(f["chan"], f["burst_ord"]) for f in frames}
    none = [r for r in recs if r["frames"] == 0]
    assert len(none) == st["bursts"] - len(with_frames) >= 1
    for r in recs:
        mine = [f for f in frames if (f["chan"], f["burst_ord"]) == (r["chan"], r["burst_ord"])]
        assert r["frames"] == len(mine) and r["frames_ok"] == sum(f["avlc_status"] == vh.AVLC_OK for f in mine)
        assert r["fec_corrections"] == (max(mine, key=lambda f: f["idx"])["num_fec_corrections"] if mine else -1)
    for r, w in zip(recs, wins):
        check_quality(r, w, label=f"{r['chan']}/{r['burst_ord']}")
    # FAILED_ONLY: exactly the records without a good frame, the same bytes but for their place in the read
    _, recs_f, wins_f, _, st_f, info_f, _ = run_config5(vh, 0, True)
    want = [(r, w) for r, w in zip(recs, wins) if r["frames_ok"] == 0]
    assert len(recs_f) == len(want) >= len(none) and info_f["bursts"] == st_f["bursts"] == st["bursts"]
    for (a, wa), b, wb in zip(want, recs_f, wins_f):
        assert {k: v for k, v in a.items() if k != "iq_off"} == {k: v for k, v in b.items() if k != "iq_off"}
        assert np.array_equal(bits(wa.view(np.float32)), bits(wb.view(np.float32)))


def test_config5_golden_with_capture_on(vh):
    """frames and counters are the golden file's with the capture on (the receiver as it ships: the referee on; one feed)"""
    frames, recs, wins, cnt, st, info, gold = run_config5(vh, 1, False)
    cases.check_against_golden(frames, cnt, gold, label="config5, capture on", exact_diagnostics=False)
    assert len(recs) == st["bursts"] and {(f["chan"], f["burst_ord"]) for f in frames} <= set(by_key(recs))


# ---------------------------------------------------------------- 4. room
def test_room(vh, config2_halves):
    _, full, wins_full, _, _, _ = config2_halves
    cfg, iq, _, _ = cases.load("config2_1s")
    raw = np.asarray(iq).reshape(-1, 2)
    half = raw.shape[0] // 2
    first_feed = [r for r in full if r["end_sample"] < half // cfg.oversample]
    assert len(first_feed) >= 3
    pool = first_feed[0]["iq_count"] + first_feed[1]["iq_count"] - 1          # just below the second burst's end
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=4 * half)
    rx.debug_option("referee", 0)
    rx.capture_enable(256, 0, pool_samples=pool)
    rx.feed(raw[:half]); rx.feed(raw[half:])
    rx.sync()
    biggest = max(r["iq_count"] for r in full)
    recs, wins = rx.capture_read(cap_recs=1, cap_pairs=biggest)             # one record a call
    info = rx.capture_info()
    assert len(recs) == len(full) == info["bursts"]
    nroom = 0
    for a, b, wa, wb in zip(full, recs, wins_full, wins):
        fits = b["flags"] == 0
        nroom += not fits
        assert b["iq_off"] == 0                                              # (one record a call)
        if fits:
            assert b["iq_count"] == a["iq_count"] and np.array_equal(bits(wa.view(np.float32)), bits(wb.view(np.float32)))
        else:
            assert b["flags"] == vh.BURST_NO_ROOM and b["iq_count"] == 0 and wb.size == 0
        skip = ("iq_off", "iq_count", "flags")
        assert {k: v for k, v in a.items() if k not in skip} == {k: v for k, v in b.items() if k not in skip}      # the quality is still valid
    first2 = [r for r in recs if r["end_sample"] < half // cfg.oversample]
    assert [r["flags"] for r in first2[:3]] == [0, 1, 1] and all(r["flags"] == 1 for r in first2[1:])
    assert info["iq_dropped"] == nroom >= len(first2) - 1 and info["pool_samples"] == pool
    assert info["iq_samples"] == sum(r["iq_count"] for r in recs)
    rx.close()


def test_read_in_small_pieces(vh, config2_halves):
    """several records a call, the IQ buffer the limit: nothing is lost, nothing comes twice"""
    _, full, wins_full, _, _, _ = config2_halves
    cfg, iq, _, _ = cases.load("config2_1s")
    raw = np.asarray(iq).reshape(-1, 2)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=2 * raw.shape[0])
    rx.debug_option("referee", 0)
    rx.capture_enable(256, 0)
    half = raw.shape[0] // 2
    rx.feed(raw[:half]); rx.feed(raw[half:])
    rx.sync()
    biggest = max(r["iq_count"] for r in full)
    L = rx.L
    rec = np.zeros(3, dtype=vh.BURST_DTYPE)
    buf = np.zeros((biggest + 10, 2), dtype=np.float32)
    used = C.c_size_t(0)
    assert L.vdl2hip_capture_read(rx.h, rec.ctypes.data, 3, buf.ctypes.data, full[0]["iq_count"] - 1, C.byref(used)) == 0 and used.value == 0
    got, calls = [], 0
    while True:
        n = L.vdl2hip_capture_read(rx.h, rec.ctypes.data, 3, buf.ctypes.data, biggest + 10, C.byref(used))
        assert n >= 0
        if n == 0:
            break
        calls += 1
        assert used.value == sum(int(r["iq_count"]) for r in rec[:n]) <= biggest + 10
        for r in rec[:n]:
            got.append((int(r["chan"]), int(r["burst_ord"]), buf[int(r["iq_off"]):int(r["iq_off"]) + int(r["iq_count"])].copy()))
    assert calls > len(full) // 3 and len(got) == len(full)
    for (c, o, w), a, wa in zip(got, full, wins_full):
        assert (c, o) == (a["chan"], a["burst_ord"]) and np.array_equal(bits(w).reshape(-1), bits(wa.view(np.float32)))
    rx.close()


# ---------------------------------------------------------------- 5. switching
def test_switching(vh, golden_wav):
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE)
    rx.debug_option("referee", 0)
    L = rx.L
    info = vh.CaptureInfo(C.sizeof(vh.CaptureInfo))
    rec = np.zeros(4, dtype=vh.BURST_DTYPE)
    # off: nothing to read
    assert L.vdl2hip_capture_info_get(rx.h, C.byref(info)) == E_INVAL
    assert L.vdl2hip_capture_read(rx.h, rec.ctypes.data, 4, None, 0, None) == E_INVAL
    rx.feed(golden_wav[:320000])                                  # 8 000 decimated samples: ahead of the burst (sync at 11 975)
    rx.capture_enable(300, 7, pool_samples=1 << 16)               # mid-stream
    for k in range(320000, golden_wav.size, 320000):
        rx.feed(golden_wav[k:k + 320000])
    rx.sync()
    s0 = rx.capture_info()
    assert (s0["bursts"], s0["pre_samples"], s0["post_samples"], s0["pool_samples"], s0["flags"]) == (1, 300, 7, 1 << 16, 0)
    # bad configurations are refused and the running capture is left as it was, its queue included
    good = dict(struct_size=C.sizeof(vh.CaptureCfg), pre_samples=256, post_samples=32, flags=0, pool_samples=0, reserved=0)
    for bad in (dict(struct_size=20), dict(struct_size=28), dict(pre_samples=4097), dict(post_samples=1025), dict(flags=2), dict(flags=3),
                dict(pool_samples=(1 << 24) + 1), dict(reserved=1)):
        cfg = vh.CaptureCfg(**{**good, **bad})
        assert L.vdl2hip_capture_enable(rx.h, C.byref(cfg)) == E_INVAL, bad
        assert {k: v for k, v in rx.capture_info().items() if k != "kernel_ms"} == {k: v for k, v in s0.items() if k != "kernel_ms"}, bad
    assert L.vdl2hip_capture_enable(rx.h, None) == E_INVAL and L.vdl2hip_capture_enable(None, C.byref(vh.CaptureCfg(**good))) == E_INVAL
    assert L.vdl2hip_capture_info_get(rx.h, C.byref(vh.CaptureInfo(48))) == E_INVAL
    recs, wins = rx.capture_read()
    assert len(recs) == 1 and recs[0]["iq_first"] == recs[0]["sync_sample"] - 300 and recs[0]["iq_count"] == recs[0]["end_sample"] + 7 - recs[0]["iq_first"] + 1
    check_iq(rx, recs, wins, label="enabled mid-stream")
    check_quality(recs[0], wins[0], label="enabled mid-stream")
    assert rx.capture_read() == ([], [])
    # the extremes that are taken
    for ok in (dict(pre_samples=4096, post_samples=1024, pool_samples=1 << 24, flags=1), dict(pre_samples=0, post_samples=0, pool_samples=1)):
        assert L.vdl2hip_capture_enable(rx.h, C.byref(vh.CaptureCfg(**{**good, **ok}))) == 0, ok
    assert rx.capture_info()["bursts"] == 0
    # disable, then feed: nothing is queued
    rx.capture_disable()
    for k in range(0, golden_wav.size, 320000):
        rx.feed(golden_wav[k:k + 320000])
    rx.sync()
    assert L.vdl2hip_capture_read(rx.h, rec.ctypes.data, 4, None, 0, None) == E_INVAL
    rx.capture_enable()
    assert rx.capture_read() == ([], []) and rx.capture_info()["bursts"] == 0
    assert len(rx.drain()) >= 2                                   # (the decoder went on as ever)
    rx.close()


def test_shard_and_group(vh, config2_halves):
    _, full, _, _, _, _ = config2_halves
    cfg, iq, _, _ = cases.load("config2_1s")
    raw = np.asarray(iq).reshape(-1, 2)
    half = raw.shape[0] // 2

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            for name in INT_FIELDS[:-1]:                      # (not weak_symbols: a shard's stream is its own to the last bit)
                assert x[name] == y[name], (name, x, y)
    shard = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=4 * half, chan_first=2, chan_count=3)
    shard.debug_option("referee", 0)
    shard.capture_enable(256, 0)
    frames, recs, wins = feed_pieces(shard, raw, [half])
    assert {r["chan"] for r in recs} <= {2, 3, 4} and len(recs) >= 3
    assert all(r["freq"] == cfg.freqs[r["chan"]] for r in recs)
    same([r for r in full if r["chan"] in (2, 3, 4)], recs)
    shard.close()
    # a group of two virtual shards on one device: vdl2hip_group_ctx(g, k) is the handle of member k's bursts
    g = vh.ReceiverGroup(cfg.centerfreq, list(cfg.freqs), [0, 0], cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=4 * half)
    for i in range(g.size()):
        assert g.L.vdl2hip_debug_option(g.member(i), b"referee", 0) == 0
    g.capture_enable(256, 0)
    g.feed(raw[:half]); g.feed(raw[half:])
    g.sync()
    got = []
    for i in range(g.size()):
        r, w = g.capture_read(i)
        assert g.capture_info(i)["bursts"] == len(r) > 0
        assert {x["chan"] for x in r} <= set(range(4 * i, 4 * i + 4))
        got += r
    key = lambda r: (r["chan"], r["burst_ord"])
    same(sorted(full, key=key), sorted(got, key=key))
    g.capture_disable()
    g.close()


# ---------------------------------------------------------------- 6. the ring of y wraps
def test_ring_wraps(vh):
    """small blocks make the decimated ring small (2^17 samples: 6 feeds of 10 001 + 65 536 + 1 024); over 4 s it wraps three times,
    with windows across the wrap"""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(freqs=synth.channel_plan(3, spacing=100000), duration_s=4.0, mean_gap_s=0.08, max_payload=600, seed=4242)
    iq, _ = synth.synthesize(cfg)
    raw = np.asarray(iq).reshape(-1, 2)
    blk = 200000                                                 # samples: 10 000 decimated per feed
    assert cfg.oversample == 20
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, max_block_bytes=4 * blk)
    rx.debug_option("referee", 0)
    rx.capture_enable()
    frames, recs, wins = feed_pieces(rx, raw, [blk])
    assert raw.shape[0] // 20 > 3 * (1 << 17) and len(recs) == rx.stats()["bursts"] >= 30
    across = [r for r in recs if (r["iq_first"] & ((1 << 17) - 1)) + r["iq_count"] > (1 << 17)]
    assert len(across) >= 1, "no window lay across the ring's end"
    assert {(f["chan"], f["burst_ord"]) for f in frames} <= set(by_key(recs))
    for r, w in zip(recs, wins):
        check_quality(r, w, label=f"{r['chan']}/{r['burst_ord']}")
    rx.close()


# ---------------------------------------------------------------- 7. the tool
def test_tool(vh, tmp_path):
    import os
    import subprocess
    from dumpvdl2_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    wav = os.path.join(root, "tests", "golden", "vdl2_model_16b_1050kHz.wav")
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    out, iqf = str(tmp_path / "bursts.txt"), str(tmp_path / "bursts.cf32")
    base = [exe, "--iq-file", wav, "--sample-format", "S16_LE"]
    p0 = subprocess.run(base, check=True, capture_output=True, text=True, timeout=120)
    p1 = subprocess.run(base + ["--bursts-out", out, "--bursts-iq", iqf, "--bursts-pre", "100", "--bursts-post", "5"], check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stdout.count("[S:") == 2 and p0.stderr == p1.stderr
    lines = open(out).read().splitlines()
    head = dict(l[2:].split(" ", 1) for l in lines if l.startswith("# "))
    rows = [l.split() for l in lines if not l.startswith("#")]
    assert set(head) == {k for k, _ in vh.CaptureInfo._fields_ if k not in ("struct_size", "reserved", "reserved2")}
    assert (int(head["pre_samples"]), int(head["post_samples"]), int(head["flags"]), int(head["bursts"]), int(head["iq_dropped"])) == (100, 5, 0, 1, 0)
    names = [k for k in vh.BURST_DTYPE.names if k != "reserved"]
    assert len(rows) == 1 and len(rows[0]) == len(names)
    r = dict(zip(names, rows[0]))
    assert int(r["freq"]) == CF and int(r["frames"]) == 2 and int(r["iq_off"]) == 0 and int(r["iq_first"]) == int(r["sync_sample"]) - 100
    assert int(r["iq_count"]) == int(r["end_sample"]) + 5 - int(r["iq_first"]) + 1 == int(head["iq_samples"])
    iq = np.fromfile(iqf, dtype=np.float32).reshape(-1, 2)
    assert iq.shape[0] == int(r["iq_count"])
    rec = {k: (float(v) if "." in v or "e" in v or k in ("dphi", "prev_phase") else int(v)) for k, v in r.items()}
    check_quality(rec, iq.view(np.complex64).reshape(-1), label="tool")      # (%.9g prints a float32 exactly)
    # failed only: the file's one burst decoded, nothing is written
    p2 = subprocess.run(base + ["--bursts-out", out, "--bursts-failed-only"], check=True, capture_output=True, text=True, timeout=120)
    lines = open(out).read().splitlines()
    assert p2.stdout == p0.stdout and [l for l in lines if not l.startswith("#")] == [] and "# bursts 1" in lines and "# flags 1" in lines
