"""The transmission capture on the GPU (include/vdl2hip.h, "Transmission capture"; kernels: dumpvdl2_amd/csrc/txcap.h): for every
transmission the transmission log closes, the channel's decimated IQ around it and a power spectrum of the channel during it.

Records are held to the model (tests/txcap_model.py) run on the device's OWN decimated stream, read back with read_decimated() behind
every feed: with the referee off that is the stream the tap read.  Every record and every bin of every record is compared: the
integer fields and the IQ exactly (the IQ by its bits), power[] within the stated bound of the float64 definition.  Oversample 10 and
at most 3 channels, captures of 1 s at the most, the referee off unless stated."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import txcap_model as cm
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
E_INVAL = -1
NOISE = 0.0005


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def cut_sizes(n, sizes):
    out, k, i = [], 0, 0
    while k < n:
        d = min(sizes[i % len(sizes)], n - k)
        out.append(d)
        k += d
        i += 1
    return out


def tone_stream(n_in, tones, seed, rate=1050000.0):
    """int16 (n_in, 2): noise and, per (first, last_exclusive, hz, amplitude) in input samples, a tone hz off the centre"""
    rng = np.random.default_rng(seed)
    x = NOISE * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    for a, b, hz, amp in tones:
        n = np.arange(a, b)
        x[a:b] += amp * np.exp(1j * (0.3 + 2 * np.pi * hz / rate * n))
    iq = np.stack([x.real, x.imag], axis=1)
    return np.clip(np.rint(32768.0 * iq), -32768, 32767).astype("<i2")


def run(vh, raw, freqs, sizes, act=(105, -40.0, 0), referee=0, cap=None, log=True, search=False, bursts=False, block=None, position=0, read_y=True,
        cf=CF, os_=10, max_ppm=0.0, late=None, reads=None, **kw):
    """raw: int16 (n, 2), fed in pieces of `sizes` samples with a sync() behind each; behind every feed the new decimated samples of
    every channel are read back.  cap: the keywords of Receiver.txcap_enable(), None: the tap stays off.  late: the log and the tap
    are enabled only ahead of feed number `late`.  position: debug_set_position() -> dict"""
    rx = vh.Receiver(cf, freqs, os_, vh.FMT_S16LE, max_ppm, max_block_bytes=4 * (block or max(sizes)), **kw)
    rx.debug_option("referee", referee)
    if position:
        rx.debug_set_position(position)
    base = position // os_

    def taps():
        if log:
            rx.txlog_enable()
        if search:
            rx.txsearch_enable()
        if cap is not None:
            rx.txcap_enable(**cap)
    if act:
        rx.activity_enable(act[0], act[1], act[2], 0)
    if late is None:
        taps()
    if bursts:
        rx.capture_enable(64, 0)
    chans = range(rx.chan_first, rx.chan_first + rx.chan_count)
    y = {c: [] for c in chans}
    frames, tx_feeds, cap_feeds, txs, burst_recs = [], [], [], [], []
    on = late is None

    def collect():
        nonlocal frames
        frames += rx.drain()
        if log and on:
            tx_feeds.append(rx.txlog_read())
        if search and on:
            txs.append(rx.txsearch_read())
        if cap is not None and on:
            cap_feeds.append(rx.txcap_read(**(reads or {})))
        if bursts:
            b, w = rx.capture_read()
            burst_recs.append((b, [x.tobytes() for x in w]))
    k = made = 0
    for i, d in enumerate(sizes):
        if late is not None and i == late:
            taps()
            on = True
        rx.feed(raw[k:k + d])
        k += d
        rx.sync()
        collect()
        now = k // os_ if not kw.get("input_rate") else None
        if read_y and now is not None and now > made:
            for c in chans:
                y[c].append(rx.read_decimated(c, base + made, now - made))
            made = now
    out = dict(frames=frames, tx_feeds=tx_feeds, cap_feeds=cap_feeds, txs=np.concatenate(txs) if txs else None, bursts=burst_recs,
               info=rx.txcap_info() if cap is not None else None, loginfo=rx.txlog_info() if log else None,
               counters=[[list(rx.counters(c).values()), list(rx.avlc_counters(c).values())] for c in chans],
               act=rx.activity() if act else None, base=base, cap=cap)
    if kw.get("input_rate") and read_y:
        # (a resampling receiver makes as many decimated samples as its resampler gives it: ask until nothing more comes)
        for c in chans:
            y[c].append(rx.read_decimated(c, 0, 1 << 16))
    out["y"] = {c: np.concatenate(v).view(np.complex64).reshape(-1) for c, v in y.items()} if read_y else None
    rx.close()
    return out


def records(res):
    r = [f[0] for f in res["cap_feeds"]]
    return np.concatenate(r) if r else np.zeros(0)


def check_model(vh, res, label=""):
    """every capture record beside the log's record of the same feed and index: the integer fields against the model's plan of that
    feed, the IQ by its bits against the stream, every bin of power[] within the bound, the host's fields against the log's; the
    totals of the info structure -> (records, the largest error / bound seen)"""
    cap = res["cap"]
    flags = (cm.IQ if cap.get("iq", True) else 0) | (cm.SPECTRUM if cap.get("spectrum", True) else 0)
    n = cap.get("nfft", 0) or cm.DEF_N
    w = vh.spectrum_window(n, cap.get("window", vh.WIN_HANN))
    base, tot, worst = res["base"], dict(records=0, iq_samples=0, iq_dropped=0, spectra=0, spectra_dropped=0), 0.0
    tx_feeds = res["tx_feeds"]
    assert len(tx_feeds) == len(res["cap_feeds"]), label
    for fi, (tx, (recs, wins, spectra)) in enumerate(zip(tx_feeds, res["cap_feeds"])):
        assert len(tx) == len(recs), (label, fi, len(tx), len(recs))
        want, _ = cm.plan(tx, flags, cap.get("pre", 0), cap.get("post", 0), cap.get("max_iq_samples", 0), n, cap.get("pool_samples", 0), cap.get("pool_spectra", 0))
        for i, (t, g, m) in enumerate(zip(tx, recs, want)):
            at = (label, fi, i)
            for k in cm.INT_FIELDS:
                assert int(g[k]) == m[k], (at, k, int(g[k]), m[k])
            assert (int(g["frames"]), int(g["frames_ok"]), g["reserved"].tolist()) == (int(t["frames"]), int(t["frames_ok"]), [0, 0]), at
            ys = res["y"][int(g["chan"])]
            lo = m["win_first"] - base
            assert wins[i].size == m["iq_count"] and np.array_equal(wins[i].view(np.uint32), ys[lo:lo + m["iq_count"]].view(np.uint32)), at
            if m["spec"] is None:
                assert spectra[i].size == 0, at
            else:
                worst = max(worst, cm.check_spectrum(spectra[i], cm.stream_get(ys, base), int(t["first_sample"]), int(t["last_sample"]), n, w, at))
                tot["spectra"] += 1
            tot["records"] += 1
            tot["iq_samples"] += m["iq_count"]
            tot["iq_dropped"] += bool(m["flags"] & cm.NO_ROOM)
            tot["spectra_dropped"] += bool(m["flags"] & cm.NO_SPECTRUM)
    assert {k: res["info"][k] for k in tot} == tot, (label, res["info"], tot)
    return tot["records"], worst


def same_integers(a, b, label=""):
    """two runs of one input cut differently: the records in an order that does not depend on the cut, every integer field but the
    two room flags identical"""
    ra, rb = (np.sort(records(r), order=["chan", "first_bin"]) for r in (a, b))
    assert len(ra) == len(rb), (label, len(ra), len(rb))
    for x, y in zip(ra, rb):
        for k in cm.INT_FIELDS:
            if k == "flags":
                assert int(x[k]) & ~cm.ROOM_FLAGS == int(y[k]) & ~cm.ROOM_FLAGS, (label, x, y)
            elif k != "iq_count" or not (int(x["flags"]) | int(y["flags"])) & cm.NO_ROOM:
                assert x[k] == y[k], (label, k, x, y)
    return len(ra)


BOTH = dict(iq=True, spectrum=True)


# ---------------------------------------------------------------- 1. tones against the model; the axis
def test_tones_and_orientation(vh):
    """three tones: at +3000 Hz, at -3000 Hz and at the centre, fed in three pieces"""
    n = 600000
    raw = tone_stream(n, [(60000, 160000, 3000.0, 0.05), (250000, 322050, -3000.0, 0.05), (420000, 480000, 0.0, 0.02)], 11)
    for nfft in (256, 64, 1024):
        res = run(vh, raw, [CF], cut_sizes(n, [200000]), cap=dict(BOTH, pre=100, post=105, nfft=0 if nfft == 256 else nfft))
        nrec, worst = check_model(vh, res, f"tones N={nfft}")
        recs, spectra = records(res), [s for f in res["cap_feeds"] for s in f[2]]
        print(f"N={nfft}: {nrec} records, largest error / bound {worst:.3f}, window lengths {[int(r['iq_count']) for r in recs]}")
        assert nrec == 3 and all(int(r["nfft"]) == nfft for r in recs)
        for s, hz in zip(spectra, (3000.0, -3000.0, 0.0)):
            want = nfft // 2 + int(round(hz * nfft / 105000.0))
            assert int(np.argmax(s)) == want, (nfft, hz, int(np.argmax(s)), want)
            m = vh.txcap_measure(s)
            assert m == cm.measure(s) and m["peak_bin"] == want and (hz == 0.0 or np.sign(m["centroid_hz"]) == np.sign(hz))
        assert int(np.argmax(spectra[1])) == nfft - int(np.argmax(spectra[0])), "the mirror bin"


# ---------------------------------------------------------------- 2. the smallest shapes: bins of 64, a transform of 128
EDGE_ACT = (64, -29.0, 2)           # (a bin is busy if more than half of it is covered by a tone of -26 dBFS)
EDGE_CAP = dict(BOTH, pre=37, post=128, nfft=128)
EDGE_N = 700000


@functools.lru_cache(maxsize=1)
def edge_stream():
    """tones that cover 1, 2 and 3 bins of 64 decimated samples exactly (extents of 64, 128 and 192: S = 0, 1, 2), one of 15 040
    decimated samples (234 segments: four pieces of 64) and one of 5 bins"""
    t = [(640 * a, 640 * (a + m), 1500.0, 0.05) for a, m in ((20, 1), (60, 2), (100, 3), (200, 235), (700, 5))]
    return tone_stream(EDGE_N, t, 12)


@pytest.fixture(scope="module")
def edge_whole(vh):
    res = run(vh, edge_stream(), [CF], [EDGE_N], act=EDGE_ACT, cap=EDGE_CAP)
    nrec, worst = check_model(vh, res, "edge whole")
    recs = records(res)
    ext = [int(t["last_sample"]) - int(t["first_sample"]) + 1 for f in res["tx_feeds"] for t in f]
    print(f"edge: extents {ext}, segments {[int(r['segments']) for r in recs]}, largest error / bound {worst:.3f}")
    assert nrec == 5 and ext[:3] == [64, 128, 192] and [int(r["segments"]) for r in recs[:3]] == [0, 1, 2]
    assert [int(r["flags"]) for r in recs[:3]] == [cm.SHORT, 0, 0] and int(recs[3]["segments"]) > 3 * 64
    assert not res["cap_feeds"][0][2][0].any() and res["cap_feeds"][0][2][0].size == 128, "a short extent's power[] is all zero"
    # windows of 64 m + 37 + 128 pairs are all odd: their places in the pool alternate between even and odd, cap_copy's two shapes
    assert all(int(r["iq_count"]) % 2 == 1 for r in recs) and [int(r["iq_off"]) % 2 for r in recs] == [0, 1, 0, 1, 0]
    return res


def test_edge_extents(edge_whole):
    """extents of 64, 128 and 192 samples (S = 0 with _SHORT, 1, 2), one of several pieces, in one feed: the fixture's own assertions"""


def edge_cuts(res):
    """cuts in input samples: inside the long transmission, between its last busy bin and its close (bin last + 3), and - any cut
    inside a transmission - such that a window begins before the closing feed's first sample"""
    t = res["tx_feeds"][0][3]
    first, last = int(t["first_sample"]), int(t["last_sample"])
    return [10 * (first + 5000) + 3, 10 * (last + 70)]


@pytest.mark.parametrize("which", ["inside", "before_close", "both"])
def test_edge_cuts(vh, edge_whole, which):
    a, b = edge_cuts(edge_whole)
    cuts = dict(inside=[a], before_close=[b], both=[a, b])[which]
    sizes = list(np.diff([0] + cuts + [EDGE_N]))
    res = run(vh, edge_stream(), [CF], [int(s) for s in sizes], act=EDGE_ACT, cap=EDGE_CAP, block=EDGE_N)
    assert check_model(vh, res, f"edge {which}")[0] == 5
    assert same_integers(res, edge_whole, which) == 5
    # the long transmission's record comes with the feed behind the cut, and its window began before that feed's first sample
    fi = [i for i, f in enumerate(res["cap_feeds"]) if any(int(r["segments"]) > 192 for r in f[0])][0]
    assert fi >= 1 and int(records(res)[3]["win_first"]) < sum(sizes[:fi]) // 10
    # where the two runs' streams agree over a record's extent, so do the bytes of its spectrum
    sa, sb = [s for f in res["cap_feeds"] for s in f[2]], [s for f in edge_whole["cap_feeds"] for s in f[2]]
    exact = 0
    for r, x, y in zip(records(res), sa, sb):
        lo, hi = int(r["win_first"]), int(r["win_last"]) + 1
        if np.array_equal(res["y"][0][lo:hi].view(np.uint64), edge_whole["y"][0][lo:hi].view(np.uint64)):
            assert x.tobytes() == y.tobytes()
            exact += 1
    assert exact >= 3


# ---------------------------------------------------------------- 3. a carrier longer than the longest extent
def test_clipped(vh):
    n = 800000
    raw = tone_stream(n, [(50000, 680000, 2000.0, 0.05)], 5)
    res = run(vh, raw, [CF], cut_sizes(n, [250000]), cap=dict(BOTH, pre=4096, post=105))
    assert check_model(vh, res, "clipped")[0] == 1
    r, t = records(res)[0], np.concatenate(res["tx_feeds"])[0]
    assert int(t["last_sample"]) - int(t["first_sample"]) + 1 > 57344 + 4096
    assert int(r["flags"]) == cm.CLIPPED and int(r["win_first"]) == int(t["last_sample"]) - 57343 and int(r["win_last"]) == int(t["last_sample"]) + 105
    assert int(r["segments"]) == (57344 - 256) // 128 + 1 and int(r["iq_count"]) == 57344 + 105


# ---------------------------------------------------------------- 4. the ring wraps inside a window
def test_ring_wraps_at_position(vh):
    """blocks of 100 000 samples make the ring 2^17 decimated samples; the stream begins 3 000 samples ahead of a multiple of that"""
    n = 200000
    k0 = 5 * (1 << 17) - 3000
    raw = tone_stream(n, [(10000, 60000, -4000.0, 0.05), (100000, 130500, 1000.0, 0.05)], 13)
    res = run(vh, raw, [CF], cut_sizes(n, [100000]), cap=dict(BOTH, pre=200, post=64, nfft=128), position=10 * k0)
    assert check_model(vh, res, "wrap")[0] == 2
    r = records(res)[0]
    assert int(r["win_first"]) >> 17 != int(r["win_last"]) >> 17 and int(r["win_first"]) > k0, "no window lay across the ring's end"


# ---------------------------------------------------------------- 5. room
def keyed(n_in, seed, count=5):
    return tone_stream(n_in, [(40000 + 31500 * i, 40000 + 31500 * i + 5250 + 10 * (i % 2), 1000.0 * i, 0.05) for i in range(count)], seed)


def test_rooms(vh):
    n = 250000
    raw = keyed(n, 7)
    full = run(vh, raw, [CF], [n], cap=dict(BOTH, pre=64, post=64, nfft=128))
    assert check_model(vh, full, "full")[0] == 5
    counts = [int(r["iq_count"]) for r in records(full)]
    tight = run(vh, raw, [CF], [n], cap=dict(BOTH, pre=64, post=64, nfft=128, pool_samples=counts[0] + counts[1] + counts[2] - 1, pool_spectra=2))
    assert check_model(vh, tight, "tight")[0] == 5
    rt = records(tight)
    assert [bool(int(r["flags"]) & cm.NO_ROOM) for r in rt] == [False, False, True, True, True] and tight["info"]["iq_dropped"] == 3
    assert [bool(int(r["flags"]) & cm.NO_SPECTRUM) for r in rt] == [False, False, True, True, True] and tight["info"]["spectra_dropped"] == 3
    for i in range(2):      # the surviving prefix is the full run's
        assert tight["cap_feeds"][0][1][i].tobytes() == full["cap_feeds"][0][1][i].tobytes() and tight["cap_feeds"][0][2][i].tobytes() == full["cap_feeds"][0][2][i].tobytes()
    trunc = run(vh, raw, [CF], [n], cap=dict(BOTH, pre=64, post=64, nfft=128, max_iq_samples=501))
    assert check_model(vh, trunc, "truncated")[0] == 5
    assert all(int(r["flags"]) & cm.TRUNCATED and int(r["iq_count"]) == 501 for r in records(trunc))
    for a, b in zip(trunc["cap_feeds"][0][1], full["cap_feeds"][0][1]):
        assert a.tobytes() == b[:501].tobytes(), "the first samples of the window survive"
    # one kind only
    iq = run(vh, raw, [CF], [n], cap=dict(iq=True, spectrum=False, pre=64, post=64))
    sp = run(vh, raw, [CF], [n], cap=dict(iq=False, spectrum=True, nfft=128))
    assert check_model(vh, iq, "iq only")[0] == 5 and check_model(vh, sp, "spectrum only")[0] == 5
    assert all(int(r["nfft"]) == 0 for r in records(iq)) and all(int(r["iq_count"]) == 0 for r in records(sp))
    assert [s.tobytes() for s in sp["cap_feeds"][0][2]] == [s.tobytes() for s in full["cap_feeds"][0][2]]
    # reading with buffers that hold one record's worth: what does not fit stays queued
    small = run(vh, raw, [CF], [n], cap=dict(BOTH, pre=64, post=64, nfft=128), reads=dict(cap_recs=4, cap_pairs=max(counts), cap_floats=128))
    assert check_model(vh, small, "small reads")[0] == 5


# ---------------------------------------------------------------- 6. the log enabled inside a transmission
def test_partial(vh):
    n = 300000
    raw = tone_stream(n, [(50000, 150000, 500.0, 0.05), (200000, 230000, 500.0, 0.05)], 14)
    res = run(vh, raw, [CF], [100000, 100000, 100000], cap=dict(BOTH, pre=64, post=0, nfft=128), late=1)
    assert check_model(vh, res, "partial")[0] == 2
    r = records(res)
    assert int(r[0]["flags"]) & cm.PARTIAL and not int(r[1]["flags"]) & cm.PARTIAL


# ---------------------------------------------------------------- 7. a shard, a resampling receiver, the referee
def test_shard(vh):
    from test_gpu_txlog import make_stream
    n = 315000
    raw, freqs, _ = make_stream(3, n, 78, step=100000)
    cap = dict(BOTH, pre=32, post=32, nfft=128)
    full = run(vh, raw, freqs, cut_sizes(n, [160000]), act=(105, -40.0, 1), cap=cap)
    assert check_model(vh, full, "full")[0] >= 4
    shard = run(vh, raw, freqs, cut_sizes(n, [160000]), act=(105, -40.0, 1), cap=cap, chan_first=1, chan_count=2)
    check_model(vh, shard, "shard")
    rs, rf = records(shard), records(full)
    assert set(rs["chan"].tolist()) == {1, 2} and all(int(r["freq"]) == freqs[int(r["chan"])] for r in rs)
    keep = lambda r: np.array([(x["chan"], x["first_bin"], x["win_first"], x["win_last"], x["iq_count"], x["segments"]) for x in r if x["chan"] in (1, 2)])
    assert np.array_equal(keep(rs), keep(rf))
    # a group of two on one device: vdl2hip_group_ctx(g, k) is the handle of member k's channels
    g = vh.ReceiverGroup(CF, freqs + [freqs[-1] + 100000], [0, 0], 10, vh.FMT_S16LE, max_block_bytes=4 * 160000)
    for i in range(g.size()):
        assert g.L.vdl2hip_debug_option(g.member(i), b"referee", 0) == 0
    g.activity_enable(105, -40.0, 1, 0)
    g.txlog_enable()
    g.txcap_enable(**cap)
    k = 0
    for d in cut_sizes(n, [160000]):
        g.feed(raw[k:k + d])
        k += d
    g.sync()
    seen = 0
    for i in range(2):
        recs, wins, spectra = g.txcap_read(i)
        assert set(recs["chan"].tolist()) <= {2 * i, 2 * i + 1} and g.txcap_info(i)["records"] == len(recs) == len(g.txlog_read(i))
        seen += int(np.count_nonzero(recs["chan"] < 3))
        for r, wv in zip(recs, wins):
            if int(r["chan"]) < 3:
                j = [q for q, x in enumerate(rf) if (int(x["chan"]), int(x["first_bin"])) == (int(r["chan"]), int(r["first_bin"]))]
                assert len(j) == 1 and wv.size == int(rf[j[0]]["iq_count"]) and (int(r["win_first"]), int(r["segments"])) == (int(rf[j[0]]["win_first"]), int(rf[j[0]]["segments"]))
    assert seen == len(rf)
    g.txcap_disable()
    g.close()


def test_resampling_receiver(vh):
    """IQ at 1 MS/s into a receiver of oversample 10: the tap reads the channeliser's stream behind the resampler"""
    n = 400000
    raw = tone_stream(n, [(50000, 120000, 3000.0, 0.05), (200000, 260000, -3000.0, 0.05)], 15, rate=1000000.0)
    res = run(vh, raw, [CF], cut_sizes(n, [200000]), cap=dict(BOTH, pre=100, post=105), input_rate=1000000)
    assert check_model(vh, res, "resampled")[0] == 2
    s = [x for f in res["cap_feeds"] for x in f[2]]
    assert int(np.argmax(s[0])) == 128 + 7 and int(np.argmax(s[1])) == 128 - 7


def test_referee_single_feed(vh):
    """the referee on, one feed: the tap reads the stream as the feed's referee left it, which is what read_decimated() returns"""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(freqs=synth.channel_plan(2, spacing=100000), oversample=10, duration_s=0.5, mean_gap_s=0.08, max_payload=200, seed=4243)
    iq, _ = synth.synthesize(cfg)
    raw = np.asarray(iq).reshape(-1, 2)
    res = run(vh, raw, list(cfg.freqs), [raw.shape[0]], os_=cfg.oversample, cf=cfg.centerfreq, act=(105, -40.0, 1), referee=1, cap=dict(BOTH, pre=256, post=105))
    nrec, worst = check_model(vh, res, "referee")
    assert nrec >= 4 and len(res["frames"]) >= 2
    print(f"referee on: {nrec} records, {len(res['frames'])} frames, largest error / bound {worst:.3f}")


# ---------------------------------------------------------------- 8. the reference's test vector
def wav_run(vh, wav, cap, **kw):
    raw = wav.view("<i2").reshape(-1, 2)
    return run(vh, raw, [CF], cut_sizes(raw.shape[0], [80000]), act=(105, -30.0, 0), cap=cap, **kw)


def test_reference_wav(vh, golden_wav):
    on = wav_run(vh, golden_wav, dict(BOTH, pre=256, post=105), search=True)
    assert check_model(vh, on, "wav")[0] == 1
    r, tx = records(on)[0], np.concatenate(on["tx_feeds"])[0]
    assert len(on["frames"]) == 2 and int(tx["frames_ok"]) == 2 and int(r["frames_ok"]) == 2 and int(r["frames"]) == 2
    assert (int(r["chan"]), int(r["first_bin"])) == (int(on["txs"][0]["chan"]), int(on["txs"][0]["first_bin"])) and int(on["txs"][0]["why"]) == vh.TXS_DECODED
    m = vh.txcap_measure(on["cap_feeds"][[i for i, f in enumerate(on["cap_feeds"]) if len(f[0])][0]][2][0])
    print(f"golden vector's burst: obw_hz {m['obw_hz']:.0f}, centroid_hz {m['centroid_hz']:.0f}, peak_hz {m['peak_hz']:.0f}")
    # _UNDECODED_ONLY removes exactly the decoded transmission's record; the device still captured it
    und = wav_run(vh, golden_wav, dict(BOTH, pre=256, post=105, undecoded_only=True), search=True)
    assert len(records(und)) == 0 and und["info"]["records"] == 1 and und["info"]["flags"] == 7 and und["info"]["spectra"] == 1
    assert und["info"]["iq_samples"] == on["info"]["iq_samples"] == int(r["iq_count"])
    off = wav_run(vh, golden_wav, None, search=True)
    assert_frames_equal(off["frames"], on["frames"], label="capture on")
    assert off["counters"] == on["counters"] and off["txs"].tobytes() == on["txs"].tobytes()
    assert np.concatenate(off["tx_feeds"]).tobytes() == np.concatenate(on["tx_feeds"]).tobytes()


# ---------------------------------------------------------------- 9. non-interference, determinism, off is off
def test_non_interference(vh):
    """a synthetic band with bursts that decode: with the tap on, frames, both counter sets, y, the activity results, the log's, the
    search's and the burst capture's records are the bytes of the run with it off; the same calls twice give the same bytes"""
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(freqs=synth.channel_plan(3, spacing=100000), oversample=10, duration_s=0.6, mean_gap_s=0.06, max_payload=300, seed=4244)
    iq, _ = synth.synthesize(cfg)
    raw = np.asarray(iq).reshape(-1, 2)
    sizes = cut_sizes(raw.shape[0], [250000])

    def one(cap):
        return run(vh, raw, list(cfg.freqs), sizes, os_=cfg.oversample, cf=cfg.centerfreq, act=(105, -40.0, 1), cap=cap, search=True, bursts=True)
    off, on, again = one(None), one(dict(BOTH, pre=128, post=105)), one(dict(BOTH, pre=128, post=105))
    assert check_model(vh, on, "band")[0] >= 6 and len(on["frames"]) >= 3
    for other in (on, again):
        assert_frames_equal(other["frames"], off["frames"], label="capture on")
        assert other["counters"] == off["counters"]
        for c in off["y"]:
            assert np.array_equal(other["y"][c].view(np.uint32), off["y"][c].view(np.uint32))
        for k, v in off["act"].items():
            assert k == "kernel_ms" or np.array_equal(np.asarray(v), np.asarray(other["act"][k])), k
        assert [t.tobytes() for t in other["tx_feeds"]] == [t.tobytes() for t in off["tx_feeds"]]
        assert other["txs"].tobytes() == off["txs"].tobytes()
        assert other["bursts"] == off["bursts"] and sum(len(b[0]) for b in off["bursts"]) >= 3
    flat = lambda r: [(f[0].tobytes(), [w.tobytes() for w in f[1]], [s.tobytes() for s in f[2]]) for f in r["cap_feeds"]]
    assert flat(on) == flat(again)


def test_off_is_off(vh):
    """with the tap never enabled what the process holds is what a run that never heard of it holds; on, it holds more; all of it
    goes back"""
    n = 250000
    raw = keyed(n, 7)
    base = vh.live_resources()
    held = []

    def one(cap):
        rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=4 * 125000)
        rx.debug_option("referee", 0)
        rx.activity_enable(105, -40.0, 0, 0)
        rx.txlog_enable()
        if cap:
            rx.txcap_enable(pre=64, post=64)
        for k in range(0, n, 125000):
            rx.feed(raw[k:k + 125000])
        rx.sync()
        held.append(vh.live_resources())
        out = (rx.drain(), rx.txlog_read().tobytes(), list(rx.counters(0).values()), rx.read_decimated(0, 0, n // 10).tobytes())
        rx.close()
        return out
    a, b, c = one(False), one(False), one(True)
    assert a == b == c and len(a[1]) == 5 * vh.TX_DTYPE.itemsize
    assert held[0] == held[1] and held[2]["device"] > held[0]["device"] and held[2]["pinned"] > held[0]["pinned"]
    assert vh.live_resources() == base


# ---------------------------------------------------------------- 10. arguments and switching
def test_arguments_and_switching(vh):
    n = 250000
    raw = keyed(n, 7)
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=4 * n)
    rx.debug_option("referee", 0)
    L = rx.L
    good = dict(struct_size=40, flags=3, pre_samples=64, post_samples=64)
    cfg = lambda **kw: C.byref(vh.TxcapCfg(**{**good, **kw}))
    info = vh.TxcapInfo(C.sizeof(vh.TxcapInfo))
    one = np.zeros(1, dtype=vh.TXC_DTYPE)
    off = lambda: L.vdl2hip_txcap_info_get(rx.h, C.byref(info)) == E_INVAL and L.vdl2hip_txcap_read(rx.h, one.ctypes.data, 1, None, 0, None, None, 0, None) == E_INVAL
    # the log is off (and the monitor): refused, and nothing to ask of a capture that is off
    assert L.vdl2hip_txcap_enable(rx.h, cfg()) == E_INVAL and off()
    assert L.vdl2hip_txcap_disable(rx.h) == 0
    rx.activity_enable(105, -40.0, 0, 0)
    assert L.vdl2hip_txcap_enable(rx.h, cfg()) == E_INVAL and off()
    rx.txlog_enable()
    for k in range(0, 60000, 10000):                              # (a slot's input buffer and copy event are made on the slot's first feed)
        rx.feed(raw[k:k + 10000])
        rx.sync()
    rx.txlog_read()
    with_log = vh.live_resources()
    rx.txcap_enable(pre=64, post=64)
    assert vh.live_resources()["device"] > with_log["device"] and vh.live_resources()["pinned"] > with_log["pinned"]
    rx.feed(raw[60000:150000])
    rx.sync()
    s0 = rx.txcap_info()
    assert s0["records"] >= 2 and s0["nfft"] == 256 and s0["pool_samples"] == 1 << 20 and s0["pool_spectra"] == 1024
    for bad in (dict(struct_size=36), dict(struct_size=44), dict(flags=0), dict(flags=4), dict(flags=8), dict(flags=11), dict(reserved=1), dict(pre_samples=4097),
                dict(post_samples=106), dict(nfft=32), dict(nfft=100), dict(nfft=2048), dict(window=3), dict(pool_samples=(1 << 24) + 1),
                dict(nfft=1024, pool_spectra=(1 << 14) + 1), dict(pool_spectra=(1 << 16) + 1)):
        assert L.vdl2hip_txcap_enable(rx.h, cfg(**bad)) == E_INVAL, bad
        assert {k: v for k, v in rx.txcap_info().items() if k != "kernel_ms"} == {k: v for k, v in s0.items() if k != "kernel_ms"}, bad
    assert L.vdl2hip_txcap_enable(rx.h, None) == E_INVAL and L.vdl2hip_txcap_enable(None, cfg()) == E_INVAL
    assert L.vdl2hip_txcap_info_get(rx.h, C.byref(vh.TxcapInfo(80))) == E_INVAL
    assert L.vdl2hip_txcap_read(rx.h, None, 1, None, 0, None, None, 0, None) == E_INVAL and L.vdl2hip_txcap_read(rx.h, None, 0, None, 0, None, None, 0, None) == 0
    # a record whose IQ or spectrum does not fit stays queued
    used = C.c_size_t(7)
    assert L.vdl2hip_txcap_read(rx.h, one.ctypes.data, 1, None, 0, C.byref(used), None, 0, None) == 0 and used.value == 0
    recs, wins, spectra = rx.txcap_read()
    assert len(recs) == s0["records"] and all(w.size == int(r["iq_count"]) > 0 for w, r in zip(wins, recs)) and all(s.size == 256 for s in spectra)
    # the largest values are taken
    rx.txcap_enable(pre=4096, post=105, nfft=1024, pool_samples=1 << 24, pool_spectra=1 << 14, window=vh.WIN_BH4)
    assert rx.txcap_info()["records"] == 0 and rx.txcap_info()["window"] == vh.WIN_BH4
    # switched off by txlog_disable(), txlog_enable(), activity_enable() and activity_disable(); everything of it given back
    rx.txlog_disable()
    assert off()
    rx.txlog_enable(); rx.txcap_enable(); rx.txlog_enable()
    # (all but the page-locked staging buffer the feed above made it grow: that one stays until the receiver goes, like the burst capture's)
    assert off() and vh.live_resources() == dict(with_log, pinned=with_log["pinned"] + 1)
    rx.txcap_enable(); rx.activity_enable(105, -40.0, 0, 0)
    assert off()
    rx.txlog_enable(); rx.txcap_enable(); rx.txsearch_enable(); rx.activity_disable()
    assert off()
    # a hang time that reaches further back than the ring is sure to hold is refused, as the search refuses it
    rx.activity_enable(105, -40.0, 40, 0); rx.txlog_enable()
    base = vh.live_resources()
    assert L.vdl2hip_txcap_enable(rx.h, cfg()) == E_INVAL and off() and vh.live_resources() == base
    rx.activity_enable(105, -40.0, 38, 0); rx.txlog_enable()
    rx.txcap_enable(post=39 * 105)
    assert L.vdl2hip_txcap_enable(rx.h, cfg(post_samples=39 * 105 + 1)) == E_INVAL and rx.txcap_info()["post_samples"] == 39 * 105
    rx.txcap_disable()
    assert off() and vh.live_resources() == base
    rx.txcap_enable()                                             # destroyed with the capture on
    rx.feed(raw[150000:])
    rx.close()


# ---------------------------------------------------------------- 11. the tool
def test_tool(vh, tmp_path, golden_wav):
    import subprocess
    from dumpvdl2_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    wav = os.path.join(root, "tests", "golden", "vdl2_model_16b_1050kHz.wav")
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    out, iqf, spf = str(tmp_path / "txc.txt"), str(tmp_path / "txc.cf32"), str(tmp_path / "txc.f32")
    base = [exe, "--iq-file", wav, "--sample-format", "S16_LE", "--activity-threshold", "-30"]
    p0 = subprocess.run(base, check=True, capture_output=True, text=True, timeout=120)
    p1 = subprocess.run(base + ["--tx-capture-out", out, "--tx-iq", iqf, "--tx-spectra", spf, "--tx-capture-nfft", "128"], check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stdout.count("[S:") == 2
    lines = open(out).read().splitlines()
    head = " ".join(l[2:] for l in lines[:2]).split()
    hd = dict(zip(head[0::2], head[1::2]))
    rows = [l.split() for l in lines[2:]]
    assert (int(hd["flags"]), int(hd["nfft"]), int(hd["records"]), int(hd["spectra"]), int(hd["pre_samples"]), int(hd["post_samples"])) == (3, 128, 1, 1, 256, 105)
    assert len(rows) == 1 and len(rows[0]) == 18
    names = [k for k in vh.TXC_DTYPE.names if k != "reserved"]
    r = dict(zip(names, (int(v) for v in rows[0][:13])))
    iq, sp = np.fromfile(iqf, dtype=np.complex64), np.fromfile(spf, dtype=np.float32)
    assert (r["iq_off"], r["spec_off"], r["iq_count"], r["nfft"], r["frames_ok"], r["flags"]) == (0, 0, iq.size, 128, 2, 0) and sp.size == 128
    assert iq.size == r["win_last"] - r["win_first"] + 1 == int(hd["iq_samples"])
    m = vh.txcap_measure(sp)
    assert int(rows[0][14]) == m["peak_bin"] and abs(float(rows[0][13]) - m["total"]) <= 1e-8 * m["total"]
    assert [round(m[k], 3) for k in ("peak_hz", "centroid_hz", "obw_hz")] == [float(v) for v in rows[0][15:]]
    # the tool gathers the file's blocks into one feed with the referee on: the same call sequence here gives the same IQ and spectrum
    raw = golden_wav.view("<i2").reshape(-1, 2)
    want = run(vh, raw, [CF], [raw.shape[0]], act=(105, -30.0, 0), referee=1, cap=dict(BOTH, pre=256, post=105, nfft=128))
    assert want["cap_feeds"][0][1][0].tobytes() == iq.tobytes() and want["cap_feeds"][0][2][0].tobytes() == sp.tobytes()
    p2 = subprocess.run(base + ["--tx-capture-out", out + "2", "--tx-capture-undecoded-only"], check=True, capture_output=True, text=True, timeout=120)
    lines2 = open(out + "2").read().splitlines()
    assert p2.stdout == p0.stdout and len(lines2) == 2 and " records 1 " in lines2[1] and lines2[0].startswith("# flags 6 ")
