"""Burst timing on the GPU (include/vdl2hip.h, "Burst timing"; kernel: dumpvdl2_amd/csrc/toa.h): of every burst handed to the burst
decoder the correlation with the unique word's waveform round the decoder's symbol clock, joined on the host with the frames it
produced.

Every record is held to the float64 model of tests/toa_model.py run on the receiver's own decimated stream, read back with
read_decimated() right after the feed that delivered the record: the curve within the model's bound, peak_lag the first argmax of the
delivered curve, toa_frac, rho and peak_sample exact from the delivered curve and the model's E_y, the phases within their bound.
The referee is off unless a test says otherwise (with it on, a later feed under way may rewrite a stretch of y while a burst is read;
one feed has no later feed).  Positions are compared across cuts only to 1e-3: the channeliser's stream is not bit-identical across
cuts."""
import ctypes as C

import numpy as np
import pytest

import cases
import toa_model as tm
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
E_INVAL = -1
SET_FIELDS = ("chan", "burst_ord", "sync_sample", "first_symbol", "nlags", "frames", "frames_ok")


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


@pytest.fixture(scope="module")
def s32(vh):
    return vh.toa_template()


def reader(rx, chan):
    def y_at(first, count):
        y = rx.read_decimated(chan, first, count)
        assert y.shape[0] == count, (chan, first, count, y.shape)
        return y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)
    return y_at


def check_records(rx, s32, recs, curves, label=""):
    """every record against the model on the decimated stream as it stands now; returns the largest curve error as a fraction of its bound"""
    worst = 0.0
    for r, cv in zip(recs, curves):
        has = not int(r["flags"]) & tm.NO_CURVE
        assert cv.size == (int(r["nlags"]) if has else 0)
        worst = max(worst, tm.check_record(r, cv if has else None, s32, reader(rx, int(r["chan"])), what=f"{label} {int(r['chan'])}/{int(r['burst_ord'])}"))
    return worst


def position(r):
    return int(r["peak_sample"]) + float(r["toa_frac"])


# ---------------------------------------------------------------- 1. the reference's test vector
def run_wav(vh, s32, wav, toa, referee, one_feed=False, position0=0, capture=True, **kw):
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE, max_block_bytes=wav.size if one_feed else 320000)
    rx.debug_option("referee", referee)
    if position0:
        rx.debug_set_position(position0)
    if toa:
        rx.toa_enable(**kw)
        if capture:
            rx.capture_enable()
    frames, recs, curves, caps = [], [], [], []
    step = wav.size if one_feed else 320000
    for k in range(0, wav.size, step):
        rx.feed(wav[k:k + step])
        rx.sync()
        if toa:
            r, cv = rx.toa_read()
            if not position0:
                worst = check_records(rx, s32, r, cv, label="wav")
                if len(r):
                    print(f"wav referee={referee}: curve error {worst:.4f} of its bound, peak_lag {int(r[0]['peak_lag'])}, toa_frac {float(r[0]['toa_frac']):+.4f}, "
                          f"rho {float(r[0]['rho']):.4f}, cfo {float(r[0]['cfo_hz']):+.2f} Hz, resid {float(r[0]['resid']):+.3e}")
            recs += list(r); curves += cv
            if capture:
                caps += rx.capture_read()[0]
        frames += rx.drain()
    info = rx.toa_info() if toa else None
    cnt = [list(rx.counters(0).values()), list(rx.avlc_counters(0).values())]
    rx.close()
    return frames, recs, curves, caps, info, cnt


@pytest.fixture(scope="module")
def wav_at_zero(vh, s32, golden_wav):
    return run_wav(vh, s32, golden_wav, True, 0)


@pytest.mark.parametrize("referee,one_feed", [(0, False), (1, True)])
def test_reference_wav(vh, s32, golden_wav, wav_at_zero, referee, one_feed):
    frames, recs, curves, caps, info, cnt = wav_at_zero if (referee, one_feed) == (0, False) else run_wav(vh, s32, golden_wav, True, referee, one_feed)
    assert len(frames) == 2 and len(recs) == 1 and len(caps) == 1
    r, cv, cap = recs[0], curves[0], caps[0]
    for f in frames:
        assert (f["sync_sample"], f["burst_ord"], f["chan"]) == (int(r["sync_sample"]), int(r["burst_ord"]), int(r["chan"]))
    assert int(r["frames"]) == 2 and int(r["frames_ok"]) == sum(f["avlc_status"] == vh.AVLC_OK for f in frames) and int(r["freq"]) == CF
    # the decoder's own figures, as the burst capture enabled beside it reports them
    assert np.float32(r["dphi"]) == np.float32(cap["dphi"]) and int(r["first_symbol"]) == cap["first_symbol"]
    assert int(r["nlags"]) == 17 and cv.size == 17 and int(r["flags"]) == 0 and int(r["curve_off"]) == 0
    assert int(r["peak_lag"]) == int(np.argmax(cv)) - 8 and int(r["peak_sample"]) == int(r["first_symbol"]) - 160 + int(r["peak_lag"])
    assert float(r["rho"]) > 0.5 and abs(int(r["peak_lag"])) <= 2                 # a clean burst: the template fits, the decoder's clock was near
    assert (info["bursts"], info["curves"], info["curves_dropped"], info["early"], info["edge"], info["max_lag"], info["pool_curves"], info["flags"]) == (1, 1, 0, 0, 0, 8, 4096, 0)
    # nothing else moves: the frames and counters of a run with the tap off
    f0, _, _, _, _, c0 = run_wav(vh, s32, golden_wav, False, referee, one_feed)
    assert_frames_equal(f0, frames, label="toa on")
    assert c0 == cnt


# ---------------------------------------------------------------- 2. bursts that straddle feeds, and the cut does not matter
def run_config2(vh, s32, sizes, **kw):
    cfg, iq, _, _ = cases.load("config2_1s")
    raw = np.asarray(iq).reshape(-1, 2)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=4 * max(sizes))
    rx.debug_option("referee", 0)
    rx.toa_enable(**kw)
    frames, recs, curves, per_feed, straddle = [], [], [], [], 0
    worst = 0.0
    k = i = 0
    while k < raw.shape[0]:
        d = min(sizes[i % len(sizes)], raw.shape[0] - k)
        k0 = k // cfg.oversample
        rx.feed(raw[k:k + d])
        k += d; i += 1
        rx.sync()
        r, cv = rx.toa_read()
        worst = max(worst, check_records(rx, s32, r, cv, label=f"feed {i}"))
        straddle += sum(int(x["sync_sample"]) < k0 for x in r)
        frames += rx.drain()
        recs += list(r); curves += cv; per_feed.append(len(r))
    st, info = rx.stats(), rx.toa_info()
    rx.close()
    return dict(frames=frames, recs=recs, curves=curves, st=st, info=info, straddle=straddle, worst=worst, per_feed=per_feed)


@pytest.fixture(scope="module")
def config2_pieces(vh, s32):
    return run_config2(vh, s32, [100000, 333333, 7])


def test_config2_in_pieces(vh, s32, config2_pieces):
    a = config2_pieces
    assert len(a["recs"]) == a["st"]["bursts"] == a["info"]["bursts"] > 8 and a["info"]["curves_dropped"] == 0 and a["info"]["curves"] == len(a["recs"])
    assert a["straddle"] >= 1, "no burst began in an earlier feed than the one that decoded it"
    print(f"config2 in pieces: {len(a['recs'])} bursts, {a['straddle']} across feeds, worst curve error {a['worst']:.4f} of its bound")
    for r, cv in zip(a["recs"], a["curves"]):
        assert int(r["peak_lag"]) == int(np.argmax(cv)) - 8
    joined = {(f["chan"], f["burst_ord"]) for f in a["frames"]}
    assert joined <= {(int(r["chan"]), int(r["burst_ord"])) for r in a["recs"]}
    for r in a["recs"]:
        mine = [f for f in a["frames"] if (f["chan"], f["burst_ord"]) == (int(r["chan"]), int(r["burst_ord"]))]
        assert int(r["frames"]) == len(mine) and int(r["frames_ok"]) == sum(f["avlc_status"] == vh.AVLC_OK for f in mine)
    # order: channel, then position, feed by feed
    at = 0
    for n in a["per_feed"]:
        order = [(int(r["chan"]), int(r["burst_ord"])) for r in a["recs"][at:at + n]]
        assert order == sorted(order)
        at += n
    # another cut: the same set of records, the same arrival times
    b = run_config2(vh, s32, [250000, 41])
    key = lambda r: tuple(int(r[k]) for k in SET_FIELDS)
    assert sorted(map(key, a["recs"])) == sorted(map(key, b["recs"]))
    pa = {key(r)[:2]: position(r) for r in a["recs"]}
    pb = {key(r)[:2]: position(r) for r in b["recs"]}
    diff = max(abs(pa[k] - pb[k]) for k in pa)
    print(f"two cuts: positions differ by at most {diff:.2e} sample")
    assert diff <= 1e-3


# ---------------------------------------------------------------- 3. room for curves
def test_pool_curves(vh, s32):
    cfg, iq, _, _ = cases.load("config2_1s")
    n = np.asarray(iq).size // 2
    one = run_config2(vh, s32, [n], pool_curves=1)                # one feed: every burst of the stream in it
    recs, curves = one["recs"], one["curves"]
    assert len(recs) == one["st"]["bursts"] >= 2
    assert not int(recs[0]["flags"]) & tm.NO_CURVE and curves[0].size == 17
    for r, cv in zip(recs[1:], curves[1:]):
        assert int(r["flags"]) & tm.NO_CURVE and int(r["curve_off"]) == 0 and cv.size == 0
    assert one["info"]["curves_dropped"] == len(recs) - 1 and one["info"]["curves"] == 1 and one["info"]["pool_curves"] == 1
    # (check_records has held the scalars of the records without a curve to the model) ... and they are those of the records with one
    full = run_config2(vh, s32, [n])
    assert len(full["recs"]) == len(recs) and full["info"]["curves_dropped"] == 0
    for a, b in zip(full["recs"], recs):
        for name in vh.BURST_TOA_DTYPE.names:
            if name not in ("flags", "curve_off"):
                assert a[name].tobytes() == b[name].tobytes(), (name, a, b)
        assert int(a["flags"]) | tm.NO_CURVE == int(b["flags"]) | tm.NO_CURVE


# ---------------------------------------------------------------- 4. hours into a stream
def test_position_past_2_32(vh, s32, golden_wav, wav_at_zero):
    """the stream begins at decimated sample 2^32 + 12345 - input sample 10 (2^32 + 12345): debug_set_position() counts input samples
    and takes multiples of the oversampling only, and peak_sample, a decimated sample, is to lie beyond 2^32"""
    _, base, _, _, _, _ = wav_at_zero
    p0 = 10 * (2 ** 32 + 12345)
    frames, recs, curves, _, info, _ = run_wav(vh, s32, golden_wav, True, 0, position0=p0, capture=False)
    assert len(recs) == 1 and len(frames) == 2
    r, b = recs[0], base[0]
    assert int(r["peak_sample"]) > 2 ** 32
    assert int(r["peak_sample"]) - int(r["sync_sample"]) == int(b["peak_sample"]) - int(b["sync_sample"]) and r["toa_frac"].tobytes() == b["toa_frac"].tobytes()
    assert int(r["peak_lag"]) == int(b["peak_lag"]) and int(r["flags"]) == int(b["flags"]) and np.array_equal(curves[0], wav_at_zero[2][0])


# ---------------------------------------------------------------- 5. refusals, switching, resources
def test_refusals_and_resources(vh, golden_wav):
    base = vh.live_resources()
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE)
    rx.debug_option("referee", 0)
    L = rx.L
    info = vh.ToaInfo(C.sizeof(vh.ToaInfo))
    rec = np.zeros(4, dtype=vh.BURST_TOA_DTYPE)
    off = lambda: L.vdl2hip_toa_info_get(rx.h, C.byref(info)) == E_INVAL and L.vdl2hip_toa_read(rx.h, rec.ctypes.data, 4, None, 0, None) == E_INVAL
    assert off()
    for k in 2 * list(range(0, golden_wav.size, 320000)):         # (the receiver takes a slot's input buffer with the slot's first feed: ten feeds, six slots)
        rx.feed(golden_wav[k:k + 320000])
    rx.sync()
    assert len(rx.drain()) == 4
    held = vh.live_resources()
    good = dict(struct_size=C.sizeof(vh.ToaCfg), max_lag=8, flags=0, pool_curves=0)
    bads = (dict(struct_size=12), dict(struct_size=20), dict(max_lag=33), dict(flags=2), dict(flags=3), dict(max_lag=32, pool_curves=(1 << 24) // 65 + 1),
            dict(max_lag=1, pool_curves=(1 << 24) // 3 + 1))
    for bad in bads:
        assert L.vdl2hip_toa_enable(rx.h, C.byref(vh.ToaCfg(**{**good, **bad}))) == E_INVAL, bad
        assert off() and vh.live_resources() == held, bad
    assert L.vdl2hip_toa_enable(rx.h, None) == E_INVAL and L.vdl2hip_toa_enable(None, C.byref(vh.ToaCfg(**good))) == E_INVAL
    # on: a bad configuration leaves the running tap as it was
    rx.toa_enable(max_lag=32, pool_curves=(1 << 24) // 65)        # the extremes that are taken
    rx.toa_enable(max_lag=3, pool_curves=5)
    s0 = rx.toa_info()
    assert (s0["max_lag"], s0["pool_curves"], s0["flags"], s0["bursts"]) == (3, 5, 0, 0)
    assert L.vdl2hip_toa_info_get(rx.h, C.byref(vh.ToaInfo(56))) == E_INVAL
    for bad in bads:
        assert L.vdl2hip_toa_enable(rx.h, C.byref(vh.ToaCfg(**{**good, **bad}))) == E_INVAL, bad
        assert rx.toa_info() == s0, bad
    for k in range(0, golden_wav.size, 320000):
        rx.feed(golden_wav[k:k + 320000])
    rx.sync()
    assert rx.toa_info()["bursts"] == 1
    # enabling again starts afresh; disabling gives everything back but the staging buffer the receiver keeps
    rx.toa_enable()
    assert rx.toa_info()["bursts"] == 0 and len(rx.toa_read()[0]) == 0
    rx.toa_disable()
    assert off()
    for k in range(0, golden_wav.size, 320000):
        rx.feed(golden_wav[k:k + 320000])
    rx.sync()
    assert off() and len(rx.drain()) >= 2                         # (the decoder went on as ever)
    assert vh.live_resources() == dict(held, pinned=held["pinned"] + 1)      # (the staging buffer stays with the receiver)
    rx.close()
    assert vh.live_resources() == base


# ---------------------------------------------------------------- 6. groups
def test_group(vh, s32):
    cfg, iq, _, _ = cases.load("config2_1s")
    raw = np.asarray(iq).reshape(-1, 2)
    freqs = list(cfg.freqs)[:2]
    half = raw.shape[0] // 2

    def single():
        rx = vh.Receiver(cfg.centerfreq, freqs, cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=4 * half)
        rx.debug_option("referee", 0)
        rx.toa_enable()
        rx.feed(raw[:half]); rx.feed(raw[half:])
        rx.sync()
        r, cv = rx.toa_read()
        check_records(rx, s32, r, cv, label="single")
        rx.close()
        return r
    want = single()
    assert len(want) >= 2 and {int(r["chan"]) for r in want} == {0, 1}
    g = vh.ReceiverGroup(cfg.centerfreq, freqs, [0, 0], cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=4 * half)
    for i in range(g.size()):
        assert g.L.vdl2hip_debug_option(g.member(i), b"referee", 0) == 0
    g.toa_enable()
    g.feed(raw[:half]); g.feed(raw[half:])
    g.sync()
    for i in range(g.size()):
        r, cv = g.toa_read(i)
        mine = [x for x in want if int(x["chan"]) == i]
        assert g.toa_info(i)["bursts"] == len(r) == len(mine) > 0 and {int(x["chan"]) for x in r} == {i}
        for a, b in zip(mine, r):
            for name in SET_FIELDS + ("freq",):
                assert int(a[name]) == int(b[name]), (name, a, b)
            # (a member's stream is its own to the last bit: the arrival time agrees as it does across cuts)
            assert abs(position(a) - position(b)) <= 1e-3
    g.toa_disable()
    g.close()


# ---------------------------------------------------------------- 7. the tool
def test_tool(vh, wav_at_zero, tmp_path):
    import os
    import subprocess
    from dumpvdl2_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    wav = os.path.join(root, "tests", "golden", "vdl2_model_16b_1050kHz.wav")
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    out = str(tmp_path / "toa.csv")
    base = [exe, "--iq-file", wav, "--sample-format", "S16_LE"]
    p0 = subprocess.run(base, check=True, capture_output=True, text=True, timeout=120)
    p1 = subprocess.run(base + ["--toa-out", out, "--toa-max-lag", "12"], check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stdout.count("[S:") == 2 and p0.stderr == p1.stderr
    lines = open(out).read().splitlines()
    head = dict(l[2:].split(" ", 1) for l in lines if l.startswith("# "))
    assert set(head) == {k for k, _ in vh.ToaInfo._fields_ if k not in ("struct_size", "reserved")}
    assert (int(head["max_lag"]), int(head["bursts"]), int(head["curves"]), int(head["curves_dropped"]), int(head["edge"])) == (12, 1, 1, 0, 0)
    body = [l.split(",") for l in lines if not l.startswith("#")]
    names = [k for k in vh.BURST_TOA_DTYPE.names if k != "curve_off"]
    names.insert(names.index("toa_frac") + 1, "toa_sample")
    assert body[0] == names and len(body) == 2 and len(body[1]) == len(names)
    r, b = dict(zip(names, body[1])), wav_at_zero[1][0]
    assert int(r["nlags"]) == 25 and int(r["frames"]) == 2 and float(r["toa_sample"]) == int(r["peak_sample"]) + float(np.float32(r["toa_frac"]))
    # the same burst with 12 lags instead of 8: the peak and what is derived from it are what they were - as far as two cuts of the
    # stream agree (the tool feeds several blocks at a time, and the channeliser's stream is not bit-identical across cuts)
    for k in ("chan", "freq", "burst_ord", "sync_sample", "first_symbol", "peak_sample", "peak_lag", "flags", "frames_ok"):
        assert int(r[k]) == int(b[k]), k
    assert abs(float(r["toa_sample"]) - position(b)) <= 1e-3
    for k in ("peak_power", "energy", "rho", "carrier_phase", "cfo_hz", "dphi", "resid"):
        assert abs(float(r[k]) - float(b[k])) <= 1e-4 * max(1.0, abs(float(b[k]))), k
