"""The receiver hours into a stream.  Every position it keeps is an absolute 64-bit index since the stream began - input samples
(n_total, K1's n0 and the NCO phase taken from it), decimated samples (k_total, the walker's state, the bursts' timing, the
evaluation log, the referee's stretches and pieces, the flag words' base, the taps' k_on) - narrowed in places that are right only
because of a mask or a bounded difference.  A fresh receiver is started at input sample n with the test hook
Receiver.debug_set_position(n): a stream that BEGINS at n, at rest.  The oracle is started there with Oracle.set_position(n).

Positions (input samples, rounded down to the oversampling; L = the capture's length): 2^31 - L/2 and 2^32 - L/2 (n crosses the
boundary inside the capture), os 2^31 - L/2 and os 2^32 - L/2 (k crosses it), 52 * 5 * 2^24 (every NCO phase 0 again: the committed
golden answers shifted hold there, whatever the oracle's set_position does) and 2^40 + 123 os.

Nothing here has a tolerance of its own: frames and counters as tests/util.py compares them at position 0 (TOL_DB, TOL_PPM), K1's
stream under k1_reference's derived bound, the referee's scan and the aligned stream bit for bit, the taps as their own GPU tests
compare them.

Wall time of the module on an MI355X: 10 s for its 49 cells (the oracle runs on the CPU included)."""
import functools
import zlib

import numpy as np
import pytest

import cases
import position
from util import assert_frames_equal, compare_reference_counters

pytestmark = pytest.mark.gpu
S16, U8 = 1, 0
CASES3 = ["dirty25k_1s", "os10_noisy_1s", "config4_0p4s"]
POSITIONS = {
    "n_2^31": lambda L, os_: 2**31 - L // 2, "n_2^32": lambda L, os_: 2**32 - L // 2,
    "k_2^31": lambda L, os_: os_ * 2**31 - L // 2, "k_2^32": lambda L, os_: os_ * 2**32 - L // 2,
    "aligned": lambda L, os_: position.ALIGNED, "2^40": lambda L, os_: 2**40 + 123 * os_,
}
PIECES = (30000, 300000)            # samples per feed: no multiples of the oversampling, so the carry path runs with a large n_total
REF_FIGURES = ("referee_unmet", "referee_refused", "referee_retried")


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()          # raises if the HIP library is missing: no fallback
    return vdl2hip


def where(name_or_L, os_, pos):
    return position.round_down(POSITIONS[pos](name_or_L, os_), os_)


def piece_sizes(nsamples, seed):
    rng = np.random.default_rng(seed); out = []; k = 0
    while k < nsamples:
        m = min(nsamples - k, int(rng.integers(*PIECES))); out.append(m); k += m
    return out


def receive(vh, cfg, raw, fmt, n, sizes=None, debug=None):
    """a fresh receiver started at input sample n (0: left as created) and fed `raw` (bytes) whole or in pieces of `sizes` samples
    -> dict(frames, counters, avlc, stats)"""
    sb = 4 if fmt == S16 else 2
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, fmt, cfg.rx_max_ppm, max_block_bytes=raw.size)
    if fmt == U8:
        rx.debug_option("referee", 0)   # (no code of an unsigned byte is the sample 0: the hook cannot give the referee a history at rest, and refuses)
    if n:
        rx.debug_set_position(n)
    for k, v in (debug or {}).items():
        rx.debug_option(k, v)           # (an option that is valid at position 0 is valid after the hook)
    k = 0
    for m in sizes or [raw.size // sb]:
        rx.feed(raw[k * sb:(k + m) * sb]); k += m
    assert k * sb == raw.size
    fr = rx.drain()
    C = len(cfg.freqs)
    out = dict(frames=fr, counters=[list(rx.counters(c).values()) for c in range(C)], avlc=[list(rx.avlc_counters(c).values()) for c in range(C)],
               stats=rx.stats())
    rx.close()
    return out


_at_zero = {}


def at_zero(vh, key, cfg, raw, fmt, sizes, debug):
    """the same capture in the same pieces at position 0 (run once per module and shared): what the referee's figures are held to"""
    if key not in _at_zero:
        _at_zero[key] = receive(vh, cfg, raw, fmt, 0, sizes, debug)
    return _at_zero[key]


def check_run(vh, oracle_mod, name, pos, feeding, debug=None):
    cfg, iq, _, gold = cases.load(name)
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    L = raw.size // 4
    n = where(L, cfg.oversample, pos)
    assert n % cfg.oversample == 0 and n > 2**31 - L
    sizes = None if feeding == "whole" else piece_sizes(L, zlib.crc32(name.encode()))
    if sizes:
        assert len(sizes) >= 3 and any(m % cfg.oversample for m in sizes[:-1])
    label = f"{name} at {pos} = {n}, {feeding}" + (f", {debug}" if debug else "")
    want = position.oracle_at(name, n)
    got = receive(vh, cfg, raw, S16, n, sizes, debug)
    K, D = want["K"], want["D"]
    if pos in ("n_2^31", "n_2^32"):
        b = 2**31 if pos == "n_2^31" else 2**32
        assert n < b < n + L
    if pos in ("k_2^31", "k_2^32"):
        b = 2**31 if pos == "k_2^31" else 2**32
        assert K < b < K + D and any(f["sync_sample"] < b for f in want["frames"]) and any(f["end_sample"] >= b for f in want["frames"])
    assert len(want["frames"]) > 0
    assert_frames_equal(want["frames"], got["frames"], exact_samples=True, label=label)
    compare_reference_counters(oracle_mod.COUNTER_NAMES, want["counters"], got["counters"], label=label, strict=True)
    assert want["avlc"] == got["avlc"], label
    if pos == "aligned":
        cases.check_against_golden(got["frames"], got["counters"], position.shifted_golden(gold, K), label=label, exact_diagnostics=False)
    st = got["stats"]
    assert st["front_sync_timeouts"] == 0, label
    z = at_zero(vh, (name, feeding, str(debug)), cfg, raw, S16, sizes, debug)
    assert_frames_equal(position.oracle_at(name, 0)["frames"], z["frames"], exact_samples=True, label=label + " (the run at 0)")
    print(label, {k: (st[k], z["stats"][k]) for k in REF_FIGURES}, "scans", st["referee_scans"], z["stats"]["referee_scans"],
          "short", st["referee_short"], z["stats"]["referee_short"])
    assert {k: st[k] for k in REF_FIGURES} == {k: z["stats"][k] for k in REF_FIGURES}, label
    return got


@pytest.mark.parametrize("feeding", ["whole", "pieces"])
@pytest.mark.parametrize("pos", list(POSITIONS))
@pytest.mark.parametrize("name", CASES3)
def test_frames_and_counters_at_a_position(vh, oracle_mod, name, pos, feeding):
    check_run(vh, oracle_mod, name, pos, feeding)


@pytest.mark.parametrize("pos", ["n_2^32", "k_2^32"])
def test_walk_ahead_and_second_stitch_at_a_position(vh, oracle_mod, pos):
    """every feed's walk goes ahead of the check of the feed before, and every channel of every long feed is stitched a second time:
    the snapshot copies of the walk state that the hook sets are the ones these paths start from"""
    check_run(vh, oracle_mod, "dirty25k_1s", pos, "pieces", debug={"walk_ahead": 1, "force_again": 1})
    check_run(vh, oracle_mod, "dirty25k_1s", pos, "whole", debug={"walk_ahead": 1, "force_again": 1})


@functools.lru_cache(maxsize=None)
def u8_capture():
    """the input tests/test_gpu_parity.py uses for unsigned bytes (test_uint8_input)"""
    from dumpvdl2_amd import synth
    CF = 136975000
    cfg = synth.SynthConfig(centerfreq=CF, freqs=[CF, CF + 40000], oversample=10, duration_s=0.6, seed=12, amplitude=0.3, noise_sigma=0.01)
    iq8, _ = synth.synthesize(cfg, dtype=np.uint8)
    raw = np.ascontiguousarray(iq8).view(np.uint8).reshape(-1)
    raw.setflags(write=False)
    return cfg, raw


def test_unsigned_bytes_at_a_position(vh, oracle_mod):
    """the unsigned-byte channeliser, the walker and the burst decoder at large indices; both runs with the referee off (receive())"""
    cfg, raw = u8_capture()
    L = raw.size // 2
    n = where(L, 10, "n_2^32")
    sizes = piece_sizes(L, 8)
    want = position.oracle_run(oracle_mod, cfg, raw, n, trace=False, sample_fmt=oracle_mod.FMT_U8)
    got = receive(vh, cfg, raw, U8, n, sizes)
    label = f"u8 at {n}"
    assert len(want["frames"]) > 0
    assert_frames_equal(want["frames"], got["frames"], exact_samples=True, label=label)
    compare_reference_counters(oracle_mod.COUNTER_NAMES, want["counters"], got["counters"], label=label, strict=True)
    assert want["avlc"] == got["avlc"]
    z = receive(vh, cfg, raw, U8, 0, sizes)
    st = got["stats"]
    print(label, {k: (st[k], z["stats"][k]) for k in REF_FIGURES}, "short", st["referee_short"], z["stats"]["referee_short"])
    assert st["front_sync_timeouts"] == 0
    assert {k: st[k] for k in REF_FIGURES} == {k: z["stats"][k] for k in REF_FIGURES}


# ---------------------------------------------------------------- K1's own stream

def k1_cell(vh, oracle_mod, os_, fmt, n, sizes, seed):
    """8 channels of k1.channel_plan, D_SMALL outputs, referee off, started at n -> (the stream read back from K on, the raw input, the
    oracle's coefficients and steps)"""
    import k1_reference as k1
    from test_gpu_k1_stream import D_SMALL
    sb = 4 if fmt == S16 else 2
    freqs, loud = k1.channel_plan(os_, 8)
    raw = k1.stimulus(k1.CF, freqs, os_, D_SMALL * os_ + 3, fmt, seed, loud=loud)
    o = oracle_mod.Oracle(k1.CF, freqs, oversample=os_, sample_fmt=fmt)
    A, B = o.lpf(); dphi = [o.dphi(c) for c in range(8)]
    o.close()
    rx = vh.Receiver(k1.CF, freqs, os_, fmt, 0.0, max_block_bytes=max(sizes) * sb)
    rx.debug_option("referee", 0)          # (ahead of the hook: it refuses unsigned bytes with the referee on)
    if n:
        rx.debug_set_position(n)
    k = 0
    for m in sizes:
        rx.feed(raw[k * sb:(k + m) * sb]); k += m
    assert k * sb == raw.size
    rx.sync()
    K = n // os_
    got = np.stack([rx.read_decimated(c, K, D_SMALL) for c in range(8)])
    st = rx.stats()
    rx.close()
    assert got.shape == (8, D_SMALL, 2) and st["front_sync_timeouts"] == 0
    return got, raw, A, B, dphi


@pytest.mark.parametrize("pos", ["n_2^32", "k_2^32"])
@pytest.mark.parametrize("fmt,os_", [(S16, 20), (U8, 10)], ids=["s16-os20", "u8-os10"])
def test_k1_stream_at_a_position(vh, oracle_mod, fmt, os_, pos):
    import types
    import k1_reference as k1
    from test_gpu_k1_stream import D_SMALL
    L = D_SMALL * os_ + 3
    n = where(L, os_, pos)
    K = n // os_
    if pos == "k_2^32":
        assert K < 2**32 < K + D_SMALL      # read_decimated() is asked for samples above 2^32
    got, raw, A, B, dphi = k1_cell(vh, oracle_mod, os_, fmt, n, piece_sizes(L, 5), seed=os_ + 8)
    cfg = types.SimpleNamespace(oversample=os_)
    y64 = k1.exact_stream(cfg, raw, fmt, A, B, dphi, D_SMALL, unrounded=True, n0=n, nthreads=k1.MAX_THREADS)
    model = k1.block_form_model(cfg, raw, fmt, A, B, dphi, D_SMALL, n0=n, nthreads=k1.MAX_THREADS)
    r = k1.compare(got, y64, model, k1.input_peak(raw, fmt))
    print(f"k1 stream {fmt} os{os_} at {pos}: model max {r['model_max'].max():.2e} kernel max {r['max'].max():.2e} "
          f"ratio max {np.max(r['max'] / r['model_max']):.2f} rms {np.max(r['rms'] / r['model_rms']):.2f}")
    rms = np.sqrt((y64 ** 2).sum(-1).mean(-1)) / k1.input_peak(raw, fmt)
    assert rms.min() >= 1e-3, f"the stimulus leaves a channel quiet: {rms.min():.1e} of the input's peak"
    bad = k1.failures(r)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("fmt,os_", [(S16, 20), (U8, 10)], ids=["s16-os20", "u8-os10"])
def test_k1_stream_at_the_aligned_position_is_the_stream_at_zero(vh, oracle_mod, fmt, os_):
    """same pieces, same segmentation, same phases: bit for bit"""
    from test_gpu_k1_stream import D_SMALL
    sizes = piece_sizes(D_SMALL * os_ + 3, 6)
    a = k1_cell(vh, oracle_mod, os_, fmt, position.ALIGNED, sizes, seed=os_ + 9)[0]
    b = k1_cell(vh, oracle_mod, os_, fmt, 0, sizes, seed=os_ + 9)[0]
    assert np.any(a) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- the referee's scan

def test_scan_at_a_position_is_the_oracles_stream(vh, oracle_mod):
    """vdl2hip_debug_exact_window at 2^32 - L/2: a stretch the scan has been over is the oracle-at-position's decimated stream bit for
    bit - at the very start of the stream (the run-up is the zeros the hook put into the history ring), across input sample 2^32, and
    out of the history ring behind short feeds"""
    name = "dirty25k_1s"
    cfg, iq, _, _ = cases.load(name)
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    L = raw.size // 4
    n = where(L, cfg.oversample, "n_2^32")
    want = position.oracle_at(name, n)
    K, D, tr = want["K"], want["D"], want["trace"]
    nch = len(cfg.freqs)
    for block in (None, 320000):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, S16, cfg.rx_max_ppm, max_block_bytes=raw.size)
        rx.debug_set_position(n)
        rx.debug_option("referee", 0)
        for k in range(0, raw.size, block or raw.size):
            rx.feed(raw[k:k + (block or raw.size)])
        rx.drain()
        rng = np.random.default_rng(5)
        b32 = (2**32 - n) // cfg.oversample                   # the decimated sample (from K) at which the input index passes 2^32
        checked = differed = 0
        for c in range(nch):
            los = (0, 17, b32 - 100, D - 400) if not block else (int(rng.integers(D - 40000, D - 6000)), D - 3000, D - 400)
            for lo in los:
                hi = min(D - 1, lo + int(rng.integers(40, 700)) + (9000 if c % 3 == 1 else 0))
                before = rx.read_decimated(c, K + lo, hi - lo + 1)
                assert rx.exact_window(c, K + lo, K + hi), f"scan refused for channel {c} [{lo}, {hi}] (block {block})"
                after = rx.read_decimated(c, K + lo, hi - lo + 1)
                w = tr[c, lo:hi + 1]
                assert after.tobytes() == w.tobytes(), f"channel {c} [{lo}, {hi}] (block {block}): scan differs from the oracle's stream (max {np.abs(after - w).max():.3e})"
                differed += before.tobytes() != w.tobytes()
                checked += 1
        s = rx.stats()
        rx.close()
        assert checked >= 3 * nch and differed >= nch
        assert s["referee_scans"] + s["referee_cached"] == checked and s["referee_refused"] == 0, s


# ---------------------------------------------------------------- the taps

def test_taps_enabled_after_the_hook(vh, oracle_mod):
    """activity monitor, transmission log, preamble search and burst capture enabled after debug_set_position(2^32 - L/2) on
    os10_noisy_1s: k_on / first_sample and every sample index are absolute, and the records are what each tap's model gives on the
    device's own stream and series for that base - compared as the tap's own GPU test compares them."""
    import activity_model as am
    import capture_model as cm
    import txlog_model as tlm
    import txsearch_model as tsm
    from test_gpu_activity import ACC_KEYS, mk, worst_ratio
    from test_gpu_capture import bits, check_quality
    name = "os10_noisy_1s"
    cfg, iq, _, _ = cases.load(name)
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    L = raw.size // 4
    os_ = cfg.oversample
    n = where(L, os_, "n_2^32")
    K = n // os_
    nch = len(cfg.freqs)
    B, THR, H, PRE, POST = 105, -40.0, 1, 256, 32
    sizes = piece_sizes(L, 4)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), os_, S16, cfg.rx_max_ppm, max_block_bytes=raw.size)
    rx.debug_set_position(n)
    rx.debug_option("referee", 0)
    rx.activity_enable(B, THR, H, 4096)
    rx.txlog_enable()
    rx.txsearch_enable()
    rx.capture_enable(PRE, POST)
    y = [[] for _ in range(nch)]
    frames, tx, txs, recs, wins = [], [], [], [], []
    k = made = 0
    for m in sizes:
        rx.feed(raw[4 * k:4 * (k + m)]); k += m
        rx.sync()
        r, w = rx.capture_read()
        for rr, ww in zip(r, w):                             # (test_gpu_capture.check_iq: every window against the stream as it stands now)
            assert ww.size == rr["iq_count"] and rr["iq_first"] >= K - PRE
            if rr["iq_count"]:
                yy = rx.read_decimated(rr["chan"], rr["iq_first"], rr["iq_count"])
                assert np.array_equal(bits(ww.view(np.float32)), bits(yy).reshape(-1)), (rr["chan"], rr["burst_ord"])
        recs += r; wins += w
        frames += rx.drain()
        tx.append(rx.txlog_read()); txs.append(rx.txsearch_read())
        now = k // os_
        if now > made:
            for c in range(nch):
                y[c].append(rx.read_decimated(c, K + made, now - made))
            made = now
    rx.sync()
    frames += rx.drain()
    tx.append(rx.txlog_read()); txs.append(rx.txsearch_read())
    tx, txs = np.concatenate(tx), np.concatenate(txs)
    a = rx.activity()
    series = [rx.activity_series(c, 0, int(a["bins"])) for c in range(nch)]
    loginfo, sinfo, cinfo, st = rx.txlog_info(), rx.txsearch_info(), rx.capture_info(), rx.stats()
    rx.close()
    y = [np.concatenate(v) for v in y]
    D = L // os_
    assert all(v.shape == (D, 2) for v in y) and len(frames) > 0

    # activity: k_on, the bins, the series against the stream, the scan against the series
    assert a["first_sample"] == K and a["bins"] == D // B and a["bin_samples"] == B and np.all(a["chan_bins"] == D // B)
    thr = am.threshold(THR)
    assert a["threshold_power"] == thr
    worst = 0.0
    for c in range(nch):
        ref = am.bin_powers(y[c], B)
        assert series[c].shape == ref.shape
        worst = max(worst, worst_ratio(series[c], ref, B))
        want = am.scan(series[c], thr, H)
        for key in ACC_KEYS:
            assert int(a[key][c]) == want[mk(key)], (c, key, int(a[key][c]), want[mk(key)])
        assert np.array_equal(a["hist"][c], want["hist"]) and a["max_power"][c] == want["max_power"] and a["min_power"][c] == want["min_power"]
    assert worst <= 1.0, worst

    # transmission log: the model on the device's own series, for the base K (first_sample / last_sample absolute)
    total = 0
    for c in range(nch):
        mine = tx[tx["chan"] == c]
        assert np.all(mine["freq"] == cfg.freqs[c])
        stt = tlm.new_state()
        want = tlm.log(series[c], thr, H, stt, B, k_on=K)
        tlm.assert_records(mine, want, ("txlog", c))
        assert all(K <= int(r["first_sample"]) <= int(r["last_sample"]) < K + D for r in mine)
        assert len(mine) + int(a["open"][c]) == int(a["transmissions"][c]) and int(stt["open"]) == int(a["open"][c])
        # the host's join: frames by their absolute sync_sample
        fr = sorted((f["sync_sample"], f["burst_ord"], True) for f in frames if f["chan"] == c)
        waiting = []
        joined = [dict(first_sample=int(r["first_sample"]), last_bin=int(r["last_bin"])) for r in mine]
        tlm.join(joined, fr, H, B, k_on=K, waiting=waiting)
        assert [(j["frames"], j["first_burst_ord"]) for j in joined] == [(int(r["frames"]), int(r["first_burst_ord"])) for r in mine], c
        total += len(mine)
    assert total == len(tx) == loginfo["transmissions"] > 0 and loginfo["dropped"] == 0
    assert sum(int(r["frames"]) for r in tx) > 0

    # preamble search: the model on the device's own stream; before K lies rest
    def getter(c):
        v = y[c].view(np.complex64).reshape(-1)

        def get(idx):
            out = np.zeros(idx.size, dtype=np.complex64)
            ok = idx >= K
            out[ok] = v[idx[ok] - K]
            return out
        return get
    assert len(tx) == len(txs)
    samples = 0
    for i, (t, s) in enumerate(zip(tx, txs)):
        assert (int(s["chan"]), int(s["freq"]), int(s["first_bin"])) == (int(t["chan"]), int(t["freq"]), int(t["first_bin"])), i
        want, _ = tsm.search(getter(int(t["chan"])), int(t["first_sample"]), int(t["last_sample"]), int(t["freq"]), int(t["flags"]))
        tsm.check(s, want, ("txsearch", i))
        assert (int(s["frames"]), int(s["frames_ok"])) == (int(t["frames"]), int(t["frames_ok"]))
        assert int(s["why"]) == tsm.why(int(t["frames"]), int(t["frames_ok"]), want["lock_points"])
        samples += want["search_last"] - want["search_first"] + 1
    assert (sinfo["records"], sinfo["samples_searched"]) == (len(txs), samples)
    assert any(int(s["first_lock"]) >= K for s in txs)

    # burst capture: timing as the frames', windows from the model, quality from the captured IQ
    assert len(recs) == st["bursts"] == cinfo["bursts"] > 0 and cinfo["iq_dropped"] == 0
    keys = {(r["chan"], r["burst_ord"]): r for r in recs}
    for f in frames:
        r = keys[(f["chan"], f["burst_ord"])]
        assert (r["sync_sample"], r["end_sample"]) == (f["sync_sample"], f["end_sample"])
    for r, w in zip(recs, wins):
        assert K <= r["sync_sample"] < r["first_symbol"] <= r["end_sample"] < K + D
        first, count = cm.window(r["sync_sample"], r["end_sample"], PRE, POST, K + D)
        assert r["iq_first"] == first and r["iq_count"] <= count          # (post: what had arrived when the burst was decoded)
        check_quality(r, w, label=f"{r['chan']}/{r['burst_ord']}")
    # ... and the frames are still the oracle's at that position wherever the channeliser's own stream decides as the reference's does:
    # held with the referee on in test_frames_and_counters_at_a_position; here only their timing's base
    assert all(K <= f["sync_sample"] < f["end_sample"] < K + D for f in frames)


# ---------------------------------------------------------------- group, refusals

def test_group_at_a_position(vh, oracle_mod):
    name = "dirty25k_1s"
    cfg, iq, _, _ = cases.load(name)
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    n = where(raw.size // 4, cfg.oversample, "n_2^32")
    want = position.oracle_at(name, n)
    g = vh.ReceiverGroup(cfg.centerfreq, list(cfg.freqs), [0, 0], cfg.oversample, S16, cfg.rx_max_ppm, max_block_bytes=raw.size)
    g.debug_set_position(n)
    sizes = piece_sizes(raw.size // 4, 2)
    k = 0
    for m in sizes:
        g.feed(raw[4 * k:4 * (k + m)]); k += m
    g.sync()
    fr = g.drain()
    cnt = [list(g.counters(c).values()) for c in range(len(cfg.freqs))]
    g.close()
    assert_frames_equal(want["frames"], fr, exact_samples=True, label="group")
    compare_reference_counters(oracle_mod.COUNTER_NAMES, want["counters"], cnt, label="group", strict=True)


def test_hook_refusals(vh):
    CF = 136975000
    rx = vh.Receiver(CF, [CF, CF + 25000], 20, S16)
    with pytest.raises(vh.Vdl2HipError):
        rx.debug_set_position(2**32 + 7)                    # not a multiple of the oversampling
    rx.debug_set_position(20 * 2**32)
    with pytest.raises(vh.Vdl2HipError):
        rx.debug_set_position(2**33)                        # a receiver that stands at a position is not a fresh one
    rx.close()
    rx = vh.Receiver(CF, [CF], 10, S16)
    rx.feed(np.zeros(2 * 7, dtype=np.int16))                # fewer samples than the oversampling: fed, and all of it carried
    with pytest.raises(vh.Vdl2HipError):
        rx.debug_set_position(10 * 2**32)
    rx.close()
    rx = vh.Receiver(CF, [CF], 10, U8)
    with pytest.raises(vh.Vdl2HipError):
        rx.debug_set_position(10 * 2**32)                   # unsigned bytes with the referee on: no history of bytes is rest
    rx.debug_option("referee", 0)
    rx.debug_set_position(10 * 2**32)
    rx.close()
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_CF32, input_rate=1250000)
    with pytest.raises(vh.Vdl2HipError):
        rx.debug_set_position(10 * 2**32)                   # a receiver that resamples: K0's position pair is not the hook's
    rx.close()
