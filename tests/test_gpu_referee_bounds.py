"""The three premises the referee's margin arithmetic rests on (vdl2_core.h "Referee"), held on the device against
the oracle (oracle_mod.Oracle(...).trace_all(): the reference's own decimated samples of the same bytes).  tests/referee_bounds.py is the
arithmetic of the measurements; the bounds are the source's constants (read from the host build of the same header), not tolerances of
these tests.

1  kRefKappa.  y = read_decimated() of a receiver with the referee off (K1's output and nothing else), at EVERY sample of every
   channel: |y[n] - y_ref[n]| <= kRefKappa x the largest |y| among n .. n-3.  Cells: the five golden captures fed whole (channel rows
   1, 2 and 4, oversample 10 and 20, 2 to 256 channels; every channel is compared - at 256 channels that holds the first and the last
   channel-group row and the quietest channels), and config2_1s in 320 000-byte blocks, in random pieces of 1 .. 3000 samples, as u8 and
   s8 (tests/rawfmt_cases.py), and through both look-back fall-backs (no_fuse, force_timeout).
2  kRefSum.  On the same streams: the device's exact phases (phase_of through the probe hook) of y and of y_ref, numpy sync_metric on
   the taps n-150 .. n, E from y as ref_eps2_of() and sync_metric_ref() define it; on every window with p < 8, E < kRefBig and no
   discontinuity event |p - p_ref| <= ref_pherr_margin(p, E) and |f - f_ref| <= ref_slope_margin(E).  Captures: config3_0p6s,
   config4_0p4s, config5_0p4s - at least 1000 such windows each (config2_1s has 394 and os10_noisy_1s 138 on the float32 model's stream:
   not enough to carry the premise, they are left to premise 1); at 256 channels the first 128 channels.
3  The marks.  Receivers with the referee on and the dense exact tier, screened (screen_all 0) and not (1), fed whole: cand[n], the mark
   (the sign of pf[n].p) and |pf| from read_sync() against the decision got_sync() takes at n on the reference's metric (fires; sclk; the
   gate) with y1 = PHERR_MAX and, where the device tabulated n-6, y1 = p[n-6]:
     (a) the reference fires at n             =>  cand[n]
     (b) cand[n] and n is not marked          =>  the reference fires at n and its code is the code computed from the device's |pf|
     (c) screened and unscreened agree on cand and, where cand is set, on the mark - on the receivers whose tier works the
         alternatives out (the FULL form: <= 64 channels).  The other form calls a window with two unwrap decisions within the margin
         "cannot tell" - a candidate, marked - wherever it evaluates one, and the unscreened receiver evaluates them all: there every
         candidate of the screened receiver is one of the unscreened with the same mark, and every further one of the unscreened is
         marked (the figure is printed).
   Captures: config4(0.3) without its ppm gate, first 8 channels (the FULL form; also in pieces of odd lengths, where only (a) holds:
   scans may have made a previous feed's tail exact), the same with its first 64 channels, config4_0p4s at 256 channels (the other form).
   Against a vacuous test each capture has to show at least half of the fires, marked candidates and marked candidates whose reference
   decision really differs that the host build (tests/hostsim: hostsim_set_exact + hostsim_read_sync, fed the float32 model's stream and
   the oracle's trace) shows on it - HOST_FOUND below; profiles/referee_bounds_device.txt has both.  The FULL form marks next to nothing
   on these captures (0 of 62 and 2 of 290 candidates; none really different): "some are marked, some really differ" rests on the
   256-channel capture.

REFEREE_BOUNDS=<file> in the environment appends every printed figure to that file: profiles/referee_bounds_device.txt is such a run.
Wall time of the module on an MI355X: see that file."""
import dataclasses
import os
import time

import numpy as np
import pytest

import cases
import core_reference as cr
import rawfmt_cases
import referee_bounds as rb

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


@pytest.fixture(scope="module")
def L(vh):
    return vh.load_library()


@pytest.fixture(scope="module")
def K():
    return rb.constants()


def record(text):
    print(text)
    path = os.environ.get("REFEREE_BOUNDS")
    if path:
        with open(path, "a") as f:
            f.write(text + "\n")


_captures = {}


def capture(oracle_mod, name):
    """-> dict(cfg, raw, sb, fmt name, D, tr [channel, D, 2]); one oracle run per capture and session, nothing in it is changed"""
    if name in _captures:
        return _captures[name]
    if name in ("u8", "s8"):
        c = rawfmt_cases.config2(oracle_mod, name)
        out = dict(cfg=c["cfg"], raw=c["raw"], sb=c["sb"], fmt=name, D=c["D"], tr=c["tr"])
    else:
        if name.startswith("c4_"):
            from dumpvdl2_amd import workloads, synth
            cfg = workloads.config4(0.3)
            cfg = dataclasses.replace(cfg, freqs=list(cfg.freqs)[:int(name[3:-2])], rx_max_ppm=0.0)
            iq, _ = synth.synthesize(cfg)
        else:
            cfg, iq, _, _ = cases.load(name)
        raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
        D = raw.size // 4 // cfg.oversample
        o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
        tr = o.trace_all(D + 4)
        o.process(raw, block_bytes=1 << 24, nthreads=16)
        tr = tr[:, :D, :].copy()
        o.close()
        tr.setflags(write=False)
        out = dict(cfg=cfg, raw=raw, sb=4, fmt="s16", D=D, tr=tr)
    _captures[name] = out
    return out


_ref_metric = {}


def reference_metric(L, oracle_mod, name, nchan):
    """(phase, p, f) of the oracle's trace at every sample of the first nchan channels - float32 [nchan, D] each"""
    key = (name, nchan)
    if key not in _ref_metric:
        c = capture(oracle_mod, name)
        ph = rb.device_phases(L, c["tr"][:nchan])
        pf = [rb.stream_metric(ph[i]) for i in range(nchan)]
        out = (ph, np.stack([a for a, _ in pf]), np.stack([b for _, b in pf]))
        for a in out:
            a.setflags(write=False)
        _ref_metric[key] = out
    return _ref_metric[key]


def whole(n):
    yield n


def blocks_320k(sb):
    def feed(n):
        step = 320000 // sb
        for k in range(0, n, step):
            yield min(step, n - k)
    return feed


def random_pieces(seed, lo=1, hi=3000, odd=False):
    def feed(n):
        rng = np.random.default_rng(seed); k = 0
        while k < n:
            m = int(rng.integers(lo, hi + 1))
            m = min(n - k, m | 1 if odd else m)
            yield m; k += m
    return feed


def two_feeds(n):
    half = (n // 2 + 263) | 1
    yield half
    yield n - half


def stream_without_referee(vh, c, feed, debug=None):
    """K1's own output of every channel, float32 [channel, D, 2], and the receiver's statistics"""
    cfg, raw, sb = c["cfg"], c["raw"], c["sb"]
    pieces = list(feed(raw.size // sb))
    assert sum(pieces) == raw.size // sb
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, rawfmt_cases.receiver_fmt(vh, c["fmt"]), cfg.rx_max_ppm, max_block_bytes=raw.size)      # (a ring that holds the whole capture)
    rx.debug_option("referee", 0)                  # what read_decimated() returns is K1's own output, nowhere the referee's scan
    for k, v in (debug or {}).items():
        rx.debug_option(k, v)
    off = 0
    for m in pieces:
        rx.feed(raw[off * sb:(off + m) * sb]); off += m
    rx.sync()
    y = np.stack([rx.read_decimated(ch, 0, c["D"]) for ch in range(len(cfg.freqs))])
    st = rx.stats()
    rx.close()
    assert y.shape == (len(cfg.freqs), c["D"], 2), y.shape      # (the ring holds the whole capture in every cell)
    return y, st


def premise_1(label, y, tr, kappa):
    t0 = time.time()
    shares = []; valids = []; worst = (0.0, -1, -1)
    for ch in range(len(y)):
        s, v = rb.kappa_share(y[ch], tr[ch], kappa)
        shares.append(s); valids.append(v)
        k = int(np.argmax(np.where(v, s, 0)))
        if s[k] > worst[0]:
            worst = (float(s[k]), ch, k)
    st = rb.share_stats(np.concatenate(shares), np.concatenate(valids))
    rows = ""
    if len(y) == 256:                                       # the first and the last channel-group row, and the 16 quietest channels by median |y_ref|
        quiet = np.argsort(np.median(np.sqrt(rb.mag2(tr.reshape(-1, 2)).reshape(tr.shape[:2])), axis=1))[:16]
        top = lambda chans: max(float(np.where(valids[ch], shares[ch], 0).max()) for ch in chans)
        rows = f"  channels 0..15 max {top(range(16)):.3f}  240..255 max {top(range(240, 256)):.3f}  quietest 16 max {top(quiet):.3f}"
    record(f"{label:<34} ch {len(y):>3} samples {st['n']:>9}  share of the kRefKappa bound: max {st['max']:.3f} (channel {worst[1]}, sample {worst[2]})  99.9 % {st['q999']:.3f}  "
           f"rms {st['rms']:.4f}{rows}  [{time.time() - t0:.1f} s]")
    assert st["n"] >= 0.99 * y.shape[0] * y.shape[1], f"{label}: only {st['n']} samples are not zero"
    assert st["max"] <= 1.0, (f"{label}: |y - y_ref| is {st['max']:.3f} of kRefKappa x the largest |y| of the last four samples at channel {worst[1]}, sample {worst[2]}: "
                              f"y {y[worst[1]][worst[2]]} y_ref {tr[worst[1]][worst[2]]}")
    return st


def premise_2(L, oracle_mod, label, name, y, kappa, nchan):
    t0 = time.time()
    c = capture(oracle_mod, name)
    nchan = min(nchan, len(y))
    _, p_ref, f_ref = reference_metric(L, oracle_mod, name, nchan)
    ph = rb.device_phases(L, y[:nchan])
    tot = 0; wp = (0.0, -1, -1); wf = (0.0, -1, -1)
    for ch in range(nchan):
        p, f = rb.stream_metric(ph[ch])
        m = rb.margin_shares(y[ch], ph[ch], p, f, p_ref[ch], f_ref[ch], kappa)
        tot += m["n"]
        if m["p_share"] > wp[0]:
            wp = (m["p_share"], ch, m["p_at"])
        if m["f_share"] > wf[0]:
            wf = (m["f_share"], ch, m["f_at"])
    record(f"{label:<34} ch {nchan:>3} windows {tot:>8}  worst share of ref_pherr_margin {wp[0]:.3f} (channel {wp[1]}, sample {wp[2]})  of ref_slope_margin {wf[0]:.3f} "
           f"(channel {wf[1]}, sample {wf[2]})  [{time.time() - t0:.1f} s]")
    assert tot >= 1000, f"{label}: {tot} windows with p < 8, E < kRefBig and no discontinuity event: too few to carry the premise"
    assert wp[0] <= 1.0, f"{label}: |p - p_ref| is {wp[0]:.3f} of ref_pherr_margin at channel {wp[1]}, sample {wp[2]}"
    assert wf[0] <= 1.0, f"{label}: |f - f_ref| is {wf[0]:.3f} of ref_slope_margin at channel {wf[1]}, sample {wf[2]}"
    assert c["D"] == y.shape[1]


PREMISE_2_CHANNELS = {"config3_0p6s": 64, "config4_0p4s": 128, "config5_0p4s": 128}


@pytest.mark.parametrize("name", ["os10_noisy_1s", "config2_1s", "config3_0p6s", "config4_0p4s", "config5_0p4s"])
def test_premises_on_whole_captures(vh, L, K, oracle_mod, name):
    c = capture(oracle_mod, name)
    y, st = stream_without_referee(vh, c, whole)
    assert st["front_sync_timeouts"] == 0
    premise_1(f"{name} whole", y, c["tr"], K["kappa"])
    if name in PREMISE_2_CHANNELS:
        premise_2(L, oracle_mod, f"{name} whole", name, y, K["kappa"], PREMISE_2_CHANNELS[name])


@pytest.mark.parametrize("cell", ["blocks320k", "pieces1to3000", "u8", "s8", "no_fuse", "force_timeout"])
def test_premise_1_config2_cells(vh, K, oracle_mod, cell):
    c = capture(oracle_mod, cell if cell in ("u8", "s8") else "config2_1s")
    feed = {"blocks320k": blocks_320k(c["sb"]), "pieces1to3000": random_pieces(7), "no_fuse": two_feeds, "force_timeout": two_feeds}.get(cell, whole)
    debug = {cell: 1} if cell in ("no_fuse", "force_timeout") else None
    y, st = stream_without_referee(vh, c, feed, debug)
    if cell == "force_timeout":
        assert st["front_sync_timeouts"] > 0
    else:
        assert st["front_sync_timeouts"] == 0
    premise_1(f"config2_1s {cell}", y, c["tr"], K["kappa"])


# what the host build finds on each capture (fed the float32 model's stream, the oracle's trace as the referee's samples), screened /
# unscreened: the floors asserted below are half of these
HOST_FOUND = {
    "c4_8ch": {0: dict(fires=62, candidates=62, marked=0, marked_and_different=0), 1: dict(fires=62, candidates=62, marked=0, marked_and_different=0)},
    "c4_64ch": {0: dict(fires=290, candidates=290, marked=2, marked_and_different=0), 1: dict(fires=290, candidates=290, marked=2, marked_and_different=0)},
    "config4_0p4s": {0: dict(fires=2216, candidates=2218, marked=6, marked_and_different=2), 1: dict(fires=2216, candidates=2355, marked=143, marked_and_different=139)},
}


def sync_with_referee(vh, c, screen_all, feed=whole):
    cfg, raw = c["cfg"], c["raw"]
    pieces = list(feed(raw.size // 4))
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=raw.size)
    rx.debug_option("exact_tier", 1); rx.debug_option("screen_all", screen_all)
    off = 0
    for m in pieces:
        rx.feed(raw[off * 4:(off + m) * 4]); off += m
    rx.drain()
    out = [rx.read_sync(ch, 0, c["D"]) for ch in range(len(cfg.freqs))]
    st = rx.stats()
    rx.close()
    assert all(len(cand) == c["D"] for _, cand in out)
    return out, st


def gate_threshold(cfg, ch):
    if cfg.rx_max_ppm == 0:
        return F32(np.inf)
    return cr.ppm_gate_threshold(np.array([cfg.freqs[ch]], dtype=np.uint32), np.array([cfg.rx_max_ppm], dtype=F32))[0]


def marks_against_reference(L, oracle_mod, name, sync, whole_feed, label):
    c = capture(oracle_mod, name)
    nch = len(c["cfg"].freqs)
    _, p_ref, f_ref = reference_metric(L, oracle_mod, name, nch)
    tot = dict(fires=0, candidates=0, marked=0, marked_and_different=0)
    missed = []; unmarked = []
    for ch in range(nch):
        pf, cand = sync[ch]
        r = rb.check_marks(pf, cand, p_ref[ch], f_ref[ch], c["cfg"].rx_max_ppm, gate_threshold(c["cfg"], ch), whole_feed)
        for k in tot:
            tot[k] += r[k]
        missed += [(ch, int(n)) for n in r["missed"]]; unmarked += [(ch, int(n)) for n in r["unmarked"]]
    record(f"{label:<44} fires {tot['fires']:>5}  candidates {tot['candidates']:>5}  marked {tot['marked']:>4}  marked and really different {tot['marked_and_different']:>4}  "
           f"missed fires {len(missed)}  unmarked and different {len(unmarked)}")
    assert not missed, f"{label}: (a) the reference fires at {len(missed)} samples whose candidate bit is not set, first (channel, sample) {missed[:5]}"
    assert not unmarked, f"{label}: (b) {len(unmarked)} unmarked candidates the reference decides otherwise, first (channel, sample) {unmarked[:5]}"
    return tot


@pytest.mark.parametrize("name", ["c4_8ch", "c4_64ch", "config4_0p4s"])
def test_marks_against_the_reference(vh, L, oracle_mod, name):
    t0 = time.time()
    c = capture(oracle_mod, name)
    full_form = len(c["cfg"].freqs) <= 64
    runs = {}
    for screen_all in (0, 1):
        sync, st = sync_with_referee(vh, c, screen_all)
        tot = marks_against_reference(L, oracle_mod, name, sync, True, f"{name} screen_all={screen_all} ({'FULL' if full_form else 'plain'} form)")
        found = HOST_FOUND[name][screen_all]
        assert tot["fires"] >= 50 and tot["candidates"] > tot["marked"]
        for k in ("fires", "marked", "marked_and_different"):
            assert tot[k] >= found[k] // 2 + (found[k] & 1), f"{name} screen_all={screen_all}: {k} {tot[k]}, the host build found {found[k]}"
        runs[screen_all] = sync
        if name == "config4_0p4s":
            record(f"    referee_scans {st['referee_scans']}")
    # (c)
    only_x = 0
    for ch, ((pfs, cs), (pfx, cx)) in enumerate(zip(runs[0], runs[1])):
        cs = cs.astype(bool); cx = cx.astype(bool)
        ms = np.signbit(pfs[:, 0]); mx = np.signbit(pfx[:, 0])
        d = np.flatnonzero(cs & (~cx | (ms != mx)))
        assert d.size == 0, f"{name}: channel {ch}: {d.size} candidates of the screened receiver are none of the unscreened, or marked otherwise; first {d[:5]}"
        extra = cx & ~cs
        only_x += int(extra.sum())
        if full_form:
            assert not extra.any(), f"{name}: channel {ch}: the unscreened receiver has {extra.sum()} candidates more, first {np.flatnonzero(extra)[:5]}"
        else:
            d = np.flatnonzero(extra & ~mx)
            assert d.size == 0, f"{name}: channel {ch}: {d.size} unmarked candidates the screened receiver does not have, first {d[:5]}"
    record(f"    {name}: candidates of the unscreened receiver alone {only_x} (all marked)  [{time.time() - t0:.1f} s]")


def test_no_missed_fire_in_pieces(vh, L, oracle_mod):
    """the 8-channel capture in pieces of odd lengths: (a) alone - what an earlier feed's scans made exact only shrinks the error"""
    c = capture(oracle_mod, "c4_8ch")
    for screen_all in (0, 1):
        sync, _ = sync_with_referee(vh, c, screen_all, random_pieces(13, 30_011, 90_017, odd=True))
        tot = marks_against_reference(L, oracle_mod, "c4_8ch", sync, False, f"c4_8ch in odd pieces screen_all={screen_all}")
        assert tot["fires"] >= 50
