"""The referee: decisions within the margin of the channeliser's distance from the reference's fp32 scan are taken on the
reference's own samples, which one wavefront recomputes from the raw input by running the reference's arithmetic sequentially
(kernels.h: ref_exact_window_dev; src/demod.c:302-329).

1. the scan itself: a stretch made exact on the device is BIT-identical to the oracle's decimated stream - every raw format (s16, u8, cf32, s8:
   tests/rawfmt_cases.py), offset-tuned and on-centre channels, whole-block and short feeds (the run-up then comes out of the history ring), at the stream's start
   (zero state, exactly) and far into it (run-up from a zero state 2^17 samples back), one at a time and 75 side by side;
2. the decisions: random captures that differ from the oracle in a frame or a counter without the referee (tests/fuzz_gpu.py's seeds
   175, 274, 1014: a symbol at a slicer boundary, a header bit, a preamble whose metric hangs on atan2()'s branch cut) are identical to
   it with the referee - frames, timing, the reference's 18 counters - strictly, no tie allowances."""
import numpy as np
import pytest

import cases
import rawfmt_cases
from util import assert_frames_equal, fed_without_referee

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def _oracle_trace(oracle_mod, cfg, raw, fmt, D):
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, sample_fmt=fmt, max_ppm=cfg.rx_max_ppm)
    tr = o.trace_all(D + 4)
    o.process(raw, block_bytes=1 << 24, nthreads=8)
    return o, tr[:, :D, :]


# the capture in every raw format (tests/rawfmt_cases.py), as one block and in blocks so short that the run-up comes out of the history
# ring.  u8 whole: k_ref_scan_multi<u8, 20> and the single-wavefront scan's 16-bit words from the stream's own start
# (fmt: the public value, so that the rows this file always had keep their ids - 1 s16, 0 u8, 2 cf32, 4 s8)
FMT_NAME = {1: "s16", 0: "u8", 2: "cf32", 4: "s8"}
SCAN_CASES = [(1, None), (1, 320000), (0, None), (0, 262144), (2, None), (2, 640000), (4, None), (4, 640000)]
MULTI_CASES = [(1, None), (0, None), (0, 262144), (2, None), (2, 640000), (4, None), (4, 640000)]


@pytest.mark.parametrize("fmt,block", SCAN_CASES)
def test_scan_is_bit_exact(vh, oracle_mod, fmt, block):
    """a stretch the single-wavefront scan has been over is the oracle's stream bit for bit, whatever the format of the raw input"""
    name = FMT_NAME[fmt]
    assert rawfmt_cases.receiver_fmt(vh, name) == fmt
    case = rawfmt_cases.config2(oracle_mod, name)
    cfg, D, tr = case["cfg"], case["D"], case["tr"]
    rx = fed_without_referee(vh, cfg, fmt, case["raw"], block)   # the stream as the channeliser leaves it ...
    nch = len(cfg.freqs)
    rng = np.random.default_rng(5)
    # ... is close to the oracle's but not it; the stretches the scan has been over are it, bit for bit
    checked = differed = 0
    for c in range(nch):
        # (with short feeds: what the LAST feed can reach - its own block and the history ring, 2^17 samples of run-up + the longest burst)
        for lo in ((0, 17, int(rng.integers(20000, D - 6000)), D - 400) if not block else (int(rng.integers(D - 40000, D - 6000)), D - 3000, D - 400)):
            hi = min(D - 1, lo + int(rng.integers(40, 700)) + (9000 if c % 3 == 1 else 0))       # (every third channel: a stretch as long as a burst)
            before = rx.read_decimated(c, lo, hi - lo + 1)
            assert rx.exact_window(c, lo, hi), f"scan refused for channel {c} [{lo}, {hi}]"
            after = rx.read_decimated(c, lo, hi - lo + 1)
            want = tr[c, lo:hi + 1]
            assert after.tobytes() == want.tobytes(), f"channel {c} [{lo}, {hi}]: scan differs from the oracle's stream (max {np.abs(after - want).max():.3e})"
            differed += before.tobytes() != want.tobytes()      # (a stretch an earlier scan went over is the oracle's already)
            checked += 1
    assert checked >= 2 * nch
    assert differed >= nch, "the channeliser's own samples were bit-identical to the oracle's: this test shows nothing"
    s = rx.stats()
    assert s["referee_scans"] + s["referee_cached"] == checked and s["referee_scans"] >= nch and s["referee_refused"] == 0, s   # (a scan covers whole blocks of 256 samples: some stretches had been done)
    rx.close()


@pytest.mark.parametrize("fmt,block", MULTI_CASES)
def test_many_scans_side_by_side_are_bit_exact(vh, oracle_mod, fmt, block):
    """k_ref_scan_multi: a workgroup runs 32 recursions at once (lane = request), two wavefronts feed it - the same arithmetic; its
    producers fetch 16-bit words (u8, s8), 32-bit words (s16) or two words per sample (cf32)"""
    name = FMT_NAME[fmt]
    assert rawfmt_cases.receiver_fmt(vh, name) == fmt
    case = rawfmt_cases.config2(oracle_mod, name)
    cfg, D, tr = case["cfg"], case["D"], case["tr"]
    rx = fed_without_referee(vh, cfg, fmt, case["raw"], block)
    nch = len(cfg.freqs)
    rng = np.random.default_rng(11)
    n = 75                                           # three workgroups, the last one partly filled
    lo_min = 0 if not block else D - 30000           # (short feeds: what the last feed can reach)
    chans = rng.integers(0, nch, n); los = rng.integers(lo_min, D - 6000, n); his = los + rng.integers(20, 900, n)
    his[::7] += 5000                                 # unequal lengths: the longest decides how long the workgroup runs
    chans[40], los[40], his[40] = chans[39], los[39], his[39]      # the same stretch twice in one workgroup
    if not block:
        los[3], his[3] = 0, 300                      # the stream's own start: zero state, exactly
    his = np.minimum(his, D - 1)
    before = [rx.read_decimated(int(c), int(a), int(b - a + 1)) for c, a, b in zip(chans, los, his)]
    ran, ms = rx.scan_multi(chans, los, his)
    assert 0 < ran <= n - 1, ran
    differed = 0
    for c, a, b, bf in zip(chans, los, his, before):
        got = rx.read_decimated(int(c), int(a), int(b - a + 1)); want = tr[int(c), int(a):int(b) + 1]
        assert got.tobytes() == want.tobytes(), f"channel {c} [{a}, {b}]: differs from the oracle's stream (max {np.abs(got - want).max():.3e})"
        differed += bf.tobytes() != want.tobytes()
    assert differed >= n // 2
    assert rx.stats()["referee_refused"] == 0
    rx.close()


def test_witness_tells_a_run_up_that_was_too_short(vh, oracle_mod):
    """Every scan of k_ref_scan_multi carries a witness: the same recursion over the same values from another state (idle lanes).  With
    the product's run-up (2^17 input samples) the two have met by the stretch's first output all but always - and then the stretch IS
    the oracle's, bit for bit; with a run-up of 2 048 samples (mean meeting time: 1.6e4) they mostly have not, the scans are counted in
    referee_unmet, and such stretches are NOT all the oracle's: what the counter says is what the data shows."""
    cfg, iq, _, _ = cases.load("config2_1s")
    raw = iq.view(np.uint8)
    D = raw.size // 4 // cfg.oversample
    o, tr = _oracle_trace(oracle_mod, cfg, raw, 1, D)
    rng = np.random.default_rng(21)
    n = 96
    out = {}
    for warm in (1 << 17, 2048):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, 1, cfg.rx_max_ppm, max_block_bytes=raw.size)
        rx.debug_option("referee", 0)
        rx.feed(raw); rx.drain()
        rx.debug_option("ref_warm", warm); rx.feed(raw[:4000]); rx.drain()          # (the run-up travels in the feed's hook)
        chans = rng.integers(0, len(cfg.freqs), n); los = rng.integers(48000, D - 6000, n) & ~255; his = los + 255          # (what the history ring still holds of the stream, run-up included)
        ran, ms = rx.scan_multi(chans, los, his)
        exact = sum(rx.read_decimated(int(c), int(a), 256).tobytes() == tr[int(c), int(a):int(a) + 256].tobytes() for c, a in zip(chans, los))
        st = rx.stats()
        out[warm] = (ran, st["referee_unmet"], exact, st["referee_retried"])
        rx.close()
    o.close()
    # (the test hook's launch lists nothing for a second try: what is unmet is counted as unmet)
    ran, unmet, exact, retried = out[1 << 17]
    assert ran > n // 2 and unmet <= 1 and retried == 0 and exact >= n - unmet, out
    ran, unmet, exact, retried = out[2048]
    assert unmet >= ran // 2 and exact <= n - unmet // 2, out        # (not met by the first output, yet some meet within the stretch's first samples)


def test_unmet_scans_are_run_again_from_further_back(vh, oracle_mod):
    """In the product's launches a scan that has not met its witness is listed and run again from further back (twice as far:
    VDL2HIP_REF_RETRY).  (1) Many scans side by side with a run-up of 2 048 samples (most unmet the first time), launched as the product
    launches them: `referee_retried` counts the second tries, and no fewer stretches are the oracle's than without the second try.  (2) With a run-up of 4 096 samples a config2 capture in long pieces
    must still come out as the golden answers say, and with the product's run-up nothing is retried on this capture."""
    cfg, iq, bursts, gold = cases.load("config2_1s")
    raw = iq.view(np.uint8)
    D = raw.size // 4 // cfg.oversample
    o, tr = _oracle_trace(oracle_mod, cfg, raw, 1, D)
    o.close()
    rng = np.random.default_rng(22)
    n = 60                                                      # (at most 64 scans of one launch are listed for a second try)
    chans = rng.integers(0, len(cfg.freqs), n); los = rng.integers(48000, D - 6000, n) & ~255
    exact = {}
    for retry in (False, True):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, 1, cfg.rx_max_ppm, max_block_bytes=raw.size)
        rx.debug_option("referee", 0)
        rx.feed(raw); rx.drain()
        rx.debug_option("ref_warm", 2048); rx.feed(raw[:4000]); rx.drain()          # (the run-up travels in the feed's hook)
        ran, _ = rx.scan_multi(chans, los, los + 255, retry=retry)
        exact[retry] = sum(rx.read_decimated(int(c), int(a), 256).tobytes() == tr[int(c), int(a):int(a) + 256].tobytes() for c, a in zip(chans, los))
        st = rx.stats()
        if retry:
            assert st["referee_retried"] >= ran // 4 and st["referee_unmet"] <= st["referee_retried"], st      # (what the second try - 4 096 samples - leaves unmet is counted)
        else:
            assert st["referee_retried"] == 0 and st["referee_unmet"] >= ran // 4, st
        rx.close()
    assert exact[True] >= exact[False], exact
    for warm in (4096, None):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, 1, cfg.rx_max_ppm, max_block_bytes=4 << 20)
        if warm:
            rx.debug_option("ref_warm", warm)
        rx.set_drain_lag(3)
        got = []
        for k in range(0, raw.size, 3 << 20):
            rx.feed(raw[k:k + (3 << 20)]); got += rx.drain()
        rx.set_drain_lag(0); got += rx.drain()
        st = rx.stats()
        cases.check_against_golden(got, [list(rx.counters(c).values()) for c in range(len(cfg.freqs))], gold, label=f"run-up {warm}", exact_diagnostics=False)
        if warm:
            assert st["referee_retried"] <= st["referee_scans"], st
        else:
            assert st["referee_retried"] <= 1 and st["referee_unmet"] <= 1, st
        rx.close()


@pytest.mark.parametrize("seed,profile", [(175, "plain"), (274, "plain"), (1014, "extreme")])
def test_decisions_that_hang_on_the_references_rounding(vh, oracle_mod, seed, profile):
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
    out = {}
    for referee in (0, 1):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, 1, cfg.rx_max_ppm, max_block_bytes=raw.size)
        rx.debug_option("referee", referee)
        for k in range(0, raw.size, 1 << 20):
            rx.feed(raw[k:k + (1 << 20)])
        fr = rx.drain()
        cg = [list(rx.counters(c).values())[:18] for c in range(nch)]
        try:
            assert_frames_equal(fo, fr, exact_samples=True, label=f"seed {seed}")
            assert cg == co, "counters"
            out[referee] = "identical"
        except AssertionError as e:
            out[referee] = str(e)[:160]
        if referee:
            s = rx.stats()
            assert s["referee_scans"] > 0 and s["referee_refused"] == 0, s
        rx.close()
    assert out[1] == "identical", out
    assert out[0] != "identical", "this capture no longer differs without the referee: pick another seed"
