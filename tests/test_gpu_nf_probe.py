"""The DEVICE build of K4b, the noise-floor replay (kernels.h: k_nf_prepare, k_nf_replay, k_nf_finish, and k_nf_all = nf_all_body, which k_nf_burst
runs too), through the test hook vdl2hip_debug_nf_probe, against the plain reference of tests/nf_reference.py: the reference program's own
recurrence (demod.c:238-243) in float32 numpy.  tests/test_nf_reference.py proves on the CPU that the cases' expectation - the recurrence from
0 over the last 256 evaluations the chunk list reaches - IS that recurrence, bit for bit, and runs the same cases through the host build; the
host build is no reference here.  Every comparison is bit for bit: mag_lp of every update (lpbuf), every entry of the history ring (the
entries no update wrote included), NfState (mag_nf, evals, the remembered tail) and the feed record, after every feed.  One call is one feed
of nchan channels on a y ring of 4096 samples; positions are masked into the ring, so millions of evaluations cost no memory.

Launch shapes: mode 0 is the three kernels of a long feed, k_nf_replay on dim3(grid, nchan) - with grid = 1 a wavefront takes up to 16 groups
of 32 updates in a row, each on the LDS the one before has left; mode 1 is the one kernel of a short feed.  Both must give the same bytes.

Tail too short.  The state remembers the newest 64 chunks (kNfTail).  Where those hold fewer than 256 evaluations, an update early in the next
feed replays only the k it can reach, and is off the reference program by up to 0.9^k max mag.  Two ways lead there:
  * a feed's end.  The walker begins a chunk with every feed (walk_load), so feeds of a few samples - a supported input,
    test_degenerate_feeds_and_errors - left the 64 remembered chunks with 64 evaluations or so: 0.9^64 = 1.2e-3 of the loudest magnitude, at
    every update for as long as such feeding lasts.  That was a bug, and these tests found it only once they fed that way: nf_prepare now
    joins a feed's first chunk to the remembered chunk it continues.  Case tiny_feeds (70 to 200 feeds of 0 to 3 evaluations before an
    update; it fails without the join, in the feed record and in mag_lp) pins it; test_feeds_of_one_sample_keep_the_noise_floor feeds a
    receiver that way.
  * a shift of the evaluation grid: a sync that fired, or a preamble the --max-ppm gate dropped.  More than 64 chunks of at most 3
    evaluations in a row that do NOT continue one another: case tail_short forces it, with the expectation "the recurrence from 0 over the
    k in reach", bit for bit, and its distance from the reference program printed by tests/test_nf_reference.py (1.0e-6 at most in the
    case's 8 such updates, k = 129 .. 248; mag_nf moves in one of them, by one ulp).  The walker does not produce this: after a sync or a
    drop pherr[1] and pherr[2] are reset, so the next fire is two evaluations away at the least, and a run of such chunks needs the sync
    metric under its threshold and rising for 6 samples per chunk - a 16-symbol preamble allows a chunk or two, not 64.
    tests/test_nf_reference.py::test_the_walkers_log_keeps_256_evaluations_in_a_few_chunks measures it with the host build on a gated
    capture: never two chunks of fewer than 4 evaluations in a row, the last 256 evaluations in 2 chunks at the most.  So the tail is
    kept by chunks.

The walker's hand-off, end to end (test_noise_floor_matches_the_oracle): the evaluation count and every update's mag_nf of whole captures
against the oracle's trace, fed four ways.

Wall time of the module on an MI355X, and the figures printed here: profiles/nf_probe_device.txt."""
import os

import numpy as np
import pytest

import nf_reference as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    return vdl2hip.load_library()


SHAPES = [(1, 1), (1, 3), (5, 1), (5, 3)]                          # (nchan, grid): neither nchan is a multiple of kNfWaves


@pytest.mark.parametrize("name", nr.CASE_NAMES)
def test_replay(L, name):
    case = nr.get_case(name)
    blobs = {}
    for nchan, grid in SHAPES:
        blobs[(0, nchan, grid)], n = nr.run_case(nr.device_runner(L, 0, grid), case, nchan, f"device mode 0 grid {grid}")
        print(f"{name}: {nchan} channels, k_nf_prepare/replay/finish on {grid} workgroups per channel: {len(case.feeds)} feeds, {n} values equal the reference bit for bit")
    for nchan in (1, 5):
        blobs[(1, nchan, 1)], n = nr.run_case(nr.device_runner(L, 1, 1), case, nchan, "device mode 1")
        print(f"{name}: {nchan} channels, k_nf_all: {len(case.feeds)} feeds, {n} values equal the reference bit for bit")
        same = [blobs[(0, nchan, g)] == blobs[(1, nchan, 1)] for g in (1, 3)]
        print(f"{name}: {nchan} channels: the three kernels on 1 and on 3 workgroups and the single kernel give the same {len(blobs[(1, nchan, 1)])} bytes: {same}")
        assert all(same)


def test_sizes_the_product_cannot_have_are_refused(L):
    case = nr.get_case("groups")
    run = nr.device_runner(L, 0, 1)
    y = np.ascontiguousarray(case.y[:1])
    feed = case.feeds[1]                                             # 31 updates and more
    ch = np.asarray(feed[0], np.int64).reshape(-1, 2)
    chunks = np.zeros((1, case.cap_log), nr.CHUNK); chunks["first"][0, :len(ch)] = ch[:, 0]; chunks["count"][0, :len(ch)] = ch[:, 1]
    nupd = int(ch[:, 1].sum()) // 1000
    INVAL = -1
    def rc(nlog, cap_hist, nf_ring=128, nf=None):
        nf = nr.initial_state(1) if nf is None else nf
        ring = np.zeros((1, nf_ring), np.float32); lp = np.zeros((1, max(cap_hist, 1)), np.float32); fd = np.zeros(1, nr.NFFEED)
        return L.vdl2hip_debug_nf_probe(0, 1, 1, y.ctypes.data, y.shape[1], chunks.ctypes.data, np.array([nlog], np.uint32).ctypes.data, case.cap_log, nf.ctypes.data, ring.ctypes.data, nf_ring,
                                        cap_hist, lp.ctypes.data, fd.ctypes.data)
    assert nupd >= 2
    assert rc(len(ch), nupd + 1) == 0
    assert rc(len(ch), nupd) == INVAL                                # a feed of cap_hist updates
    assert rc(case.cap_log + 1, nupd + 1) == INVAL                   # nlog > cap_log
    assert rc(len(ch), 256, nf_ring=128) == INVAL                    # a history ring shorter than a feed's updates may be
    bad = nr.initial_state(1); bad["evals"] = 5                      # a state whose tail does not add up to its count
    assert rc(len(ch), nupd + 1, nf=bad) == INVAL


@pytest.fixture(scope="module")
def vh(L):
    from dumpvdl2_amd import vdl2hip
    return vdl2hip


WAYS = ["whole", "blocks_320000", "five_pieces", "segments_700x32"]


def _noise_floor_of(vh, cfg, iq, way, monkeypatch):
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    with monkeypatch.context() as m:
        if way == "segments_700x32":
            m.setenv("VDL2HIP_SEG_MIN", "700"); m.setenv("VDL2HIP_SEG_MAX", "32")
        step = {"whole": raw.size, "blocks_320000": 320000, "five_pieces": (raw.size // 5 + 3) & ~3, "segments_700x32": raw.size}[way]
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=step)
        for k in range(0, raw.size, step):
            rx.feed(raw[k:k + step])
        rx.drain()
        out = [rx.read_noise_floor(c) for c in range(len(cfg.freqs))]
        st = rx.stats()
        rx.close()
    return out, st


@pytest.mark.parametrize("name", ["config2_1s", "config4_0p4s", "os10_noisy_1s"])
def test_noise_floor_matches_the_oracle(vh, oracle_mod, monkeypatch, name):
    """The walker's hand-off, end to end, referee on (the default): the evaluation log of a whole capture decides which evaluation triggers
    which update, so `evals` must be the oracle's count exactly, per channel, and every update's mag_nf must be the oracle's within
    1e-4 of the channel's peak |y|.  The bound is derived: mag_lp is a convex combination of magnitudes and the mag_nf step is 1-Lipschitz in
    the sup norm, so |d mag_nf| <= max |d mag| <= sqrt(2) max |d y|, and test_decimated_stream_close_to_reference holds d y to 5e-5 of the
    peak.  The capture is fed whole, in 320 000-byte blocks (the k_nf_burst path), in 5 long pieces, and whole with segments of 700 samples
    (most boundaries inside a burst, the logs stitched): the same stream, so the four must agree with each other bit for bit."""
    import cases
    cfg, iq, _, _ = cases.load(name)
    nch = len(cfg.freqs)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
    D = iq.size // 2 // cfg.oversample
    tr = o.trace_all(D)
    nf_ref = o.trace_noise_floor(D // 3000 + 8)
    o.process(np.ascontiguousarray(iq).view(np.uint8).reshape(-1), block_bytes=1 << 24, nthreads=min(nch, os.cpu_count() or 8))
    evals_ref = [o.sync_evals(c) for c in range(nch)]
    peak = [float(np.hypot(tr[c, :, 0].astype(np.float64), tr[c, :, 1].astype(np.float64)).max()) for c in range(nch)]
    got = {}
    worst = 0.0
    for way in WAYS:
        got[way], st = _noise_floor_of(vh, cfg, iq, way, monkeypatch)
        if way == "segments_700x32":
            assert st["seg_adopted"] > 0, st
        wmax = 0.0
        for c in range(nch):
            nf, ev = got[way][c]
            assert ev == evals_ref[c], f"{name} {way} channel {c}: {ev} evaluations, the oracle {evals_ref[c]}"
            nupd = ev // 1000
            assert len(nf) == nupd + 1 and nf[0] == np.float32(2.0)
            d = float(np.abs(nf[1:].astype(np.float64) - nf_ref[c, :nupd].astype(np.float64)).max()) if nupd else 0.0
            wmax = max(wmax, d / peak[c])
            assert d <= 1e-4 * peak[c], f"{name} {way} channel {c}: mag_nf off by {d:.3e} = {d / peak[c]:.2e} of the peak {peak[c]:.3f}"
        worst = max(worst, wmax)
        print(f"{name} {way}: {nch} channels, evaluations {min(evals_ref)} .. {max(evals_ref)} equal the oracle's; max |mag_nf - oracle| = {wmax:.3e} of the channel's peak (bound 1e-4)")
    for way in WAYS[1:]:
        for c in range(nch):
            assert got[way][c][0].tobytes() == got["whole"][c][0].tobytes(), f"{name}: channel {c} fed as {way} differs from the whole feed"
    print(f"{name}: the four ways of feeding agree bit for bit; max |mag_nf - oracle| = {worst:.3e} of the peak")


def test_feeds_of_one_sample_keep_the_noise_floor(vh, oracle_mod):
    """A feed's evaluation log begins a chunk of its own.  os10_noisy_1s, its first 320 000 bytes in feeds of 40 bytes - one decimated sample
    each, an evaluation every third feed, 8 000 feeds and two updates - and the rest whole: every update's window lies in hundreds of feeds,
    where the state remembers 64 chunks.  nf_prepare joins a feed's first chunk to the chunk it continues, so the evaluation count is the
    oracle's and every mag_nf the oracle's within the bound of test_noise_floor_matches_the_oracle.  (Without the join the 64 remembered
    chunks hold 64 evaluations and mag_lp is off by up to 0.9^64 = 1.2e-3 of the loudest magnitude in the window, at every update.  On
    this capture's noise that is some 4e-5 of the peak, under the bound: the sharp check of the join is the probe's case tiny_feeds, bit for
    bit; this test holds the walker's side of it - that a feed's first chunk does continue the last one - since otherwise nothing would
    be joined and `evals` or the floor would drift.)
    The whole feed's floor is printed beside it and NOT required to be the same bytes: the samples a replay reads are not the same in the two
    runs.  (The likely reason, not traced further:) the referee makes the stretch around a candidate the reference's own once the samples behind it have arrived - for a whole feed
    before any replay, for one-sample feeds up to that many feeds after a replay has read the channeliser's samples there (DESIGN.md
    section 5).  Measured: channel 0 the same bytes, channel 1 one ulp (3.0e-8) apart in some entries."""
    import cases
    cfg, iq, _, _ = cases.load("os10_noisy_1s")
    nch = len(cfg.freqs)
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
    D = iq.size // 2 // cfg.oversample
    tr = o.trace_all(D)
    nf_ref = o.trace_noise_floor(D // 3000 + 8)
    o.process(raw, block_bytes=1 << 24, nthreads=nch)
    got = {}
    for way, tiny in (("whole", 0), ("tiny", 320000)):
        rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=raw.size)
        for k in range(0, tiny, 40):
            rx.feed(raw[k:k + 40])
        rx.feed(raw[tiny:])
        rx.drain()
        got[way] = [rx.read_noise_floor(c) for c in range(nch)]
        rx.close()
    for c in range(nch):
        peak = float(np.hypot(tr[c, :, 0].astype(np.float64), tr[c, :, 1].astype(np.float64)).max())
        for way in ("whole", "tiny"):
            nf, ev = got[way][c]
            assert ev == o.sync_evals(c), f"channel {c} {way}: {ev} evaluations, the oracle {o.sync_evals(c)}"
            assert len(nf) == ev // 1000 + 1
            d = float(np.abs(nf[1:].astype(np.float64) - nf_ref[c, :ev // 1000].astype(np.float64)).max())
            print(f"channel {c} {way}: {ev} evaluations; max |mag_nf - oracle| = {d / peak:.3e} of the peak (bound 1e-4)")
            assert d <= 1e-4 * peak
        a, b = got["tiny"][c][0], got["whole"][c][0]
        print(f"channel {c}: one-sample feeds against the whole feed: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {len(a)} entries differ, by {float(np.abs(a.astype(np.float64) - b).max()):.3e} at the most")
