"""Who owns what in the host library (dumpvdl2_amd/csrc/hostmem.h, DESIGN.md "Ownership"): every device buffer, page-locked buffer and
event of a receiver is a member that frees itself, and the library counts the live ones per kind.  live() below is that count
(vdl2hip_debug_live_resources); the tests hold it to what it was before a receiver existed - after a plain create and destroy, after
a destroy with feeds still running, across taps switched on and off and back - and check that the two staging buffers grow once.

The standard receiver: two channels, oversample 10, 16-bit input, blocks of 320 000 bytes, fed the first three blocks of the
reference's test vector.  The vector's one burst begins in the second block (sync at decimated sample 11 975 of 8 000 per block) and
ends in the fourth: these three blocks deliver no frame and no capture record, so nothing here depends on when one arrives."""
import numpy as np
import pytest

import cases
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
FREQS = [CF, CF + 25000]
BLOCK = 320000
MAIL_FRAMES = 8          # kernels.h: kMailFrames - the frames of a feed that come to the host with its control block


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def standard(vh, **kw):
    return vh.Receiver(CF, FREQS, 10, vh.FMT_S16LE, **kw)


@pytest.fixture(scope="module")
def baseline(vh):
    """the counts once one receiver has come and gone: the stream pool and the runtime have settled"""
    standard(vh).close()
    return vh.live_resources()


def blocks(wav, n=3):
    return [wav[k * BLOCK:(k + 1) * BLOCK] for k in range(n)]


def all_taps_on(rx):
    rx.spectrum_enable(1024)
    rx.activity_enable()
    rx.capture_enable()
    rx.txlog_enable()
    rx.txsearch_enable()


@pytest.mark.parametrize("how", ["standard", "referee off", "resampling"])
def test_create_destroy_returns_everything(vh, golden_wav, baseline, monkeypatch, how):
    if how == "referee off":
        monkeypatch.setenv("VDL2HIP_REFEREE", "0")
    rx = standard(vh, input_rate=1250000) if how == "resampling" else standard(vh)
    held = vh.live_resources()
    assert all(held[k] > baseline[k] for k in held), (how, held, baseline)
    for b in blocks(golden_wav):
        rx.feed(b)
    rx.sync()
    rx.close()
    assert vh.live_resources() == baseline, how


def test_destroy_with_feeds_in_flight(vh, golden_wav, baseline):
    """profiling level 2 and every tap: each feed carries its timing events and the taps' launches; nothing is waited for before the
    receiver goes - destroy has to wait for every stream before it frees what they work on"""
    rx = standard(vh)
    rx.set_profiling(2)
    all_taps_on(rx)
    for b in blocks(golden_wav):
        rx.feed(b)
    rx.close()
    assert vh.live_resources() == baseline


def test_tap_switching_does_not_grow(vh, golden_wav, baseline):
    """A tap that is enabled again, with other parameters or the same, holds what it held the first time; disabled, the receiver holds
    what it held after the first disable (the tap's read event and landing buffer stay with the receiver by design).
    Every feed is the first block.  Six of them come first: a slot's input buffer and copy event are made on the slot's first feed."""
    b0 = blocks(golden_wav, 1)[0]
    rx = standard(vh)

    def feed():
        rx.feed(b0)
        rx.sync()
        return vh.live_resources()

    for _ in range(6):
        settled = feed()
    taps = [
        ("spectrum", lambda p: rx.spectrum_enable(p), rx.spectrum_disable, [256, 1024], None),
        ("activity", lambda p: rx.activity_enable(bin_samples=p), rx.activity_disable, [105, 210], None),
        ("capture", lambda p: rx.capture_enable(pool_samples=p), rx.capture_disable, [1 << 16, 1 << 18], None),
        # (the log runs beside the activity monitor, which is enabled once more and left on; the search beside the log, likewise)
        ("log", lambda p: rx.txlog_enable(pool_records=p), rx.txlog_disable, [1024, 4096], rx.activity_enable),
        ("search", lambda p: rx.txsearch_enable(undecoded_only=p), rx.txsearch_disable, [False, True], rx.txlog_enable),
    ]
    for name, enable, disable, params, first in taps:
        if first:
            first()
            settled = feed()
        enable(params[0])
        on = {params[0]: feed()}
        assert on[params[0]]["device"] > settled["device"], name
        off = None
        for cycle in range(4):
            p = params[(cycle + 1) % 2]
            enable(p)
            got = feed()
            assert got == on.setdefault(p, got), (name, "enable", p, cycle)
            disable()
            got = vh.live_resources()
            off = off or got
            assert got == off, (name, "disable", cycle)
            assert got["device"] == settled["device"], (name, "the tap's device buffers are back", cycle)
        settled = off
    rx.close()
    assert vh.live_resources() == baseline


def test_staging_grows_once(vh, baseline):
    """os10_noisy_1s (two channels, oversample 10, one second) in ONE feed: 24 frames in the golden answers, three times what comes
    with the control block, and nine bursts with their IQ - the frames' staging buffer and the capture's are both needed, each grows
    once, and a second feed of the same size finds them large enough."""
    cfg, iq, _, gold = cases.load("os10_noisy_1s")
    raw = np.asarray(iq).view(np.uint8).reshape(-1)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=raw.size)
    rx.capture_enable()
    p0 = vh.live_resources()["pinned"]
    rx.feed(raw)
    rx.sync()
    frames = rx.drain()
    recs, _ = rx.capture_read()
    print(f"os10_noisy_1s in one feed: {len(frames)} frames, {len(recs)} capture records")
    assert len(frames) == len(gold["frames"]) > MAIL_FRAMES and len(recs) > 0
    p1 = vh.live_resources()["pinned"]
    assert 1 <= p1 - p0 <= 2, "one block per staging site at the most"
    rx.feed(raw)
    rx.sync()
    assert len(rx.drain()) > MAIL_FRAMES
    assert vh.live_resources()["pinned"] == p1
    rx.close()
    assert vh.live_resources() == baseline


def test_results_unchanged_with_everything_on(vh, golden_wav):
    def run(everything):
        rx = standard(vh)
        if everything:
            rx.set_profiling(2)
            all_taps_on(rx)
        for k in range(0, golden_wav.size, BLOCK):
            rx.feed(golden_wav[k:k + BLOCK])
        rx.sync()
        frames = rx.drain()
        rx.close()
        return frames

    plain = run(False)
    assert len(plain) == 2
    assert_frames_equal(plain, run(True), exact_samples=True, label="all taps on, profiling 2")
