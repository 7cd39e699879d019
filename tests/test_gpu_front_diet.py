"""The parts of the front kernels that were rewritten to issue fewer vector instructions, at the smallest shapes at which they can go
wrong.  Nothing here has a bound or a reference of its own: the helpers, references and bounds are those of tests/test_gpu_k1_stream.py
(the channeliser against the channel filter in double precision) and of tests/test_gpu_sync_screen.py (the screening kernel's flag
words against the flags predicted from the device's phase_fast of y).

K1 (k_chanfir): a lane's first block waits in LDS for the scan instead of in registers, the cross-lane moves of the scan keep what
they used to select, the stores of the carried state and the segment-end branch moved out of the channel loop.  What that can break
shows at a partial last tile - its last block on either output of a lane (ib = 0, 1), in the first lanes and in the last - at a ring
offset that is odd (the unaligned store path), with channels that do not exist in a wavefront and wavefronts without channels, on the
fused look-back and on the separate fix-up kernel.  Every cell is three feeds: 1 025 outputs (odd: the second feed starts on an odd
ring slot), the feed under test, then 100 outputs (shorter than a tile); the whole stream is compared.  4 and 5 channels run the one
channel-per-wavefront build (the receiver gives a wavefront four channels from 16 channels up), 17 channels the build the flagship
runs, k_chanfir<20, 2, 4>: its fifth group holds one channel of four, and three wavefronts of the second workgroup hold none.

K3a (k_sync_screen): tiles that lie wholly inside the feed write their flag words without per-sample range tests; the edge tiles
keep the old code.  Feeds of 2 560 m + {0, 1, 63, 64, 65} decimated samples, a first feed shorter than the 150 samples of history,
three feeds in a row: full and edge tiles side by side, tiles that start on any word of the ring, last words of every filling."""
import numpy as np
import pytest

import k1_reference as k1
import test_gpu_k1_stream as ks
import test_gpu_sync_screen as ss

pytestmark = pytest.mark.gpu
OS20 = 20
FIRST, SHORT = 1025, 100                # outputs of the feed before (odd) and of the feed after (less than a tile of 128)


vh = ks.vh                              # (the helpers' own fixtures: the library, the host build of the screen arithmetic)
hs = ss.hs


def plan(nch):
    freqs, loud = k1.channel_plan(OS20, max(nch, 9))
    return freqs[:nch], loud


def three_feeds(d, os_=OS20):
    return lambda total: iter([FIRST * os_, d * os_, SHORT * os_])


@pytest.mark.parametrize("fuse", ["fused", "no_fuse"])
@pytest.mark.parametrize("r", [1, 2, 127])
@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("nch", [4, 5, 17])
def test_k1_partial_tiles(vh, oracle_mod, monkeypatch, nch, k, r, fuse):
    if fuse == "no_fuse":
        monkeypatch.setenv("VDL2HIP_NO_FUSE", "1")        # read when the receiver is created
    d = 128 * k + r
    freqs, loud = plan(nch)
    raw = ks.dense(OS20, freqs, loud, ks.S16, (FIRST + d + SHORT) * OS20, seed=1000 * nch + d)
    ks.run_cell(vh, oracle_mod, f"diet {nch}ch {d} outputs {fuse}", OS20, freqs, ks.S16, raw, three_feeds(d))


def test_k1_unsigned_bytes(vh, oracle_mod):
    d = 128 * 3 + 127
    freqs, loud = plan(17)
    raw = ks.dense(OS20, freqs, loud, ks.U8, (FIRST + d + SHORT) * OS20, seed=8)
    ks.run_cell(vh, oracle_mod, f"diet 17ch {d} outputs u8", OS20, freqs, ks.U8, raw, three_feeds(d))


def test_k1_float32(vh, oracle_mod):
    """a float32 rendering of the s16 capture: the s16 receiver's stream is held to the double-precision filter, and the float32
    receiver's stream is the same bits (the two builds share everything after the staging; tests/test_gpu_cf32.py)"""
    d = 128 * 3 + 1
    freqs, loud = plan(17)
    raw = ks.dense(OS20, freqs, loud, ks.S16, (FIRST + d + SHORT) * OS20, seed=32)
    r = ks.run_cell(vh, oracle_mod, f"diet 17ch {d} outputs s16 (for cf32)", OS20, freqs, ks.S16, raw, three_feeds(d))
    f32 = (raw.view("<i2").astype(np.float32) / np.float32(32768.0)).view(np.uint8)
    rx = vh.Receiver(k1.CF, freqs, OS20, vh.FMT_CF32, 0.0, max_block_bytes=FIRST * OS20 * 8 + d * OS20 * 8)
    try:
        rx.debug_option("referee", 0)
        off = 0
        for m in three_feeds(d)(None):
            rx.feed(f32[off * 8:(off + m) * 8]); off += m
        rx.sync()
        total = FIRST + d + SHORT
        got = np.stack([rx.read_decimated(c, 0, total) for c in range(len(freqs))])
    finally:
        rx.close()
    assert got.shape == r["got"].shape
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(r["got"]).view(np.uint32))


# ---- K3a

def screen_case(vh, hs, label, pieces_dec):
    total = sum(pieces_dec)
    raw = ss.as_s16(ss.capture(3)[:total * ss.OS])
    freqs = ss.FREQS[3][:2]
    pieces = [p * ss.OS for p in pieces_dec] if len(pieces_dec) > 1 else None
    S, X = ss.both(vh, freqs, raw, vh.FMT_S16LE, pieces=pieces, max_block=raw.size * 2)
    assert S.ndec == total
    ends = [int(e) for e in np.cumsum(pieces_dec)]
    ss.check_pair(vh, hs, S, X, label, populated=False, ends=ends)
    for c in range(2):
        # the flags are no constant: the screen passes most of the noise and flags the bursts
        n = int(S.flags[c][:total].sum())
        assert 0 < n < total // 2, f"{label}: channel {c}: {n} of {total} samples flagged"
        # screen_all: every sample of the feed, full tile or edge tile, and nothing past the last one
        assert X.flags[c][:total].all() and not X.flags[c][total:].any(), f"{label}: channel {c}: screen_all"


@pytest.mark.parametrize("extra", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("m", [1, 2])
def test_k3a_feed_lengths(vh, hs, m, extra):
    screen_case(vh, hs, f"diet screen {m} x 2560 + {extra}", [ss.TILE * m + extra])


@pytest.mark.parametrize("pieces", [[100, ss.TILE + 63, 2 * ss.TILE + 1], [ss.TILE + 64, ss.TILE + 65, 2 * ss.TILE], [149, 2 * ss.TILE + 65, ss.TILE]],
                         ids=["short-first", "word-edges", "history-minus-1"])
def test_k3a_feeds_in_a_row(vh, hs, pieces):
    screen_case(vh, hs, f"diet screen feeds {pieces}", pieces)
