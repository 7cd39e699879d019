"""One scan round per feed: the pieces of bursts that hold a symbol within the referee's margin are listed right behind the walk
(k_burst_mark) and scanned in the same launch as the walk's noted decisions; the burst decoder's first pass finds them done.

The receiver is config4 WITHOUT its --max-ppm gate (idle channels lock on to their neighbours' leakage: weak bursts, a symbol in a few
hundred within the margin), 1 s, 3 / 8 / 32 channels around the capture's busiest one, against the CPU oracle, strictly: frames,
burst timing and the reference's 18 counters.  `referee_symbol_pieces_ahead` counts the pieces scanned with the check,
`referee_symbol_pieces_late` those the first pass still had to list for a scan round and a second pass of its own - none, feed by
feed, unless a channel was stitched again (its bursts may be others), the mark list ran over or a scan was refused: those go the old
way, which the hooks `force_again`, `force_mismatch` and `mark_cap` make certain."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import cases
from util import assert_frames_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


@functools.lru_cache(maxsize=None)
def capture():
    """-> (cfg of all 256 channels, iq, the middle one of the three neighbouring channels with the most bursts, (channel, first IQ
    sample) of every burst)"""
    from dumpvdl2_amd import workloads, synth
    cfg = dataclasses.replace(workloads.config4(1.0), rx_max_ppm=0.0)
    iq, bursts = synth.synthesize(cfg)
    per = np.bincount([b.chan for b in bursts], minlength=len(cfg.freqs))
    three = per[:-2] + per[1:-1] + per[2:]
    c = int(np.argmax(three[15:-15])) + 16
    return cfg, iq, c, sorted((b.chan, b.start_sample) for b in bursts)


@functools.lru_cache(maxsize=None)
def reference(nchan):
    """-> (cfg of nchan channels around the busiest one, raw bytes, the oracle's frames, its counters): computed once per size"""
    from oracle import pyoracle
    pyoracle.build()
    cfg, iq, c, _ = capture()
    first = c - nchan // 2
    cfg = dataclasses.replace(cfg, freqs=tuple(cfg.freqs[first:first + nchan]))
    o = pyoracle.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=20, max_ppm=0.0)
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    o.process(raw, block_bytes=1 << 24, nthreads=min(nchan, os.cpu_count() or 8, 16))
    return cfg, raw, o.frames(), [list(o.counters(k).values()) for k in range(nchan)]


def cuts(how, nbytes, nchan):
    """where the capture is cut into feeds (byte offsets)"""
    if how == "whole":
        return [0, nbytes]
    if how == "blocks":
        return list(range(0, nbytes, 320000)) + [nbytes]
    if how == "thirds":      # three long feeds (35 000 decimated samples each: two walk segments and more)
        return [0, nbytes // 12 * 4, nbytes // 12 * 8, nbytes]
    # inside the unique word (10 symbols = 2 000 IQ samples after the burst's first sample: ramp-up 5 symbols, 16 of preamble) of every
    # other burst of the receiver's channels, and inside the data (60 symbols on) of the bursts between those
    _, _, c, bursts = capture()
    starts = sorted(s for k, s in bursts if c - nchan // 2 <= k < c - nchan // 2 + nchan)
    at = sorted({4 * (s + 2000) for s in starts[0::2]} | {4 * (s + 12000) for s in starts[1::2]})
    return [0] + [a for a in at if 0 < a < nbytes] + [nbytes]


PER_FEED = ("referee_rewalks", "referee_symbol_pieces_ahead", "referee_symbol_pieces_late")


def decode(vh, nchan, how="whole", debug=None, per_feed=False):
    """-> the receiver's statistics at the end; per_feed: every feed is drained before the next one is fed and st["per_feed"] lists
    what each added to the counters of PER_FEED"""
    cfg, raw, fo, co = reference(nchan)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), 20, vh.FMT_S16LE, 0.0, max_block_bytes=raw.size)
    for k, v in (debug or {}).items():
        rx.debug_option(k, v)
    edge = cuts(how, raw.size, nchan)
    fg, deltas, before = [], [], rx.stats()
    for a, b in zip(edge[:-1], edge[1:]):
        rx.feed(raw[a:b])
        if per_feed:
            fg += rx.drain()
            now = rx.stats()
            deltas.append({k: now[k] - before[k] for k in PER_FEED}); before = now
    fg += rx.drain()
    cg = [list(rx.counters(k).values()) for k in range(nchan)]
    st = rx.stats()
    rx.close()
    label = f"{nchan} channels, {how}, {debug}"
    assert len(fo) > 0, label
    assert_frames_equal(fo, fg, label=label)
    n18 = cases.N_REFERENCE_COUNTERS      # (the two behind them are this project's own diagnostics)
    assert [c[:n18] for c in cg] == [c[:n18] for c in co], f"{label}: reference counters differ"
    assert st["referee_refused"] == 0, st
    print(label, {k: v for k, v in st.items() if k.startswith("referee_")})
    st["per_feed"] = deltas
    return st


def assert_nothing_late_without_a_second_stitch(st):
    """feed by feed: where no channel was stitched again, pass 1 listed nothing - and there are such feeds, with pieces scanned ahead"""
    clean = [d for d in st["per_feed"] if d["referee_rewalks"] == 0]
    assert clean and sum(d["referee_symbol_pieces_ahead"] for d in clean) > 0, st["per_feed"]
    assert all(d["referee_symbol_pieces_late"] == 0 for d in clean), st["per_feed"]


@pytest.mark.parametrize("how", ["whole", "pieces", "blocks"])
@pytest.mark.parametrize("nchan", [3, 8])
def test_pieces_are_scanned_with_the_check(vh, nchan, how):
    st = decode(vh, nchan, how, per_feed=True)
    assert st["referee_symbol_pieces_ahead"] > 0, st
    assert_nothing_late_without_a_second_stitch(st)


@pytest.mark.parametrize("nchan", [3, 8])
def test_feeds_in_flight_give_the_same(vh, nchan):
    """(the cases above drain feed by feed to read the statistics; here the feeds follow each other as a caller's do)"""
    st = decode(vh, nchan, "pieces")
    assert st["referee_symbol_pieces_ahead"] > 0, st


@pytest.mark.parametrize("mismatch", [0, 1])
@pytest.mark.parametrize("nchan", [3, 8, 32])
def test_channels_stitched_again_fall_back_to_the_second_pass(vh, nchan, mismatch):
    """Three long feeds, the next feed's walk ahead of every feed's check (hook walk_ahead: receivers under 16 channels do not choose
    that themselves), every channel of every feed flagged (force_again) - and, with force_mismatch, every second walk taken to have
    ended elsewhere than the next feed's walk began, so that the next feed's burst rows are written once more AFTER its marks were taken."""
    st = decode(vh, nchan, "thirds", {"walk_ahead": 1, "force_again": 1, "force_mismatch": mismatch})
    assert st["referee_rewalks"] >= 2 * nchan, st      # (every channel of every feed that has a check)
    if mismatch:
        assert st["referee_redone_next"] >= nchan, st   # (at least one feed had its successor's walk ahead of its check)


@pytest.mark.parametrize("how", ["whole", "blocks"])
def test_a_mark_list_that_runs_over_goes_the_old_way(vh, how):
    st = decode(vh, 8, how, {"mark_cap": 1})
    assert st["referee_symbol_pieces_late"] > 0, st


@pytest.mark.parametrize("nchan", [3, 8])
def test_without_the_referee_nothing_is_marked(vh, monkeypatch, nchan):
    """The mark kernel is not launched, nothing is listed or scanned.  Without the referee the receiver is held to the oracle as
    tests/fuzz_gpu.py holds a referee-off run: counted ties (at most 2 % of the frames, two samples) and the failure bookkeeping of
    bursts that deliver nothing on at most a quarter of the channels; everything else identical."""
    from util import compare_at_full_size, compare_reference_counters
    monkeypatch.setenv("VDL2HIP_REFEREE", "0")
    cfg, raw, fo, co = reference(nchan)
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), 20, vh.FMT_S16LE, 0.0, max_block_bytes=raw.size)
    rx.feed(raw)
    fg = rx.drain()
    st = rx.stats()
    cg = [list(rx.counters(k).values()) for k in range(nchan)]
    names = list(rx.counters(0).keys())
    rx.close()
    assert st["referee_symbol_pieces_ahead"] == 0 and st["referee_symbol_pieces_late"] == 0 and st["referee_scans"] == 0, st
    assert len(fo) > 0
    print(compare_at_full_size(fo, fg, label=f"{nchan} channels, referee off", max_tie_frac=0.02))
    compare_reference_counters(names, co, cg, label=f"{nchan} channels, referee off", strict=False, max_channels=max(1, nchan // 4))


@pytest.mark.parametrize("how", ["whole", "pieces"])
def test_thirty_two_channels_with_scans_ahead_of_the_walk(vh, how):
    st = decode(vh, 32, how, per_feed=True)
    assert st["referee_symbol_pieces_ahead"] > 0, st
    assert_nothing_late_without_a_second_stitch(st)
    if how == "pieces":
        assert decode(vh, 32, how)["referee_symbol_pieces_ahead"] > 0      # (and with the feeds in flight)
