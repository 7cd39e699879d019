"""The exact sync tier's dense form (kernels.h: k_sync_dense - list the busy words, one lane per evaluation, decide per word) against
the word-at-a-time form it replaced (k_sync_exact4, kept as the yardstick: test hook "exact_tier" = 0).  The same feeds go through
two receivers, one of each form, and everything the tier writes is compared with read_sync():

  cand  equal at every sample read;
  pf    BIT-equal (the float's bits, sign - the referee's mark - included) at every sample read.  pf is zeroed when a receiver is
        created and written by this tier alone, at the samples with work (`need`): equality everywhere is equality on the `need` set
        of either form, and says besides that the two forms write the same set.  With the test hook "screen_all" = 1 the screening
        tier flags every sample, `need` is every sample, and every sample's evaluation is compared;
  frames, timing, integer metadata and counters of both receivers against the committed golden answers; the referee's statistics
        equal between the two (with the scans ahead of the walk that covers the set of stretch requests the tier lists).

"screen_all" = 1 with the dense form is also its worst case - every word of every feed on the list, 70 evaluations a word - through
the same tiles as the sparse case: the golden answers again (flags are only ever conservative).

Wall time of the module on an MI355X: 14-15 s (37 tests)."""
import dataclasses

import numpy as np
import pytest

import cases
from util import assert_frames_equal

pytestmark = pytest.mark.gpu

GOLDEN = ["config2_1s", "config4_0p4s", "config5_0p4s", "os10_noisy_1s", "config3_0p6s"]
# input samples per feed (lo, hi) and the largest block the receiver is made for (bytes; None: the whole capture in one feed)
CHUNKINGS = {
    "one": (None, None),
    "in_word": ((30_011, 90_017), 1_600_000),       # feed boundaries inside a 64-sample word of the decimated stream (odd lengths)
    "short": ((100, 9_000), 40_000),                 # one feed in eight of fewer than 64 decimated samples (os 20: < 1 280 input samples)
    "wrap": ((20_000, 60_000), 240_000),             # a ring of a few feeds: the captures go round it several times
}


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def decode(vh, cfg, iq, tier, chunking, referee=1, screen_all=0, seed=11):
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    chunks, max_block = CHUNKINGS[chunking]
    rx = vh.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=max_block or raw.size)
    rx.debug_option("exact_tier", tier)
    rx.debug_option("screen_all", screen_all)
    if not referee:
        rx.debug_option("referee", 0)
    if chunks is None:
        rx.feed(raw)
    else:
        rng = np.random.default_rng(seed); k = 0
        while k < raw.size:
            m = min(raw.size - k, int(rng.integers(*chunks)) * 4)
            rx.feed(raw[k:k + m]); k += m
    fr = rx.drain()
    cnt = [list(rx.counters(c).values()) for c in range(len(cfg.freqs))]
    # what the ring still holds for certain: the last block's worth of decimated samples
    D = raw.size // 4 // cfg.oversample
    first = max(0, D - (max_block or raw.size) // 4 // cfg.oversample)
    sync = [rx.read_sync(c, first, D - first) for c in range(len(cfg.freqs))]
    st = rx.stats()
    rx.close()
    return fr, cnt, sync, st


def assert_same_sync(a, b, label):
    assert len(a) == len(b)
    for c, ((pfa, ca), (pfb, cb)) in enumerate(zip(a, b)):
        assert len(ca) == len(cb) and len(ca) > 0, f"{label}: channel {c}: {len(ca)} / {len(cb)} samples read"
        d = np.flatnonzero(ca != cb)
        assert d.size == 0, f"{label}: channel {c}: cand differs at {d.size} samples, first {d[:5]}"
        ua, ub = pfa.view(np.uint32), pfb.view(np.uint32)
        d = np.flatnonzero((ua != ub).any(axis=1))
        assert d.size == 0, f"{label}: channel {c}: pf differs at {d.size} samples, first {d[:5]}: {pfa[d[:3]]} / {pfb[d[:3]]}"


def both_forms(vh, cfg, iq, gold, label, scans_ahead=False, **kw):
    old = decode(vh, cfg, iq, 0, **kw)
    new = decode(vh, cfg, iq, 1, **kw)
    assert_same_sync(old[2], new[2], label)
    if gold is not None:
        cases.check_against_golden(old[0], old[1], gold, label=f"{label} exact_tier=0", exact_diagnostics=False)
        cases.check_against_golden(new[0], new[1], gold, label=f"{label} exact_tier=1", exact_diagnostics=False)
    else:
        assert len(old[0]) > 0
        assert_frames_equal(old[0], new[0], label=label)
        assert old[1] == new[1], label
    if scans_ahead:                                         # (the stretches scanned are then the ones the exact tier has listed)
        ref = lambda st: {k: v for k, v in st.items() if k.startswith("referee_")}
        assert ref(old[3]) == ref(new[3]), f"{label}: {ref(old[3])} / {ref(new[3])}"
    return new


def scans_ahead(cfg, prescan):
    return prescan == 1 or (prescan is None and len(cfg.freqs) <= 64)


def prescans(cfg):
    """the library's own choice, and - where the capture has few enough channels for the scans ahead of the walk - the other one"""
    return (None, 0, 1) if len(cfg.freqs) <= 64 else (None,)


@pytest.mark.parametrize("referee", [1, 0])
@pytest.mark.parametrize("name", GOLDEN)
def test_one_feed(vh, monkeypatch, name, referee):
    cfg, iq, _, gold = cases.load(name)
    for prescan in prescans(cfg) if referee else (None,):
        if prescan is None:
            monkeypatch.delenv("VDL2HIP_REF_PRESCAN", raising=False)
        else:
            monkeypatch.setenv("VDL2HIP_REF_PRESCAN", str(prescan))
        both_forms(vh, cfg, iq, gold, f"{name} referee={referee} prescan={prescan}", chunking="one", referee=referee, scans_ahead=bool(referee) and scans_ahead(cfg, prescan))


@pytest.mark.parametrize("chunking", ["in_word", "short", "wrap"])
@pytest.mark.parametrize("name", GOLDEN)
def test_chunked_feeds(vh, monkeypatch, name, chunking):
    cfg, iq, _, gold = cases.load(name)
    for prescan in prescans(cfg)[-1:]:                      # (few channels: the scans ahead of the walk, the FULL form of the metric's margins)
        if prescan is None:
            monkeypatch.delenv("VDL2HIP_REF_PRESCAN", raising=False)
        else:
            monkeypatch.setenv("VDL2HIP_REF_PRESCAN", str(prescan))
        both_forms(vh, cfg, iq, gold, f"{name} {chunking} prescan={prescan}", chunking=chunking, scans_ahead=scans_ahead(cfg, prescan))
    if name in ("config2_1s", "config4_0p4s"):
        monkeypatch.delenv("VDL2HIP_REF_PRESCAN", raising=False)
        both_forms(vh, cfg, iq, gold, f"{name} {chunking} referee=0", chunking=chunking, referee=0)


@pytest.mark.parametrize("chunking", ["one", "in_word"])
@pytest.mark.parametrize("name", GOLDEN)
def test_every_sample_flagged(vh, name, chunking):
    """screen_all = 1: every sample evaluated and compared between the forms; the dense form's worst-case list gives the golden answers"""
    cfg, iq, _, gold = cases.load(name)
    both_forms(vh, cfg, iq, gold, f"{name} {chunking} screen_all", chunking=chunking, screen_all=1)


@pytest.mark.parametrize("chunking", ["one", "in_word"])
def test_weak_bursts_without_the_ppm_gate(vh, chunking):
    """config4 without its --max-ppm gate: idle channels lock on to what leaks over from their neighbours - weak bursts by the hundred,
    candidates within the referee's margin by the dozen (no golden answers are kept for it: the two forms against each other)"""
    from dumpvdl2_amd import workloads, synth
    cfg = dataclasses.replace(workloads.config4(0.5), rx_max_ppm=0.0)
    iq, _ = synth.synthesize(cfg)
    both_forms(vh, cfg, iq, None, f"no gate {chunking}", chunking=chunking)
