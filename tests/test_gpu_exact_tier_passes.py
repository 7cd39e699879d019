"""The dense exact sync tier's list step (kernels.h: k_sync_dense) - every wavefront lists its quarter of a workgroup's passes on its
own, no workgroup barrier between passes, a bounded list that is worked off whenever a reservation is refused - against the
word-at-a-time form (k_sync_exact4: test hook "exact_tier" = 0) on the same feeds.  Compared at EVERY sample of every channel looked
at: the candidate bits and the bits of pf (the referee's mark is its sign; pf is zero where the tier did not write, so equality
everywhere says the two forms wrote the same set of samples); and frames, counters and - where the receiver scans ahead of the walk - the referee's statistics (those
scans serve the set of stretch requests the tier lists; rq_flag* and the control block show in the frames and counters).

The pass count (vdl2hip.hip, feed_common: the largest wpl <= kK3dRounds = 32 that leaves ceil(words / (256 wpl)) x channels >=
kK3dMinGroups = 2 048 workgroups, else 1) is reached through the feed length and the channel count alone:
  1, 2 channels                      wpl = 1 whatever the length: seams between wavefronts and workgroups, feed and ring edges;
  256 channels x  7 232 words        wpl = 4: with every sample flagged a workgroup's 1 024 words go through a list of 512 - refused
                                     reservations, the list worked off several times, wavefronts resuming at different passes;
  256 channels x 14 400 words        wpl = 8 (the benchmark's);
  256 channels x 57 408 words        wpl = 32 = kK3dRounds.
The flags of a feed are all its screening kernel's: "screen_all" flags whole feeds.  Flagged and idle stretches WITHIN a feed are
made by the signal: complex float32 input whose stretches of noise alternate with stretches of float32 denormals.  There the
decimated samples are too small for the screening tier's reciprocal (phase_fast: an infinity, a NaN in every window it enters,
"flag it"), so two words in three are busy, in runs, and a workgroup of 1 024 words refuses reservations among idle words, with
wavefronts stopped at different passes (test_refusals_among_idle_words asserts that the flags came out so).

Wall time of the module on an MI355X: profiles/exact_tier_passes_ab.txt."""
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


def run(vh, cfg, freqs, iq, tier, feeds, referee=1, max_block=None, look=None, cf32=False):
    """feeds: [(input samples, screen_all)] - the last one takes what is left.  -> frames, counters, [(pf, cand)] of the channels
    `look` over the samples the ring still holds for certain, the flags there, statistics.  cf32: iq is complex64, not int16 pairs"""
    raw = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    B = 8 if cf32 else 4                                        # bytes per input sample
    rx = vh.Receiver(cfg.centerfreq, list(freqs), cfg.oversample, vh.FMT_CF32 if cf32 else vh.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=max_block or raw.size)
    rx.debug_option("exact_tier", tier)
    if not referee:
        rx.debug_option("referee", 0)
    k = 0
    for i, (n, dense) in enumerate(feeds):
        m = raw.size - k if i == len(feeds) - 1 else min(B * n, raw.size - k)
        rx.debug_option("screen_all", dense)
        if m > 0:
            rx.feed(raw[k:k + m]); k += m
    assert k == raw.size
    fr = rx.drain()
    cnt = [list(rx.counters(c).values()) for c in range(len(freqs))]
    D = raw.size // B // cfg.oversample
    first = max(0, D - (max_block or raw.size) // B // cfg.oversample)
    look = range(len(freqs)) if look is None else look
    sync = [rx.read_sync(c, first, D - first) for c in look]
    flags = [rx.read_flags(c, first, D - first) for c in look]
    st = rx.stats()
    rx.close()
    return fr, cnt, sync, flags, st


def both(vh, cfg, freqs, iq, feeds, label, frames=True, scans_ahead=True, **kw):
    old = run(vh, cfg, freqs, iq, 0, feeds, **kw)
    new = run(vh, cfg, freqs, iq, 1, feeds, **kw)
    for c, ((pfa, ca), (pfb, cb)) in enumerate(zip(old[2], new[2])):
        assert len(ca) == len(cb) and len(ca) > 0, f"{label}: channel {c}: {len(ca)} / {len(cb)} samples read"
        d = np.flatnonzero(ca != cb)
        assert d.size == 0, f"{label}: channel {c}: cand differs at {d.size} samples, first {d[:5]}"
        d = np.flatnonzero((pfa.view(np.uint32) != pfb.view(np.uint32)).any(axis=1))
        assert d.size == 0, f"{label}: channel {c}: pf differs at {d.size} samples, first {d[:5]}: {pfa[d[:3]]} / {pfb[d[:3]]}"
    for fa, fb in zip(old[3], new[3]):
        assert np.array_equal(fa, fb), f"{label}: the two receivers were not given the same flags"
    if frames:
        assert_frames_equal(old[0], new[0], label=label)
    assert old[1] == new[1], f"{label}: counters"
    if scans_ahead:
        # (the stretches scanned are then the ones the exact tier has listed.  Without the scans ahead of the walk - more than 64
        # channels, or switched off - the tier lists none, and how the walk's own requests divide into scanned and found done
        # already differs from run to run of either form: 490 + 486 against 491 + 485 at 256 channels)
        ref = lambda st: {k: v for k, v in st.items() if k.startswith("referee_")}
        assert ref(old[4]) == ref(new[4]), f"{label}: {ref(old[4])} / {ref(new[4])}"
    return new


def dec(cfg, n_dec, at_input=0, odd=7):
    """input samples that carry the stream from input sample `at_input` to n_dec more decimated samples and `odd` input samples on"""
    return (at_input // cfg.oversample + n_dec) * cfg.oversample + odd - at_input


@pytest.mark.parametrize("p", [1, 2, 5])
@pytest.mark.parametrize("nchan", [1, 2])
def test_pass_and_wavefront_seams(vh, nchan, p):
    """feeds of 64 x 256 x p + r decimated samples cut at arbitrary input samples: the first and last word of a feed, and the partial
    last word the next feed does again, on the seams between wavefronts and workgroups"""
    cfg, iq, _, _ = cases.load("config2_1s")
    freqs = list(cfg.freqs)[:nchan]
    for r in (0, 1, 63, 64, 67):
        a0 = 1237 + 20 * r
        n1 = dec(cfg, 64 * 256 * p + r, a0, odd=3 + r % 11)
        both(vh, cfg, freqs, iq, [(a0, 0), (n1, 0), (0, 0)], f"seams {nchan} ch p={p} r={r}")


@pytest.mark.parametrize("referee", [1, 0])
def test_busy_word_at_a_wavefront_edge(vh, referee):
    """the first and the last flagged word of a burst's run of flagged words put on lane 0 and on lane 63 of each of a workgroup's four
    wavefronts (the feed is cut so): their work masks reach into the neighbouring wavefront's word (fprev >> 61, fnext << 61), and the
    six samples before a word are another wavefront's"""
    cfg, iq, _, _ = cases.load("config2_1s")
    freqs = list(cfg.freqs)[:1]
    probe = run(vh, cfg, freqs, iq, 1, [(0, 0)], referee=referee)
    fl = probe[3][0]
    words = np.flatnonzero(fl[:fl.size // 64 * 64].reshape(-1, 64).any(axis=1))
    words = words[words >= 320]
    assert words.size >= 2, "the capture has flagged words"
    runs = np.split(words, np.flatnonzero(np.diff(words) > 1) + 1)
    picks = [int(runs[0][0]), int(runs[0][-1]), int(runs[-1][0]), int(runs[-1][-1])]
    for W in sorted(set(picks)):
        for j in range(4):
            for lane in (0, 63):
                w0 = W - lane - 64 * j                          # the feed's first word: W is word 64 j + lane of the workgroup
                feeds = [(dec(cfg, 64 * w0 + 5, 0, odd=3), 0), (0, 0)]
                # where the second feed begins: the word of the first decimated sample the first feed has not produced (the partial
                # word is done again).  One workgroup of one pass (wpl = 1) starts there; W is its thread W - base.
                base = (feeds[0][0] // cfg.oversample) >> 6
                assert base == w0 and 0 <= W - base < 256 and (W - base) // 64 == j and (W - base) % 64 == lane, (W, base, j, lane)
                new = both(vh, cfg, freqs, iq, feeds, f"edge W={W} wavefront {j} lane {lane} referee={referee}", referee=referee)
                assert new[3][0][64 * W:64 * W + 64].any(), "the word is flagged in this run too"


@pytest.mark.parametrize("referee", [1, 0])
def test_flagged_and_idle_feeds(vh, referee):
    """2 channels x 40 000 samples with every sample flagged (every word busy, 70 evaluations a word), then short feeds flagged and
    idle by turns: a flagged stretch of a few words on an idle stream, the stream's first word (w = 0, fp6 = 0) flagged and not.
    (Two channels take one pass a workgroup: 256 words on a list of 512, many tiles, no reservation is ever refused here - that is
    test_refusals_among_idle_words, test_every_sample_flagged_without_the_referee and test_many_passes[7232-1].)"""
    cfg, iq, _, _ = cases.load("config2_1s")
    freqs = list(cfg.freqs)[:2]
    for first_dense in (1, 0):
        feeds = [(dec(cfg, 40_000, 0), first_dense)]
        at = feeds[0][0]
        for i, n in enumerate((64, 3, 130, 4_000, 640, 64 * 256 + 1, 200)):
            m = dec(cfg, n, at, odd=1 + 2 * i); feeds.append((m, (i + first_dense) % 2)); at += m
        feeds.append((0, 0))
        both(vh, cfg, freqs, iq, feeds, f"flagged / idle feeds, first flagged={first_dense} referee={referee}", referee=referee)


def test_ring_wrap(vh):
    """feeds that carry the stream round a ring of a few feeds several times, idle and flagged by turns"""
    cfg, iq, _, _ = cases.load("config2_1s")
    freqs = list(cfg.freqs)[:2]
    rng = np.random.default_rng(5)
    feeds, left = [], iq.size // 2
    while left > 60_000:
        n = int(rng.integers(20_000, 60_000)); feeds.append((n, len(feeds) % 3 == 1)); left -= n
    feeds.append((0, 0))
    both(vh, cfg, freqs, iq, feeds, "ring wrap", max_block=240_000)


@pytest.mark.parametrize("prescan", [1, 0])
def test_full_form_and_its_requests(vh, monkeypatch, prescan):
    """a receiver of 64 channels scans ahead of the walk (the FULL form of the metric's margins, the pq stretch requests): one feed,
    and feeds cut inside words with a flagged one among them"""
    monkeypatch.setenv("VDL2HIP_REF_PRESCAN", str(prescan))
    cfg, iq, _, _ = cases.load("config3_0p6s")
    both(vh, cfg, cfg.freqs, iq, [(0, 0)], f"config3 one feed prescan={prescan}", look=(0, 1, 31, 63), scans_ahead=prescan == 1)
    feeds = [(dec(cfg, 20_011, 0), 0)]
    feeds.append((dec(cfg, 1_000, feeds[0][0], odd=9), 1))
    feeds.append((0, 0))
    both(vh, cfg, cfg.freqs, iq, feeds, f"config3 three feeds prescan={prescan}", look=(0, 1, 31, 63), scans_ahead=prescan == 1)


def noise(n):
    """n complex int16 samples: a block of 2^20 samples of noise again and again (the content is beside the point: which words are
    busy is the screening tier's business, and the two forms get the same flags)"""
    blk = np.random.default_rng(77).integers(-300, 301, size=2 << 20, dtype=np.int16)
    return np.tile(blk, (2 * n + blk.size - 1) // blk.size)[:2 * n]


def test_refusals_among_idle_words(vh, referee=0):
    """256 channels x 7 232 words (wpl = 4), flagged and idle stretches alternating within every workgroup: stretches of 23 words of
    denormal input (flagged once the channel filter has run down: 2-4 words) and 11 of noise, so that a workgroup's 1 024 words hold
    more busy ones than the list's 512 and a couple of hundred idle ones - the list is worked off in the middle of a round, the
    wavefronts stop at different passes, some are through.  Without the referee: on samples this small every candidate is within
    its margin, and the checks behind the walk then take 15 s - the list step is the same code with it and without, and refusals
    with the referee on are test_many_passes[7232-1]"""
    from dumpvdl2_amd import workloads
    cfg = workloads.config4(1.0)
    words, word = 7_232, 64 * cfg.oversample
    n = (64 * words - 20) * cfg.oversample + 5
    rng = np.random.default_rng(78)
    iq = (rng.standard_normal(2 * n, dtype=np.float32) * np.float32(0.01)).view(np.complex64)
    # (bit patterns 1..900 with either sign: +-k x 1.4e-45)
    tiny = (rng.integers(1, 901, size=2 * n).astype(np.uint32) | (rng.integers(0, 2, size=2 * n).astype(np.uint32) << 31)).view(np.float32).view(np.complex64)
    quiet = (np.arange(n) // word) % 34 < 23
    iq = np.where(quiet, tiny, iq)
    new = both(vh, cfg, cfg.freqs, iq, [(0, 0)], f"noise / denormals referee={referee}", frames=False, look=(0, 127, 255), scans_ahead=False, referee=referee, cf32=True)
    for fl in new[3]:
        busy = fl[:fl.size // 64 * 64].reshape(-1, 64).any(axis=1)
        per_group = [int(busy[k:k + 1024].sum()) for k in range(0, busy.size - 1023, 1024)]
        assert max(per_group) > 512 + 64 and min(per_group) < 1024 - 128, f"busy words per workgroup of 1 024: {per_group}"


def test_every_sample_flagged_without_the_referee(vh):
    """wpl = 4 with every word busy (refused reservations throughout), the plain verdicts"""
    from dumpvdl2_amd import workloads
    cfg = workloads.config4(1.0)
    iq = noise((64 * 7_232 - 20) * cfg.oversample + 5)
    both(vh, cfg, cfg.freqs, iq, [(0, 1)], "256 channels x 7232 words dense, referee off", frames=False, look=(0, 127, 255), scans_ahead=False, referee=0)


@pytest.mark.parametrize("words,dense", [(7_232, 1), (7_232, 0), (14_400, 0), (57_408, 0)])
def test_many_passes(vh, words, dense):
    """256 channels: wpl = 4 (every sample flagged: the list is worked off many times within a workgroup, reservations are refused;
    and idle), 8 and kK3dRounds = 32 (see the module's docstring); three channels are read back"""
    from dumpvdl2_amd import workloads
    cfg = workloads.config4(1.0)
    iq = noise((64 * words - 20) * cfg.oversample + 5)
    if dense:
        feeds = [(0, 1)]
    else:                                                       # (a short flagged feed behind the long one: words busy at the start of the ring's next stretch)
        feeds = [(dec(cfg, 64 * words - 200, 0), 0), (0, 1)]
    both(vh, cfg, cfg.freqs, iq, feeds, f"256 channels x {words} words dense={dense}", frames=False, look=(0, 127, 255), scans_ahead=False)
