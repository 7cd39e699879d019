"""The second look on the GPU, beyond the one scenario of tests/test_gpu_relook.py: the rounds, strides and staged copies that only a
crowded feed reaches, several frames from one attempt, the ring's end, a stream hours old, the settings and outcomes that only the host
build had seen, and feeds far smaller than a transmission.

Every run is held to the model (tests/relook_model.py) on the device's OWN decimated stream, the referee off, as check_model() of
tests/test_gpu_relook.py holds it: every integer field and octet exact, floats by their bits, frame_pwr_dbfs within util.TOL_DB.  No
tolerance is added here.  Every test asserts on its run that the path it is named for ran.

Measured, on the CPU design of each capture (the oracle's decimated trace through activity_model, txlog_model and relook_model) and
alike on an MI355X:
  crowded feed    410 log records closed by the one feed, 410 attempts (one a record), 154 of them on records of index 256 and above;
                  the reference delivers 391 of the 410 bursts (those are SEEN), the other 19 come out NEW; mail boundary 32 and 33
  ring            2^17 = 131 072 decimated samples (6 feeds of 10 001 in flight + 65 536 of history + 1 024, rounded up to a power of
                  two); anchors at 2^17 + 70, 2^17 - 45 and 2^18 - 400, each attempt 1 930 samples long
  position        anchors at 2^32 - 11 508 (A, which ends at 2^32 + 8 152) and 2^32 - 9 508 (C) ahead of decimated sample 2^32,
                  2^32 + 1 492 (B) and 2^32 + 1 489 (what B leaks into channel 1) behind it
  threshold 30    94 anchors found, 44 attempts kept; A's record: 66 found, 16 kept; max_ppm 3: 29 of the 44 attempts rejected
  tiny feeds      B's attempt comes with feed 236; its record began in feed 38, 198 feeds back

Wall time of the module on an MI355X: 5 s for its 11 cells (the captures made and the models run on the CPU included)."""
import functools

import numpy as np
import pytest

import relook_model as rm
import txsearch_model as tm
from dumpvdl2_amd import synth
from test_gpu_relook import ACT, CF, FREQS, N, OS, _place, check_model, cut_sizes, run, scenario, single, stable, vh  # noqa: F401 (vh, single: fixtures)
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
B = ACT[0]
UNEVEN = [100003, 103333, 111664]       # (no multiple of an oversampling)


def place(acc, fs, df, start, wave, amp):
    idx = np.arange(start, start + wave.size, dtype=np.float64)
    acc[start:start + wave.size] += (amp * wave * np.exp(1j * (2.0 * np.pi * df / fs) * idx)).astype(np.complex64)


def to_raw(acc, seed):
    rng = np.random.default_rng(seed)
    iq = np.stack([acc.real, acc.imag], axis=1) + rng.standard_normal((acc.size, 2), dtype=np.float32) * np.float32(0.0004)
    assert np.abs(iq).max() < 0.9, "the int16 sum does not clip"
    return np.rint(iq * 32768.0).astype(np.int16)


def tx_index(res):
    """the index in the run's log of the record every attempt belongs to"""
    where = {(int(t["chan"]), int(t["first_bin"])): i for i, t in enumerate(res["tx"])}
    return np.array([where[(int(g["chan"]), int(g["first_bin"]))] for g in res["recs"]], dtype=np.int64)


def frames_of(res, g):
    return res["rlf"][int(g["frame_first"]):int(g["frame_first"]) + int(g["frames"])]


def check_join(res):
    """New or seen (vdl2hip.h, "Second look"), from the run's own main path: a good frame of an attempt is new unless the main path
    delivered the same octets within the window of the attempt's log record -> (attempts with a good frame and nothing new, frames new)"""
    seen = new_frames = 0
    for g, i in zip(res["recs"], tx_index(res)):
        t = res["tx"][i]
        lo, hi = int(t["first_sample"]), res["K"] + (int(t["last_bin"]) + ACT[2] + 2) * B
        main = {f["octets"] for f in res["frames"] if f["chan"] == int(g["chan"]) and lo <= f["sync_sample"] < hi}
        new = [k for k, f in enumerate(frames_of(res, g)) if f["avlc_status"] == 0 and f["octets"] not in main]
        assert int(g["frames_new"]) == len(new) and int(g["new_mask"]) == sum(1 << k for k in new), (int(g["chan"]), int(g["anchor"]))
        seen += int(g["frames_ok"]) >= 1 and not new
        new_frames += len(new)
    assert res["info"]["frames_new"] == new_frames
    return seen, new_frames


def same_records(a, b, label, at_least, only=None):
    """two runs of one capture as test_cuts compares them: records alike, integer fields and octets byte-identical, the floats too
    wherever the two runs' streams are identical over the samples the attempt read (at_least: how many must be); only(chan, anchor
    from the run's first sample on): the attempts whose fields are compared (None: all) -> how many were compared"""
    sa, sb = stable(a), stable(b)
    assert len(sa) == len(sb), (label, len(sa), len(sb))
    key = lambda r: [(int(g["chan"]), int(g["first_bin"])) for g in np.sort(r["recs"], order=["chan", "first_bin", "anchor"])]  # noqa: E731
    assert key(a) == key(b), (label, "the same attempts of the same log records")
    exact = compared = 0
    for (ia, fa, (c, lo, hi)), (ib, fb, _) in zip(sa, sb):
        if only is not None and not only(c, lo + 150):
            continue
        compared += 1
        assert ia == ib, (label, "integer fields and octets are byte-identical")
        if np.array_equal(a["y"][c][lo:hi].view(np.uint64), b["y"][c][lo:hi].view(np.uint64)):
            assert fa == fb, (label, "over identical samples the records are identical byte for byte")
            exact += 1
    print(f"{label}: {len(sa)} records, {compared} compared, {exact} over identical samples and identical byte for byte")
    assert exact >= at_least, (label, exact)
    return compared


# ---------------------------------------------------------------- 1. a crowded feed
CROWD_OS = 20
CROWD_FREQS = [CF + 50000 * (i - 20) for i in range(41)]         # what 2.1 MHz hold at the 50 kHz of the log's and the monitor's tests
CROWD_BURSTS, CROWD_PERIOD, CROWD_BINS = 10, 13, 148              # ten bursts of 9 bins a channel, one every 13 bins; bins of the capture


def mail_keep(n):
    """32 bursts that are all over before the 33rd begins, which lies on the highest channel in use: the last record of the feed"""
    return frozenset([(c, j) for c in range(8) for j in range(4)] + ([(7, 9)] if n == 33 else []))


@functools.lru_cache(maxsize=3)
def crowd(keep=None):
    """-> (raw, freqs, {(chan, j): AVLC frame}); keep: the bursts that are keyed (None: all) - every burst and the noise are the same
    whatever else is keyed"""
    fs, n = 105000 * CROWD_OS, CROWD_BINS * B * CROWD_OS
    acc = np.zeros(n, dtype=np.complex64)
    fr = {}
    for c, f in enumerate(CROWD_FREQS):
        for j in range(CROWD_BURSTS):
            if keep is not None and (c, j) not in keep:
                continue
            rng = np.random.default_rng([20261023, c, j])
            fr[(c, j)] = synth.make_avlc_frame(rng.integers(0, 256, size=16, dtype=np.uint8).tobytes())
            wave = synth.modulate(synth.build_burst([fr[(c, j)]]).symbols, 10 * CROWD_OS, start_phase=float(rng.uniform(0, 6.28)))
            start = (2 * B + (j * CROWD_PERIOD + (5 * c) % CROWD_PERIOD) * B + (29 * c) % B) * CROWD_OS      # staggered from channel to channel
            place(acc, fs, f - CF, start, wave, 0.012)
    return to_raw(acc, 20261024), CROWD_FREQS, fr


@pytest.fixture(scope="module")
def crowd_single(vh):
    raw, freqs, _ = crowd()
    return run(vh, [raw.shape[0]], relook={}, capture=(raw, freqs, CROWD_OS), per_feed=True)


def test_crowded_feed(vh, crowd_single, oracle_mod):
    """41 channels, ten short bursts each, ONE feed: k_relook_select and k_relook_pack_plan go round more than once and carry their
    sums over, k_relook_decode's wavefronts and k_relook_pack_copy's take a second attempt, and the records come through the staging
    buffer ahead of the frames and the octets"""
    raw, freqs, fr = crowd()
    res = crowd_single
    print(f"crowded feed: {res['feeds_tx']} log records and {res['feeds_recs']} attempts per read")
    # the conditions
    assert res["feeds_tx"][0] >= 257 and res["feeds_recs"][0] >= 257, "one feed closes more records, and has more attempts, than a round holds"
    ti = tx_index(res)
    assert np.count_nonzero(ti[:res["feeds_recs"][0]] >= 256) >= 1, "a record of a later round has an attempt"
    assert res["loginfo"]["dropped"] == 0 and res["info"]["dropped"] == 0
    # the model, every attempt and frame; the totals
    want = check_model(res, "crowded", feeds_tx=res["feeds_tx"])
    info = res["info"]
    assert (info["frames"], info["frames_ok"]) == (sum(r["frames"] for _, r, _ in want), sum(r["frames_ok"] for _, r, _ in want))
    late = [(g, w) for i, (g, (_, _, w)) in enumerate(zip(res["recs"], want)) if i >= 256 and len(w)]
    assert len(late) >= 1
    for g, w in late:
        assert [f["octets"] for f in frames_of(res, g)] == [f["octets"] for f in w] and all(f["avlc_status"] == 0 for f in frames_of(res, g))
    # the main path is the reference's, and delivered every burst: every attempt on one is SEEN
    o = oracle_mod.Oracle(CF, freqs, oversample=CROWD_OS)
    o.process(raw)
    ref = o.frames()
    assert_frames_equal(ref, res["frames"], label="main path")
    for c in range(len(freqs)):
        assert res["counters"][c][0] == list(o.counters(c).values())
    main = [f for f in ref if oracle_mod.avlc_screen(f["octets"])[0] == 0]
    seen, new = check_join(res)
    print(f"crowded feed: the reference delivers {len(main)} of {len(fr)} bursts; {seen} attempts SEEN, {new} frames NEW")
    assert seen >= 257 and len(main) >= 257 and seen == len(main) and new == len(fr) - len(main)
    assert sorted(f["octets"] for g in res["recs"] for f in frames_of(res, g)) == sorted(fr.values()), "the second look delivers every burst"


def test_crowded_feed_cut(vh, crowd_single):
    raw, freqs, _ = crowd()
    res = run(vh, cut_sizes(raw.shape[0], UNEVEN), relook={}, capture=(raw, freqs, CROWD_OS), per_feed=True)
    check_model(res, "crowded, three uneven feeds", feeds_tx=res["feeds_tx"])
    same_records(crowd_single, res, "crowded, one feed against three", 1)


@functools.lru_cache(maxsize=2)
def mail_run(vh, n):
    raw, freqs, _ = crowd(mail_keep(n))
    return run(vh, [raw.shape[0]], relook={}, capture=(raw, freqs, CROWD_OS), per_feed=True)


@pytest.mark.parametrize("natt", [32, 33])
def test_mail_boundary(vh, natt):
    """as many attempts in one feed as come to the host with the header, and one more: then the records are staged ahead of the frames
    and the octets (relook_fetch).  The 33rd burst begins when the 32 are over and its record is the feed's last: up to it the two
    captures are the same samples"""
    res = mail_run(vh, natt)
    assert res["feeds_recs"][0] == natt == res["feeds_tx"][0] == len(res["recs"]) and res["info"]["dropped"] == 0
    want = check_model(res, f"mail {natt}", feeds_tx=res["feeds_tx"])
    assert sum(r["frames_ok"] for _, r, _ in want) == natt == res["info"]["frames_ok"]
    a, b = mail_run(vh, 32), mail_run(vh, 33)
    sa, sb = stable(a), stable(b)
    assert len(sa) == 32 and len(sb) == 33 and int(b["recs"][32]["chan"]) == 7
    for (ia, fa, (c, lo, hi)), (ib, fb, _) in zip(sa, sb[:32]):
        assert np.array_equal(a["y"][c][lo:hi].view(np.uint64), b["y"][c][lo:hi].view(np.uint64)), "the captures agree up to the 33rd burst"
        assert ia == ib and fa == fb


# ---------------------------------------------------------------- 2. several frames from one attempt
UW_END = 242                             # a burst placed at input sample 10 s has its anchor - the last symbol of its unique word - at s + 242
INNER_AT, CLEAR_AT = 120000, 245000


@functools.lru_cache(maxsize=1)
def covered3():
    """scenario()'s construction with a burst of three AVLC frames inside A, and the same burst in the clear on channel 1 - behind A,
    whose leakage the reference may be locked on in channel 1 as long as A lasts"""
    rng = np.random.default_rng(20261025)
    a = synth.make_avlc_frame(rng.integers(0, 256, size=700, dtype=np.uint8).tobytes())
    three = [synth.make_avlc_frame(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()) for n in (30, 17, 41)]
    wa = synth.modulate(synth.build_burst([a]).symbols, 10 * OS, start_phase=1.0)
    w3 = synth.modulate(synth.build_burst(three).symbols, 10 * OS, start_phase=2.0)
    acc = np.zeros(N, dtype=np.complex64)
    _place(acc, 0, 40000, wa, 0.008)
    _place(acc, 0, INNER_AT, w3, 0.09)
    _place(acc, 1, CLEAR_AT, w3, 0.05)
    assert 40000 + wa.size > INNER_AT + w3.size and 40000 + wa.size + 4 * B * OS < CLEAR_AT and CLEAR_AT + w3.size + 8 * B * OS < N
    return to_raw(acc, 20261026), three


def test_three_frames(vh, oracle_mod):
    raw, three = covered3()
    o = oracle_mod.Oracle(CF, FREQS, oversample=OS)
    o.process(raw)
    ref = o.frames()
    inner, clear = INNER_AT // OS + UW_END, CLEAR_AT // OS + UW_END
    # the conditions: the reference delivers the three frames of the burst in the clear, and nothing of the covered one
    assert [f["octets"] for f in ref if f["chan"] == 1 and abs(f["sync_sample"] - clear) <= 6] == three
    assert not any(f["chan"] == 0 and f["sync_sample"] < clear - 500 and oracle_mod.avlc_screen(f["octets"])[0] == 0 for f in ref)
    res = run(vh, [N], relook={}, capture=(raw, FREQS, OS))
    check_model(res, "three frames")
    check_join(res)
    assert_frames_equal(ref, res["frames"], label="main path")
    hit = {c: [g for g in res["recs"] if int(g["chan"]) == c and abs(int(g["anchor"]) - at) <= 3] for c, at in ((0, inner), (1, clear))}
    assert len(hit[0]) == 1 and len(hit[1]) == 1
    g = hit[0][0]
    assert int(g["frames"]) == 3 and int(g["frames_ok"]) == 3 and int(g["frames_new"]) == 3 and int(g["new_mask"]) == 0b111
    fr = frames_of(res, g)
    assert [f["octets"] for f in fr] == three and [f["idx"] for f in fr] == [0, 1, 2] and all(f["avlc_status"] == 0 and f["sync_sample"] == int(g["anchor"]) for f in fr)
    g = hit[1][0]
    assert int(g["frames"]) == 3 and int(g["frames_ok"]) == 3 and int(g["frames_new"]) == 0 and int(g["new_mask"]) == 0, "the main path delivered all three: SEEN"
    assert [f["octets"] for f in frames_of(res, g)] == three
    assert res["info"]["frames_new"] >= 3


# ---------------------------------------------------------------- 3. the ring wraps
RING = 1 << 17
RING_BLOCK = 100000                      # input samples a feed: 10 000 decimated
RING_FREQS = synth.channel_plan(3, CF, spacing=100000)


@functools.lru_cache(maxsize=1)
def ring_capture():
    """three bursts, each across a multiple of the ring's length: the unique word of the first (anchor 70 behind it), the nine header
    symbols of the second (anchor 45 ahead of it), the payload of the third (anchor 400 ahead of the next multiple)
    -> (raw, [(chan, multiple, anchor as placed, frame)])"""
    n = (2 * RING + 6000) * OS
    acc = np.zeros(n, dtype=np.complex64)
    out = []
    for c, (m, anchor) in enumerate([(RING, RING + 70), (RING, RING - 45), (2 * RING, 2 * RING - 400)]):
        rng = np.random.default_rng([20261027, c])
        f = synth.make_avlc_frame(rng.integers(0, 256, size=60, dtype=np.uint8).tobytes())
        wave = synth.modulate(synth.build_burst([f]).symbols, 10 * OS, start_phase=float(rng.uniform(0, 6.28)))
        place(acc, 105000 * OS, RING_FREQS[c] - CF, (anchor - UW_END) * OS, wave, 0.05)
        out.append((c, m, anchor, f))
    return to_raw(acc, 20261028), out


def test_ring_wraps(vh):
    """Feeds of 100 000 samples make the decimated ring 2^17 samples long, as in tests/test_gpu_txsearch.py::test_ring_wraps: six feeds
    of 10 001 in flight, 65 536 of history and 1 024, rounded up to a power of two.  The stream is 2 * 2^17 + 6 000 samples: the ring
    wraps twice, and a piece's phases, an anchor's header read and an attempt's decode_burst each read across its end"""
    raw, bursts = ring_capture()
    sizes = cut_sizes(raw.shape[0], [RING_BLOCK])
    assert 6 * (RING_BLOCK // OS + 1) + 65536 + 1024 <= RING < 2 * (6 * (RING_BLOCK // OS + 1) + 65536 + 1024) and raw.shape[0] // OS > 2 * RING
    res = run(vh, sizes, relook={}, capture=(raw, RING_FREQS, OS), per_feed=True)
    check_model(res, "ring", feeds_tx=res["feeds_tx"])
    for (c, m, placed, f), (lo, hi) in zip(bursts, [(-150, 0), (0, 90), (90, None)]):
        # the part that lies across the multiple: the unique word's samples, the header's, the payload's
        got = [g for g in res["recs"] if int(g["chan"]) == c and abs(int(g["anchor"]) - placed) <= 3]
        assert len(got) == 1, (c, [int(g["anchor"]) for g in res["recs"] if int(g["chan"]) == c])
        g = got[0]
        a, e = int(g["anchor"]), int(g["end_sample"])
        assert a - 150 < m <= e and a + lo < m <= (a + hi if hi is not None else e), (c, a, e, m)
        fr = frames_of(res, g)
        assert int(g["frames_ok"]) == 1 and fr[0]["octets"] == f and fr[0]["avlc_status"] == 0


# ---------------------------------------------------------------- 4. hours into a stream
def test_position(vh):
    """scenario()'s capture, B moved behind the boundary, on a receiver whose stream begins at n = os 2^32 - L/2: decimated sample 2^32
    lies inside the capture, C and B on either side of it and A across it.

    Against the run at position 0 the attempts exist alike, and those on A, B and C have every integer field and octet identical, the
    samples shifted by K.  The fourth attempt is not compared across the positions: it lies on what B leaks into channel 1, 25 kHz
    off the channel's frequency - 137 degrees a symbol, which the metric's phase unwrapping resolves by the absolute phase, and the NCO
    phase a stream begins with depends on its position.  The yardstick says so itself: the oracle's trace through the models puts that
    anchor at K + 17 239 with set_position(n) and at 17 240 from 0 (p 0.2607 and 0.2389 there, above 40 beside them).  Each run's
    attempt is held to the model on its own stream like every other"""
    b_at = 170000
    raw, fr = scenario(b_at=b_at)
    n = (OS * 2**32 - N // 2) // OS * OS
    K = n // OS
    sizes = cut_sizes(N, UNEVEN)
    assert K < 2**32 < K + N // OS and all(s % OS for s in sizes)
    res = run(vh, sizes, relook={}, capture=(raw, FREQS, OS), base=n, per_feed=True)
    assert res["K"] == K
    # the conditions
    recs = res["recs"]
    assert any(int(g["end_sample"]) < 2**32 for g in recs) and any(int(g["anchor"]) > 2**32 for g in recs)
    assert any(int(g["anchor"]) < 2**32 <= int(g["end_sample"]) for g in recs)
    # the model on the stream read back from K on; before K lies rest
    check_model(res, "position", feeds_tx=res["feeds_tx"])
    for g in recs:
        assert K <= int(g["anchor"]) <= int(g["end_sample"]) < K + N // OS
        assert all(f["sync_sample"] == int(g["anchor"]) and f["end_sample"] == int(g["end_sample"]) for f in frames_of(res, g))
    new = [g for g in recs if int(g["frames_new"]) == 1 and frames_of(res, g)[0]["octets"] == fr["B"]]
    assert len(new) == 1 and int(new[0]["anchor"]) > 2**32 and int(new[0]["chan"]) == 0 and int(new[0]["new_mask"]) == 1, "B is delivered NEW, behind 2^32"
    # the run at position 0: the same integer fields, the samples shifted by K
    zero = run(vh, sizes, relook={}, capture=(raw, FREQS, OS), per_feed=True)
    check_model(zero, "position 0", feeds_tx=zero["feeds_tx"])
    check_join(res); check_join(zero)                            # (the log's join of the main path's frames by their absolute sync_sample)
    placed = [(0, 40000 // OS + UW_END), (0, b_at // OS + UW_END), (1, 60000 // OS + UW_END)]        # A, B, C
    assert same_records(zero, res, "position 0 against os 2^32 - L/2", 0, only=lambda c, a: any(c == pc and abs(a - pa) <= 3 for pc, pa in placed)) == 3
    print("position: anchors", sorted(int(g["anchor"]) - 2**32 for g in recs), "relative to 2^32")


# ---------------------------------------------------------------- 5. settings and outcomes on the device
CUT_AT = 150000


@pytest.fixture(scope="module")
def cut_capture():
    return scenario(cut_at=CUT_AT)[0], FREQS, OS


def test_wide_threshold(vh, cut_capture):
    """threshold 30 and 16 anchors a record: pieces with several anchors go through k_relook_anchors' list and its sort, and rl_keep
    discards"""
    cfg = dict(threshold=30.0, max_anchors=16)
    res = run(vh, [N], relook=cfg, capture=cut_capture)
    want = check_model(res, "threshold 30", **cfg)
    found = kept = 0
    crowded_piece = False
    for t in res["tx"]:
        mine = [r for tt, r, _ in want if (int(tt["chan"]), int(tt["first_bin"])) == (int(t["chan"]), int(t["first_bin"]))]
        if mine and mine[0]["found"] > len(mine):
            found, kept = mine[0]["found"], len(mine)
        sf, _ = tm.search_range(int(t["first_sample"]), int(t["last_sample"]))
        pieces = [(r["anchor"] - sf) // 1024 for r in mine]              # (the search's plan: pieces of 1 024 samples from search_first on)
        crowded_piece |= len(pieces) != len(set(pieces))
    print(f"threshold 30: {found} anchors found in a record, {kept} kept; info {res['info']}")
    assert found > kept == 16, "a record has more anchors than are kept"
    assert crowded_piece, "a piece of 1 024 samples holds two anchors or more"
    assert res["info"]["anchors_found"] > res["info"]["attempts"]


MAX_PPM = 3.0


def test_max_ppm(vh, cut_capture):
    cfg = dict(threshold=30.0, max_anchors=16, max_ppm=MAX_PPM)
    res = run(vh, [N], relook=cfg, capture=cut_capture)
    want = check_model(res, "max_ppm", **cfg)
    rej = [bool(r["flags"] & rm.PPM_REJECT) for _, r, _ in want]
    print(f"max_ppm {MAX_PPM}: {sum(rej)} of {len(rej)} attempts rejected")
    assert any(rej) and not all(rej)
    got = [bool(int(g["flags"]) & rm.PPM_REJECT) for g in res["recs"]]
    assert got == rej
    assert all(int(g["tl_bits"]) == 0 and int(g["frames"]) == 0 and int(g["stop"]) == -1 and not np.any(g["counters"]) for g, x in zip(res["recs"], got) if x)


def test_truncated(vh, cut_capture):
    """a transmitter that stops in mid-burst: the header promises more symbols than the transmission has"""
    res = run(vh, [N], relook={}, capture=cut_capture)
    want = check_model(res, "truncated")
    placed = CUT_AT // OS + UW_END
    mine = [(g, r) for g, (_, r, _) in zip(res["recs"], want) if int(g["chan"]) == 1 and abs(int(g["anchor"]) - placed) <= 3]
    assert len(mine) == 1
    g, r = mine[0]
    assert r["flags"] & rm.TRUNCATED and r["tl_bits"] > 0 and r["frames"] == 0 and r["stop"] == -1, "as the model has it"
    assert int(g["flags"]) & rm.TRUNCATED and int(g["tl_bits"]) > 0 and int(g["frames"]) == 0 and int(g["stop"]) == -1 and not np.any(g["counters"])


# ---------------------------------------------------------------- 6. feeds far smaller than a transmission
def test_tiny_feeds(vh, single):
    """feeds of 4 096 bytes: the attempt that delivers B reads samples written some 100 feeds before the feed that closes A's record, and
    the record began more than 100 feeds before it"""
    _, fr = scenario()
    sizes = cut_sizes(N, [1024])
    res = run(vh, sizes, relook={}, per_feed=True)
    hit = [i for i, g in enumerate(res["recs"]) if int(g["frames_new"]) == 1 and frames_of(res, g)[0]["octets"] == fr["B"]]
    assert len(hit) == 1
    read = int(np.searchsorted(np.cumsum(res["feeds_recs"]), hit[0], side="right"))      # the read, so the feed, that brought the attempt
    t = res["tx"][tx_index(res)[hit[0]]]
    back = read - int(t["first_sample"]) * OS // 1024
    print(f"tiny feeds: B's attempt came with feed {read}, its record began in feed {int(t['first_sample']) * OS // 1024}: {back} feeds back")
    assert read < len(sizes) and back > 100
    check_model(res, "tiny feeds", feeds_tx=res["feeds_tx"])
    check_join(res)
    # (the integer fields: behind the first cut, at sample 102, the two runs' streams differ in their last bits - test_cuts)
    assert same_records(single, res, "one feed against feeds of 4 096 bytes", 0) == len(res["recs"]) >= 4
