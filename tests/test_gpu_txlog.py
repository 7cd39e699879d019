"""The transmission log on the GPU (include/vdl2hip.h, "Transmission log"; kernels: dumpvdl2_amd/csrc/txlog.h): one record per
transmission the activity monitor sees on a channel, joined on the host with the frames it yielded.

Records are held to the sequential model (tests/txlog_model.py) run on the device's OWN float32 series, read back with
activity_series(): busy flags are then exact and no margin to the threshold is needed.  Integer fields and peak_power are exact,
mean_power is within 2^-23 relative.  Streams are keyed carriers as in test_gpu_activity.py (noise at about -60 dBFS, a tone per
channel of about -20 dBFS keyed on and off in the middle of 105-sample bins, threshold -40 dBFS), oversample 10, s16 input, about
0.5 s, the referee off unless stated."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import activity_model as am
import txlog_model as tm
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAV = os.path.join(ROOT, "tests", "golden", "vdl2_model_16b_1050kHz.wav")
E_INVAL = -1
THR = -40.0
N = 525013                                                      # 52 501 decimated samples: 500 bins of 105
KEYS = ("first_bin", "last_bin", "busy_bins", "flags")          # what must not depend on how the stream was cut


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


# ---------------------------------------------------------------- streams (the builders of test_gpu_activity.py)
def plan(nchan, step=50000):
    return [CF + step * (i - nchan // 2) for i in range(nchan)]


def keying(nbins, seed, first=3):
    """[(first busy bin, last busy bin)] of 105-sample bins: lengths 2 .. 40 and one of 70, gaps of 1, 2 and 4 idle bins among others"""
    rng = np.random.default_rng(seed)
    gaps = [1, 2, 4, 1, 2, 4, 7, 20, 3]
    out, m, i = [], first, 0
    while True:
        length = 70 if i == 2 else int(rng.integers(2, 41))
        if m + length + 2 >= nbins:
            break
        out.append((m, m + length - 1))
        m += length + gaps[i % len(gaps)]
        i += 1
    return out


def build_stream(freqs, n_in, seed, keys):
    """-> int16 (n_in, 2): noise and, per channel, a tone on from the middle of bin s to the middle of bin e of every (s, e) of its keying"""
    rng = np.random.default_rng(seed)
    t = np.arange(n_in, dtype=np.float64)
    x = np.sqrt(0.5e-6) * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    per_bin = 1050
    for c, f in enumerate(freqs):
        gate = np.zeros(n_in)
        for s, e in keys[c]:
            gate[s * per_bin + per_bin // 2:e * per_bin + per_bin // 2] = 1.0
        x += 0.1 * (1.0 + 0.02 * c) * gate * np.exp(2j * np.pi * ((f - CF) / 1050000) * t + 1j * c)
    iq = np.stack([x.real, x.imag], axis=1)
    return np.clip(np.rint(32768.0 * iq), -32768, 32767).astype("<i2")


@functools.lru_cache(maxsize=8)
def make_stream(nchan, n_in, seed, step=50000):
    freqs = plan(nchan, step)
    keys = [keying(n_in // 1050, seed * 100 + c, first=3 + 2 * c) for c in range(nchan)]
    return build_stream(freqs, n_in, seed, keys), freqs, keys


def cut_sizes(n, sizes):
    out, k, i = [], 0, 0
    while k < n:
        d = min(sizes[i % len(sizes)], n - k)
        out.append(d)
        k += d
        i += 1
    return out


def receiver(vh, freqs, referee=0, **kw):
    rx = vh.Receiver(CF, freqs, 10, vh.FMT_S16LE, **kw)
    rx.debug_option("referee", referee)
    return rx


def feed_log(rx, raw, sizes, B, series=None, fed=0, read=True):
    """feed raw in pieces; after every feed collect it, take the log's records and the bins it completed (the series ring may be
    short) -> (records per feed, bins complete after every feed, samples fed)"""
    per_feed, bins_after = [], []
    C_ = range(rx.chan_first, rx.chan_first + rx.chan_count)
    k = 0
    for d in sizes:
        rx.feed(raw[k:k + d])
        k += d
        rx.sync()
        if read:
            per_feed.append(rx.txlog_read())
        nb = ((fed + k) // 10 - series["k_on"]) // B if series is not None else 0
        if series is not None and nb > series["bins"]:
            for c in C_:
                series[c].append(rx.activity_series(c, series["bins"], nb - series["bins"]))
            series["bins"] = nb
        bins_after.append(nb)
    return per_feed, bins_after, fed + k


def new_series(rx, k_on=0):
    s = {c: [] for c in range(rx.chan_first, rx.chan_first + rx.chan_count)}
    s.update(bins=0, k_on=k_on)
    return s


def series_of(series, c):
    return np.concatenate(series[c]) if series[c] else np.zeros(0, np.float32)


def run(vh, raw, freqs, sizes, B=105, H=0, series_bins=0, pool=0, **kw):
    rx = receiver(vh, freqs, **kw)
    rx.activity_enable(B, THR, H, series_bins)
    rx.txlog_enable(pool_records=pool)
    series = new_series(rx)
    per_feed, bins_after, _ = feed_log(rx, raw, sizes, B, series)
    out = dict(per_feed=per_feed, bins_after=bins_after, recs=np.concatenate(per_feed), act=rx.activity(), info=rx.txlog_info(),
               series={c: series_of(series, c) for c in range(rx.chan_first, rx.chan_first + rx.chan_count)}, freqs=freqs,
               chan_first=rx.chan_first)
    rx.close()
    return out


def check_feeds(res, H):
    """order within a feed, and every record in the feed that completed its closing bin"""
    lo = 0
    for batch, hi in zip(res["per_feed"], res["bins_after"]):
        key = list(zip(batch["chan"].tolist(), batch["first_bin"].tolist()))
        assert key == sorted(key)
        close = batch["last_bin"].astype(np.int64) + H + 1
        assert np.all((close >= lo) & (close < hi)), (lo, hi, close)
        lo = hi


def check_model(res, B, H, label=""):
    """every channel's records against the model on the device's own series; the monitor's accumulators beside them -> records"""
    worst, total = 0.0, 0
    thr = am.threshold(THR)
    for c, p in res["series"].items():
        mine = res["recs"][res["recs"]["chan"] == c]
        assert np.all(mine["freq"] == res["freqs"][c])
        st = tm.new_state()
        want = tm.log(p, thr, H, st, B)
        worst = max(worst, tm.assert_records(mine, want, (label, c)))
        j = c - res["chan_first"]
        assert len(mine) + int(res["act"]["open"][j]) == int(res["act"]["transmissions"][j]) and int(st["open"]) == int(res["act"]["open"][j])
        assert int(mine["busy_bins"].sum()) <= int(res["act"]["busy_bins"][j])
        total += len(mine)
    assert total == len(res["recs"]) == res["info"]["transmissions"] and res["info"]["dropped"] == 0
    check_feeds(res, H)
    print(f"{label}: {total} records, worst |mean - model| / model = {worst:.3g}")
    return total


# ---------------------------------------------------------------- 1. records against the model
@pytest.mark.parametrize("nchan,H,B", [(1, 0, 105), (1, 1, 10), (1, 3, 1000), (9, 0, 10), (9, 1, 1000), (9, 3, 105), (17, 0, 1000), (17, 1, 105), (17, 3, 10)])
def test_records_against_model(vh, nchan, H, B):
    raw, freqs, keys = make_stream(nchan, N, 33)
    # 304, 66 and 142 bins of 105 in a feed: more than 64, more than 128, several words
    res = run(vh, raw, freqs, cut_sizes(N, [320000, 70000, 150000]), B, H, max_block_bytes=4 * 320000)
    assert res["act"]["bins"] == (N // 10) // B
    total = check_model(res, B, H, f"nchan={nchan} H={H} B={B}")
    if B == 105 and H == 0:
        for c in range(nchan):                                   # every keyed stretch but a last one still open is one record
            mine = res["recs"][res["recs"]["chan"] == c]
            assert len(mine) >= len(keys[c]) - 1 and np.all(mine["flags"] == 0)
    assert B == 1000 or total >= nchan * 5                       # (bins of 9.5 ms merge most of the keying)


# ---------------------------------------------------------------- 2. the cut does not matter
def test_cuts(vh):
    raw, freqs, keys = make_stream(3, N, 22, step=200000)
    B, H = 105, 2
    whole = run(vh, raw, freqs, [N], B, H, max_block_bytes=4 * N)
    again = run(vh, raw, freqs, [N], B, H, max_block_bytes=4 * N)
    # channel 0: a cut inside a transmission, inside a hang gap (2 idle bins, bridged), inside a closing bin and at its end
    gaps = [(a, b) for a, b in zip(keys[0], keys[0][1:]) if b[0] - a[1] - 1 == 2]
    closes = [(a, b) for a, b in zip(keys[0], keys[0][1:]) if b[0] - a[1] - 1 > H + 1]
    assert gaps and closes and gaps[0][0][1] < closes[-1][0][1]
    s, e = keys[0][1]
    hang_bin = gaps[0][0][1] + 2
    close_bin = closes[-1][0][1] + H + 1
    marks = sorted({10 * (B * (s + 1) + 40), 10 * (B * hang_bin + 50), 10 * (B * close_bin + 50), 10 * B * (close_bin + 1)})
    assert marks[0] > 400
    sizes = [1, 300, 7, marks[0] - 308]
    for a, b in zip(marks, marks[1:]):
        sizes += [1, b - a - 1]
    sizes += cut_sizes(N - sum(sizes), [50000, 333, 1, 20011])
    assert sum(sizes) == N and min(sizes) > 0
    ragged = run(vh, raw, freqs, sizes, B, H, max_block_bytes=4 * N)
    for name, res in (("whole", whole), ("ragged", ragged)):
        check_model(res, B, H, name)
    for c in range(3):
        w, r = whole["recs"][whole["recs"]["chan"] == c], ragged["recs"][ragged["recs"]["chan"] == c]
        assert len(w) == len(r) >= 5
        for k in KEYS + ("first_sample", "last_sample"):
            assert np.array_equal(w[k], r[k]), (c, k)
        assert np.all(np.abs(w["mean_power"].astype(np.float64) - r["mean_power"]) <= 2 * am.bound(B) * w["mean_power"])
    # the hang time did bridge the gap, and the record of the closing bin came with the feed that completed it
    rec0 = whole["recs"][whole["recs"]["chan"] == 0]
    assert any(r["first_bin"] <= gaps[0][0][0] and r["last_bin"] >= gaps[0][1][1] for r in rec0)
    assert any(r["last_bin"] + H + 1 == close_bin for r in rec0)
    # the same calls, the same bytes
    assert whole["recs"].tobytes() == again["recs"].tobytes()


# ---------------------------------------------------------------- 3. long hang times, long transmissions
@pytest.mark.parametrize("H", [64, 100])
def test_long_hang_and_long_transmissions(vh, H):
    freqs = plan(2, 200000)
    # channel 0: 150 and 200 busy bins, apart by more than the hang time; channel 1: short ones, gaps below and above it
    keys = [[(5, 154), (154 + H + 30, 154 + H + 30 + 199)], [(3, 10), (40, 45), (45 + H, 50 + H), (50 + 2 * H + 5, 60 + 2 * H + 5)]]
    n = 1050 * (max(k[-1][1] for k in keys) + H + 10) + 13
    raw = build_stream(freqs, n, 5, keys)
    res = run(vh, raw, freqs, cut_sizes(n, [200000, 70000, 1050 * 64]), 105, H, max_block_bytes=4 * 200000)
    check_model(res, 105, H, f"H={H}")
    r0, r1 = (res["recs"][res["recs"]["chan"] == c] for c in (0, 1))
    assert [int(v) for v in r0["busy_bins"]] == [150, 200] and len(r1) == 2
    assert int(r1[0]["first_bin"]) == 3 and int(r1[0]["last_bin"]) == 50 + H and int(r1[0]["busy_bins"]) == 8 + 6 + 6


# ---------------------------------------------------------------- 4. room
def test_room(vh):
    raw, freqs, _ = make_stream(9, N, 33)
    sizes = [N // 2, N - N // 2]
    full = run(vh, raw, freqs, sizes, max_block_bytes=4 * N)
    tight = run(vh, raw, freqs, sizes, pool=4, max_block_bytes=4 * N)
    assert tight["info"]["pool_records"] == 4 and full["info"]["pool_records"] == 65536
    dropped = 0
    for a, b in zip(full["per_feed"], tight["per_feed"]):
        assert len(a) > 4 and a[:4].tobytes() == b.tobytes()     # the survivors are the prefix in record order
        dropped += len(a) - 4
    assert tight["info"]["dropped"] == dropped and tight["info"]["transmissions"] == 8
    for k in ("transmissions", "busy_bins", "open"):
        assert np.array_equal(tight["act"][k], full["act"][k])


# ---------------------------------------------------------------- 4b. as many records as come with the header, and one more
MAIL_N = 1050 * tm.MAIL_BINS + 13


@functools.lru_cache(maxsize=2)
def mail_stream(nrec):
    """tm.mail_keys(nrec) keyed onto 11 channels: 32 or 33 transmissions that all close within the stream -> (raw, freqs)"""
    freqs = plan(tm.MAIL_CHANS)
    return build_stream(freqs, MAIL_N, 41, tm.mail_keys(nrec)), freqs


@functools.lru_cache(maxsize=2)
def mail_run(vh, nrec):
    """the stream as ONE feed, so that every record closes in that feed: 32 come with the header, 33 are fetched through the staging buffer"""
    raw, freqs = mail_stream(nrec)
    return run(vh, raw, freqs, [MAIL_N], 105, 0, max_block_bytes=4 * MAIL_N)


@pytest.mark.parametrize("nrec", [tm.MAIL_RECS, tm.MAIL_RECS + 1])
def test_mail_boundary(vh, nrec):
    res = mail_run(vh, nrec)
    print(f"nrec={nrec}: {len(res['per_feed'][0])} records in the feed, dropped {res['info']['dropped']}")
    assert len(res["per_feed"]) == 1 and len(res["per_feed"][0]) == nrec
    assert check_model(res, 105, 0, f"mail {nrec}") == nrec
    assert res["info"]["dropped"] == 0
    # the staged copy brings what the mail would have: channel by channel the two runs' records are the same bytes wherever the keying
    # is the same - every channel but the last, whose third transmission only one of the streams has, alone in its bins (the noise is
    # the same seed's in both)
    a, b = mail_run(vh, tm.MAIL_RECS)["recs"], mail_run(vh, tm.MAIL_RECS + 1)["recs"]
    assert b[:tm.MAIL_RECS].tobytes() == a.tobytes()             # (records are ordered by channel: the odd one is the last of all)
    for c in range(tm.MAIL_CHANS - 1):
        assert a[a["chan"] == c].tobytes() == b[b["chan"] == c].tobytes() and np.count_nonzero(a["chan"] == c) == 3, c
    assert np.count_nonzero(a["chan"] == tm.MAIL_CHANS - 1) == 2 and np.count_nonzero(b["chan"] == tm.MAIL_CHANS - 1) == 3


# ---------------------------------------------------------------- 5. partial records
def test_partial(vh):
    raw, freqs, keys = make_stream(2, N, 44, step=200000)
    B, H = 105, 1
    s, e = next(k for k in keys[0] if k[1] - k[0] >= 8 and k[0] > 60)
    n1 = 10 * (B * (s + 4) + 20)                                 # in the middle of a transmission of channel 0
    rx = receiver(vh, freqs, max_block_bytes=4 * N)
    rx.activity_enable(B, THR, H, 1024)
    series = new_series(rx)
    with pytest.raises(vh.Vdl2HipError):
        rx.txlog_read()                                          # off: nothing to read
    _, _, fed = feed_log(rx, raw[:n1], [n1], B, series, read=False)
    nb1 = series["bins"]
    rx.txlog_enable()
    per_feed, _, _ = feed_log(rx, raw[n1:], cut_sizes(N - n1, [100000]), B, series, fed=fed)
    recs = np.concatenate(per_feed)
    thr = am.threshold(THR)
    for c in range(2):
        p = series_of(series, c)
        st = tm.new_state()
        tm.log(p[:nb1], thr, H, st, B)                           # what the monitor's state is when the log takes effect
        st.update(busy=0, sum=0.0, peak=None, partial=st["open"])
        want = tm.log(p[nb1:], thr, H, st, B)
        mine = recs[recs["chan"] == c]
        tm.assert_records(mine, want, ("partial", c))
        if c == 0:
            assert mine[0]["flags"] == vh.TX_PARTIAL and mine[0]["first_bin"] == s < nb1 and mine[0]["busy_bins"] < mine[0]["last_bin"] - s + 1
        assert np.all(mine[1:]["flags"] == 0)
    rx.close()


# ---------------------------------------------------------------- 6. the series ring at its minimum, many feeds
def test_series_ring_wraps(vh):
    raw, freqs, _ = make_stream(3, N, 55, step=200000)
    res = run(vh, raw, freqs, cut_sizes(N, [79990, 8000, 77770]), 105, 1)      # default block size: 8 002 / 105 + 2 bins -> a ring of 128
    assert res["act"]["series_bins"] == 128 and res["act"]["bins"] == 500 and len(res["per_feed"]) > 8
    check_model(res, 105, 1, "ring")


# ---------------------------------------------------------------- 7. outcome
def wav_run(vh, wav, log, referee=1, undecoded=False):
    rx = vh.Receiver(CF, [CF], 10, vh.FMT_S16LE)
    rx.debug_option("referee", referee)
    rx.activity_enable(105, -30.0, 0, 512)
    if log:
        rx.txlog_enable(undecoded_only=undecoded)
    frames, recs = [], []
    for k in range(0, wav.size, 320000):
        rx.feed(wav[k:k + 320000])
        frames += rx.drain()
        if log:
            recs.append(rx.txlog_read())
    rx.sync()
    out = dict(frames=frames, recs=np.concatenate(recs + [rx.txlog_read()]) if log else None, info=rx.txlog_info() if log else None,
               act=rx.activity(), counters=[list(rx.counters(0).values()), list(rx.avlc_counters(0).values())], stats=rx.stats())
    rx.close()
    return out


def test_reference_wav_and_read_only(vh, golden_wav):
    base = vh.live_resources()
    off = wav_run(vh, golden_wav, False)
    on = wav_run(vh, golden_wav, True)
    assert vh.live_resources() == base
    # read-only: frames, counters and everything the monitor reports are what they are without the log
    assert len(off["frames"]) == 2
    assert_frames_equal(off["frames"], on["frames"], label="transmission log on")
    assert off["counters"] == on["counters"]
    for k, v in off["act"].items():
        assert k == "kernel_ms" or np.array_equal(np.asarray(v), np.asarray(on["act"][k])), k
    for k, v in off["stats"].items():
        assert k.endswith("_ms") or v == on["stats"][k], k
    # the burst is one record, and its outcome is that of the delivered frames
    recs, fr = on["recs"], on["frames"]
    assert len(recs) == 1 and on["act"]["transmissions"][0] == 1
    r = recs[0]
    assert r["chan"] == 0 and r["freq"] == CF and r["flags"] == 0 and r["first_bin"] == 112 and r["first_sample"] == 112 * 105
    assert r["first_sample"] <= min(f["sync_sample"] for f in fr) and max(f["end_sample"] for f in fr) <= r["last_sample"] + 105
    assert r["frames"] == 2 >= 1 and r["frames_ok"] == sum(f["avlc_status"] == vh.AVLC_OK for f in fr) and r["first_burst_ord"] == fr[0]["burst_ord"]
    assert -12.05 <= 10 * np.log10(r["mean_power"]) <= -9.55 and r["peak_power"] >= r["mean_power"]
    info = on["info"]
    assert (info["transmissions"], info["decoded"], info["dropped"], info["frames_matched"], info["frames_unmatched"]) == (1, int(r["frames_ok"] > 0), 0, 2, 0)
    # UNDECODED_ONLY: the record is counted, not delivered
    und = wav_run(vh, golden_wav, True, undecoded=True)
    assert len(und["recs"]) == (0 if r["frames_ok"] else 1) and und["info"]["transmissions"] == 1 and und["info"]["decoded"] == info["decoded"]
    assert und["info"]["flags"] == vh.TXLOG_UNDECODED_ONLY


def burst_stream(specs, n_in, seed):
    """one channel at the centre frequency, oversample 10: a VDL2 burst of one AVLC frame per (start second, amplitude, corrupt) -
    corrupt: more octet errors in every RS block than its parity can mend"""
    from dumpvdl2_amd import synth
    rng = np.random.default_rng(seed)
    x = 0.0005 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    for start_s, amp, corrupt in specs:
        frames = [synth.make_avlc_frame(bytes(rng.integers(0, 256, size=100, dtype=np.uint8)))]
        probe = synth.build_burst(frames)
        bb = synth.build_burst(frames, rng, [7] * probe.num_blocks if corrupt else None)
        assert bb.decodable == (not corrupt)
        wave = synth.modulate(bb.symbols, synth.SPS * 10, start_phase=float(rng.uniform(0, 2 * np.pi)))
        k = int(start_s * 1050000)
        assert k + wave.size < n_in
        x[k:k + wave.size] += amp * wave
    iq = np.stack([x.real, x.imag], axis=1)
    return np.clip(np.rint(32768.0 * iq), -32768, 32767).astype("<i2")


@functools.lru_cache(maxsize=1)
def bursts_raw():
    # strong, weak (about -37 dBFS: under the -30 dBFS threshold, far above the noise), strong but corrupted, strong
    return burst_stream([(0.02, 0.1, False), (0.12, 0.014, False), (0.22, 0.1, True), (0.32, 0.1, False)], 450000, 9)


def bursts_run(vh, undecoded=False):
    raw = bursts_raw()
    rx = receiver(vh, [CF], referee=1)
    rx.activity_enable(105, -30.0, 2, 512)
    rx.txlog_enable(undecoded_only=undecoded)
    frames, recs = [], []
    for k in range(0, raw.shape[0], 80000):
        rx.feed(raw[k:k + 80000])
        rx.sync()
        frames += rx.drain()
        recs.append(rx.txlog_read())
    out = (frames, np.concatenate(recs), rx.txlog_info(), rx.activity())
    rx.close()
    return out


def test_outcome_of_bursts(vh):
    frames, recs, info, act = bursts_run(vh)
    good = [f for f in frames if f["avlc_status"] == vh.AVLC_OK]
    assert len(good) == 3 and len(recs) == 3 == act["transmissions"][0]
    # the weak burst decoded but never rose above the threshold: no record, and its frame is unmatched once the next record comes
    weak = [f for f in frames if not any(r["first_sample"] <= f["sync_sample"] <= r["last_sample"] for r in recs)]
    assert len(weak) == 1 and weak[0]["avlc_status"] == vh.AVLC_OK and recs[0]["last_sample"] < weak[0]["sync_sample"] < recs[1]["first_sample"]
    assert info["frames_unmatched"] == 1 and info["frames_matched"] == len(frames) - 1 and info["decoded"] == 2 and info["transmissions"] == 3
    # the corrupted one is a transmission like the others, without a good frame
    assert [int(r["frames_ok"]) for r in recs] == [1, 0, 1] and recs[0]["frames"] == 1 == recs[2]["frames"]
    for r in (recs[0], recs[2]):
        mine = [f for f in good if r["first_sample"] <= f["sync_sample"] <= r["last_sample"]]
        assert len(mine) == 1 and r["first_burst_ord"] == mine[0]["burst_ord"]
    assert recs[1]["frames"] > 0 or recs[1]["first_burst_ord"] == -1
    # UNDECODED_ONLY delivers exactly the records without a good frame, and counts everything
    _, und, info_u, _ = bursts_run(vh, undecoded=True)
    assert und.tobytes() == recs[recs["frames_ok"] == 0].tobytes() and len(und) == 1
    assert {k: v for k, v in info_u.items() if k not in ("kernel_ms", "flags")} == {k: v for k, v in info.items() if k not in ("kernel_ms", "flags")}


# ---------------------------------------------------------------- 8. arguments, re-enabling, switching off, resources
def test_arguments_and_switching(vh):
    raw, freqs, _ = make_stream(3, N, 22, step=200000)
    base = vh.live_resources()
    rx = receiver(vh, freqs, max_block_bytes=4 * N)
    L = rx.L
    good = dict(struct_size=16, pool_records=0, flags=0, reserved=0)
    info = vh.TxlogInfo(C.sizeof(vh.TxlogInfo))
    one = np.zeros(1, dtype=vh.TX_DTYPE)
    # the activity monitor is off: refused; and nothing to ask of a log that is off
    assert L.vdl2hip_txlog_enable(rx.h, C.byref(vh.TxlogCfg(**good))) == E_INVAL
    assert L.vdl2hip_txlog_info_get(rx.h, C.byref(info)) == E_INVAL and L.vdl2hip_txlog_read(rx.h, one.ctypes.data, 1) == E_INVAL
    assert L.vdl2hip_txlog_disable(rx.h) == 0
    rx.activity_enable(105, THR, 0, 1024)
    for k in range(0, 100000, 12500):                            # (a slot's input buffer and copy event are made on the slot's first feed)
        rx.feed(raw[k:k + 12500])
        rx.sync()
    with_monitor = vh.live_resources()                           # with the log off nothing of it is allocated
    rx.txlog_enable(pool_records=100)
    assert vh.live_resources()["device"] > with_monitor["device"] and vh.live_resources()["pinned"] > with_monitor["pinned"]
    rx.feed(raw[100000:300000])
    rx.sync()
    s0 = rx.txlog_info()
    assert s0["transmissions"] > 5 and s0["pool_records"] == 100
    for bad in (dict(struct_size=12), dict(struct_size=20), dict(pool_records=(1 << 22) + 1), dict(flags=2), dict(flags=3), dict(reserved=1)):
        assert L.vdl2hip_txlog_enable(rx.h, C.byref(vh.TxlogCfg(**{**good, **bad}))) == E_INVAL, bad
        assert {k: v for k, v in rx.txlog_info().items() if k != "kernel_ms"} == {k: v for k, v in s0.items() if k != "kernel_ms"}, bad
    assert L.vdl2hip_txlog_enable(rx.h, None) == E_INVAL and L.vdl2hip_txlog_enable(None, C.byref(vh.TxlogCfg(**good))) == E_INVAL
    assert L.vdl2hip_txlog_info_get(rx.h, C.byref(vh.TxlogInfo(56))) == E_INVAL and L.vdl2hip_txlog_read(rx.h, None, 1) == E_INVAL
    # what does not fit stays queued; the records are still all there
    assert L.vdl2hip_txlog_read(rx.h, None, 0) == 0
    assert L.vdl2hip_txlog_read(rx.h, one.ctypes.data, 1) == 1
    assert len(rx.txlog_read(cap_recs=3)) == s0["transmissions"] - 1
    # enabling again drops what is queued unread and starts afresh, from the monitor's state as it stands
    rx.feed(raw[300000:400000])
    rx.sync()
    assert rx.txlog_info()["transmissions"] > s0["transmissions"]
    rx.txlog_enable(pool_records=1 << 22)                        # (the largest pool that is taken)
    s1 = rx.txlog_info()
    assert (s1["transmissions"], s1["pool_records"], s1["dropped"]) == (0, 1 << 22, 0) and len(rx.txlog_read()) == 0
    rx.txlog_enable()
    nb = 40000 // 105
    rx.feed(raw[400000:])
    rx.sync()
    recs = rx.txlog_read()
    assert len(recs) >= 3 and np.all(recs["last_bin"] >= nb - 1) and rx.txlog_info()["transmissions"] == len(recs)
    a = rx.activity()
    assert a["bins"] == 500                                      # (the monitor ran on through all of it)
    # activity_read(reset) does not touch the log; switching the monitor off, or on again, switches the log off first
    rx.activity(reset=True)
    assert rx.txlog_info()["transmissions"] == len(recs)
    rx.activity_enable(105, THR, 0, 1024)
    assert L.vdl2hip_txlog_info_get(rx.h, C.byref(info)) == E_INVAL
    rx.txlog_enable()
    rx.activity_disable()
    assert L.vdl2hip_txlog_info_get(rx.h, C.byref(info)) == E_INVAL and L.vdl2hip_txlog_read(rx.h, one.ctypes.data, 1) == E_INVAL
    rx.activity_enable(105, THR, 0, 1024)
    assert vh.live_resources() == with_monitor
    rx.txlog_enable()
    rx.txlog_disable()
    assert vh.live_resources() == with_monitor
    rx.txlog_enable()                                            # destroyed with the log on
    rx.feed(raw[:50000])
    rx.close()
    assert vh.live_resources() == base


# ---------------------------------------------------------------- 9. shards and groups
def test_shards_and_group(vh):
    raw, freqs, _ = make_stream(6, N, 77, step=100000)
    sizes = cut_sizes(N, [200000])
    full = run(vh, raw, freqs, sizes, 105, 1, max_block_bytes=4 * 200000)
    check_model(full, 105, 1, "full")
    shard = run(vh, raw, freqs, sizes, 105, 1, max_block_bytes=4 * 200000, chan_first=2, chan_count=3)
    check_model(shard, 105, 1, "shard")
    assert set(shard["recs"]["chan"].tolist()) == {2, 3, 4}
    for c in (2, 3, 4):
        a, b = full["recs"][full["recs"]["chan"] == c], shard["recs"][shard["recs"]["chan"] == c]
        for k in KEYS + ("freq",):
            assert np.array_equal(a[k], b[k]), (c, k)
    # a group of two on one device: vdl2hip_group_ctx(g, k) is the handle of member k's channels
    g = vh.ReceiverGroup(CF, freqs, [0, 0], 10, vh.FMT_S16LE, max_block_bytes=4 * 200000)
    for i in range(g.size()):
        assert g.L.vdl2hip_debug_option(g.member(i), b"referee", 0) == 0
    g.activity_enable(105, THR, 1, 1024)
    g.txlog_enable()
    k = 0
    for d in sizes:
        g.feed(raw[k:k + d])
        k += d
    g.sync()
    seen = 0
    for i in range(2):
        recs = g.txlog_read(i)
        assert set(recs["chan"].tolist()) == {3 * i, 3 * i + 1, 3 * i + 2} and g.txlog_info(i)["transmissions"] == len(recs)
        for c in range(3 * i, 3 * i + 3):
            a, b = full["recs"][full["recs"]["chan"] == c], recs[recs["chan"] == c]
            for kk in KEYS + ("freq",):
                assert np.array_equal(a[kk], b[kk]), (c, kk)
        seen += len(recs)
    assert seen == len(full["recs"])
    g.txlog_disable()
    g.close()


# ---------------------------------------------------------------- 10. the tool
def test_tool(vh, tmp_path, golden_wav):
    from dumpvdl2_amd import build
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    out = str(tmp_path / "tx.txt")
    base = [exe, "--iq-file", WAV, "--sample-format", "S16_LE"]
    p0 = subprocess.run(base, check=True, capture_output=True, text=True, timeout=120)
    p1 = subprocess.run(base + ["--tx-out", out, "--activity-threshold", "-30"], check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stdout.count("[S:") == 2 and p0.stderr == p1.stderr
    lines = open(out).read().splitlines()
    head = dict(l[2:].split(" ", 1) for l in lines if l.startswith("# ") and not l.startswith("# channel"))
    rows = [l.split() for l in lines if not l.startswith("#")]
    summary = [l.split() for l in lines if l.startswith("# channel")]
    want = wav_run(vh, golden_wav, True)
    info, r = want["info"], want["recs"][0]
    assert set(head) == {k for k, _ in vh.TxlogInfo._fields_ if k not in ("struct_size", "reserved", "reserved2")}
    for k in ("pool_records", "flags", "transmissions", "decoded", "dropped", "frames_matched", "frames_unmatched"):
        assert int(head[k]) == info[k], k
    assert len(rows) == 1 and len(rows[0]) == 9
    chan, freq, first_sample, length_ms, peak_db, mean_db, frames, frames_ok, flags = rows[0]
    assert (int(chan), int(freq), int(first_sample), int(frames), int(frames_ok), int(flags)) == (0, CF, r["first_sample"], r["frames"], r["frames_ok"], 0)
    assert abs(float(length_ms) - (r["last_sample"] - r["first_sample"] + 1) / 105.0) < 1e-3
    assert abs(float(peak_db) - 10 * np.log10(r["peak_power"])) < 0.006 and abs(float(mean_db) - 10 * np.log10(r["mean_power"])) < 0.006
    assert summary == [["#", "channel", "0", str(CF), f"transmissions={info['transmissions']}", f"decoded={info['decoded']}",
                        f"ratio={info['decoded'] / info['transmissions']:.4f}"]]
