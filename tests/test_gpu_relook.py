"""The second look on the GPU (include/vdl2hip.h, "Second look"; kernels: dumpvdl2_amd/csrc/relook.h): for every transmission the log
closes, a decode attempt anchored on every preamble in it.

Records and frames are held to the model (tests/relook_model.py) run on the device's OWN decimated stream, read back with
read_decimated() after sync(): with the referee off that is the stream the second look read.  Two channels, oversample 10, one capture
of 0.3 s made here: on channel 0 a long weak burst A with a short burst B some 21 dB stronger inside it - the reference locks on A,
slices through B and decodes neither - and on channel 1 a burst the main path decodes."""
import ctypes as C
import functools

import numpy as np
import pytest

import relook_model as rm
import txsearch_model as tm
from dumpvdl2_amd import synth
from util import assert_frames_equal

pytestmark = pytest.mark.gpu
CF = 136975000
FREQS = synth.channel_plan(2, CF)
OS = 10
FS = 105000 * OS
N = int(0.3 * FS)
ACT = (105, -50.0, 2)          # bins of 1 ms, busy above -50 dBFS, two idle bins bridged
BACK = (ACT[2] + 1) * ACT[0]


# ---------------------------------------------------------------- the capture
def _place(acc, chan, start, wave, amp):
    w = 2.0 * np.pi * (FREQS[chan] - CF) / FS
    idx = np.arange(start, start + wave.size, dtype=np.float64)
    acc[start:start + wave.size] += (amp * wave * np.exp(1j * w * idx)).astype(np.complex64)


@functools.lru_cache(maxsize=3)
def scenario(b_at=120000, cut_at=0):
    """-> (raw int16 [N, 2], frames: {"A", "B", "C"} -> the AVLC frame of the burst); b_at: the input sample at which B begins;
    cut_at: a fourth burst begins there on channel 1 whose transmitter stops halfway through it (0: none)"""
    rng = np.random.default_rng(20261021)
    fr = {k: synth.make_avlc_frame(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()) for k, n in (("A", 700), ("B", 40), ("C", 60))}
    wave = {k: synth.modulate(synth.build_burst([f]).symbols, 10 * OS, start_phase=float(rng.uniform(0, 6.28))) for k, f in fr.items()}
    acc = np.zeros(N, dtype=np.complex64)
    _place(acc, 0, 40000, wave["A"], 0.008)
    _place(acc, 0, b_at, wave["B"], 0.09)                       # begins and ends inside A (A: 1.9e5 input samples, B: 1.9e4)
    _place(acc, 1, 60000, wave["C"], 0.05)
    assert 40000 + wave["A"].size > b_at + wave["B"].size and b_at > 40000
    if cut_at:
        r2 = np.random.default_rng(20261022)                     # (its own generator: A, B, C and the noise are those of scenario())
        w = synth.modulate(synth.build_burst([synth.make_avlc_frame(r2.integers(0, 256, size=300, dtype=np.uint8).tobytes())]).symbols, 10 * OS)
        _place(acc, 1, cut_at, w[:w.size // 2], 0.05)
        assert cut_at > 60000 + wave["C"].size + 10 * OS * ACT[0] * (ACT[2] + 2) and cut_at + w.size // 2 < N - 10000
    iq = np.stack([acc.real, acc.imag], axis=1) + rng.standard_normal((N, 2)).astype(np.float32) * np.float32(0.0004)
    return np.clip(np.rint(iq * 32768.0), -32768, 32767).astype(np.int16), fr


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


def cut_sizes(n, sizes):
    out, k, i = [], 0, 0
    while k < n:
        d = min(sizes[i % len(sizes)], n - k)
        out.append(d); k += d; i += 1
    return out


def run(vh, sizes, relook=None, search=True, chan_first=0, chan_count=0, reenable_at=None, capture=None, base=0, per_feed=False):
    """the capture fed in pieces of `sizes` samples; relook: the arguments of relook_enable (None: off); capture: (raw int16 [n, 2],
    freqs, oversample) in place of scenario()'s; base: the input sample the stream begins at (debug_set_position on the fresh receiver,
    ahead of every tap); per_feed: a sync() behind every feed, so that every read holds the records of that feed alone - feeds_tx, by
    which model() shares a feed's room - and the new decimated samples are read back behind every feed (a short ring keeps no more)
    -> dict; y[c][i] is decimated sample K + i, K = base / oversample"""
    raw, freqs, os_ = capture if capture is not None else (scenario()[0], FREQS, OS)
    n, K = raw.shape[0], base // os_
    rx = vh.Receiver(CF, freqs, os_, vh.FMT_S16LE, 0.0, max_block_bytes=4 * max(sizes), chan_first=chan_first, chan_count=chan_count)
    if base:
        rx.debug_set_position(base)
    rx.debug_option("referee", 0)
    rx.activity_enable(*ACT, 0)
    rx.txlog_enable()
    if search:
        rx.txsearch_enable()
    if relook is not None:
        rx.relook_enable(**relook)
    chans = range(rx.chan_first, rx.chan_first + rx.chan_count)
    frames, tx, txs, recs, rlf, y = [], [], [], [], [], {c: [] for c in chans}

    def collect():
        frames.extend(rx.drain())
        tx.append(rx.txlog_read())
        if search:
            txs.append(rx.txsearch_read())
        if relook is not None:
            r, f = rx.relook_read()
            r["frame_first"] = np.where(r["frames"] > 0, r["frame_first"] + len(rlf), 0)
            recs.append(r); rlf.extend(f)
    k = made = 0
    for i, d in enumerate(sizes):
        if reenable_at == i:
            rx.sync(); collect()
            rx.relook_enable(**relook)
        rx.feed(raw[k:k + d])
        k += d
        if per_feed:
            rx.sync()
        collect()
        if per_feed and k // os_ > made:
            for c in chans:
                y[c].append(rx.read_decimated(c, K + made, k // os_ - made))
            made = k // os_
    assert k == n
    rx.sync()
    collect()
    for c in chans:
        y[c].append(rx.read_decimated(c, K + made, n // os_ - made))
    out = dict(frames=frames, tx=np.concatenate(tx), txs=np.concatenate(txs) if search else None,
               recs=np.concatenate(recs) if relook is not None else None, rlf=rlf, info=rx.relook_info() if relook is not None else None,
               loginfo=rx.txlog_info(), feeds_tx=[len(t) for t in tx] if per_feed else None, feeds_recs=[len(r) for r in recs], K=K,
               counters=[[list(rx.counters(c).values()), list(rx.avlc_counters(c).values())] for c in chans],
               y={c: np.concatenate(v).view(np.complex64).reshape(-1) for c, v in y.items()})
    rx.close()
    assert all(v.size == n // os_ for v in out["y"].values())
    return out


def getter(res, c):
    """channel c's stream of a run as the model reads it: absolute sample n; ahead of the run's first sample K lies rest"""
    v, K = res["y"][c], res["K"]
    if K == 0:
        return tm.stream_get(v)

    def get(n):
        n = np.asarray(n, dtype=np.int64)
        out = np.zeros(n.shape, dtype=np.complex64)
        ok = n >= K
        out[ok] = v[n[ok] - K]
        return out
    return get


@pytest.fixture(scope="module")
def single(vh):
    return run(vh, [N], relook={})


def model(res, feeds_tx=None, **cfg):
    """the model on the run's own stream: the attempts of every log record in the log's order; the room of a feed is shared by the
    records of that feed (feeds_tx: the number of log records of each feed; None: one feed) -> ([(log record, attempt, frames)], anchors found)"""
    want, found = [], 0
    bounds = np.cumsum(feeds_tx if feeds_tx is not None else [len(res["tx"])])
    # (vdl2hip.h, "Room": the defaults are 256 records and 8192 octets per channel of the receiver, at least 4096 and 2^20)
    pf, pc = cfg.get("pool_frames", 0) or max(rm.DEF_FRAMES, 256 * len(res["y"])), cfg.get("pool_octets", 0) or max(rm.DEF_OCTETS, 8192 * len(res["y"]))
    off = [0, 0]
    for i, t in enumerate(res["tx"]):
        if i in bounds:
            off = [0, 0]
        att, nf = rm.second_look(getter(res, int(t["chan"])), int(t["first_sample"]), int(t["last_sample"]), int(t["last_sample"]) + BACK,
                                 int(t["freq"]), cfg.get("threshold", 0.0), cfg.get("max_anchors", 0), cfg.get("max_ppm", 0.0), 1 << 30, 1 << 30, int(t["flags"]))
        found += nf
        for r, frames in att:
            r["found"] = nf                                      # (the anchors found in its record, of which max_anchors are kept)
            cf, cp = rm.claim(r["tl_bits"]) if r["tl_bits"] and not r["flags"] & (rm.TRUNCATED | rm.PPM_REJECT) else (0, 0)
            if cf and (off[0] + cf > pf or off[1] + cp > pc):
                r.update(flags=r["flags"] | rm.NO_ROOM, stop=-1, counters=[0] * 20, frames=0, frames_ok=0, fec_corrections=-1)
                frames = []
            off[0] += cf; off[1] += cp
            want.append((t, r, frames))
    return want, found


def check_model(res, label, **cfg):
    want, found = model(res, **cfg)
    recs, rlf = res["recs"], res["rlf"]
    assert len(recs) == len(want), (label, len(recs), len(want))
    for i, (g, (t, r, frames)) in enumerate(zip(recs, want)):
        assert (int(g["chan"]), int(g["freq"]), int(g["first_bin"])) == (int(t["chan"]), int(t["freq"]), int(t["first_bin"])), (label, i)
        ff = int(g["frame_first"])
        got = rlf[ff:ff + int(g["frames"])]
        rm.check(g, got, r, frames, f"{label} attempt {i}")
        assert all(f["chan"] == int(t["chan"]) and f["freq"] == int(t["freq"]) for f in got)
    assert res["info"]["anchors_found"] == found and res["info"]["attempts"] == len(want) and res["info"]["records"] == len(res["tx"]), (label, res["info"])
    return want


# ---------------------------------------------------------------- 1. the covered burst
def test_covered_burst(vh, single, oracle_mod):
    raw, fr = scenario()
    o = oracle_mod.Oracle(CF, FREQS, oversample=OS)
    o.process(raw)
    ref = o.frames()
    # the conditions: the reference yields C and nothing with B's octets, and the log's record of the transmission on channel 0 is undecoded
    assert [f["octets"] for f in ref if f["chan"] == 1] == [fr["C"]]
    assert not any(f["octets"] == fr["B"] for f in ref) and not any(f["chan"] == 0 and oracle_mod.avlc_screen(f["octets"])[0] == 0 for f in ref)
    tx0 = [t for t in single["tx"] if int(t["chan"]) == 0]
    assert len(tx0) == 1 and int(tx0[0]["frames_ok"]) == 0
    want = check_model(single, "single feed")
    hits = [(r, frames) for t, r, frames in want if int(t["chan"]) == 0 and any(f["octets"] == fr["B"] for f in frames)]
    assert len(hits) == 1 and float(hits[0][0]["pherr"]) < 4.0, "the model finds B's anchor below 4 and decodes B"
    # the main path is the reference's
    assert_frames_equal(ref, single["frames"], label="main path")
    for c in range(2):
        assert single["counters"][c][0] == list(o.counters(c).values())
    # the second look delivers B: octets, OK, NEW
    got = [(g, single["rlf"][int(g["frame_first"])]) for g in single["recs"] if int(g["chan"]) == 0 and int(g["frames_ok"]) == 1]
    got = [(g, f) for g, f in got if f["octets"] == fr["B"]]
    assert len(got) == 1
    g, f = got[0]
    assert f["avlc_status"] == 0 and int(g["frames_new"]) == 1 and int(g["new_mask"]) == 1 and f["burst_ord"] == -1 and f["sync_sample"] == int(g["anchor"]) and np.isnan(f["nf_pwr_dbfs"])
    assert single["info"]["frames_new"] >= 1


# ---------------------------------------------------------------- 2. records equal the model, whatever the cut
def stable(res):
    """records and frames in an order and a form that does not depend on the cut: by (chan, first_bin, anchor); frame_first is an index
    of the read and frames_new the host's join (vdl2hip.h, "Second look": New or seen), both left out.  Per record: the bytes of its
    integer fields and of its frames' octets and integer fields; the bytes of its float fields and of its frames' frame_pwr_dbfs; the
    samples it read.  Samples are counted from the run's first, K (first_bin is: the log counts its bins from where it was enabled),
    so that a run hours into a stream gives what the run at 0 gives"""
    out, K = [], res["K"]
    for g in np.sort(res["recs"], order=["chan", "first_bin", "anchor"]):
        ff = int(g["frame_first"])
        h = g.copy(); h["frame_first"] = 0; h["frames_new"] = 0; h["new_mask"] = 0
        h["anchor"] -= K; h["end_sample"] -= K
        fr = [dict(f, sync_sample=f["sync_sample"] - K, end_sample=f["end_sample"] - K) for f in res["rlf"][ff:ff + int(g["frames"])]]
        floats = b"".join(h[k].tobytes() for k in rm.FLOAT_FIELDS) + b"".join(np.float32(f["frame_pwr_dbfs"]).tobytes() + np.float32(f["ppm_error"]).tobytes() for f in fr)
        for k in rm.FLOAT_FIELDS:
            h[k] = 0
        ints = h.tobytes() + b"".join(f["octets"] + bytes(str((f["idx"], f["avlc_status"], f["num_fec_corrections"], f["sync_sample"], f["end_sample"])), "ascii") for f in fr)
        out.append((ints, floats, (int(g["chan"]), max(0, int(h["anchor"]) - 150), int(h["end_sample"]) + 1)))
    return out


@pytest.mark.parametrize("sizes", [[100003, 103333, 111664], [80000]], ids=["three uneven feeds", "blocks of 320000 bytes"])
def test_cuts(vh, single, sizes):
    """The same capture cut differently.  Each run is held to the model on its own stream, every field exact: the records are a function
    of y_c alone.  Across the cuts the records exist alike and every integer field and every octet is byte-identical; the float fields
    (pherr, slope, ppm_error, prev_phase, the frames' frame_pwr_dbfs) are byte-identical wherever the two runs' y_c are over the samples
    the attempt read.  They are not everywhere: WITHOUT THE REFEREE THE CHANNELISER'S STREAM ITSELF DEPENDS ON THE CUT in its last bits
    (tests/test_gpu_txsearch.py, same_across_cuts: its filter scan starts afresh from a carried state at every feed).  Measured on this
    capture: behind the first cut the streams differ, and there the float fields differ in their last bits with them - e.g. B's pherr
    0.0611 in both runs, unequal bit patterns - while the model on each run's own stream gives each run's bits."""
    res = run(vh, cut_sizes(N, sizes), relook={})
    check_model(res, f"cut {sizes}")
    a, b = stable(single), stable(res)
    assert len(a) == len(b)
    exact = 0
    for (ia, fa, (c, lo, hi)), (ib, fb, _) in zip(a, b):
        assert ia == ib, "integer fields and octets are byte-identical across the cuts"
        if np.array_equal(res["y"][c][lo:hi].view(np.uint64), single["y"][c][lo:hi].view(np.uint64)):
            assert fa == fb, "over identical samples the records are identical byte for byte"
            exact += 1
    print(f"cut {sizes}: {len(a)} records, {exact} over identical samples and identical byte for byte")
    if len(sizes) == 3:
        assert exact >= 1, "the burst on channel 1 ends ahead of the first of the three cuts: its record is compared byte for byte"
    else:
        # blocks of 320 000 bytes: C's unique word ends at decimated sample 6 245, ahead of the first cut at 8 000, but its last symbol
        # lies behind it: what is wholly ahead of the cut is the anchor's own evidence, and that is compared byte for byte
        c1a, c1b = ([g for g in r["recs"] if int(g["chan"]) == 1 and int(g["anchor"]) < 8000] for r in (single, res))
        assert len(c1a) == len(c1b) >= 1
        lo, hi = int(c1a[0]["anchor"]) - 150, int(c1a[0]["anchor"]) + 91
        assert np.array_equal(res["y"][1][lo:hi].view(np.uint64), single["y"][1][lo:hi].view(np.uint64))
        for ga, gb in zip(c1a, c1b):
            for k in ("anchor", "pherr", "slope", "ppm_error", "prev_phase", "tl_bits", "nsym", "synd_weight"):
                assert ga[k].tobytes() == gb[k].tobytes(), k


# ---------------------------------------------------------------- 3. a decoded transmission
def test_seen_and_new_only(vh, single):
    _, fr = scenario()
    c1 = [g for g in single["recs"] if int(g["chan"]) == 1 and int(g["frames_ok"]) >= 1]
    assert len(c1) >= 1 and all(int(g["frames_new"]) == 0 for g in c1), "the main path delivered C: its attempt is SEEN"
    assert any(single["rlf"][int(g["frame_first"])]["octets"] == fr["C"] for g in c1)
    only = run(vh, [N], relook=dict(new_only=True))
    assert len(only["recs"]) >= 1 and all(int(g["frames_new"]) > 0 for g in only["recs"]) and not any(int(g["chan"]) == 1 for g in only["recs"])
    assert only["info"]["attempts"] == single["info"]["attempts"] and only["info"]["frames_new"] == single["info"]["frames_new"]


# ---------------------------------------------------------------- 4. on versus off
def test_on_versus_off(vh, single):
    before = vh.live_resources()
    off = run(vh, [N])
    assert_frames_equal(off["frames"], single["frames"], label="second look on")
    assert off["counters"] == single["counters"]
    assert off["tx"].tobytes() == single["tx"].tobytes() and off["txs"].tobytes() == single["txs"].tobytes()
    for c in range(2):
        assert np.array_equal(off["y"][c].view(np.uint64), single["y"][c].view(np.uint64))
    assert vh.live_resources() == before
    # off after on gives everything back
    raw, _ = scenario()
    rx = vh.Receiver(CF, FREQS, OS, vh.FMT_S16LE, 0.0, max_block_bytes=4 * N)
    rx.activity_enable(*ACT, 0); rx.txlog_enable(); rx.txsearch_enable()
    step = N // 16
    for i in range(8):                                           # (every slot of the receiver has carried a feed: what it creates on first use exists)
        rx.feed(raw[i * step:(i + 1) * step]); rx.sync()
    base = vh.live_resources()
    rx.relook_enable()
    assert vh.live_resources()["device"] > base["device"]
    for i in range(8, 16):
        rx.feed(raw[i * step:(i + 1) * step]); rx.sync()
    assert rx.relook_info()["attempts"] >= 1
    rx.relook_disable()
    assert vh.live_resources() == base
    rx.close()


# ---------------------------------------------------------------- 5. room
def test_room(vh, single):
    want, _ = model(single)
    claims = [rm.claim(r["tl_bits"]) for _, r, _ in want if r["tl_bits"] and not r["flags"] & (rm.TRUNCATED | rm.PPM_REJECT)]
    assert len(claims) >= 2
    total_p = sum(c[1] for c in claims)
    res = run(vh, [N], relook=dict(pool_frames=1 << 12, pool_octets=total_p - 1))
    check_model(res, "octets one short", pool_frames=1 << 12, pool_octets=total_p - 1)
    flagged = [bool(int(g["flags"]) & rm.NO_ROOM) for g in res["recs"] if int(g["tl_bits"]) and not int(g["flags"]) & rm.TRUNCATED]
    assert flagged == [False] * (len(claims) - 1) + [True], "what survives is a prefix"
    assert res["info"]["dropped"] == 1
    res = run(vh, [N], relook=dict(pool_frames=1))
    check_model(res, "one record of room", pool_frames=1)
    assert res["info"]["dropped"] == len(claims) and res["info"]["frames"] == 0 and len(res["rlf"]) == 0
    assert all(int(g["tl_bits"]) > 0 for g in res["recs"] if int(g["flags"]) & rm.NO_ROOM)


# ---------------------------------------------------------------- 6. lifecycle
def test_lifecycle(vh, single):
    raw, fr = scenario()
    rx = vh.Receiver(CF, FREQS, OS, vh.FMT_S16LE, 0.0, max_block_bytes=4 * N)
    rx.activity_enable(*ACT, 0); rx.txlog_enable()
    with pytest.raises(vh.Vdl2HipError, match=r"\(-1\)"):
        rx.relook_enable()                                       # the search is off
    rx.txsearch_enable()
    for bad in (dict(threshold=30.5), dict(threshold=-1.0), dict(threshold=float("nan")), dict(max_anchors=17), dict(max_ppm=-1.0),
                dict(pool_frames=(1 << 20) + 1), dict(pool_octets=(1 << 26) + 1)):
        with pytest.raises(vh.Vdl2HipError, match=r"\(-1\)"):
            rx.relook_enable(**bad)
    rx.relook_enable(threshold=30.0, max_anchors=16)
    assert rx.relook_info()["threshold"] == 30.0 and rx.relook_info()["max_anchors"] == 16
    rx.txlog_disable()                                           # switches the search and the second look off
    with pytest.raises(vh.Vdl2HipError):
        rx.relook_info()
    rx.close()
    # re-enabled in mid-stream: the totals start afresh, the transmissions closed afterwards are looked at as ever
    res = run(vh, cut_sizes(N, [100000]), relook={}, reenable_at=1)
    want, _ = model(res)
    late = [(t, r, f) for t, r, f in want if int(t["last_sample"]) + BACK >= 100000 // OS]
    assert len(res["recs"]) >= len(late) >= 1
    got = {(int(g["chan"]), int(g["anchor"])): g for g in res["recs"]}
    for t, r, frames in late:
        g = got[(int(t["chan"]), r["anchor"])]
        rm.check(g, res["rlf"][int(g["frame_first"]):int(g["frame_first"]) + int(g["frames"])], r, frames, "re-enabled")
    # a receiver of the second channel alone reports it as channel 1
    part = run(vh, [N], relook={}, chan_first=1, chan_count=1)
    assert len(part["recs"]) >= 1 and all(int(g["chan"]) == 1 and int(g["freq"]) == FREQS[1] for g in part["recs"])
    assert any(f["octets"] == fr["C"] and f["chan"] == 1 for f in part["rlf"])


# ---------------------------------------------------------------- the tool
def test_tool(vh, tmp_path):
    """tools/vdl2hip_iqfile --relook-out / --relook-frames / --relook-threshold: the attempts of the capture in a file of their own, B -
    NEW, good - in an archive of its own that parses back, the main output what it is without the options"""
    import struct
    import subprocess
    from dumpvdl2_amd import build
    import test_rawframe_format as trf
    raw, fr = scenario()
    exe = build.build_cli(str(tmp_path / "vdl2hip_iqfile"))
    iq = str(tmp_path / "capture.cs16")
    raw.tofile(iq)
    base = [exe, "--iq-file", iq, "--sample-format", "S16_LE", "--oversample", str(OS), "--centerfreq", str(CF), "--station-id", "TEST",
            "--activity-threshold", str(ACT[1]), "--activity-hang", str(ACT[2])]
    main_raw, out, arch = str(tmp_path / "main.bin"), str(tmp_path / "relook.txt"), str(tmp_path / "relook.bin")
    p0 = subprocess.run(base + ["--raw-frames-out", main_raw] + [str(f) for f in FREQS], check=True, capture_output=True, text=True, timeout=120)
    main0 = open(main_raw, "rb").read()
    p1 = subprocess.run(base + ["--raw-frames-out", main_raw, "--relook-out", out, "--relook-frames", arch, "--relook-threshold", "4"] + [str(f) for f in FREQS],
                        check=True, capture_output=True, text=True, timeout=120)
    assert p0.stdout == p1.stdout and p0.stderr == p1.stderr and p0.stdout.count("[S:") == 1, "the main output does not change"

    def archive(path):
        RawFrame = trf.build_schema()
        blob, off, got = open(path, "rb").read(), 0, []
        while off < len(blob):
            (ln,) = struct.unpack(">H", blob[off:off + 2])
            m = RawFrame(); m.ParseFromString(blob[off + 2:off + ln]); got.append(m); off += ln
        return got
    assert [m.data for m in archive(main_raw)] == [fr["C"]] and len(open(main_raw, "rb").read()) == len(main0), "second-look frames are never mixed into the main archive"
    new = archive(arch)
    assert [m.data for m in new] == [fr["B"]] and new[0].metadata.station_id == "TEST" and new[0].metadata.frequency == FREQS[0]
    lines = open(out).read().splitlines()
    hd = dict(zip(lines[0].split()[1::2], lines[0].split()[2::2]))
    rows = [l.split() for l in lines[1:]]
    # the tool feeds the file as one feed, the referee on: the same through the binding
    rx = vh.Receiver(CF, FREQS, OS, vh.FMT_S16LE, 0.0, max_block_bytes=4 * N)
    rx.activity_enable(*ACT, 0); rx.txlog_enable(); rx.txsearch_enable(); rx.relook_enable(threshold=4.0)
    rx.feed(raw); rx.sync(); rx.drain()
    recs, _ = rx.relook_read()
    info = rx.relook_info()
    rx.close()
    assert [int(hd[k]) for k in ("records", "anchors_found", "attempts", "frames", "frames_ok", "frames_new", "dropped")] == \
        [info[k] for k in ("records", "anchors_found", "attempts", "frames", "frames_ok", "frames_new", "dropped")] and int(hd["frames_new"]) == 1
    names = [k for k in vh.RELOOK_DTYPE.names if k not in ("frame_first", "new_mask", "reserved", "counters")]
    assert len(rows) == len(recs) and all(len(r) == len(names) == 18 for r in rows)
    for row, g in zip(rows, recs):
        for k, v in zip(names, row):
            if k in rm.FLOAT_FIELDS:
                assert tm.same_bits(np.float32(float(v)), g[k]), k   # (%.9g brings a float32 back exactly)
            else:
                assert int(v) == int(g[k]), k


# ---------------------------------------------------------------- 7. ABI and binding
def test_abi_and_binding(vh):
    L = vh.load_library()
    for name in ("vdl2hip_relook_enable", "vdl2hip_relook_disable", "vdl2hip_relook_info_get", "vdl2hip_relook_read", "vdl2hip_debug_relook_range"):
        assert hasattr(L, name), name
    assert all(n in vh.EXPORTS for n in ("vdl2hip_relook_enable", "vdl2hip_relook_disable", "vdl2hip_relook_info_get", "vdl2hip_relook_read"))
    assert vh.RELOOK_DTYPE.itemsize == 256 and C.sizeof(vh.RelookCfg) == 32 and C.sizeof(vh.RelookInfo) == 96
    assert vh.RELOOK_DTYPE.fields["counters"][1] == 96 and vh.RELOOK_DTYPE.fields["flags"][1] == 84
    assert L.vdl2hip_abi_version() == 6
    rx = vh.Receiver(CF, FREQS, OS, vh.FMT_S16LE)
    info = vh.RelookInfo(C.sizeof(vh.RelookInfo))
    assert L.vdl2hip_relook_info_get(rx.h, C.byref(info)) == -1          # off
    rx.close()
