"""The second look's kernels on the host (dumpvdl2_amd/csrc/relook.h).  Their per-lane steps - the phases and the metric of a piece with
its halo of 160 samples, the local-minimum test, the selection of the best anchors, the planning of an attempt (gate, header, limit,
claim), the attempt itself through decode_burst() and finish_frame() - are plain functions that the library also builds for the CPU,
behind a test hook that needs no GPU:
  - vdl2hip_debug_relook_range: one record's first_sample .. last_sample over a ring -> its attempt records and their frames.
The yardstick: tests/relook_model.py.  Every comparison is exact but frame_pwr_dbfs (util.TOL_DB)."""
import ctypes as C

import numpy as np
import pytest

import core_reference as cr
import relook_model as rm
import txsearch_model as tm
from dumpvdl2_amd import synth, vdl2hip

E_INVAL = -1
FREQ = 136975000
RING = 8192
HDR_STOPS = (rm.CNT["CRC_BAD"], rm.CNT["ERR_TOO_LONG"], rm.CNT["ERR_NO_FEC"])


@pytest.fixture(scope="module")
def lib(oracle_mod):
    L = vdl2hip.load_library()
    L.vdl2hip_debug_relook_range.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_float, C.c_uint32, C.c_float,
                                             C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(vdl2hip.PackedFrame), C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.POINTER(C.c_uint64)]
    return L


def noise_ring(n, seed, sigma=0.01):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * sigma).astype(np.float32)


def burst(seed=20261021, payload=40, errors=None, cfo=0.0):
    """(waveform at 10 samples a symbol, its frame): the last symbol of the unique word is sample 240 of the waveform"""
    rng = np.random.default_rng(seed)
    frame = synth.make_avlc_frame(rng.integers(0, 256, size=payload, dtype=np.uint8).tobytes())
    bb = synth.build_burst([frame], rng, errors)
    w = synth.modulate(bb.symbols, 10, start_phase=0.7)
    w = w * np.exp(1j * 2.0 * np.pi * cfo * np.arange(w.size))
    return w.astype(np.complex64), frame, bb


def add(y, at, w, amp=0.05):
    w = w * np.float32(amp)
    lo = max(0, -at)
    y[at + lo:at + w.size, 0] += w.real[lo:]
    y[at + lo:at + w.size, 1] += w.imag[lo:]


def run(lib, y, first, last, limit, thr=0.0, K=0, max_ppm=0.0, pf=0, pc=0, freq=FREQ, expect=None):
    y = np.ascontiguousarray(y, dtype=np.float32)
    recs = np.zeros(16, dtype=vdl2hip.RELOOK_DTYPE)
    pk = (vdl2hip.PackedFrame * 4096)()
    po = (C.c_uint8 * (1 << 16))()
    out = (C.c_uint64 * 4)()
    r = lib.vdl2hip_debug_relook_range(y.ctypes.data, y.shape[0], first, last, limit, freq, thr, K, max_ppm, pf, pc, recs.ctypes.data, 16, pk, 4096, po, 1 << 16, out)
    if expect is not None:
        assert r == expect, r
        return None
    assert r >= 0 and r == out[1], (r, list(out))
    frames = vdl2hip.unpack_frames(int(out[2]), pk, memoryview(po)[:int(out[3])])
    return recs[:r], frames, int(out[0])


def check(lib, y, first, last, limit, label="", **cfg):
    """the hook against the model on the same ring: every attempt, every frame"""
    recs, frames, found = run(lib, y, first, last, limit, **cfg)
    want, wfound = rm.second_look(tm.ring_get(y), first, last, limit, FREQ, threshold=cfg.get("thr", 0.0), max_anchors=cfg.get("K", 0),
                                  max_ppm=cfg.get("max_ppm", 0.0), pool_frames=cfg.get("pf", 0), pool_octets=cfg.get("pc", 0))
    assert found == wfound and len(recs) == len(want), (label, found, wfound, len(recs), len(want))
    for i, (r, (w, wf)) in enumerate(zip(recs, want)):
        assert (int(r["chan"]), int(r["freq"]), int(r["first_bin"]), int(r["frames_new"])) == (0, FREQ, 0, 0)
        ff = int(r["frame_first"])
        rm.check(r, frames[ff:ff + int(r["frames"])], w, wf, f"{label} attempt {i}")
    assert sum(int(r["frames"]) for r in recs) == len(frames)
    return recs, frames, want


def preamble_ring(n, at, seed, jitter=0.0):
    """unit samples of random phase, with the 16 taps of a perfect unique word (plus a little phase jitter) ending at each n of `at`"""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-np.pi, np.pi, n)
    for a in at:
        th[a - 150 + 10 * np.arange(16)] = cr.PR_PHASE.astype(np.float64) + 0.3 + rng.standard_normal(16) * jitter
    return np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32)


def test_record_size():
    assert vdl2hip.RELOOK_DTYPE.itemsize == 256 and C.sizeof(vdl2hip.RelookCfg) == 32 and C.sizeof(vdl2hip.RelookInfo) == 96


def test_arguments(lib):
    y = noise_ring(1024, 1)
    run(lib, y, 0, 1023, 1023, thr=31.0, expect=E_INVAL)
    run(lib, y, 0, 1023, 1023, thr=-1.0, expect=E_INVAL)
    run(lib, y, 0, 1023, 1023, thr=float("nan"), expect=E_INVAL)
    run(lib, y, 0, 1023, 1023, K=17, expect=E_INVAL)
    run(lib, y, 0, 1023, 1000, expect=E_INVAL)
    run(lib, y[:1000], 0, 999, 999, expect=E_INVAL)


def test_noise_has_no_anchor(lib):
    y = noise_ring(1024, 20261021)
    recs, frames, _ = check(lib, y, 0, 1023, 1023, "noise")
    assert len(recs) == 0 and len(frames) == 0


def test_all_zero_ring_at_the_highest_threshold(lib):
    """An all-zero ring, the threshold at 30, the highest the interface takes.  Every p is equal - Phi is 0 everywhere, also before the
    stream - but what it equals is 35.99321 (the unique word's own phases against a constant, mean and slope removed): not below 30, so
    there is no anchor, and none on any ring of constant phase or constant phase step.  The tie rule that would leave exactly the first
    of equal minima is held by test_separation_edge, whose two minima 160 apart are equal to the bit."""
    y = np.zeros((2048, 2), dtype=np.float32)
    p, _ = tm.metric(tm.ring_get(y), 300, 1500)
    assert np.all(p == p[0]) and tm.same_bits(p[0], np.float32(35.99321)), float(p[0])
    recs, _, _ = check(lib, y, 300, 1500, 1600, "zeros", thr=30.0)
    assert len(recs) == 0
    assert rm.anchors(np.full(1201, 29.0, dtype=np.float32), 30.0) == [0]      # (the model's rule on equal values below the threshold)


def test_a_run_of_equal_minima(lib):
    """unique words a whole symbol apart on one grid of taps give bit-equal values of the metric: of a run of five equal minima, 160
    samples from one to the next, the tie rule leaves the first and only the first (each later one has an equal value within 160
    before it); 161 apart, each is an anchor"""
    for sep, want in ((160, [1000]), (161, [1000 + 161 * k for k in range(5)])):
        at = [1000 + sep * k for k in range(5)]
        y = preamble_ring(4096, at, 17)
        p, _ = tm.metric(tm.ring_get(y), 1000, at[-1])
        assert all(tm.same_bits(p[a - 1000], p[0]) for a in at) and p[0] < 4.0
        recs, _, _ = check(lib, y, 500, 3500, 3600, f"run of equal minima {sep} apart", K=16)
        assert [int(r["anchor"]) for r in recs if 1000 <= int(r["anchor"]) <= at[-1]] == want


@pytest.mark.parametrize("where", [1023, 1024, 1025, 2047, 2048])
def test_minimum_at_a_piece_boundary(lib, where):
    """the burst's minimum on the last sample of a piece, on the first of the next and one inside: its halo lies in the neighbour piece"""
    first = 1000
    y = noise_ring(RING, 7, sigma=0.002)
    w, frame, _ = burst()
    add(y, first + where - 240, w)
    recs, frames, _ = check(lib, y, first, first + 4500, first + 4600, f"boundary {where}")
    hit = [r for r in recs if int(r["anchor"]) == first + where]
    assert len(hit) == 1 and int(hit[0]["frames_ok"]) == 1
    assert frames[int(hit[0]["frame_first"])]["octets"] == frame


@pytest.mark.parametrize("sep, n_anchors", [(160, 1), (161, 2)])
def test_separation_edge(lib, sep, n_anchors):
    y = preamble_ring(4096, [1000, 1000 + sep], 11)
    recs, _, want = check(lib, y, 500, 3000, 3100, f"separation {sep}", K=16)
    near = [int(r["anchor"]) for r in recs if 1000 <= int(r["anchor"]) <= 1000 + sep]
    assert near == [1000, 1000 + sep][:n_anchors], near          # (160 apart: equal minima, the tie rule leaves the first)
    p, _ = tm.metric(tm.ring_get(y), 1000, 1000 + sep)
    assert tm.same_bits(p[0], p[-1]) and p[0] < 4.0


def test_more_anchors_than_kept(lib):
    at = [600 + 300 * k for k in range(6)]
    y = preamble_ring(4096, at, 13, jitter=0.05)
    all_recs, _, _ = check(lib, y, 300, 3000, 3100, "all", K=16)
    assert [int(r["anchor"]) for r in all_recs] == at
    recs, _, _ = check(lib, y, 300, 3000, 3100, "best three", K=3)
    best = sorted(sorted(all_recs, key=lambda r: (float(r["pherr"]), int(r["anchor"])))[:3], key=lambda r: int(r["anchor"]))
    assert [int(r["anchor"]) for r in recs] == [int(r["anchor"]) for r in best]
    _, _, found = run(lib, y, 300, 3000, 3100, K=3)
    assert found == 6


def test_clean_burst(lib):
    y = noise_ring(RING, 3, sigma=0.002)
    w, frame, bb = burst(payload=60)
    add(y, 2000, w)
    recs, frames, _ = check(lib, y, 1500, 5500, 5600, "clean")
    r = [r for r in recs if int(r["anchor"]) == 2240][0]
    assert int(r["tl_bits"]) == bb.tl_bits and int(r["frames"]) == 1 and int(r["frames_ok"]) == 1 and int(r["stop"]) == -1 and int(r["fec_corrections"]) == 0
    f = frames[int(r["frame_first"])]
    assert f["octets"] == frame and f["avlc_status"] == 0 and f["sync_sample"] == 2240 and f["burst_ord"] == -1


def test_rs_corrections(lib):
    y = noise_ring(RING, 4, sigma=0.002)
    w, frame, bb = burst(payload=60, errors=[2])
    assert bb.decodable and bb.injected_byte_errors == [2]
    add(y, 2000, w)
    recs, frames, _ = check(lib, y, 1500, 5500, 5600, "rs")
    r = [r for r in recs if int(r["anchor"]) == 2240][0]
    assert int(r["fec_corrections"]) == 2 and frames[int(r["frame_first"])]["octets"] == frame and int(r["counters"][rm.CNT["BLOCKS_FEC_OK"]]) == 1


def test_noise_anchor_stops_at_the_header(lib):
    y = noise_ring(4096, 5)
    recs, _, _ = check(lib, y, 200, 3800, 4000, "noise, threshold 30", thr=30.0, K=16)
    assert len(recs) > 0 and any(int(r["stop"]) in HDR_STOPS for r in recs), [int(r["stop"]) for r in recs]


def test_limit(lib):
    y = noise_ring(RING, 6, sigma=0.002)
    w, frame, bb = burst(payload=40)
    add(y, 2000, w)
    full, _, _ = check(lib, y, 1500, 3000, 6000, "limit far")
    r0 = [r for r in full if int(r["anchor"]) == 2240][0]
    end = int(r0["end_sample"])
    assert end == 2240 + 10 * int(r0["nsym"]) and int(r0["frames_ok"]) == 1
    exact, frames, _ = check(lib, y, 1500, 3000, end, "limit exactly sufficient")
    r1 = [r for r in exact if int(r["anchor"]) == 2240][0]
    assert int(r1["frames_ok"]) == 1 and frames[int(r1["frame_first"])]["octets"] == frame
    short, frames, _ = check(lib, y, 1500, 3000, end - 1, "limit one sample short of the last symbol")
    r2 = [r for r in short if int(r["anchor"]) == 2240][0]
    assert int(r2["flags"]) & rm.TRUNCATED and int(r2["frames"]) == 0 and not np.any(r2["counters"]) and int(r2["tl_bits"]) == bb.tl_bits and int(r2["stop"]) == -1
    hdr, _, _ = check(lib, y, 1500, 2300, 2240 + 89, "limit inside the header")
    r3 = [r for r in hdr if int(r["anchor"]) == 2240][0]
    assert int(r3["flags"]) & rm.TRUNCATED and int(r3["tl_bits"]) == 0 and not np.any(r3["counters"])


def test_max_ppm_gate(lib):
    y = noise_ring(RING, 8, sigma=0.002)
    w, frame, _ = burst(payload=40, cfo=3e-3)                    # cycles per decimated sample: 315 Hz, some 2.3 ppm at 136.975 MHz
    add(y, 2000, w)
    open_, _, _ = check(lib, y, 1500, 5500, 5600, "gate off")
    r = [r for r in open_ if int(r["anchor"]) == 2240][0]
    ppm = abs(float(r["ppm_error"]))
    assert ppm > 1.0 and int(r["frames_ok"]) == 1
    above, _, _ = check(lib, y, 1500, 5500, 5600, "gate above", max_ppm=float(np.nextafter(np.float32(ppm), np.float32(np.inf))))
    assert int([r for r in above if int(r["anchor"]) == 2240][0]["frames_ok"]) == 1
    at, _, _ = check(lib, y, 1500, 5500, 5600, "gate at the figure itself", max_ppm=ppm)
    assert int([r for r in at if int(r["anchor"]) == 2240][0]["frames_ok"]) == 1
    below, _, _ = check(lib, y, 1500, 5500, 5600, "gate below", max_ppm=float(np.nextafter(np.float32(ppm), np.float32(0))))
    rb = [r for r in below if int(r["anchor"]) == 2240][0]
    assert int(rb["flags"]) & rm.PPM_REJECT and int(rb["frames"]) == 0 and not np.any(rb["counters"]) and int(rb["tl_bits"]) == 0


def test_range_from_sample_zero(lib):
    """Phi(n) = 0 for n < 0: the taps of the first 150 samples reach before the stream"""
    y = noise_ring(RING, 9, sigma=0.002)
    w, frame, _ = burst(payload=40)
    add(y, -140, w)                                              # the unique word ends at sample 100
    check(lib, y, 0, 3000, 3100, "from zero", thr=30.0, K=16)
    y2 = noise_ring(RING, 10, sigma=0.002)
    add(y2, 0, w)
    recs, frames, _ = check(lib, y2, 0, 3000, 3100, "burst behind sample zero")
    r = [r for r in recs if int(r["anchor"]) == 240][0]
    assert frames[int(r["frame_first"])]["octets"] == frame


def test_room(lib):
    y = noise_ring(RING, 12, sigma=0.002)
    w, frame, bb = burst(payload=40)
    add(y, 1000, w)
    add(y, 4000, w)
    cf, cp = rm.claim(bb.tl_bits)
    both, _, _ = check(lib, y, 500, 7000, 7100, "room for both", pf=2 * cf, pc=2 * cp)
    assert [int(r["frames_ok"]) for r in both if int(r["anchor"]) in (1240, 4240)] == [1, 1]
    one, frames, _ = check(lib, y, 500, 7000, 7100, "octets one short", pf=2 * cf, pc=2 * cp - 1)
    a, b = [r for r in one if int(r["anchor"]) in (1240, 4240)]
    assert int(a["frames_ok"]) == 1 and int(b["flags"]) & rm.NO_ROOM and int(b["frames"]) == 0 and int(b["tl_bits"]) == bb.tl_bits and not np.any(b["counters"])
    few, _, _ = check(lib, y, 500, 7000, 7100, "records one short", pf=2 * cf - 1, pc=2 * cp)
    assert int([r for r in few if int(r["anchor"]) == 4240][0]["flags"]) & rm.NO_ROOM
