"""The transmission capture's kernels on the host (dumpvdl2_amd/csrc/txcap.h).  Their per-record and per-piece steps - the window and
the room, a piece's samples into the padded staging buffer, the groups' overlapping segments through the input monitor's transform
pass by pass, the float64 sums of rounds, groups and pieces in their fixed order - are plain functions that the library also builds
for the CPU, behind test hooks that need no GPU:
  - vdl2hip_debug_txcap_plan: the log's records of one feed -> the records as the device writes them, the piece offsets, the pool in use
  - vdl2hip_debug_txcap_spectrum: one record's first_sample .. last_sample over a ring -> power[], segments
and vdl2hip_txcap_measure() is host code anyway.  The yardstick: tests/txcap_model.py."""
import ctypes as C

import numpy as np
import pytest

import txcap_model as cm
from dumpvdl2_amd import vdl2hip

E_INVAL = -1
SMALL, BIG = 1024, 131072
NFFTS = (64, 128, 256, 512, 1024)


@pytest.fixture(scope="module")
def lib():
    L = vdl2hip.load_library()
    L.vdl2hip_debug_txcap_plan.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(vdl2hip.TxcapCfg), C.c_void_p, C.c_void_p, C.c_void_p]
    L.vdl2hip_debug_txcap_spectrum.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def noise_ring(n, seed, sigma=0.01):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * sigma).astype(np.float32)


@pytest.fixture(scope="module")
def small():
    return noise_ring(SMALL, 20261021)


@pytest.fixture(scope="module")
def big():
    """noise, a strong tone at +9 kHz over a stretch of it, and a few large samples (the bound is relative to each segment's own norm)"""
    y = noise_ring(BIG, 20261022, sigma=0.002)
    n = np.arange(30000, 60000)
    t = 0.2 * np.exp(2j * np.pi * 9000.0 / 105000.0 * n)
    y[30000:60000, 0] += t.real.astype(np.float32)
    y[30000:60000, 1] += t.imag.astype(np.float32)
    y[90000:90010] *= 300
    return y


def test_record_size():
    d = vdl2hip.TXC_DTYPE
    assert d.itemsize == 80 and d.fields["win_first"][1] == 16 and d.fields["spec_off"][1] == 40 and d.fields["iq_count"][1] == 48 and d.fields["frames"][1] == 64
    assert C.sizeof(vdl2hip.TxcapCfg) == 40 and C.sizeof(vdl2hip.TxcapInfo) == 88 and C.sizeof(vdl2hip.TxShape) == 48


# ---------------------------------------------------------------- the plan
def tx_records(spans, flags=None, chan=3, freq=136975000):
    tx = np.zeros(len(spans), dtype=vdl2hip.TX_DTYPE)
    for i, (a, b) in enumerate(spans):
        tx[i]["chan"], tx[i]["freq"], tx[i]["first_bin"], tx[i]["first_sample"], tx[i]["last_sample"] = chan + i % 2, freq + i % 2, 7 + i, a, b
        tx[i]["flags"] = flags[i] if flags else 0
    return tx


def run_plan(lib, tx, expect=0, **kw):
    cfg = vdl2hip.TxcapCfg(struct_size=40, **kw)
    recs = np.zeros(max(1, len(tx)), dtype=vdl2hip.TXC_DTYPE)
    poff = np.zeros(len(tx) + 1, dtype=np.uint32)
    out = np.zeros(2, dtype=np.uint64)
    r = lib.vdl2hip_debug_txcap_plan(tx.ctypes.data, len(tx), C.byref(cfg), recs.ctypes.data, poff.ctypes.data, out.ctypes.data)
    assert r == expect, r
    return recs[:len(tx)], poff, int(out[0]), int(out[1])


def check_plan(lib, tx, **kw):
    recs, poff, used, pieces = run_plan(lib, tx, **kw)
    want, wused = cm.plan(tx, kw["flags"], kw.get("pre_samples", 0), kw.get("post_samples", 0), kw.get("max_iq_samples", 0), kw.get("nfft", 0),
                          kw.get("pool_samples", 0), kw.get("pool_spectra", 0))
    n = kw.get("nfft", 0) or 256
    at = 0
    for i, (g, w) in enumerate(zip(recs, want)):
        for k in cm.INT_FIELDS:
            assert int(g[k]) == w[k], (i, k, int(g[k]), w[k])
        assert int(g["iq_off"]) == w["iq_off"] and int(g["spec_off"]) == (w["spec"] * n if w["spec"] is not None else 0), i
        assert (int(g["frames"]), int(g["frames_ok"]), g["reserved"].tolist()) == (0, 0, [0, 0])
        assert int(poff[i]) == at
        at += -(-w["segments"] // (8192 // n))
    assert (used, pieces, int(poff[len(tx)])) == (wused, at, at)
    return recs


SPANS = [(0, 63), (100, 227), (1000, 1191), (5000, 5000 + 57343), (70000, 70000 + 57344), (200000, 200000 + 70000), (300000, 300999), (300500, 300300)]


@pytest.mark.parametrize("nfft", (0,) + NFFTS)
def test_plan(lib, nfft):
    """windows at the stream's start, of odd and even length, the longest extent that is not clipped (its window is, by pre) and the
    shortest that is, a partial record nothing was seen of (last_sample so far before first_sample that the window is empty), and every
    transform size"""
    tx = tx_records(SPANS, flags=[0, 0, 1, 0, 0, 1, 0, 1])
    recs = check_plan(lib, tx, flags=3, pre_samples=100, post_samples=64, nfft=nfft)
    assert [bool(int(r["flags"]) & cm.CLIPPED) for r in recs] == [False, False, False, True, True, True, False, False]
    assert int(recs[0]["win_first"]) == 0 and int(recs[1]["win_first"]) == 0 and int(recs[2]["win_first"]) == 900
    assert int(recs[3]["win_first"]) == 5000 and int(recs[4]["win_first"]) == 70001 and int(recs[7]["iq_count"]) == 0
    assert [int(r["flags"]) & cm.PARTIAL for r in recs] == [0, 0, 1, 0, 0, 1, 0, 1]
    check_plan(lib, tx, flags=1, pre_samples=4096, post_samples=4096)
    check_plan(lib, tx, flags=2, nfft=nfft)


def test_plan_clipped_by_pre_only(lib):
    """first - pre lies further back than last - 57 343 while first does not: the window is clipped, the extent is not"""
    recs = check_plan(lib, tx_records([(100000, 100000 + 57000)]), flags=3, pre_samples=1000)
    assert int(recs[0]["flags"]) == cm.CLIPPED and int(recs[0]["win_first"]) == 100000 + 57000 - 57343 and int(recs[0]["segments"]) == (57001 - 256) // 128 + 1


def test_plan_room(lib):
    tx = tx_records([(1000 * i, 1000 * i + 299 + i % 2) for i in range(1, 8)])
    recs = check_plan(lib, tx, flags=3, pool_samples=700, pool_spectra=2, nfft=128)
    assert [bool(int(r["flags"]) & cm.NO_ROOM) for r in recs] == [False, False] + [True] * 5
    assert [bool(int(r["flags"]) & cm.NO_SPECTRUM) for r in recs] == [False, False] + [True] * 5
    recs = check_plan(lib, tx, flags=1, max_iq_samples=150, pool_samples=451)
    assert [int(r["iq_count"]) for r in recs] == [150, 150, 150, 0, 0, 0, 0] and all(int(r["flags"]) & cm.TRUNCATED for r in recs)
    check_plan(lib, tx, flags=1, max_iq_samples=300)             # (the limit bites every other window)
    many = tx_records([(500 * i, 500 * i + 120) for i in range(700)])
    check_plan(lib, many, flags=3, nfft=64, pool_spectra=300, pool_samples=50000)


def test_plan_arguments(lib):
    tx = tx_records(SPANS[:2])
    run_plan(lib, tx, expect=E_INVAL, flags=3, nfft=100)
    run_plan(lib, tx, expect=E_INVAL, flags=3, nfft=2048)
    run_plan(lib, tx, expect=E_INVAL, flags=3, pre_samples=4097)


# ---------------------------------------------------------------- the spectrum
def run_spectrum(lib, y, first, last, nfft, window=vdl2hip.WIN_HANN, expect=0):
    y = np.ascontiguousarray(y, dtype=np.float32)
    power = np.full(max(nfft or 256, 64) + 8, np.nan, dtype=np.float32)
    seg = C.c_uint32(0xffffffff)
    r = lib.vdl2hip_debug_txcap_spectrum(y.ctypes.data, y.shape[0], first, last, nfft, window, power.ctypes.data, C.byref(seg))
    assert r == expect, r
    if expect == 0:
        assert np.all(np.isnan(power[nfft or 256:])), "a store beyond power[nfft]"
    return power[:nfft or 256], seg.value


def check_spectrum(lib, y, first, last, nfft, window=vdl2hip.WIN_HANN, label=""):
    power, S = run_spectrum(lib, y, first, last, nfft, window)
    w = vdl2hip.spectrum_window(nfft, window)
    want_S = cm.segments(min(last - first + 1, cm.SPAN), nfft)
    assert S == want_S, (label, S, want_S)
    worst = cm.check_spectrum(power, cm.ring_get(y), first, last, nfft, w, label or f"{first}..{last} N={nfft}")
    return power, S, worst


@pytest.mark.parametrize("length,S", [(64, 0), (127, 0), (128, 1), (191, 1), (192, 2), (256, 3)])
def test_short_extents(lib, small, length, S):
    power, got, _ = check_spectrum(lib, small, 3000, 3000 + length - 1, 128)
    assert got == S and (S or not power.any())


@pytest.mark.parametrize("nfft", NFFTS)
def test_piece_boundaries(lib, big, nfft):
    """a piece is 8192 / N segments, a round 1024 / N of them: one segment less, exactly and one more than a round and than a piece,
    several pieces with a ragged last one, the longest extent"""
    q, g, h = 8192 // nfft, 1024 // nfft, nfft // 2
    worst = 0.0
    for S in sorted({1, g - 1, g, g + 1, q - 1, q, q + 1, 3 * q + g + 1} - {0}):
        length = (S - 1) * h + nfft + (S % 3)                     # (a few samples over: they belong to no segment)
        _, got, wr = check_spectrum(lib, big, 29000, 29000 + length - 1, nfft)
        assert got == S
        worst = max(worst, wr)
    _, S, wr = check_spectrum(lib, big, 20000, 20000 + 70000, nfft)
    assert S == (57344 - nfft) // h + 1
    print(f"N={nfft}: largest error / bound {max(worst, wr):.3f}")


@pytest.mark.parametrize("window", [vdl2hip.WIN_RECT, vdl2hip.WIN_HANN, vdl2hip.WIN_BH4])
def test_windows_and_large_samples(lib, big, window):
    check_spectrum(lib, big, 85000, 95000, 256, window)
    check_spectrum(lib, big, 85000, 95000, 128, window)


@pytest.mark.parametrize("ring,first,last", [(SMALL, 900, 1300), (SMALL, 0, 5000), (BIG, BIG - 700, BIG + 2100), (BIG, 3 * BIG - 5000, 3 * BIG + 5000)])
def test_wrap(lib, small, big, ring, first, last):
    """extents that cross the ring's wrap (on the small ring a piece goes round four times): every index is masked per element"""
    for nfft in (64, 256, 1024):
        check_spectrum(lib, small if ring == SMALL else big, first, last, nfft)


def test_same_samples_same_bytes(lib, big):
    """the same samples at another place of the stream, and across the ring's wrap, give the same bytes: the order of the float64
    additions is a function of the segment count alone"""
    a, _, _ = check_spectrum(lib, big, 30000, 49999, 256)
    moved = np.roll(big, 777 - 30000 + BIG - 5000, axis=0)          # sample 30000 now sits at BIG - 5000 + 777: the extent wraps
    b, _ = run_spectrum(lib, moved, 3 * BIG - 5000 + 777, 3 * BIG - 5000 + 777 + 19999, 256)
    assert a.tobytes() == b.tobytes()


def test_spectrum_arguments(lib, small):
    run_spectrum(lib, small, 0, 500, 100, expect=E_INVAL)
    run_spectrum(lib, small, 0, 500, 2048, expect=E_INVAL)
    run_spectrum(lib, small, 0, 500, 256, window=3, expect=E_INVAL)
    run_spectrum(lib, small, 10, 5, 256, expect=E_INVAL)
    assert run_spectrum(lib, small, 0, 999, 0)[1] == cm.segments(1000, 256)


@pytest.mark.parametrize("hz", [3000.0, -3000.0, 9000.0])
def test_orientation(lib, hz):
    """a tone at the channel frequency + hz peaks in bin N / 2 + round(hz N / 105000); centroid and peak carry the planted sign"""
    n = np.arange(8192)
    t = 0.1 * np.exp(2j * np.pi * hz / 105000.0 * n)
    y = np.stack([t.real, t.imag], axis=1).astype(np.float32)
    for nfft in NFFTS:
        power, _, _ = check_spectrum(lib, y, 100, 6000, nfft)
        want = nfft // 2 + int(round(hz * nfft / 105000.0))
        assert int(np.argmax(power)) == want, (nfft, int(np.argmax(power)), want)
        m = vdl2hip.txcap_measure(power)
        assert m == cm.measure(power) and m["peak_bin"] == want
        assert np.sign(m["peak_hz"]) == np.sign(hz) and np.sign(m["centroid_hz"]) == np.sign(hz)
        assert abs(m["centroid_hz"] - hz) < 105000.0 / nfft and abs(m["peak_hz"] - hz) <= 0.5 * 105000.0 / nfft + 1e-9
    # the model's own float64 spectrum of the same tone, narrowed: the same answers
    p64, _, _ = cm.spectrum64(cm.ring_get(y), 100, 6000, 256, vdl2hip.spectrum_window(256))
    m = vdl2hip.txcap_measure(p64.astype(np.float32))
    assert m == cm.measure(p64.astype(np.float32)) and np.sign(m["centroid_hz"]) == np.sign(hz) == np.sign(m["peak_hz"])


# ---------------------------------------------------------------- the four figures
def test_measure_synthetic():
    rng = np.random.default_rng(5)
    for nfft in NFFTS:
        zero = np.zeros(nfft, dtype=np.float32)
        assert vdl2hip.txcap_measure(zero) == cm.measure(zero) == dict(total=0.0, peak_hz=0.0, centroid_hz=0.0, obw_hz=0.0, peak_bin=0, obw_lo=0, obw_hi=0)
        for k in (0, 1, nfft // 2, nfft - 1):
            one = zero.copy()
            one[k] = 3.5
            m = vdl2hip.txcap_measure(one)
            assert m == cm.measure(one) and (m["peak_bin"], m["obw_lo"], m["obw_hi"]) == (k, k, k) and m["obw_hz"] == 105000.0 / nfft
            assert m["centroid_hz"] == m["peak_hz"] == (k - nfft // 2) * 105000.0 / nfft
        tie = zero.copy()
        tie[[5, 9, nfft - 3]] = 2.0
        m = vdl2hip.txcap_measure(tie)
        assert m == cm.measure(tie) and m["peak_bin"] == 5 and (m["obw_lo"], m["obw_hi"]) == (5, nfft - 3)
        for _ in range(4):
            p = (rng.random(nfft) ** 8).astype(np.float32) * np.float32(10.0 ** rng.uniform(-12, 3))
            assert vdl2hip.txcap_measure(p) == cm.measure(p)
        flat = np.ones(nfft, dtype=np.float32)
        m = vdl2hip.txcap_measure(flat)
        assert m == cm.measure(flat) and m["centroid_hz"] == -0.5 * 105000.0 / nfft


def test_measure_arguments():
    L = vdl2hip.load_library()
    p = np.ones(256, dtype=np.float32)
    out = vdl2hip.TxShape()
    assert L.vdl2hip_txcap_measure(None, 256, C.byref(out)) == E_INVAL and L.vdl2hip_txcap_measure(p.ctypes.data, 256, None) == E_INVAL
    for bad in (0, 32, 100, 2048):
        assert L.vdl2hip_txcap_measure(p.ctypes.data, bad, C.byref(out)) == E_INVAL
    assert L.vdl2hip_txcap_measure(p.ctypes.data, 256, C.byref(out)) == 0 and out.total == 256.0
