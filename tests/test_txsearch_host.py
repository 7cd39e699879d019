"""The preamble search's kernels on the host (dumpvdl2_amd/csrc/txsearch.h).  Their per-piece steps - the phases of a piece once per
sample, the metric and the lane's best, the lock test, the fixed tree over 256 lanes, the pieces combined in ascending order - are
plain functions that the library also builds for the CPU, behind a test hook that needs no GPU:
  - vdl2hip_debug_txsearch_range: one record's first_sample .. last_sample over a ring -> the device-written fields of its record.
The yardstick: tests/txsearch_model.py.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import txsearch_model as tm
from dumpvdl2_amd import synth, vdl2hip

E_INVAL = -1
FREQ = 136975000
SMALL, BIG = 1024, 131072


@pytest.fixture(scope="module")
def lib():
    L = vdl2hip.load_library()
    L.vdl2hip_debug_txsearch_range.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p]
    return L


def noise_ring(n, seed, sigma=0.01):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * sigma).astype(np.float32)


def burst_wave(seed=20261020, payload=40):
    rng = np.random.default_rng(seed)
    body = rng.integers(0, 256, size=payload, dtype=np.uint8).tobytes()
    bb = synth.build_burst([synth.make_avlc_frame(body)])
    return synth.modulate(bb.symbols, 10, start_phase=0.7).astype(np.complex64)


def run(lib, y, first, last, freq=FREQ, expect=0):
    rec = np.zeros(1, dtype=vdl2hip.TXS_DTYPE)
    y = np.ascontiguousarray(y, dtype=np.float32)
    r = lib.vdl2hip_debug_txsearch_range(y.ctypes.data, y.shape[0], first, last, freq, rec.ctypes.data)
    assert r == expect, r
    return rec[0]


def check(lib, y, first, last, freq=FREQ, label=""):
    rec = run(lib, y, first, last, freq)
    want, ps = tm.search(tm.ring_get(y), first, last, freq)
    tm.check(rec, want, label or f"{first}..{last}")
    assert (int(rec["chan"]), int(rec["freq"]), int(rec["first_bin"])) == (0, freq, 0)
    assert (int(rec["frames"]), int(rec["frames_ok"]), int(rec["why"]), int(rec["reserved"]), int(rec["reserved2"])) == (0, 0, 0, 0, 0)
    return rec, want, ps


@pytest.fixture(scope="module")
def small():
    return noise_ring(SMALL, 20261020)


@pytest.fixture(scope="module")
def big():
    """noise, and a synthetic burst at sample 70 000 under a little of it"""
    y = noise_ring(BIG, 20261021, sigma=0.002)
    w = burst_wave() * np.float32(0.05)
    y[70000:70000 + w.size, 0] += w.real
    y[70000:70000 + w.size, 1] += w.imag
    return y


def test_record_size():
    assert vdl2hip.TXS_DTYPE.itemsize == 96 and vdl2hip.TXS_DTYPE.fields["flags"][1] == 72 and vdl2hip.TXS_DTYPE.fields["why"][1] == 84
    assert C.sizeof(vdl2hip.TxsearchCfg) == 16 and C.sizeof(vdl2hip.TxsearchInfo) == 40


@pytest.mark.parametrize("ring", [SMALL, BIG])
@pytest.mark.parametrize("length", [1, 3, 4, 1023, 1024, 1025, 57344])
def test_lengths(lib, small, big, ring, length):
    """one sample (no lock point can exist), up to the lock test's reach and one beyond, a piece less one / exactly / plus one, the
    longest range (56 pieces; on the small ring it goes round 56 times)"""
    y = small if ring == SMALL else big
    first = 3000
    rec, want, _ = check(lib, y, first, first + length - 1)
    assert int(rec["search_first"]) == first and not int(rec["flags"]) & tm.CLIPPED
    if length <= 3:
        assert int(rec["lock_points"]) == 0 and int(rec["first_lock"]) == -1


def test_clipped(lib, big):
    rec, want, _ = check(lib, big, 20000, 20000 + 57344)
    assert int(rec["flags"]) == tm.CLIPPED and int(rec["search_first"]) == 20001
    rec, _, _ = check(lib, big, 1000, 100000)
    assert int(rec["flags"]) == tm.CLIPPED and int(rec["search_first"]) == 100000 - 57343


@pytest.mark.parametrize("ring,first,last", [(SMALL, 900, 1300), (BIG, BIG - 700, BIG + 2100), (BIG, 3 * BIG - 100, 3 * BIG + 50)])
def test_wrap(lib, small, big, ring, first, last):
    """ranges that cross the ring's wrap: every index is masked per element"""
    check(lib, small if ring == SMALL else big, first, last)


@pytest.mark.parametrize("last", [0, 2, 149, 152, 153, 1500])
def test_stream_start(lib, small, last):
    """first = 0: the taps before the stream's first sample are phases of 0, not the ring's last samples"""
    rec, want, (p, s) = check(lib, small, 0, last)
    # (the ring read at the masked negative indices instead gives another p(0): the case is not vacuous)
    c = small.view(np.complex64).reshape(-1)
    ph = np.arctan2(c.imag.astype(np.float64), c.real.astype(np.float64)).astype(np.float32)
    p_wrong, _ = tm.cr.sync_metric(ph[(np.arange(-150, 1, 10)) & (SMALL - 1)][None, :])
    assert p_wrong[0] != p[0]


def test_constant_carrier(lib):
    """every p(n) is equal: the best is the range's first sample, whichever lane and piece holds it"""
    y = np.zeros((BIG, 2), dtype=np.float32)
    y[:, 0] = 0.03; y[:, 1] = 0.04
    rec, want, (p, s) = check(lib, y, 5000, 5000 + 3000)
    assert np.all(p.view(np.uint32) == p.view(np.uint32)[0])
    assert int(rec["best_sample"]) == 5000 and int(rec["lock_points"]) == 0
    assert float(rec["best_pherr"]) > 4.0 and int(rec["below_thr"]) == 0


def test_burst(lib, big):
    """a synthetic burst: the preamble is found, and the reference would have locked whatever its grid's phase"""
    rec, want, (p, s) = check(lib, big, 69000, 72500)
    assert float(rec["best_pherr"]) < 4.0 and int(rec["lock_phases"]) == 7
    # the unique word's last symbol: 5 ramp symbols, 16 of the unique word, the pulse's 4-symbol run-in
    assert abs(int(rec["best_sample"]) - (70000 + (4 + 5 + 15) * 10)) <= 2
    assert int(rec["first_lock"]) > int(rec["best_sample"]) - 30 and int(rec["lock_points"]) >= 3
    assert abs(float(rec["best_ppm"])) < 0.5


def test_noise(lib):
    """noise alone, the seed committed here: the model itself says no lock point, and the library says what the model says"""
    y = noise_ring(BIG, 20261023)
    want, _ = tm.search(tm.ring_get(y), 10000, 10000 + 20000, FREQ)
    assert want["lock_points"] == 0 and want["below_thr"] == 0 and want["first_lock"] == -1 and want["lock_phases"] == 0
    rec, _, _ = check(lib, y, 10000, 10000 + 20000)
    assert float(rec["best_pherr"]) > 4.0 and int(rec["best_sample"]) >= 10000


def test_noise_false_lock(lib):
    """... and noise that does come within the threshold once in 20 000 samples (another seed; the model says so): a single lock
    point, on a single phase of the grid"""
    y = noise_ring(BIG, 20261022)
    want, _ = tm.search(tm.ring_get(y), 10000, 10000 + 20000, FREQ)
    assert want["lock_points"] == 1 and want["below_thr"] == 1
    rec, _, _ = check(lib, y, 10000, 10000 + 20000)
    assert int(rec["first_lock"]) == int(rec["best_sample"]) + 3 and int(rec["lock_phases"]) == 1 << (int(rec["first_lock"]) % 3)


def test_nan_sample(lib, big):
    """a NaN sample makes a NaN of the 16 windows that hold it: none of them is the best, below the threshold or a lock point"""
    y = big.copy()
    y[70240, 0] = np.nan                                   # (inside the burst's unique word: the best of the clean ring goes)
    rec, want, (p, s) = check(lib, y, 69000, 72500)
    assert np.count_nonzero(np.isnan(p)) == 16
    clean = run(lib, big, 69000, 72500)
    assert not np.isnan(rec["best_pherr"]) and int(rec["best_sample"]) != int(clean["best_sample"])
    y = np.full((SMALL, 2), np.nan, dtype=np.float32)
    rec, want, _ = check(lib, y, 200, 900)
    assert int(rec["best_sample"]) == -1 and np.isposinf(rec["best_pherr"]) and float(rec["best_slope"]) == 0.0 and float(rec["best_ppm"]) == 0.0
    assert (int(rec["lock_points"]), int(rec["below_thr"]), int(rec["first_lock"]), int(rec["lock_phases"])) == (0, 0, -1, 0)


def test_partition_independent(lib, big):
    """the same samples give the same p whichever piece and lane evaluates them: a range and the range that begins one sample later
    (every sample in another lane, the pieces cut elsewhere) agree on what they share"""
    a = run(lib, big, 69000, 72500)
    b = run(lib, big, 68999, 72500)
    assert same(a, b, ("best_sample", "best_pherr", "best_slope", "best_ppm", "search_last"))
    want_a, (pa, _) = tm.search(tm.ring_get(big), 69000, 72500, FREQ)
    want_b, (pb, _) = tm.search(tm.ring_get(big), 68999, 72500, FREQ)
    assert np.array_equal(pa.view(np.uint32), pb[1:].view(np.uint32))


def same(a, b, keys):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def test_validation(lib, small):
    rec = np.zeros(1, dtype=vdl2hip.TXS_DTYPE)
    y = small
    f = lib.vdl2hip_debug_txsearch_range
    assert f(None, SMALL, 0, 10, FREQ, rec.ctypes.data) == E_INVAL
    assert f(y.ctypes.data, SMALL, 0, 10, FREQ, None) == E_INVAL
    assert f(y.ctypes.data, 1000, 0, 10, FREQ, rec.ctypes.data) == E_INVAL          # not a power of two
    assert f(y.ctypes.data, 0, 0, 10, FREQ, rec.ctypes.data) == E_INVAL
    assert f(y.ctypes.data, 1, 0, 10, FREQ, rec.ctypes.data) == E_INVAL
    assert f(y.ctypes.data, SMALL, -1, 10, FREQ, rec.ctypes.data) == E_INVAL
    assert f(y.ctypes.data, SMALL, 11, 10, FREQ, rec.ctypes.data) == E_INVAL         # last < first
    assert f(y.ctypes.data, SMALL, 0, 10, 0, rec.ctypes.data) == E_INVAL
    assert not rec.view(np.uint8).any(), "a refused call writes nothing"
    assert f(y.ctypes.data, SMALL, 10, 10, FREQ, rec.ctypes.data) == 0
