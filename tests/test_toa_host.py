"""Burst timing on the host (dumpvdl2_amd/csrc/toa.h, toa_design.h).  The template is host code anyway; the kernel's per-burst steps -
the window through the ring mask, u[], a lag's sum by lane and tree level, peak and vertex, the record - are plain functions that the
library also builds for the CPU behind a test hook that needs no GPU: vdl2hip_debug_toa_burst.  The yardstick: tests/toa_model.py."""
import ctypes as C

import numpy as np
import pytest

import toa_model as tm
from dumpvdl2_amd import vdl2hip

E_INVAL, E_TOOBIG = -1, -4
RING = 4096


@pytest.fixture(scope="module")
def lib():
    L = vdl2hip.load_library()
    L.vdl2hip_debug_toa_burst.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def s32():
    return vdl2hip.toa_template()


def test_sizes_and_exports(lib):
    d = vdl2hip.BURST_TOA_DTYPE
    assert d.itemsize == 96 and d.fields["peak_sample"][1] == 32 and d.fields["toa_frac"][1] == 48 and d.fields["flags"][1] == 80 and d.fields["curve_off"][1] == 92
    assert C.sizeof(vdl2hip.ToaCfg) == 16 and C.sizeof(vdl2hip.ToaInfo) == 64
    for name in ("vdl2hip_toa_template", "vdl2hip_toa_enable", "vdl2hip_toa_disable", "vdl2hip_toa_info_get", "vdl2hip_toa_read"):
        assert name in vdl2hip.EXPORTS and hasattr(lib, name), name
    buf = np.zeros((151, 2), dtype=np.float32)
    assert lib.vdl2hip_toa_template(buf.ctypes.data, 150) == E_TOOBIG and lib.vdl2hip_toa_template(None, 151) == E_INVAL
    assert lib.vdl2hip_toa_template(buf.ctypes.data, 151) == 151


def test_template_against_numpy(s32):
    """each value equal to the float64 design's rounding or an adjacent float32; the symbol centres are the unique word's phases"""
    want = tm.design()
    assert s32.size == tm.TAPS
    for got, w in ((s32.real, want.real), (s32.imag, want.imag)):
        w32 = w.astype(np.float32)
        ok = (got == w32) | (got == np.nextafter(w32, np.float32(np.inf))) | (got == np.nextafter(w32, np.float32(-np.inf)))
        assert np.all(ok), np.flatnonzero(~ok)
    assert np.max(np.abs(s32[::10].astype(np.complex128) - np.exp(1j * tm.Q * np.pi / 4.0))) <= 1e-6


def plant(ring, at, amp=0.05, phase=0.7, cfo=0.0, frac=0.0, lead=40, trail=60):
    """the unique word's waveform with symbol 0's centre at sample at + frac of the ring (absolute index, wrapped), a constant-phase
    ramp ahead of it and a few more symbols behind, rotating by cfo rad per sample"""
    n = np.arange(-lead, tm.TAPS + trail, dtype=np.float64)
    w = np.zeros(n.size, dtype=np.complex128)
    ph = list(tm.Q * np.pi / 4.0)
    syms = [(-4 + i, 0.0) for i in range(4)] + [(i, ph[i]) for i in range(16)] + [(16 + i, ph[-1] + (i + 1) * 3 * np.pi / 4) for i in range(6)]
    for i, p in syms:
        w += np.exp(1j * p) * tm.pulse((n - frac - 10.0 * i) / 10.0)
    w *= amp * np.exp(1j * (phase + cfo * n))
    idx = (at + n.astype(np.int64)) % ring.shape[0]
    ring[idx, 0] += w.real.astype(np.float32)
    ring[idx, 1] += w.imag.astype(np.float32)


def noise_ring(seed, sigma=0.002):
    return (np.random.default_rng(seed).standard_normal((RING, 2)) * sigma).astype(np.float32)


def ring_reader(ring):
    def y_at(first, count):
        idx = (first + np.arange(count)) % ring.shape[0]
        return ring[idx, 0].astype(np.float64) + 1j * ring[idx, 1].astype(np.float64)
    return y_at


def run(lib, ring, first_symbol, dphi, max_lag, expect=0):
    rec = np.zeros(1, dtype=vdl2hip.BURST_TOA_DTYPE)
    W = max_lag or 8
    curve = np.full(2 * W + 1 + 4, np.nan, dtype=np.float32)
    ring = np.ascontiguousarray(ring)
    r = lib.vdl2hip_debug_toa_burst(ring.ctypes.data, ring.shape[0], first_symbol, dphi, max_lag, rec.ctypes.data, curve.ctypes.data, 2 * W + 1)
    assert r == expect, r
    assert np.all(np.isnan(curve[2 * W + 1:]))
    return rec[0], curve[:2 * W + 1]


def check(lib, s32, ring, first_symbol, dphi, max_lag, what):
    rec, curve = run(lib, ring, first_symbol, dphi, max_lag)
    assert int(rec["nlags"]) == 2 * (max_lag or 8) + 1 and int(rec["first_symbol"]) == first_symbol and np.float32(rec["dphi"]) == np.float32(dphi)
    worst = tm.check_record(rec, curve, s32, ring_reader(ring), what)
    print(f"{what}: peak_lag {int(rec['peak_lag'])} toa_frac {float(rec['toa_frac']):+.4f} rho {float(rec['rho']):.4f} cfo {float(rec['cfo_hz']):+.1f} Hz "
          f"flags {int(rec['flags'])} curve error {worst:.3f} of its bound")
    return rec, curve


@pytest.mark.parametrize("max_lag", (0, 1, 5, 32))
def test_planted_burst(lib, s32, max_lag):
    """a burst planted a fraction of a sample off the anchor, with a carrier offset 20 Hz beyond the slope: the curve within the bound
    of the model, every derived field exact from the hook's own curve - the exact checks - and the estimate where the burst was
    planted.  How near: the vertex of a parabola through three points of a peak that is no parabola is a few hundredths of a sample
    off (the float64 model: -0.06 here), and a slope that is off moves the peak of this unsymmetric waveform by 0.0053 sample per Hz
    (the model, +-130 Hz) - 0.11 for 20 Hz: a quarter of a sample tells a misplaced window (a whole sample) from both."""
    ring = noise_ring(7 + max_lag, 0.0005)
    cfo = 2.0 * np.pi * 250.0 / 105000.0
    plant(ring, 1000, cfo=cfo, frac=0.3)
    dphi = np.float32(10.0 * 2.0 * np.pi * 230.0 / 105000.0)
    rec, _ = check(lib, s32, ring, 1000 + 160, dphi, max_lag, f"W={max_lag or 8}")
    assert int(rec["flags"]) == 0 and abs(int(rec["peak_lag"]) + float(rec["toa_frac"]) - 0.3) < 0.25
    assert float(rec["rho"]) > 0.95 and abs(float(rec["cfo_hz"]) - 250.0) < 25.0


def test_window_wraps_the_ring(lib, s32):
    ring = noise_ring(11)
    at = 3 * RING + RING - 70                                     # the template straddles the ring's end
    plant(ring, at, cfo=-0.004, frac=-0.2)
    rec, _ = check(lib, s32, ring, at + 160 + 2, np.float32(-0.03), 8, "wrap")
    assert int(rec["flags"]) == 0 and abs(int(rec["peak_lag"]) + float(rec["toa_frac"]) + 2.2) < 0.25 and int(rec["peak_sample"]) == at


def test_early(lib, s32):
    """t0 - W < 0: zeros are taken for the samples before the stream's start"""
    ring = noise_ring(12)
    ring[RING - 64:] = 50.0                                       # what a mask without the rule would read
    plant(ring, 3, frac=0.1)
    rec, curve = check(lib, s32, ring, 3 + 160, np.float32(0.0), 8, "early")
    assert int(rec["flags"]) == tm.EARLY and int(rec["peak_lag"]) == 0 and float(curve.max()) < 100.0
    rec, _ = check(lib, s32, ring, 160 + 8, np.float32(0.0), 8, "not early")
    assert not int(rec["flags"]) & tm.EARLY


def test_edge(lib, s32):
    """a peak planted at +W"""
    ring = noise_ring(13, 0.0002)
    plant(ring, 2000 + 5)
    rec, _ = check(lib, s32, ring, 2000 + 160, np.float32(0.0), 5, "edge")
    assert int(rec["flags"]) == tm.EDGE and int(rec["peak_lag"]) == 5 and float(rec["toa_frac"]) == 0.0 and int(rec["peak_sample"]) == 2005


def test_all_zero_ring(lib, s32):
    ring = np.zeros((RING, 2), dtype=np.float32)
    rec, curve = check(lib, s32, ring, 1160, np.float32(0.01), 8, "zero")
    assert int(rec["flags"]) & tm.FLAT and float(rec["rho"]) == 0.0 and float(rec["toa_frac"]) == 0.0 and float(rec["energy"]) == 0.0 and not curve.any()
    assert int(rec["peak_lag"]) == -8                             # the lowest lag among equals


def test_refusals(lib):
    ring = noise_ring(14)
    rec = np.zeros(1, dtype=vdl2hip.BURST_TOA_DTYPE)
    curve = np.zeros(65, dtype=np.float32)
    f = lib.vdl2hip_debug_toa_burst
    assert f(ring.ctypes.data, RING, 1000, 0.0, 33, rec.ctypes.data, curve.ctypes.data, 65) == E_INVAL
    assert f(ring.ctypes.data, RING - 1, 1000, 0.0, 8, rec.ctypes.data, curve.ctypes.data, 65) == E_INVAL
    assert f(ring.ctypes.data, RING, 1000, 0.0, 8, rec.ctypes.data, curve.ctypes.data, 16) == E_TOOBIG
    assert f(None, RING, 1000, 0.0, 8, rec.ctypes.data, curve.ctypes.data, 65) == E_INVAL
