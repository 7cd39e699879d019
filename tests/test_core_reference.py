"""tests/core_reference.py (plain numpy restatements of vdl2_core.h's sync_metric, slice_symbol, parabola_vertex, ppm_of and
ppm_gate_threshold) against the host build of that source (tests/hostsim): bit for bit, on core_reference.py's own input sets.
tests/test_hostsim.py pins the host build to the oracle; this makes plain numpy a yardstick for any other build of these helpers."""
import ctypes as C

import numpy as np
import pytest

import core_reference as cr
import pyhostsim


@pytest.fixture(scope="module")
def hs():
    L = C.CDLL(pyhostsim.build())
    L.hostsim_metric_pairs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hostsim_slice.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.hostsim_vertex.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.hostsim_ppm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.hostsim_metric_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.hostsim_pi_below.restype = C.c_float
    L.hostsim_phase.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.hostsim_screen_guard.restype = C.c_float
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(a, b):
    """bit-equal, except that a NaN is a NaN whatever its sign and payload (0/0 is -nan on x86 and +nan elsewhere)"""
    a = np.asarray(a, dtype=np.float32); b = np.asarray(b, dtype=np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def test_constants_are_the_sources(hs):
    pr = np.zeros(16, dtype=np.float32); lrx = np.zeros(16, dtype=np.float32); den = np.zeros(1, dtype=np.float32)
    hs.hostsim_metric_tables(pr.ctypes.data, lrx.ctypes.data, den.ctypes.data)
    assert np.array_equal(bits(pr), bits(cr.PR_PHASE)) and np.array_equal(bits(lrx), bits(cr.LRX)) and bits(den)[0] == bits(cr.LR_DEN)
    assert np.float32(hs.hostsim_pi_below()) == cr.PI_BELOW and float(cr.PI_BELOW) < np.pi < float(np.float32(np.pi))


def test_phase_inputs_hold_what_they_promise(hs):
    """core_reference.phase_inputs(): tests/test_phase.py's condition for the host build's phase_of() holds on the whole set, and the
    set does hold the signed zeros, the subnormals and the k/16 switch points"""
    xy, where = cr.phase_inputs()
    out = np.empty(len(xy), dtype=np.float32)
    hs.hostsim_phase(xy.ctypes.data, out.ctypes.data, len(xy))
    ref = np.arctan2(xy[:, 1].astype(np.float64), xy[:, 0].astype(np.float64)).astype(np.float32)
    diff = bits(out) != bits(ref)
    assert diff.sum() <= 2, f"{diff.sum()} of {len(xy)} phases differ from libm after narrowing"
    assert np.all(np.abs(out[diff].astype(np.float64) - ref[diff]) <= np.spacing(np.abs(ref[diff])))
    assert sorted(bits(xy[where["zeros"]]).reshape(-1, 2).tolist()) == sorted([[0, 0], [0, 1 << 31], [1 << 31, 0], [1 << 31, 1 << 31]])
    sub = np.abs(xy[where["subnormal"]])
    assert sub.min() == np.float32(1e-45) and (sub.max(axis=1) < np.float32(2.0 ** -126)).any()
    sw = np.abs(xy[where["switch"]]).astype(np.float64)
    r = sw.min(axis=1) / sw.max(axis=1)
    for k in range(17):
        near = np.abs(r - k / 16) < 2.5e-7                 # within two floats of the switch point
        assert (k == 0 or (near & (r < k / 16)).any()) and (r == k / 16).any() and (k == 16 or (near & (r > k / 16)).any()), k
    assert np.float32(hs.hostsim_screen_guard()) == cr.SCREEN_GUARD


def test_sync_metric_bit_for_bit(hs):
    ph, ndesign = cr.metric_windows()
    n = len(ph)
    exact = np.zeros(n, dtype=np.float32); slope = np.zeros(n, dtype=np.float32); screen = np.zeros(n, dtype=np.float32)
    hs.hostsim_metric_pairs(ph.ctypes.data, n, exact.ctypes.data, slope.ctypes.data, screen.ctypes.data)
    p, s = cr.sync_metric(ph)
    d = np.flatnonzero((bits(p) != bits(exact)) | (bits(s) != bits(slope)))
    assert d.size == 0, f"{d.size} of {n} windows differ, first {d[:5]}: {p[d[:3]]} / {exact[d[:3]]}"
    # the added windows do sit on the unwrap decision: tap differences exactly at +-kPiBelow and one float either side of it
    td = cr.tap_differences(ph[ndesign:])
    for t in cr.ulp_neighbours(cr.PI_BELOW):
        assert (td == t).any() and (td == -t).any(), float(t)
    assert (exact < 4).sum() > 50000 and ((exact > 3) & (exact < 5)).sum() > 2000


def test_slice_symbol_bit_for_bit(hs):
    a = cr.slice_inputs()
    n = len(a)
    idx = np.zeros(n, dtype=np.int32); neg = np.zeros(n, dtype=np.int32)
    hs.hostsim_slice(a.ctypes.data, n, idx.ctypes.data, neg.ctypes.data)
    ri, rn = cr.slice_symbol(a[:, 0], a[:, 1], a[:, 2])
    d = np.flatnonzero((ri != idx) | (rn != neg))
    assert d.size == 0, f"{d.size} of {n} decisions differ, first {a[d[:3]]}: {ri[d[:3]]} {rn[d[:3]]} / {idx[d[:3]]} {neg[d[:3]]}"
    assert neg.sum() > 1000 and all((idx == k).sum() > 1000 for k in range(8))           # the negative-index path and every symbol are populated
    # the ties are in the set: steps whose quotient by pi/4 is exactly a whole number and a half
    dphi = (a[:, 0] - a[:, 1]) - a[:, 2]
    q = (dphi.astype(np.float64) / (np.pi / 4)).astype(np.float32)
    assert (np.abs(q - np.floor(q)) == 0.5).sum() >= 20


def test_parabola_vertex_bit_for_bit(hs):
    a = cr.vertex_inputs()
    out = np.zeros(len(a), dtype=np.float32)
    hs.hostsim_vertex(a.ctypes.data, len(a), out.ctypes.data)
    ref = cr.parabola_vertex(a[:, 0], a[:, 1], a[:, 2])
    d = np.flatnonzero(~same_floats(ref, out))
    assert d.size == 0, f"{d.size} of {len(a)} vertices differ, first {a[d[:3]]}: {ref[d[:3]]} / {out[d[:3]]}"
    assert np.isnan(out).sum() >= 1000 and np.isinf(out).sum() > 0                       # y1 = y2 = y3 (0/0) and a = 0 (x/0)


def test_ppm_gate_bit_for_bit(hs):
    from dumpvdl2_amd import synth
    vd, fr, mp = cr.ppm_inputs(synth.channel_plan(256))
    n = len(vd)
    ppm = np.zeros(n, dtype=np.float32); thr = np.zeros(n, dtype=np.float32)
    hs.hostsim_ppm(vd.ctypes.data, fr.ctypes.data, mp.ctypes.data, n, ppm.ctypes.data, thr.ctypes.data)
    rp = cr.ppm_of(vd, fr); rt = cr.ppm_gate_threshold(fr, mp)
    d = np.flatnonzero(~same_floats(rp, ppm) | (bits(rt) != bits(thr)))
    assert d.size == 0, f"{d.size} of {n} differ, first {vd[d[:3]]} {fr[d[:3]]}: {rp[d[:3]]} {rt[d[:3]]} / {ppm[d[:3]]} {thr[d[:3]]}"
    # the threshold is the gate: |ppm_of| passes at it and fails at the next float up
    assert np.all(np.abs(cr.ppm_of(thr, fr)) <= mp) and np.all(np.abs(cr.ppm_of(np.nextafter(thr, np.float32(np.inf)), fr)) > mp)
