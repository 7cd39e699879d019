"""The DEVICE builds of vdl2_core.h's element-wise pieces (the `#if VDL2_DEVICE_PASS` sides, as hipcc compiles them for the GPU), through
the test hook vdl2hip_debug_core_probe (kernels.h: k_core_probe - one lane per element, every helper called as the product calls it),
against plain references: libm's atan2 in float64, float64 arithmetic, and tests/core_reference.py's numpy restatements (which
tests/test_core_reference.py holds bit for bit to the host build, itself pinned to the oracle).  The host build is only a second witness
here.  Every figure is printed before it is asserted; profiles/core_probe_device.txt keeps the measured ones.

Wall time of the module on an MI355X: see profiles/core_probe_device.txt."""
import ctypes as C

import numpy as np
import pytest

import core_reference as cr
import pyhostsim

pytestmark = pytest.mark.gpu
F32 = np.float32
TINY = F32(2.0 ** -126)                  # smallest normal float


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()
    return vdl2hip


@pytest.fixture(scope="module")
def L(vh):
    return vh.load_library()


@pytest.fixture(scope="module")
def hs():
    H = C.CDLL(pyhostsim.build())
    H.hostsim_phase.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    H.hostsim_phase_fast.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    H.hostsim_screen_guard.restype = C.c_float
    H.hostsim_metric_pairs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    H.hostsim_metric_early.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    return H


@pytest.fixture(scope="module")
def phase_set():
    xy, where = cr.phase_inputs()
    xy.setflags(write=False)
    return xy, where


@pytest.fixture(scope="module")
def windows():
    ph, ndesign = cr.metric_windows()
    ph.setflags(write=False)
    exact, slope = cr.sync_metric(ph)
    return ph, ndesign, exact, slope


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_floats(a, b):
    """bit-equal, except that a NaN is a NaN whatever its sign and payload"""
    a = np.asarray(a, dtype=F32); b = np.asarray(b, dtype=F32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def host(fn, xy):
    out = np.empty(len(xy), dtype=F32)
    fn(xy.ctypes.data, out.ctypes.data, len(xy))
    return out


def test_phase_of_is_libm_after_narrowing(L, hs, phase_set):
    xy, where = phase_set
    dev = cr.device_probe(L, "phase", xy)[:, 0]
    ref = np.arctan2(xy[:, 1].astype(np.float64), xy[:, 0].astype(np.float64)).astype(F32)
    zero = (xy[:, 0] == 0) & (xy[:, 1] == 0)
    nz = ~zero
    diff = nz & (bits(dev) != bits(ref))
    print(f"device phase_of: {diff.sum()} of {nz.sum()} narrowings differ from libm")
    # tests/test_phase.py's condition for the host build, the same cap: at most 2 per 4 10^6, one float apart
    assert diff.sum() <= 2, f"{diff.sum()} of {nz.sum()} phases differ from libm after narrowing: {xy[diff][:5]} {dev[diff][:5]} / {ref[diff][:5]}"
    if diff.any():
        assert np.all(np.abs(dev[diff].astype(np.float64) - ref[diff]) <= np.spacing(np.abs(ref[diff])))
        assert np.all(np.signbit(dev[diff]) == np.signbit(ref[diff]))
    # zeros and signed zeros: libm's answer exactly, sign included - both components zero, and one of them
    for part in ("zeros", "axes"):
        s = where[part]
        bad = np.flatnonzero(bits(dev[s]) != bits(ref[s]))
        assert bad.size == 0, f"{part}: {xy[s][bad][:6]} -> {dev[s][bad][:6]} / libm {ref[s][bad][:6]}"
    assert zero.sum() >= 4
    # the host build of the same source: every operation is IEEE and correctly rounded on both, so the same bits
    h = host(hs.hostsim_phase, xy)
    d = np.flatnonzero(nz & (bits(dev) != bits(h)))
    assert d.size == 0, f"{d.size} phases differ between the device and the host build, first {xy[d[:5]]}: {dev[d[:5]]} / {h[d[:5]]}"


def test_phase_fast_is_within_the_guard(L, hs, phase_set):
    xy, where = phase_set
    dev = cr.device_probe(L, "phase_fast", xy)[:, 0]
    h = host(hs.hostsim_phase_fast, xy)
    ref = np.arctan2(xy[:, 1].astype(np.float64), xy[:, 0].astype(np.float64)) / (2 * np.pi)
    mx = np.maximum(np.abs(xy[:, 0]), np.abs(xy[:, 1]))
    normal = mx >= TINY
    zero = mx == 0
    fin = np.isfinite(dev)
    # not finite only where the larger component is subnormal (the reciprocal overflows): the kernel flags those
    assert fin[normal | zero].all(), xy[(normal | zero) & ~fin][:5]
    print(f"device phase_fast: {(~fin).sum()} of {(~normal & ~zero).sum()} samples with a subnormal larger component are not finite, {np.isnan(dev).sum()} NaN")
    assert np.abs(dev[fin]).max() <= 0.5
    assert np.all(dev[zero] == 0) and zero.sum() >= 4                       # a zero sample has phase 0, whichever zero it is
    k = np.flatnonzero((xy[:, 0] == -1) & (xy[:, 1] == 0) & np.signbit(xy[:, 1]))
    assert k.size >= 1 and np.all(np.abs(dev[k]) == 0.5)

    def worst(v):
        d = np.abs(ref[normal] - v[normal].astype(np.float64))
        return np.minimum(d, 1.0 - d).max()                                 # +half a turn and -half a turn are the same direction
    d_dev, d_host = worst(dev), worst(h)
    print(f"phase_fast worst error, turns: device {d_dev:.4e}, host build {d_host:.4e}")
    guard = float(hs.hostsim_screen_guard())
    assert F32(guard) == cr.SCREEN_GUARD
    # tests/test_phase.py's inequality with the DEVICE's worst error: what the screen's unwrap guard rests on
    ref_side = (2 * 0.5 * np.spacing(F32(4.0)) + 0.5 * np.spacing(F32(8.0))) / (2 * np.pi)
    ours = 2 * d_dev + 0.5 * np.spacing(F32(0.5)) + 0.5 * np.spacing(F32(1.0))
    assert ours + ref_side < 0.25 * guard, (ours, ref_side, guard)
    assert d_host < 1.2e-7, d_host
    # v_rcp_f32 is good to 1 ulp and the product to half of one where the host divides (half an ulp): at most ~2 ulps of t <= 1
    # more, through a slope of 1 / 2 pi: 2 * 1.2e-7 / 6.28 = 4e-8 turn
    assert d_dev <= d_host + 4e-8, (d_dev, d_host)


def test_mag_of_is_the_double_hypot(L, phase_set):
    xy, where = phase_set
    dev = cr.device_probe(L, "mag", xy)[:, 0]
    x = xy.astype(np.float64)
    ref = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(F32)         # the products are exact in double
    d = np.flatnonzero(bits(dev) != bits(ref))
    assert d.size == 0, f"{d.size} magnitudes differ, first {xy[d[:5]]}: {dev[d[:5]]} / {ref[d[:5]]}"
    assert (ref[where["subnormal"]] < TINY).any() and (ref[where["big"]] > 1e18).any()


def test_sync_metric_bit_for_bit(L, windows):
    ph, ndesign, exact, slope = windows
    dev = cr.device_probe(L, "metric", ph)
    d = np.flatnonzero((bits(dev[:, 0]) != bits(exact)) | (bits(dev[:, 1]) != bits(slope)))
    assert d.size == 0, f"{d.size} of {len(ph)} windows differ, first {d[:5]}: {dev[d[:3]]} / {exact[d[:3]]} {slope[d[:3]]}"
    td = cr.tap_differences(ph[ndesign:])
    for t in cr.ulp_neighbours(cr.PI_BELOW):
        assert (td == t).any() and (td == -t).any(), float(t)
    assert (exact < 4).sum() > 50000 and ((exact > 3) & (exact < 5)).sum() > 2000


def test_screen_never_hides_a_sub_threshold_metric(L, hs, windows):
    """tests/test_design.py's safety conditions of the screening value, on the device's values"""
    ph, ndesign, exact, _ = windows
    turns = np.ascontiguousarray(ph * cr.TURNS)
    assert turns.dtype == F32
    dev = cr.device_probe(L, "screen", turns)
    screen, early = dev[:, 0], dev[:, 1]
    assert np.isfinite(screen).all() and np.isfinite(early).all()
    guarded = screen == 0.0
    assert guarded[ndesign - 50000:ndesign].mean() > 0.001 and guarded[:200000].mean() < 1e-3
    err = np.abs(screen.astype(np.float64) - exact.astype(np.float64))[~guarded]
    print(f"device screen: largest |screen - exact| outside guarded windows {err.max():.4f} rad^2 ({guarded.sum()} of {len(ph)} windows guarded)")
    # the host build, as a second witness (and what tests/test_gpu_sync_screen.py predicts the kernel's flags with)
    n = len(ph)
    he = np.zeros(n, dtype=F32); hsl = np.zeros(n, dtype=F32); hscr = np.zeros(n, dtype=F32); hea = np.zeros(n, dtype=F32)
    hs.hostsim_metric_pairs(ph.ctypes.data, n, he.ctypes.data, hsl.ctypes.data, hscr.ctypes.data)
    hs.hostsim_metric_early(ph.ctypes.data, n, hea.ctypes.data)
    nd = int((bits(screen) != bits(hscr)).sum() + (bits(early) != bits(hea)).sum())
    far = max(np.abs(screen.astype(np.float64) - hscr).max(), np.abs(early.astype(np.float64) - hea).max())
    print(f"device screen bit-identical to the host build: {'yes' if nd == 0 else 'no'} ({nd} values differ, by at most {far:.3e})")
    assert not np.any((exact < 4.0) & (screen >= cr.SCREEN_THR))
    assert (early.astype(np.float64) - screen.astype(np.float64))[~guarded].max() < 0.2
    assert not np.any((screen < cr.SCREEN_THR) & ~guarded & (early >= cr.SCREEN_EARLY_THR))
    assert not np.any((exact < 4.0) & (early >= cr.SCREEN_EARLY_THR))
    assert err.max() < 0.2, err.max()
    assert (early[:200000] >= cr.SCREEN_EARLY_THR).mean() > 0.99


def test_slice_symbol_bit_for_bit(L):
    a = cr.slice_inputs()
    dev = cr.device_probe(L, "slice", a).view(np.int32)
    ri, rn = cr.slice_symbol(a[:, 0], a[:, 1], a[:, 2])
    d = np.flatnonzero((ri != dev[:, 0]) | (rn != dev[:, 1]))
    assert d.size == 0, f"{d.size} of {len(a)} decisions differ, first {a[d[:3]]}: {ri[d[:3]]} {rn[d[:3]]} / {dev[d[:3]]}"
    assert rn.sum() > 1000 and all((ri == k).sum() > 1000 for k in range(8))


def test_parabola_vertex_bit_for_bit(L):
    a = cr.vertex_inputs()
    dev = cr.device_probe(L, "vertex", a)[:, 0]
    ref = cr.parabola_vertex(a[:, 0], a[:, 1], a[:, 2])
    d = np.flatnonzero(~same_floats(ref, dev))
    assert d.size == 0, f"{d.size} of {len(a)} vertices differ, first {a[d[:3]]}: {ref[d[:3]]} / {dev[d[:3]]}"
    assert np.isnan(ref).sum() >= 1000 and np.isinf(ref).sum() > 0           # y1 = y2 = y3 (0/0) and a = 0 (x/0)


def test_ppm_gate_bit_for_bit(L):
    from dumpvdl2_amd import synth

    def probe(vd, fr, mp):
        a = np.empty((len(vd), 3), dtype=np.uint32)
        a[:, 0] = np.ascontiguousarray(vd, dtype=F32).view(np.uint32); a[:, 1] = fr; a[:, 2] = np.ascontiguousarray(mp, dtype=F32).view(np.uint32)
        o = cr.device_probe(L, "ppm", a)
        return o[:, 0], o[:, 1]

    vd, fr, mp = cr.ppm_inputs(synth.channel_plan(256))
    ppm, thr = probe(vd, fr, mp)
    rp = cr.ppm_of(vd, fr); rt = cr.ppm_gate_threshold(fr, mp)
    d = np.flatnonzero(~same_floats(rp, ppm) | (bits(rt) != bits(thr)))
    assert d.size == 0, f"{d.size} of {len(vd)} differ, first {vd[d[:3]]} {fr[d[:3]]}: {rp[d[:3]]} {rt[d[:3]]} / {ppm[d[:3]]} {thr[d[:3]]}"
    # the device's threshold is the device's gate: |ppm_of| passes at it and fails at the next float up
    at, _ = probe(thr, fr, mp); above, _ = probe(np.nextafter(thr, F32(np.inf)), fr, mp)
    assert np.all(np.abs(at) <= mp) and np.all(np.abs(above) > mp)
