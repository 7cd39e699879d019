"""tests/core_reference.py's restatements of the referee's margin arithmetic (vdl2_core.h: sync_metric_ref in both forms with
sync_metric_flipped, sync_metric_two and sync_metric_unwrap_alts behind it, ref_pherr_range, ref_candidate_verdict, ref_vertex_marginal,
ref_symbol_dist, ref_symbol_marginal) against the host build of that source (tests/hostsim: hostsim_ref_probe), on core_reference.py's own
input sets: bit for bit.  Then, independent of the restatement: the metric run again in float64 with every listed decision - and every
pair of them - taken the other way lies in [alo, ahi], and E is kRefBig exactly where it has to be.  tests/test_gpu_referee_probe.py
holds the device build to the same references on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import core_reference as cr
import pyhostsim

F32 = np.float32


@pytest.fixture(scope="module")
def hs():
    L = C.CDLL(pyhostsim.build())
    L.hostsim_ref_probe.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    L.hostsim_ref_constants.argtypes = [C.c_void_p]
    return L


def host_probe(hs, name, a):
    kind, win, wout = cr.PROBE[name]
    a = np.ascontiguousarray(a, dtype=F32)
    assert a.ndim == 2 and a.shape[1] == win
    out = np.full((len(a), wout), np.nan, dtype=F32)
    assert hs.hostsim_ref_probe(kind, a.ctypes.data, len(a), out.ctypes.data) == 0
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def windows():
    ph, eps2, where = cr.ref_windows()
    ph.setflags(write=False); eps2.setflags(write=False)
    return ph, eps2, where


def test_constants_are_the_sources(hs):
    c = np.zeros(5, dtype=F32)
    hs.hostsim_ref_constants(c.ctypes.data)
    assert [bits(c)[i] for i in range(5)] == [bits(v)[()] for v in (cr.REF_KAPPA, cr.REF_SUM, cr.REF_BIG, cr.SYNC_THR, cr.PHERR_BIG)]


def test_ref_windows_hold_what_they_promise(windows):
    ph, eps2, where = windows
    nev, ev, kind, flip, cut = cr.ref_events(ph, eps2)
    sq = np.sqrt(eps2)
    ncut = (((cr.PI_BELOW - np.abs(ph)) <= sq + F32(1e-6)) & (eps2 > 0)).sum(axis=1)
    nunw = nev - ncut
    for k in range(4):                                   # 0, 1, 2 and 3 events of each kind alone, and mixed
        assert ((ncut == k) & (nunw == 0)).sum() >= 20 and ((nunw == k) & (ncut == 0)).sum() >= 20, k
    for a, b in ((1, 1), (1, 2), (2, 1)):
        assert ((ncut == a) & (nunw == b)).sum() >= 20, (a, b)
    assert (eps2[where["own"]] == 0).all() and (nev[where["own"]] == 0).all()
    assert (nev[where["big"]] >= 1).all()                # (a tap of unknown phase is "at the branch cut" too)
    # the edge windows sit on the unwrap test: tap differences at +-kPiBelow and a float either side, listed as events once a tap has an error
    td = cr.tap_differences(ph[where["decision"]])
    for t in cr.ulp_neighbours(cr.PI_BELOW):
        assert (td == t).any() and (td == -t).any(), float(t)
    assert (nunw[where["decision"]] >= 1).mean() > 0.9
    # ... and the cut windows on the branch-cut test: both outcomes, from phases within three floats of its edge
    c = where["cut"]
    edge = cr.PI_BELOW - (sq[c] + F32(1e-6))
    at = np.abs(np.abs(ph[c]) - edge) <= 4 * np.spacing(F32(3.0))
    assert at.any(axis=1).all()
    hit = ((cr.PI_BELOW - np.abs(ph[c])) <= sq[c] + F32(1e-6)) & at
    assert 0.2 < hit.any(axis=1).mean() < 0.8


@pytest.mark.parametrize("full", [True, False], ids=["full", "plain"])
def test_sync_metric_ref_bit_for_bit(hs, windows, full):
    ph, eps2, where = windows
    out = host_probe(hs, "ref_full" if full else "ref_plain", np.concatenate([ph, eps2], axis=1))
    ref = np.stack(cr.sync_metric_ref(ph, eps2, full), axis=1)
    d = np.flatnonzero((bits(out) != bits(ref)).any(axis=1))
    assert d.size == 0, f"{d.size} of {len(ph)} windows differ, first {d[:5]}: {out[d[:3]]} / {ref[d[:3]]}"
    n = cr.check_alternatives_and_E(ph, eps2, out, full, f"host build, full={full}")
    assert n >= 20000
    E = out[:, 2]
    assert (E[where["stream"]] < 0.2).mean() > 0.5 and (E == cr.REF_BIG).sum() > 1000 and (out[:, 4] > out[:, 0]).sum() > 5000


def test_verdict_bit_for_bit(hs):
    a = cr.verdict_inputs()
    out = host_probe(hs, "verdict", a)
    r0 = cr.ref_pherr_range(a[:, 0], a[:, 1], a[:, 2], a[:, 3]); r3 = cr.ref_pherr_range(a[:, 4], a[:, 5], a[:, 6], a[:, 7])
    r6 = cr.ref_pherr_range(a[:, 9], a[:, 10], a[:, 11], a[:, 12])
    rr = np.stack([r0[0], r0[1], r3[0], r3[1], r6[0], r6[1]], axis=1)
    d = np.flatnonzero((bits(out[:, 1:]) != bits(rr)).any(axis=1))
    assert d.size == 0, f"ref_pherr_range: {d.size} of {len(a)} differ, first {a[d[:2]]}: {out[d[:2], 1:]} / {rr[d[:2]]}"
    vd = cr.ref_candidate_verdict(r0, r3, a[:, 8], a[:, 7], r6, a[:, 13], a[:, 14])
    got = out[:, 0].copy().view(np.int32)
    d = np.flatnonzero(got != vd)
    assert d.size == 0, f"ref_candidate_verdict: {d.size} of {len(a)} differ, first {a[d[:2]]}: {got[d[:3]]} / {vd[d[:3]]}"
    # every outcome, with and without n-6, gate on and off; the gate alone decides some; the threshold test is met from both sides
    absent = a[:, 9] >= cr.PHERR_BIG
    for v in (0, 1, 3):
        for m in (absent, ~absent):
            for g in (a[:, 13] == 0, a[:, 13] != 0):
                assert ((vd == v) & m & g).sum() >= 200, v
    off = cr.ref_candidate_verdict(r0, r3, a[:, 8], a[:, 7], r6, np.zeros(len(a), dtype=F32), a[:, 14])
    assert ((vd == 3) & (off == 1)).sum() >= 200
    edge = slice(300000, None)
    assert (r3[1][edge] < cr.SYNC_THR).sum() > 1000 and (r3[1][edge] >= cr.SYNC_THR).sum() > 1000
    assert (r3[0][edge] < cr.SYNC_THR).sum() > 1000 and (r3[0][edge] >= cr.SYNC_THR).sum() > 100
    assert len(set(vd[edge].tolist())) == 3


def test_vertex_marginal_bit_for_bit(hs):
    a = cr.vertex_boxes()
    got = host_probe(hs, "vertex_marginal", a).view(np.int32)[:, 0]
    ref = cr.ref_vertex_marginal(*[a[:, k] for k in range(6)])
    d = np.flatnonzero(got != ref.astype(np.int32))
    assert d.size == 0, f"{d.size} of {len(a)} differ, first {a[d[:3]]}: {got[d[:3]]} / {ref[d[:3]]}"
    assert 0.1 < ref[:200000].mean() < 0.9 and 0.1 < ref[200000:260000].mean() < 0.9 and ref[260000:].mean() > 0.9
    # independent of the restatement: where a box is NOT marginal, -roundf(vertex) worked out in float64 is one number at the box's centre
    # and with each value alone at either end of its range (what the function claims; float32 against float64: 2e-5 about a boundary)
    k = np.flatnonzero(~ref)
    b = a[k].astype(np.float64)

    def vert(y1, y2, y3):
        return -((9 * (y3 - y1) + 36 * (y2 - y3)) / -54.0) / (2 * ((-3 * (y1 - y3) - 6 * (y3 - y2)) / -54.0))
    ctr = [0.5 * (b[:, 0] + b[:, 1]), 0.5 * (b[:, 2] + b[:, 3]), 0.5 * (b[:, 4] + b[:, 5])]
    c = np.round(vert(*ctr))
    assert np.isfinite(c).all()
    for j in range(3):
        for end in range(2):
            y = list(ctr); y[j] = b[:, 2 * j + end]
            v = vert(*y)
            differs = (np.round(v) != c) & (np.abs(v - np.floor(v) - 0.5) > 2e-5)
            assert not differs.any(), (j, end, a[k][differs][:3], v[differs][:3], c[differs][:3])


def test_symbol_margin_bit_for_bit(hs):
    a = cr.symbol_inputs()
    out = host_probe(hs, "symbol", a)
    dist = cr.ref_symbol_dist(a[:, 0], a[:, 1], a[:, 2]); marg = cr.ref_symbol_marginal(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    d = np.flatnonzero((bits(out[:, 0]) != bits(dist)) | (out[:, 1].copy().view(np.int32) != marg.astype(np.int32)))
    assert d.size == 0, f"{d.size} of {len(a)} differ, first {a[d[:3]]}: {out[d[:3]]} / {dist[d[:3]]} {marg[d[:3]]}"
    assert 0.2 < marg.mean() < 0.8
    at = dist == a[:, 3] + F32(2e-6)
    assert at.sum() > 1000                                # the test is met with equality, and from both sides
    # independent: the distance is that of the step (float64, whole turns removed) from the nearest odd multiple of pi/8, to float32 rounding
    step = (a[:, 0].astype(np.float64) - a[:, 1]) - a[:, 2]
    inside = (step > -2 * np.pi) & (step < 4 * np.pi)     # (the reference removes one turn at the most)
    x = np.mod(step[inside], np.pi / 4)
    d64 = np.abs(x - np.pi / 8)
    assert np.abs(d64 - dist[inside]).max() < 4e-6, np.abs(d64 - dist[inside]).max()
