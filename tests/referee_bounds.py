"""What tests/test_gpu_referee_bounds.py measures, as plain numpy on streams: the three premises the referee's margin arithmetic
(vdl2_core.h "Referee") rests on.  y is a decimated stream float32 [D, 2] that starts at sample 0 - the channeliser's -,
y_ref the reference's own samples of the same input (the oracle's trace).  Nothing here knows where y comes from: the GPU tests pass
the kernel's stream, tests/test_referee_bounds_model.py the float32 model's and the host build's marks.

  kappa_share()            premise 1: |y[n] - y_ref[n]| as a share of kRefKappa x the largest |y| among n .. n-3
  stream_metric()          got_sync()'s metric and slope at every sample (taps n-150 .. n step 10, zero phase ahead of the stream)
  margin_shares()          premise 2: |p - p_ref| and |f - f_ref| as shares of ref_pherr_margin(p, E) and ref_slope_margin(E), on the
                           windows where the margins are all that stands between the two (p < 8, E < kRefBig, no discontinuity event)
  reference_decisions()    what got_sync() decides at every sample on the reference's metric: fires, and the code (sclk, gate)
  check_marks()            premise 3: the marks the exact sync tier left (read_sync) against those decisions

The constants are the source's, read from the host build (hostsim_ref_constants): they are the claims under test."""
import ctypes as C

import numpy as np

import core_reference as cr

F32 = np.float32
TAPS = 10 * np.arange(16)


def constants():
    """kRefKappa, kRefSum, kRefBig as the source under test has them"""
    import pyhostsim
    H = C.CDLL(pyhostsim.build())
    c = np.zeros(5, dtype=F32)
    H.hostsim_ref_constants.argtypes = [C.c_void_p]
    H.hostsim_ref_constants(c.ctypes.data)
    assert c[1] == cr.REF_SUM and c[2] == cr.REF_BIG and c[3] == cr.SYNC_THR and c[4] == cr.PHERR_BIG     # (core_reference restates these)
    return {"kappa": F32(c[0]), "sum": F32(c[1]), "big": F32(c[2])}


def mag2(y):
    y = np.asarray(y, dtype=F32)
    return y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]


def kappa_share(y, y_ref, kappa):
    """-> (share float64 [D], valid bool [D]); valid: |y[n]|^2 > 0"""
    m2 = mag2(y).astype(np.float64)
    loc = m2.copy()
    for k in (1, 2, 3):
        loc[k:] = np.maximum(loc[k:], m2[:-k])
    d = np.asarray(y, dtype=np.float64) - np.asarray(y_ref, dtype=np.float64)
    err = np.sqrt((d * d).sum(axis=1))
    valid = m2 > 0
    return err / np.where(valid, float(kappa) * np.sqrt(loc), 1.0), valid


def share_stats(share, valid):
    s = share[valid]
    return {"max": float(s.max()), "q999": float(np.quantile(s, 0.999)), "rms": float(np.sqrt((s * s).mean())), "n": int(s.size)}


def windows_at(a, n, fill=0):
    """a [D] -> [len(n), 16]: a at the taps n - 150 + 10 i of the windows ending at the samples n, `fill` ahead of the stream"""
    pad = np.concatenate([np.full(150, fill, dtype=a.dtype), a])
    return pad[np.asarray(n)[:, None] + TAPS[None, :]]


def stream_metric(ph, chunk=1 << 19):
    """ph float32 [D]: the phase of every sample -> (p, f) float32 [D]"""
    D = len(ph)
    pad = np.concatenate([np.zeros(150, dtype=F32), np.asarray(ph, dtype=F32)])
    W = np.lib.stride_tricks.as_strided(pad, shape=(D, 16), strides=(pad.strides[0], 10 * pad.strides[0]), writeable=False)     # W[n, i] = pad[n + 10 i]
    p = np.empty(D, dtype=F32); f = np.empty(D, dtype=F32)
    for k in range(0, D, chunk):
        p[k:k + chunk], f[k:k + chunk] = cr.sync_metric(W[k:k + chunk])
    return p, f


def margin_shares(y, ph, p, f, p_ref, f_ref, kappa):
    """-> dict: n windows selected, the worst share of the metric's and of the slope's margin, and where.  E and the events from y, as
    ref_eps2_of() and sync_metric_ref() define them"""
    n = np.flatnonzero(p < 8)
    eps2 = cr.stream_eps2(y, kappa)
    W = windows_at(ph, n); Q = windows_at(eps2, n, fill=F32(0))
    nev = cr.ref_events(W, Q)[0]
    s = np.zeros(len(n), dtype=F32)
    for i in range(16):
        s = s + Q[:, i]
    keep = (nev == 0) & ~(Q >= cr.REF_BIG).any(axis=1)
    n = n[keep]; E = np.sqrt(s[keep])
    assert np.all(E < cr.REF_BIG)
    with np.errstate(all="ignore"):
        sp = np.abs(p[n].astype(np.float64) - p_ref[n]) / cr.ref_pherr_margin(p[n], E)
        sf = np.abs(f[n].astype(np.float64) - f_ref[n]) / cr.ref_slope_margin(E)
    out = {"n": int(n.size), "p_share": 0.0, "f_share": 0.0, "p_at": -1, "f_at": -1}
    if n.size:
        out.update(p_share=float(sp.max()), f_share=float(sf.max()), p_at=int(n[sp.argmax()]), f_at=int(n[sf.argmax()]))
    return out


def _shift(a, k, fill):
    """a[n - k] at n, `fill` where n - k lies ahead of the stream"""
    return np.concatenate([np.full(k, fill, dtype=a.dtype), a[:len(a) - k]])


def decisions(p, f, tab, max_ppm, ppm_thr):
    """got_sync()'s decision at every sample n on the metric values p, slopes f (ref_candidate_code restated): -> fires bool [D], and
    the codes with y1 = PHERR_MAX and with y1 = p[n-6] (-1 where n-6, n-3 or n is not tabulated - tab - or lies ahead of the stream)"""
    p = np.asarray(p, dtype=F32); f = np.asarray(f, dtype=F32)
    D = len(p)
    ok3 = tab & _shift(tab, 3, False)
    p3 = _shift(p, 3, cr.PHERR_BIG); f3 = _shift(f, 3, F32(0)); p6 = _shift(p, 6, cr.PHERR_BIG)
    fires = ok3 & (p3 < cr.SYNC_THR) & (p > p3)
    big = np.full(D, cr.PHERR_BIG, dtype=F32)
    code_big = np.where(ok3, cr.ref_candidate_code(big, p3, p, f3, max_ppm, ppm_thr), -1)
    code_6 = np.where(ok3 & _shift(tab, 6, False), cr.ref_candidate_code(p6, p3, p, f3, max_ppm, ppm_thr), -1)
    return fires, code_big, code_6


def check_marks(pf, cand, p_ref, f_ref, max_ppm, ppm_thr, whole_feed=True):
    """pf [D, 2], cand [D]: read_sync() of one channel (a receiver with the referee on); p_ref, f_ref: the reference's metric.
    -> dict of counts and of violations (sample lists):
       missed       the reference fires at n and cand[n] is not set                                                     (a)
       unmarked     cand[n] set, n not marked, and the reference does not fire there or decides otherwise than |pf|     (b; whole feeds only)"""
    D = len(cand)
    cand = np.asarray(cand).astype(bool)
    mark = np.signbit(pf[:, 0]); ap = np.abs(pf[:, 0]); tab = pf[:, 0] != 0
    everywhere = np.ones(D, dtype=bool)
    fires, rbig, r6 = decisions(p_ref, f_ref, everywhere, max_ppm, ppm_thr)
    fires[:3] = False                                    # (the tier decides samples n >= 3)
    _, dbig, d6 = decisions(ap, pf[:, 1], tab, max_ppm, ppm_thr)
    differs = ~fires | (dbig != rbig) | ((d6 >= 0) & (d6 != r6))
    out = {"fires": int(fires.sum()), "candidates": int(cand.sum()), "marked": int((cand & mark).sum()),
           "marked_and_different": int((cand & mark & differs).sum()), "missed": np.flatnonzero(fires & ~cand)}
    out["unmarked"] = np.flatnonzero(cand & ~mark & differs) if whole_feed else np.zeros(0, dtype=np.int64)
    return out


def device_phases(L, y):
    """the device's exact phase (phase_of) of every sample of y [..., 2] -> float32 [...]"""
    y = np.ascontiguousarray(y, dtype=F32)
    return cr.device_probe(L, "phase", y.reshape(-1, 2))[:, 0].reshape(y.shape[:-1])


def host_phases(y):
    """... and the host build's (bit-identical to the device's: tests/test_gpu_core_probe.py), for the CPU tests"""
    import pyhostsim
    H = C.CDLL(pyhostsim.build())
    H.hostsim_phase.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    y = np.ascontiguousarray(y, dtype=F32)
    out = np.empty(y.size // 2, dtype=F32)
    H.hostsim_phase(y.ctypes.data, out.ctypes.data, out.size)
    return out.reshape(y.shape[:-1])
