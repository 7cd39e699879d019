"""The yardstick for the element-wise pieces of dumpvdl2_amd/csrc/vdl2_core.h that mix float and double the way the reference does
(src/demod.c:98-198, 256-264): plain numpy, no GPU, nothing compiled.

sync_metric()          got_sync() up to the threshold test: pherr and slope of n windows of 16 phases
slice_symbol()         one D8PSK decision: the phase-step index and whether the reference's index went negative
parabola_vertex()      calc_para_vertex(0, 3, y1, y2, y3)
ppm_of(), ppm_gate_threshold()   the --max-ppm gate
sync_metric_ref() ... ref_candidate_code()   the referee's margin arithmetic: the metric with its error figure and alternatives
                       (sync_metric_flipped, sync_metric_two, sync_metric_unwrap_alts), ref_pherr_range, ref_candidate_verdict,
                       ref_vertex_marginal, ref_symbol_dist / ref_symbol_marginal (held to the host build by
                       tests/test_core_reference_referee.py)

Every float32 operation is one numpy float32 operation (rounded once, never fused), every step the C source takes in double is
taken in float64.  tests/test_core_reference.py holds them BIT FOR BIT to the host build of the same source (tests/hostsim, which
tests/test_hostsim.py pins to the oracle).  That makes them a yardstick that needs nothing compiled: what the device build of these
helpers is to be held to.

The input sets are made here too - the places where these pieces can break (the +-pi unwrap decision to the float, the roundf() ties
of the slicer, 0/0 and x/0 of the vertex, the gate's threshold and the floats either side, signed zeros, subnormals, the k/16 switch
points of the atan2 reduction) - so that whoever uses the references uses them on inputs the CPU test has vouched for."""
import numpy as np

F32 = np.float32
PI_BELOW = F32(np.nextafter(F32(np.pi), F32(0)))       # largest float < M_PI (float(pi) is above pi): vdl2_core.h kPiBelow
TWO_PI = 2.0 * np.pi                                   # "2.0f * M_PI": a double
Q_EIGHTHS = np.array([0, 3, -3, 1, 1, 2, 0, 4, -3, 4, -2, 3, 1, -2, -3, 0])        # demod.c:107-124, units of pi/4
PR_PHASE = (Q_EIGHTHS * np.pi / 4).astype(F32)         # (float)(q * M_PI / 4)
SYNC_THR = F32(4.0)
SCREEN_THR, SCREEN_EARLY_THR, SCREEN_GUARD = F32(5.5), F32(5.8), F32(3.2e-6)     # vdl2_core.h: kScreenThr, kScreenEarlyThr, kScreenGuard (turns)
TURNS = F32(0.5 / np.pi)                               # radians -> turns as tests/hostsim does it: one float product


def _regression_abscissae():
    mean_x = F32(0)
    for i in range(16):
        mean_x = F32(mean_x + F32(i))
    mean_x = F32(mean_x / F32(16))
    lrx = np.array([F32(F32(i) - mean_x) for i in range(16)], dtype=F32)
    den = F32(0)
    for i in range(16):
        den = F32(den + F32(lrx[i] * lrx[i]))
    return lrx, den


LRX, LR_DEN = _regression_abscissae()


def sync_metric(ph):
    """ph: float32 [n, 16], ph[:, i] = the phase 150 - 10 i samples ago -> (pherr, slope) float32 [n]"""
    ph = np.asarray(ph, dtype=F32)
    n = ph.shape[0]
    e = np.empty((n, 16), dtype=F32)
    e[:, 0] = ph[:, 0] - PR_PHASE[0]
    prev = e[:, 0].copy(); mean = e[:, 0].copy()
    unwrap = np.zeros(n, dtype=F32)
    for i in range(1, 16):
        cur = ph[:, i] - PR_PHASE[i]
        diff = cur - prev
        prev = cur
        step = np.where(diff > PI_BELOW, -TWO_PI, np.where(diff < -PI_BELOW, TWO_PI, 0.0))
        unwrap = (unwrap.astype(np.float64) + step).astype(F32)
        e[:, i] = cur + unwrap
        mean = mean + e[:, i]
    mean = mean / F32(16)
    e = e - mean[:, None]
    slope = np.zeros(n, dtype=F32)
    for i in range(16):
        slope = slope + LRX[i] * e[:, i]
    slope = slope / LR_DEN
    acc = np.zeros(n, dtype=F32)
    for i in range(16):
        r = e[:, i] - slope * LRX[i]
        acc = acc + r * r
    assert acc.dtype == F32 and slope.dtype == F32
    return acc, slope


def _roundf(x):
    """C's roundf() (halves away from zero) of float32 values, as float64 whole numbers: |x| + 0.5 is exact in double"""
    x = np.asarray(x, dtype=F32).astype(np.float64)
    return np.copysign(np.floor(np.abs(x) + 0.5), x)


def slice_symbol(phi, prev_phi, vdphi):
    """-> (index 0..7, neg 0/1) int32 [n]"""
    phi = np.asarray(phi, dtype=F32); prev_phi = np.asarray(prev_phi, dtype=F32); vdphi = np.asarray(vdphi, dtype=F32)
    dphi = (phi - prev_phi) - vdphi
    d64 = dphi.astype(np.float64)
    dphi = np.where(dphi < 0, (d64 + TWO_PI).astype(F32), np.where(d64 > TWO_PI, (d64 - TWO_PI).astype(F32), dphi)).astype(F32)
    dphi = (dphi.astype(np.float64) / (np.pi / 4)).astype(F32)
    r = _roundf(dphi).astype(np.int64)
    idx = np.where(r >= 0, r % 8, -((-r) % 8))            # C's %: the sign of the dividend
    neg = (idx < 0).astype(np.int32)
    return (idx & 7).astype(np.int32), neg


def parabola_vertex(y1, y2, y3):
    y1 = np.asarray(y1, dtype=F32); y2 = np.asarray(y2, dtype=F32); y3 = np.asarray(y3, dtype=F32)
    x = F32(0); d = F32(3); denom = F32(3 * 2 * 3 * -3)
    with np.errstate(all="ignore"):
        a = ((x * (y2 - y1) + (x - d) * (y1 - y3)) + (x - F32(2) * d) * (y3 - y2)) / denom
        b = ((F32(x * x) * (y1 - y2) + F32((x - d) * (x - d)) * (y3 - y1)) + F32((x - F32(2) * d) * (x - F32(2) * d)) * (y2 - y3)) / denom
        v = -b / (F32(2) * a)
    assert v.dtype == F32
    return v


def ppm_of(vdphi, freq):
    vdphi = np.asarray(vdphi, dtype=F32); freq = np.asarray(freq, dtype=np.uint32)
    with np.errstate(all="ignore"):
        num = (F32(10500) * vdphi).astype(np.float64)
        return (num / (TWO_PI * freq.astype(np.float64)) * 1e+6).astype(F32)


def ppm_gate_threshold(freq, max_ppm):
    """the largest float x with |ppm_of(x, freq)| <= max_ppm, by bisection on the bit pattern of x (|ppm_of| is non-decreasing in |x|)"""
    freq = np.asarray(freq, dtype=np.uint32); max_ppm = np.asarray(max_ppm, dtype=F32)
    lo = np.zeros(freq.shape, dtype=np.uint32); hi = np.full(freq.shape, 0x7f800000, dtype=np.uint32)
    for _ in range(32):
        mid = lo + (hi - lo) // np.uint32(2)
        over = np.abs(ppm_of(mid.view(F32), freq)) > max_ppm
        go = (hi - lo) > 1
        hi = np.where(go & over, mid, hi); lo = np.where(go & ~over, mid, lo)
    assert np.all(hi - lo == 1)
    return lo.view(F32)


# ------------------------------------------------------------------------------------------------------------------------------
# the referee's margin arithmetic (vdl2_core.h: "Referee"), restated the same way.  tests/test_core_reference_referee.py holds these to
# the host build, tests/test_gpu_referee_probe.py the device build to these.
# ------------------------------------------------------------------------------------------------------------------------------
REF_KAPPA, REF_SUM, REF_BIG, PHERR_BIG = F32(3.0e-4), F32(0.085), F32(1.0e30), F32(1000.0)     # kRefKappa, kRefSum, kRefBig, kPherrBig
TP32 = F32(TWO_PI)                                     # (float)(2.0 * M_PI)


def ref_eps2_of(m0, m1, m2, m3, kappa=REF_KAPPA):
    """squared bound on the phase error of a sample from |y|^2 of it and of its three predecessors (0 for one ahead of the stream)"""
    m0 = np.asarray(m0, dtype=F32); kappa = F32(kappa)
    a = np.maximum(np.maximum(m0, np.asarray(m1, dtype=F32)), np.maximum(np.asarray(m2, dtype=F32), np.asarray(m3, dtype=F32)))
    with np.errstate(all="ignore"):
        return np.where(m0 > 0, F32(kappa * kappa) * a / m0, REF_BIG).astype(F32)


def stream_eps2(y, kappa=REF_KAPPA):
    """ref_eps2() at every sample of a stream y float32 [D, 2] that starts at sample 0 (what lies ahead of it counts as zero)"""
    y = np.asarray(y, dtype=F32)
    m = y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]
    pre = [np.concatenate([np.zeros(k, dtype=F32), m[:len(m) - k]]) for k in (1, 2, 3)]
    return ref_eps2_of(m, pre[0], pre[1], pre[2], kappa)


def ref_pherr_margin(p, E):
    p = np.asarray(p, dtype=F32); e = REF_SUM * np.asarray(E, dtype=F32)
    with np.errstate(all="ignore"):
        return (((F32(2.0) * np.sqrt(p)) * e + e * e) + F32(4e-6) * p) + F32(1e-6)


def ref_slope_margin(E):
    return F32(F32(0.0543) * REF_SUM) * np.asarray(E, dtype=F32) + F32(1e-7)


def _metric_tail(e, mean):
    """mean and slope removal and the residual's square sum, in sync_metric()'s order; also the residuals"""
    mean = mean / F32(16)
    e = e - mean[:, None]
    slope = np.zeros(len(e), dtype=F32)
    for i in range(16):
        slope = slope + LRX[i] * e[:, i]
    slope = slope / LR_DEN
    r = e - slope[:, None] * LRX[None, :]
    acc = np.zeros(len(e), dtype=F32)
    for i in range(16):
        acc = acc + r[:, i] * r[:, i]
    return acc, slope, r


def _unwrapped(ph, flip=None):
    """e[i] = cur[i] + unwrap as sync_metric() forms them, their running sum, the steps taken and the tap differences; flip int [n]: the
    tap whose unwrap decision is taken the other way (-1: none)"""
    n = len(ph)
    e = np.empty((n, 16), dtype=F32); step_taken = np.zeros((n, 16)); diffs = np.zeros((n, 16), dtype=F32)
    e[:, 0] = ph[:, 0] - PR_PHASE[0]
    prev = e[:, 0].copy(); mean = e[:, 0].copy()
    unwrap = np.zeros(n, dtype=F32)
    for i in range(1, 16):
        cur = ph[:, i] - PR_PHASE[i]
        diff = cur - prev
        prev = cur
        step = np.where(diff > PI_BELOW, -TWO_PI, np.where(diff < -PI_BELOW, TWO_PI, 0.0))
        step_taken[:, i] = step; diffs[:, i] = diff
        if flip is not None:
            step = np.where(flip == i, np.where(step != 0.0, 0.0, np.where(diff > 0, -TWO_PI, TWO_PI)), step)
        unwrap = (unwrap.astype(np.float64) + step).astype(F32)
        e[:, i] = cur + unwrap
        mean = mean + e[:, i]
    return e, mean, step_taken, diffs


def sync_metric_flipped(ph, flip, cut):
    """the metric with the unwrap decision at tap flip[k] taken the other way and tap cut[k] read as -phase (-1: none) -> float32 [n]"""
    ph = np.asarray(ph, dtype=F32); flip = np.asarray(flip); cut = np.asarray(cut)
    q = np.where(np.arange(16)[None, :] == cut[:, None], -ph, ph).astype(F32)
    e, mean, _, _ = _unwrapped(q, flip)
    return _metric_tail(e, mean)[0]


def _alts_G(i, j):
    i = np.asarray(i); j = np.asarray(j)
    Li = F32(0.5) * (i * (16 - i)).astype(F32); Lj = F32(0.5) * (j * (16 - j)).astype(F32)
    return ((16 - np.maximum(i, j)).astype(F32) - ((16 - i) * (16 - j)).astype(F32) / F32(16)) - Li * Lj / LR_DEN


def sync_metric_unwrap_alts(ph, ev, nev, pherr):
    """sync_metric_unwrap_alts(): ev int [n, 2] taps (>= 1) of the nev [n] (1 or 2) unwrap decisions -> (lo, hi) float32 [n]"""
    ph = np.asarray(ph, dtype=F32); ev = np.asarray(ev); nev = np.asarray(nev); pherr = np.asarray(pherr, dtype=F32)
    n = len(ph)
    e, mean, step, diff = _unwrapped(ph)
    _, _, r = _metric_tail(e, mean)
    rows = np.arange(n)
    sgn = np.zeros((n, 2), dtype=F32); rho = np.zeros((n, 2), dtype=F32)
    for k in range(2):
        st = step[rows, ev[:, k]]; df = diff[rows, ev[:, k]]
        sgn[:, k] = np.where(st != 0.0, np.where(st < 0.0, 1.0, -1.0), np.where(df > 0, -1.0, 1.0))
        for i in range(15, 0, -1):
            rho[:, k] = np.where(i >= ev[:, k], rho[:, k] + r[:, i], rho[:, k])
    two = F32(2.0)
    lo = pherr.copy(); hi = pherr.copy()
    g = [_alts_G(ev[:, 0], ev[:, 0]), _alts_G(ev[:, 1], ev[:, 1])]; g01 = _alts_G(ev[:, 1], ev[:, 0])
    term = [two * TP32 * sgn[:, k] * rho[:, k] + TP32 * TP32 * g[k] for k in range(2)]
    cross = two * TP32 * TP32 * sgn[:, 1] * sgn[:, 0] * g01
    for c in (1, 2, 3):
        v = pherr.copy()
        if c & 1:
            v = v + term[0]
        if c & 2:
            v = v + term[1]
        if c == 3:
            v = v + cross
        slack = F32(1e-3) + F32(2e-5) * np.abs(v)
        on = (nev == 2) | (c == 1)
        lo = np.where(on & (v - slack < lo), v - slack, lo); hi = np.where(on & (v + slack > hi), v + slack, hi)
    return np.where(lo < 0, F32(0), lo).astype(F32), hi.astype(F32)


def sync_metric_two(ph, ev, kind, pherr):
    """sync_metric_two(): two discontinuities, ev int [n, 2] taps, kind [n, 2] (0 unwrap decision, 1 branch cut) -> (lo, hi)"""
    ph = np.asarray(ph, dtype=F32); ev = np.asarray(ev); kind = np.asarray(kind); pherr = np.asarray(pherr, dtype=F32)
    lo = pherr.copy(); hi = pherr.copy()
    taps = np.arange(16)[None, :]
    for c in (1, 2, 3):
        q = ph.copy(); flip = np.full(len(ph), -1)
        for k in range(2):
            if (c >> k) & 1:
                q = np.where((kind[:, k] == 1)[:, None] & (taps == ev[:, k][:, None]), -q, q).astype(F32)
                flip = np.where(kind[:, k] == 0, ev[:, k], flip)
        v = sync_metric_flipped(q, flip, np.full(len(ph), -1))
        lo = np.where(v < lo, v, lo); hi = np.where(v > hi, v, hi)
    both = (kind[:, 0] == 0) & (kind[:, 1] == 0)                    # two unwrap decisions: "cannot tell"
    return np.where(both, F32(0), lo).astype(F32), np.where(both, REF_BIG, hi).astype(F32)


def ref_events(ph, eps2):
    """the discontinuities within the stream's error as sync_metric_ref() lists them: branch-cut taps first, then unwrap decisions, each
    in tap order -> (nev [n], ev [n, 2], kind [n, 2] of the first two, flip [n], cut [n]: the last of each kind or -1)"""
    ph = np.asarray(ph, dtype=F32); eps2 = np.asarray(eps2, dtype=F32)
    n = len(ph)
    sq = np.sqrt(eps2)
    is_cut = ((PI_BELOW - np.abs(ph)) <= sq + F32(1e-6)) & (eps2 > 0)
    cur = ph - PR_PHASE[None, :]
    diff = cur[:, 1:] - cur[:, :-1]
    es = sq[:, 1:] + sq[:, :-1]
    is_unw = np.zeros((n, 16), dtype=bool)
    is_unw[:, 1:] = (es > 0) & (np.abs(np.abs(diff) - PI_BELOW) <= es + F32(4e-6))
    order = np.concatenate([is_cut, is_unw], axis=1)                 # 32 slots in the order the source meets them
    nev = order.sum(axis=1)
    ev = np.zeros((n, 2), dtype=np.int64); kind = np.zeros((n, 2), dtype=np.int64)
    rank = np.cumsum(order, axis=1)
    for k in range(2):
        hit = order & (rank == k + 1)
        slot = hit.argmax(axis=1); has = hit.any(axis=1)
        ev[:, k] = np.where(has, slot % 16, 0); kind[:, k] = np.where(has, slot < 16, 0)
    last = lambda m: np.where(m.any(axis=1), 15 - m[:, ::-1].argmax(axis=1), -1)
    return nev, ev, kind, last(is_unw), last(is_cut)


def sync_metric_ref(ph, eps2, full=True):
    """sync_metric_ref(): ph, eps2 float32 [n, 16] -> (pherr, slope, E, alo, ahi) float32 [n]"""
    ph = np.asarray(ph, dtype=F32); eps2 = np.asarray(eps2, dtype=F32)
    pherr, slope = sync_metric(ph)
    s = np.zeros(len(ph), dtype=F32)
    for i in range(16):
        s = s + eps2[:, i]
    big = (eps2 >= REF_BIG).any(axis=1)
    nev, ev, kind, flip, cut = ref_events(ph, eps2)
    alo = pherr.copy(); ahi = pherr.copy()
    own = (s == 0) & ~big                                            # every tap is the reference's own
    unw = ~own & bool(full) & (nev >= 1) & (nev <= 2) & ~big & (kind[:, 0] == 0) & ((nev == 1) | (kind[:, 1] == 0))
    one = ~own & ~unw & (nev == 1) & ~big
    two = ~own & ~unw & (nev == 2) & ~big
    k = np.flatnonzero(unw)
    if k.size:
        alo[k], ahi[k] = sync_metric_unwrap_alts(ph[k], np.where(ev[k] < 1, 1, ev[k]), nev[k], pherr[k])
    k = np.flatnonzero(one)
    if k.size:
        alo[k] = ahi[k] = sync_metric_flipped(ph[k], flip[k], cut[k])
    k = np.flatnonzero(two)
    if k.size:
        alo[k], ahi[k] = sync_metric_two(ph[k], ev[k], kind[k], pherr[k])
        big = big.copy(); big[k] |= ahi[k] >= REF_BIG
    E = np.where(own, F32(0), np.where(big | (nev > 2), REF_BIG, np.sqrt(s))).astype(F32)
    return pherr, slope, E, alo, ahi


def ref_pherr_range(p, alo, ahi, E):
    p = np.asarray(p, dtype=F32); alo = np.asarray(alo, dtype=F32); ahi = np.asarray(ahi, dtype=F32); E = np.asarray(E, dtype=F32)
    a = np.where(p < alo, p, alo); b = np.where(p > ahi, p, ahi)
    with np.errstate(all="ignore"):
        lo = a - ref_pherr_margin(a, E); hi = b + ref_pherr_margin(b, E)
    untab = ~(p < PHERR_BIG); cannot = E >= REF_BIG
    lo = np.where(untab, PHERR_BIG, np.where(cannot, F32(0), lo)); hi = np.where(untab, PHERR_BIG, np.where(cannot, REF_BIG, hi))
    return lo.astype(F32), hi.astype(F32)


def ref_vertex_marginal(y1lo, y1hi, y2lo, y2hi, y3lo, y3hi):
    lo = [np.asarray(v, dtype=F32) for v in (y1lo, y2lo, y3lo)]; hi = [np.asarray(v, dtype=F32) for v in (y1hi, y2hi, y3hi)]
    with np.errstate(all="ignore"):
        c = [F32(0.5) * (lo[k] + hi[k]) for k in range(3)]
        out = (hi[0] - lo[0] > F32(100)) | (hi[1] - lo[1] > F32(100)) | (hi[2] - lo[2] > F32(100))
        v0 = parabola_vertex(c[0], c[1], c[2])
        d2 = np.zeros(v0.shape, dtype=F32)
        for k in range(3):
            a = parabola_vertex(*[lo[j] if j == k else c[j] for j in range(3)])
            b = parabola_vertex(*[hi[j] if j == k else c[j] for j in range(3)])
            out = out | np.isnan(a) | np.isnan(b) | (np.abs(a) > F32(1.0e6)) | (np.abs(b) > F32(1.0e6))
            d = np.maximum(np.abs(a - v0), np.abs(b - v0))          # (fmaxf: a NaN operand is dropped - those elements are decided already)
            d2 = d2 + d * d
        out = out | np.isnan(v0)
        d = np.sqrt(d2) + F32(1e-5)
        ra = _roundf(v0 - d); rb = _roundf(v0 + d)
        return out | (ra != rb)


def ref_candidate_verdict(r0, r3, f3, E3, r6, max_ppm, ppm_thr):
    """r0, r3, r6: (lo, hi) pairs of float32 [n] -> int32 [n]: bit 0 may fire, bit 1 within the margin"""
    (r0lo, r0hi), (r3lo, r3hi), (r6lo, r6hi) = [(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)) for a, b in (r0, r3, r6)]
    f3 = np.asarray(f3, dtype=F32); E3 = np.asarray(E3, dtype=F32); max_ppm = np.asarray(max_ppm, dtype=F32); ppm_thr = np.asarray(ppm_thr, dtype=F32)
    tab = (r3lo < PHERR_BIG) & (r0lo < PHERR_BIG)
    possibly = tab & (r3lo < SYNC_THR) & (r0hi > r3lo)
    surely = (r3hi < SYNC_THR) & (r0lo > r3hi)
    big = np.full(r3lo.shape, PHERR_BIG, dtype=F32)
    marg = ~surely | ref_vertex_marginal(big, big, r3lo, r3hi, r0lo, r0hi) | ((r6lo < PHERR_BIG) & ref_vertex_marginal(r6lo, r6hi, r3lo, r3hi, r0lo, r0hi))
    with np.errstate(all="ignore"):
        marg = marg | ((max_ppm != 0) & (np.abs(np.abs(f3) - ppm_thr) <= ref_slope_margin(E3)))
    return np.where(possibly, 1 + 2 * marg, 0).astype(np.int32)


def ref_symbol_dist(phi, prev_phi, vdphi):
    phi = np.asarray(phi, dtype=F32); prev_phi = np.asarray(prev_phi, dtype=F32); vdphi = np.asarray(vdphi, dtype=F32)
    dphi = (phi - prev_phi) - vdphi
    d64 = dphi.astype(np.float64)
    dphi = np.where(dphi < 0, (d64 + TWO_PI).astype(F32), np.where(d64 > TWO_PI, (d64 - TWO_PI).astype(F32), dphi)).astype(F32)
    dphi = (dphi.astype(np.float64) / (np.pi / 4)).astype(F32)
    fr = dphi - np.floor(dphi)
    return np.abs(fr - F32(0.5)) * F32(np.pi / 4)


def ref_symbol_marginal(phi, prev_phi, vdphi, e_sum):
    return ref_symbol_dist(phi, prev_phi, vdphi) <= np.asarray(e_sum, dtype=F32) + F32(2e-6)


def ref_candidate_code(y1, y2, y3, prevd, max_ppm, ppm_thr):
    """got_sync()'s outcome (vdl2_core.h: ref_candidate_code): bit 0 fires, bit 1 passes the --max-ppm gate, bits 8-15 sclk + 64"""
    y1 = np.asarray(y1, dtype=F32); y2 = np.asarray(y2, dtype=F32); y3 = np.asarray(y3, dtype=F32); prevd = np.asarray(prevd, dtype=F32)
    fires = (y2 < SYNC_THR) & (y3 > y2)
    with np.errstate(all="ignore"):
        v = np.where(fires, parabola_vertex(y1, y2, y3), F32(0))
    sclk = (-_roundf(np.where(np.isfinite(v), v, 0))).astype(np.int64)       # (a fire has y3 > y2: its vertex with y1 >= y2 is finite)
    passes = ~((F32(max_ppm) != 0) & (np.abs(prevd) > F32(ppm_thr)))
    return np.where(fires, 1 | (passes.astype(np.int64) << 1) | (((sclk + 64) & 0xff) << 8), 0).astype(np.int64)


# what sync_metric_ref() promises, checked without its arithmetic: the metric run again in float64 with the listed decisions taken the
# other way, and where E has to be kRefBig (for any build's output: the host's in tests/test_core_reference_referee.py, the device's in
# tests/test_gpu_referee_probe.py)
def metric64(ph, flips, cuts):
    """the sync metric in float64 on the float32 phases ph [n, 16] with the unwrap steps the float32 metric takes,
    the decisions at the taps flips (bool [n, 16]) taken the other way and the taps cuts (bool [n, 16]) read as -phase"""
    q = np.where(cuts, -ph, ph).astype(np.float64)
    cur = q - PR_PHASE.astype(np.float64)[None, :]
    # a negated tap changes the differences either side of it: their decisions are the float32 metric's on the negated phases
    q32 = np.where(cuts, -ph, ph).astype(F32)
    _, _, st, diff = _unwrapped(q32)
    st = np.where(flips, np.where(st != 0, 0.0, np.where(diff > 0, -TWO_PI, TWO_PI)), st)
    e = cur + np.cumsum(st, axis=1)
    e = e - e.mean(axis=1, keepdims=True)
    x = np.arange(16) - 7.5
    slope = (e * x).sum(axis=1) / (x * x).sum()
    r = e - slope[:, None] * x
    return (r * r).sum(axis=1)


def check_alternatives_and_E(ph, eps2, out, full, label):
    """out: (pherr, slope, E, alo, ahi) of some build.  Independent of the restatement's arithmetic (its list of events is used)"""
    pherr, E, alo, ahi = out[:, 0], out[:, 2], out[:, 3], out[:, 4]
    nev, ev, kind, _, _ = ref_events(ph, eps2)
    zero_tap = (eps2 >= REF_BIG).any(axis=1)
    two_unwraps = (nev == 2) & (kind[:, 0] == 0) & (kind[:, 1] == 0)
    must_be_big = zero_tap | (nev > 2) | (two_unwraps & (not full))
    own = (eps2 == 0).all(axis=1)
    got_big = E == REF_BIG
    bad = np.flatnonzero(got_big != must_be_big)
    assert bad.size == 0, f"{label}: E == kRefBig at {got_big.sum()} windows, expected at {must_be_big.sum()}; first {bad[:5]}: nev {nev[bad[:5]]}"
    assert np.all(E[own] == 0) and np.all(alo[own].view(np.uint32) == pherr[own].view(np.uint32)) and np.all(ahi[own].view(np.uint32) == pherr[own].view(np.uint32)), label
    taps = np.arange(16)[None, :]
    worst = 0.0; checked = 0
    for subset in ((0,), (1,), (0, 1)):
        sel = ~got_big & (nev > max(subset))
        k = np.flatnonzero(sel)
        if k.size == 0:
            continue
        flips = np.zeros((k.size, 16), dtype=bool); cuts = np.zeros((k.size, 16), dtype=bool)
        for j in subset:
            hit = taps == ev[k, j][:, None]
            flips |= hit & (kind[k, j] == 0)[:, None]; cuts |= hit & (kind[k, j] == 1)[:, None]
        v = metric64(ph[k], flips, cuts)
        # float32 against float64 on the metric itself: the source's own figure for it (vdl2_core.h, sync_metric_unwrap_alts: "a few 1e-5
        # on values of tens to hundreds") - 1e-3 + 2e-5 |v|
        tol = 1e-3 + 2e-5 * np.abs(v)
        out_by = np.maximum(alo[k].astype(np.float64) - v, v - ahi[k].astype(np.float64))
        worst = max(worst, float((out_by / tol).max())); checked += k.size
        b = np.flatnonzero(out_by > tol)
        assert b.size == 0, (f"{label}: decisions {subset} taken the other way: {b.size} of {k.size} float64 values outside [alo, ahi]; first window {k[b[0]]}: "
                             f"{v[b[0]]:.6f} not in [{alo[k[b[0]]]:.6f}, {ahi[k[b[0]]]:.6f}], events {ev[k[b[0]]]} kinds {kind[k[b[0]]]}")
    print(f"{label}: {checked} alternatives re-run in float64, the worst outside [alo, ahi] by {worst:.3f} of the allowance; E = kRefBig at {got_big.sum()} windows")
    return checked



# ------------------------------------------------------------------------------------------------------------------------------
# input sets
# ------------------------------------------------------------------------------------------------------------------------------
def ulp_neighbours(x):
    """x, the float32 below and the float32 above, for every x"""
    x = np.asarray(x, dtype=F32).reshape(-1)
    return np.concatenate([x, np.nextafter(x, F32(-np.inf)), np.nextafter(x, F32(np.inf))]).astype(F32)


def wrap(x):
    return (x + np.pi) % (2 * np.pi) - np.pi


def metric_windows():
    """float32 [n, 16] phases in radians: tests/test_design.py's sets (random windows, preambles with slope +-3 rad/symbol and noise
    of sigma 0 .. 0.8, windows at the +-pi decision), then windows with one tap difference exactly at +-kPiBelow and one float
    either side of it, all-zero phases and phases of +-pi.  Returns (windows, number of windows of the test_design.py sets)"""
    rng = np.random.default_rng(5)
    q = Q_EIGHTHS.astype(np.float64) * np.pi / 4
    sets = [rng.uniform(-np.pi, np.pi, size=(200000, 16))]
    for sigma in (0.0, 0.05, 0.3, 0.5, 0.6, 0.8):
        n = 60000
        slope = rng.uniform(-3.0, 3.0, size=(n, 1)); off = rng.uniform(-np.pi, np.pi, size=(n, 1))
        sets.append(wrap(q[None, :] + off + slope * np.arange(16)[None, :] + sigma * rng.standard_normal((n, 16))))
    sets.append(wrap(q[None, :] + np.pi * np.arange(16)[None, :] * rng.choice([-1.0, 1.0], size=(50000, 1)) + 1e-3 * rng.standard_normal((50000, 16))))
    design = np.concatenate(sets).astype(F32)
    # one tap difference at the unwrap decision: cur[i] - cur[i-1] = target, with cur = ph - pr_phase in float.  Phases under 4 in
    # magnitude differ by whole multiples of 2^-22 or less, so ph[i] is searched among the floats next to the one aimed at
    rng = np.random.default_rng(6)
    extra = []
    for sign in (1.0, -1.0):
        for target in ulp_neighbours(PI_BELOW):
            for i in range(1, 16):
                w = wrap(q[None, :] + 0.3 * rng.standard_normal((40, 16))).astype(F32)
                w[:, i - 1] = rng.uniform(-1.0, 1.0, 40).astype(F32) * F32(0.5) + PR_PHASE[i - 1]
                prev = w[:, i - 1] - PR_PHASE[i - 1]
                aim = (prev.astype(np.float64) + sign * float(target) + float(PR_PHASE[i])).astype(F32)
                best = aim.copy(); err = np.full(40, np.inf)
                for off in range(-2, 3):                     # the float aimed at and two either side
                    cand = aim
                    for _ in range(abs(off)):
                        cand = np.nextafter(cand, F32(9 if off > 0 else -9))
                    d = (cand - PR_PHASE[i]) - prev
                    e_ = np.abs(d.astype(np.float64) - sign * float(target))
                    take = e_ < err
                    best = np.where(take, cand, best); err = np.where(take, e_, err)
                w[:, i] = best
                extra.append(w)
    extra.append(np.zeros((4, 16), dtype=F32))
    for v in (F32(np.pi), -F32(np.pi), PI_BELOW, -PI_BELOW):
        extra.append(np.full((2, 16), v, dtype=F32))
    alt = np.full((4, 16), F32(np.pi), dtype=F32); alt[0, ::2] *= -1; alt[1, 1::2] *= -1; alt[2, :8] *= -1; alt[3, 8:] *= -1
    extra.append(alt)
    extra = np.concatenate(extra).astype(F32)
    return np.ascontiguousarray(np.concatenate([design, extra])), len(design)


def tap_differences(ph):
    """cur[i] - cur[i-1] of sync_metric() (float32 [n, 15]): what the unwrap decision looks at"""
    cur = np.asarray(ph, dtype=F32) - PR_PHASE[None, :]
    return cur[:, 1:] - cur[:, :-1]


def slice_inputs():
    """float32 [n, 3] = (phi, prev_phi, vdphi): random phases and slopes, phase steps within a float of 0, of 2 pi and of every odd
    multiple of pi/8 (where roundf() of dphi / (pi/4) ties), and steps under -2 pi (the reference's negative index)"""
    rng = np.random.default_rng(7)
    n = 600000
    a = np.empty((n, 3), dtype=F32)
    a[:, 0] = rng.uniform(-np.pi, np.pi, n); a[:, 1] = rng.uniform(-np.pi, np.pi, n); a[:, 2] = rng.uniform(-0.5, 0.5, n)
    sets = [a]
    # ties: phi - prev - vdphi lands next to k pi/8 (k odd), to 0 and to +-2 pi, before or after the +-2 pi step
    targets = np.concatenate([np.arange(-31, 32, 2) * np.pi / 8, [0.0, TWO_PI, -TWO_PI, 4 * np.pi, -4 * np.pi]])
    for vd in (0.0, 0.1, -0.25):
        for t in targets:
            m = 400
            prev = rng.uniform(-np.pi, np.pi, m).astype(F32)
            phi = (prev.astype(np.float64) + vd + t).astype(F32)
            k = rng.integers(-3, 4, m)
            for _ in range(3):
                phi = np.where(k > 0, np.nextafter(phi, F32(99)), np.where(k < 0, np.nextafter(phi, F32(-99)), phi)).astype(F32)
                k = k - np.sign(k)
            sets.append(np.stack([phi, prev, np.full(m, vd, dtype=F32)], axis=1).astype(F32))
    # with prev = vdphi = 0 the step IS phi: every float around the ties themselves
    t32 = np.concatenate([ulp_neighbours((np.arange(-63, 64) * np.pi / 8).astype(F32)), ulp_neighbours(ulp_neighbours(F32(TWO_PI))), ulp_neighbours(-F32(TWO_PI)),
                          np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38], dtype=F32)])
    # ... and the floats whose quotient by pi/4 is next to a half: x = (k + 0.5) pi/4 rounded, and its neighbours
    t32 = np.concatenate([t32, ulp_neighbours(ulp_neighbours(((np.arange(-20, 20) + 0.5) * np.pi / 4).astype(F32)))])
    z = np.zeros(len(t32), dtype=F32)
    sets.append(np.stack([t32, z, z], axis=1))
    sets.append(np.stack([z, -t32, z], axis=1))
    sets.append(np.stack([z, z, -t32], axis=1))
    # far negative steps: the index stays negative after one +2 pi (neg path), up to a few turns
    m = 20000
    b = np.empty((m, 3), dtype=F32)
    b[:, 0] = rng.uniform(-np.pi, np.pi, m); b[:, 1] = rng.uniform(-np.pi, np.pi, m); b[:, 2] = rng.uniform(-20.0, 20.0, m)
    sets.append(b)
    return np.ascontiguousarray(np.concatenate(sets).astype(F32))


def vertex_inputs():
    """float32 [n, 3] = (y1, y2, y3): random metrics, equal triples (a = b = 0: 0/0), collinear triples (a -> 0) and near-collinear ones"""
    rng = np.random.default_rng(8)
    n = 500000
    a = rng.uniform(0.0, 8.0, size=(n, 3)).astype(F32)
    eq = np.repeat(rng.uniform(0.0, 8.0, size=(1000, 1)), 3, axis=1).astype(F32)
    y1 = rng.uniform(0.0, 8.0, 20000); st = rng.uniform(-2.0, 2.0, 20000)
    col = np.stack([y1, y1 + st, y1 + 2 * st], axis=1).astype(F32)
    near = col.copy(); near[:, 1] = np.nextafter(near[:, 1], F32(99))
    grid = np.stack([np.full(8, 2.0), np.array([1.0, 1.5, 1.75, 2.0, 2.25, 2.5, 3.0, 0.0]), np.full(8, 3.0)], axis=1).astype(F32)     # exact small numbers
    big = (rng.uniform(0.0, 1.0, size=(2000, 3)) * 1e30).astype(F32)
    tiny = (rng.uniform(0.0, 1.0, size=(2000, 3)) * 1e-38).astype(F32)
    zero = np.zeros((2, 3), dtype=F32); zero[1, 1] = -0.0
    return np.ascontiguousarray(np.concatenate([a, eq, col, near, grid, big, tiny, zero]).astype(F32))


def ppm_inputs(plan_freqs):
    """(vdphi float32 [n], freq uint32 [n], max_ppm float32 [n]): random slopes on random VHF frequencies and gates, then every channel
    of plan_freqs with max_ppm 5 and 15, each with vdphi at its own gate threshold and the floats either side"""
    rng = np.random.default_rng(12)
    n = 200000
    vd = rng.uniform(-1.0, 1.0, n).astype(F32)
    fr = rng.integers(118_000_000, 137_000_000, n).astype(np.uint32)
    mp = rng.uniform(0.5, 50.0, n).astype(F32)
    pf = np.asarray(plan_freqs, dtype=np.uint32)
    for g in (5.0, 15.0):
        gate = np.full(len(pf), g, dtype=F32)
        thr = ppm_gate_threshold(pf, gate)
        for v in (thr, np.nextafter(thr, F32(9)), np.nextafter(thr, F32(0)), -thr, -np.nextafter(thr, F32(9))):
            vd = np.concatenate([vd, v.astype(F32)]); fr = np.concatenate([fr, pf]); mp = np.concatenate([mp, gate])
    edge_v = np.array([0.0, -0.0, 1e-45, 3.0e38, -3.0e38, 1e-30], dtype=F32)
    vd = np.concatenate([vd, edge_v]); fr = np.concatenate([fr, np.full(len(edge_v), 136975000, dtype=np.uint32)]); mp = np.concatenate([mp, np.full(len(edge_v), 5.0, dtype=F32)])
    return np.ascontiguousarray(vd.astype(F32)), np.ascontiguousarray(fr.astype(np.uint32)), np.ascontiguousarray(mp.astype(F32))


def _steps(x, k):
    """x moved k floats up (k < 0: down), element-wise k"""
    x = np.asarray(x, dtype=F32).copy(); k = np.asarray(k).copy()
    while np.any(k != 0):
        x = np.where(k > 0, np.nextafter(x, F32(np.inf)), np.where(k < 0, np.nextafter(x, F32(-np.inf)), x)).astype(F32)
        k = k - np.sign(k)
    return x


def ref_windows():
    """(ph float32 [n, 16], eps2 float32 [n, 16], name -> slice): metric_windows() thinned, with the error figures of their taps
    own       every eps2 zero: all sixteen taps are the reference's own (E = 0, alo = ahi = pherr)
    stream    sqrt(eps2) = kRefKappa x 1 .. 150: what ref_eps2() gives on a stream whose level moves by up to 43 dB within four samples
    faded     sqrt(eps2) 1e-3 .. 0.3 rad, a quarter of the taps exact: discontinuities by the handful - none to five per window, of both kinds
    decision  metric_windows()'s own edge windows (a tap difference at +-kPiBelow and the floats either side, all-zero and +-pi phases)
              with every sqrt(eps2) = 1e-7, and again with 1e-3
    cut       one tap's phase at +-(kPiBelow - sqrt(eps2) - 1e-6), the edge of the branch-cut test, and up to three floats either side
    big       `stream` windows with one tap's eps2 = kRefBig, or the float below it"""
    rng = np.random.default_rng(21)
    ph, ndesign = metric_windows()
    parts = []

    def add(name, p, e):
        parts.append((name, np.ascontiguousarray(p, dtype=F32), np.ascontiguousarray(e, dtype=F32)))
    own = ph[:ndesign][3::40]
    add("own", own, np.zeros(own.shape))
    st = ph[:ndesign][::10]
    add("stream", st, (REF_KAPPA * np.exp(rng.uniform(0.0, 5.0, st.shape))) ** 2)
    fd = ph[:ndesign][5::10]
    sq = np.exp(rng.uniform(np.log(1e-3), np.log(0.3), fd.shape)) * (rng.uniform(size=fd.shape) > 0.25)
    add("faded", fd, sq ** 2)
    ed = ph[ndesign:]
    add("decision", np.concatenate([ed, ed]), np.concatenate([np.full(ed.shape, 1e-14), np.full(ed.shape, 1e-6)]))
    q = Q_EIGHTHS.astype(np.float64) * np.pi / 4
    n = 6000
    w = wrap(q[None, :] + rng.uniform(-np.pi, np.pi, (n, 1)) + rng.uniform(-0.2, 0.2, (n, 1)) * np.arange(16)[None, :] + 0.3 * rng.standard_normal((n, 16))).astype(F32)
    e = np.full((n, 16), 1e-8, dtype=F32)
    tap = rng.integers(0, 16, n); rows = np.arange(n)
    e[rows, tap] = rng.choice(np.array([1e-6, 1e-4, 2.5e-3], dtype=F32), n)
    edge = PI_BELOW - (np.sqrt(e[rows, tap]) + F32(1e-6))
    w[rows, tap] = _steps(edge, rng.integers(-3, 4, n)) * rng.choice(np.array([-1.0, 1.0], dtype=F32), n)
    add("cut", w, e)
    bg = ph[:ndesign][7::100]
    eb = ((REF_KAPPA * np.exp(rng.uniform(0.0, 5.0, bg.shape))) ** 2).astype(F32)
    rows = np.arange(len(bg))
    eb[rows, rng.integers(0, 16, len(bg))] = np.where(rng.uniform(size=len(bg)) < 0.5, REF_BIG, np.nextafter(REF_BIG, F32(0)))
    add("big", bg, eb)
    where = {}; k = 0
    for name, p, _ in parts:
        where[name] = slice(k, k + len(p)); k += len(p)
    return np.concatenate([p for _, p, _ in parts]), np.concatenate([e_ for _, _, e_ in parts]), where


VERDICT_FREQ = 136975000


def verdict_inputs():
    """float32 [n, 15] = (p, alo, ahi, E) of n, (p, alo, ahi, E, slope) of n-3, (p, alo, ahi, E) of n-6, max_ppm, ppm_thr: metrics
    around kSyncThr and around each other; E zero, small, large and kRefBig; alternatives equal to p, below and above; n-6 absent
    (kPherrBig) in a third; the gate off and at 5 ppm with |slope| anywhere and within two margins of the gate's threshold; then p(n-3)
    within a few floats of the places where an end of its range crosses kSyncThr, and p(n) likewise around the ends of p(n-3)'s range"""
    rng = np.random.default_rng(22)
    n = 300000
    thr = ppm_gate_threshold(np.array([VERDICT_FREQ], dtype=np.uint32), np.array([5.0], dtype=F32))[0]

    def err(m):
        kind = rng.integers(0, 8, m)
        return np.where(kind == 0, 0.0, np.where(kind == 7, float(REF_BIG), np.exp(rng.uniform(np.log(1e-3), np.log(3.0), m)))).astype(F32)

    def alts(p):
        kind = rng.integers(0, 4, len(p))
        lo = np.where(kind == 1, p - rng.uniform(0, 3, len(p)), p); hi = np.where(kind >= 2, p + rng.uniform(0, 30, len(p)), p)
        return np.maximum(lo, 0).astype(F32), hi.astype(F32)
    a = np.zeros((n, 15), dtype=F32)
    p3 = rng.uniform(0.0, 8.0, n).astype(F32)
    p0 = np.maximum(p3 + rng.uniform(-1.0, 3.0, n) * rng.choice([1.0, 1e-2, 1e-4], n), 0).astype(F32)
    p6 = np.where(rng.uniform(size=n) < 1 / 3, PHERR_BIG, np.maximum(p3 + rng.uniform(-1.0, 5.0, n), 0)).astype(F32)
    a[:, 0] = p0; a[:, 1], a[:, 2] = alts(p0); a[:, 3] = err(n)
    a[:, 4] = p3; a[:, 5], a[:, 6] = alts(p3); a[:, 7] = err(n)
    a[:, 9] = p6; a[:, 10], a[:, 11] = alts(p6); a[:, 12] = err(n)
    near = rng.uniform(size=n) < 0.5
    with np.errstate(all="ignore"):
        f_near = (thr + rng.uniform(-2.0, 2.0, n) * ref_slope_margin(np.minimum(a[:, 7], F32(10)))).astype(F32)
    a[:, 8] = np.where(near, f_near, rng.uniform(0.0, 0.6, n)).astype(F32) * rng.choice(np.array([-1.0, 1.0], dtype=F32), n)
    a[:, 13] = np.where(rng.uniform(size=n) < 0.5, 0.0, 5.0); a[:, 14] = np.where(a[:, 13] != 0, thr, np.inf)
    # the threshold and the candidate test to the float: E = 0 leaves the margin 4e-6 p + 1e-6, an end of the range crosses within floats
    m = 40000
    b = np.zeros((m, 15), dtype=F32)
    side = rng.integers(0, 2, m)
    x = np.where(side == 0, 4.0 / (1 - 4e-6) + 1e-6, 4.0 / (1 + 4e-6) - 1e-6)          # where lo = 4 / where hi = 4, to first order
    b3 = _steps(x.astype(F32), rng.integers(-6, 7, m))
    b[:, 4] = b3; b[:, 5] = b3; b[:, 6] = b3
    lo3, hi3 = ref_pherr_range(b3, b3, b3, np.zeros(m, dtype=F32))
    also = rng.integers(0, 3, m)                                                       # p(n) far above, or at an end of p(n-3)'s range
    b0 = np.where(also == 0, b3 + F32(2), _steps(np.where(also == 1, lo3, hi3) * F32(1 + 4e-6), rng.integers(-40, 41, m)))
    b[:, 0] = b0; b[:, 1] = b0; b[:, 2] = b0
    b[:, 9] = np.where(rng.uniform(size=m) < 0.5, PHERR_BIG, b3 + F32(1)); b[:, 10] = b[:, 9]; b[:, 11] = b[:, 9]
    b[:, 14] = np.inf
    b[::2, 4] = _steps(np.full(m // 2, 3.5, dtype=F32), rng.integers(-3, 4, m // 2)); b[::2, 5] = b[::2, 4]; b[::2, 6] = b[::2, 4]
    lo3, hi3 = ref_pherr_range(b[::2, 4], b[::2, 4], b[::2, 4], np.zeros(m // 2, dtype=F32))
    b[::2, 0] = _steps(np.where(rng.uniform(size=m // 2) < 0.5, lo3, hi3), rng.integers(-60, 61, m // 2)); b[::2, 1] = b[::2, 0]; b[::2, 2] = b[::2, 0]
    return np.ascontiguousarray(np.concatenate([a, b]).astype(F32))


def vertex_for(v, y2, y3):
    """y1 for which parabola_vertex(y1, y2, y3) = v, in exact arithmetic"""
    return (36 * y2 - 27 * y3 + v * (12 * y2 - 6 * y3)) / (9 + 6 * v)


def vertex_boxes():
    """float32 [n, 6] = (y1.lo, y1.hi, y2.lo, y2.hi, y3.lo, y3.hi): boxes around fires (y2 < 4 < y3 or so) with y1 = kPherrBig exactly or
    a value of its own, widths 1e-6 .. 10 and, rarely, beyond 100; boxes whose centre's vertex is within a few 1e-4 of a rounding
    boundary k + 1/2, narrower and wider than that distance; boxes around collinear triples (the denominator changes sign inside)"""
    rng = np.random.default_rng(23)

    def boxes(c, wd):
        out = np.empty((len(c), 6), dtype=F32)
        out[:, 0::2] = c - 0.5 * wd; out[:, 1::2] = c + 0.5 * wd
        return out
    n = 200000
    y2 = rng.uniform(0.0, 5.0, n); y3 = y2 + rng.uniform(-0.2, 4.0, n)
    y1 = np.where(rng.uniform(size=n) < 0.4, float(PHERR_BIG), y2 + rng.uniform(-0.5, 6.0, n))
    wd = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), (n, 3))) * (rng.uniform(size=(n, 3)) > 0.2)
    wd[rng.uniform(size=n) < 0.01, 1] = 150.0
    wd[:, 0] = np.where(y1 == float(PHERR_BIG), 0.0, wd[:, 0])
    sets = [boxes(np.stack([y1, y2, y3], axis=1), wd)]
    m = 60000
    y2 = rng.uniform(0.5, 4.0, m); y3 = y2 + rng.uniform(0.05, 3.0, m)
    v = rng.integers(-3, 3, m) + 0.5 + rng.uniform(-3e-4, 3e-4, m)
    wd = np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), (m, 3)))
    sets.append(boxes(np.stack([vertex_for(v, y2, y3), y2, y3], axis=1), wd))
    m = 20000
    y2 = rng.uniform(0.5, 4.0, m); y3 = y2 + rng.uniform(0.05, 3.0, m)
    wd = np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), (m, 3)))
    sets.append(boxes(np.stack([2 * y2 - y3 + rng.uniform(-1.0, 1.0, m) * wd[:, 0], y2, y3], axis=1), wd))
    return np.ascontiguousarray(np.concatenate(sets).astype(F32))


def symbol_inputs():
    """float32 [n, 4] = (phi, prev_phi, vdphi, e_sum): slice_inputs() thinned; e_sum anywhere from 1e-6 to 0.5 rad, and at the decision
    itself: ref_symbol_dist() - 2e-6 and up to three floats either side"""
    rng = np.random.default_rng(24)
    a = slice_inputs()[::4]
    n = len(a)
    d = ref_symbol_dist(a[:, 0], a[:, 1], a[:, 2])
    at = _steps(d - F32(2e-6), rng.integers(-3, 4, n))
    e = np.where(rng.uniform(size=n) < 0.5, at, np.exp(rng.uniform(np.log(1e-6), np.log(0.5), n))).astype(F32)
    return np.ascontiguousarray(np.concatenate([a, e[:, None]], axis=1).astype(F32))


PHASE_EDGES = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [1, 1], [-1, 1], [1, -1], [-1, -1], [1e-30, 1], [1, 1e-30], [-1e-30, -1],
                        [3, 0.1875], [0.1875, 3], [1, 0.0625], [1, 0.062500004], [-2, 1e-38], [1e-38, -2], [-1, -0.0],
                        [5e-39, 1e-45], [1e-45, -5e-39]], dtype=F32)          # tests/test_phase.py's edge list


def phase_inputs():
    """float32 [n, 2] = (re, im): tests/test_phase.py's random set (4 10^6 samples, magnitudes e^-20 .. e^2, every angle), its edge
    list and the negated edge list; all four signed-zero pairs, (+-0, +-x) and (+-x, +-0); subnormal components down to 1e-45; ratios
    min/max within a float either side of every k/16 (where atan2_f64's reduction switches), in every octant; 1e19-scale samples.
    Returns (xy, name -> slice)"""
    rng = np.random.default_rng(9)                       # (tests/test_phase.py's own seed: the very same 4 10^6 samples)
    n = 4_000_000
    mag = np.exp(rng.uniform(-20, 2, n)); ang = rng.uniform(-np.pi, np.pi, n)
    rnd = np.empty((n, 2), dtype=F32)
    rnd[:, 0] = mag * np.cos(ang); rnd[:, 1] = mag * np.sin(ang)
    zz = np.array([[0.0, 0.0], [0.0, -0.0], [-0.0, 0.0], [-0.0, -0.0]], dtype=F32)
    xs = np.array([1.0, 3.5e-3, 2.0e19, 1.17549435e-38, 1e-38, 5e-39, 1e-42, 1e-45, 3.0e38], dtype=F32)
    axes = []
    for x in xs:
        for s in (1.0, -1.0):
            for z in (0.0, -0.0):
                axes.append([s * x, z]); axes.append([z, s * x])
    axes = np.array(axes, dtype=F32)
    sub = []
    subs = np.array([1e-45, 3e-45, 1e-42, 1e-40, 2.9e-39, 3.0e-39, 5e-39, 1.1e-38, 1.17549421e-38], dtype=F32)
    others = np.concatenate([subs, np.array([1.17549435e-38, 2e-38, 1e-30, 1.0], dtype=F32)])
    for a in subs:
        for b in others:
            for sa in (1.0, -1.0):
                for sb in (1.0, -1.0):
                    sub.append([sa * a, sb * b]); sub.append([sb * b, sa * a])
    sub = np.array(sub, dtype=F32)
    sw = []
    for mx in (F32(1.0), F32(1.7), F32(3.1e-5), F32(2.0e19)):
        for k in range(0, 17):
            r = ulp_neighbours(ulp_neighbours(F32(k / 16.0)))
            mn = (r * mx).astype(F32)
            mn = np.concatenate([mn, np.nextafter(mn, F32(99)), np.nextafter(mn, F32(-99))])
            mn = mn[(mn >= 0) & (mn <= mx)]
            for sx in (1.0, -1.0):
                for sy in (1.0, -1.0):
                    sw.append(np.stack([np.full(len(mn), sx * mx), sy * mn], axis=1)); sw.append(np.stack([sy * mn, np.full(len(mn), sx * mx)], axis=1))
    sw = np.concatenate(sw).astype(F32)
    big = (rng.standard_normal((2000, 2)) * 1e19).astype(F32)
    parts = [("random", rnd), ("edges", PHASE_EDGES), ("neg_edges", -PHASE_EDGES), ("zeros", zz), ("axes", axes), ("subnormal", sub), ("switch", sw), ("big", big)]
    where = {}; k = 0
    for name, p in parts:
        where[name] = slice(k, k + len(p)); k += len(p)
    return np.ascontiguousarray(np.concatenate([p for _, p in parts]).astype(F32)), where


# ------------------------------------------------------------------------------------------------------------------------------
# the device builds (vdl2hip_debug_core_probe: kernels.h k_core_probe), for the GPU tests
# ------------------------------------------------------------------------------------------------------------------------------
PROBE = {"phase": (0, 2, 1), "phase_fast": (1, 2, 1), "mag": (2, 2, 1), "metric": (3, 16, 2), "screen": (4, 16, 2), "slice": (5, 3, 2),
         "vertex": (6, 3, 1), "ppm": (7, 3, 2), "ref_full": (9, 32, 5), "ref_plain": (10, 32, 5), "verdict": (11, 15, 7),
         "vertex_marginal": (12, 6, 1), "symbol": (13, 4, 2)}           # name -> (kind, 32-bit words in, words out) per element


def device_probe(L, name, a):
    """a: [n, words in] float32 (or uint32 bit patterns) -> float32 [n, words out] as the device build of the helper computes it"""
    import ctypes as C
    kind, win, wout = PROBE[name]
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4 and a.ndim == 2 and a.shape[1] == win, (name, a.dtype, a.shape)
    out = np.full((len(a), wout), np.nan, dtype=F32)
    L.vdl2hip_debug_core_probe.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    rc = L.vdl2hip_debug_core_probe(kind, a.ctypes.data, len(a), out.ctypes.data)
    assert rc == 0, f"vdl2hip_debug_core_probe({name}) = {rc}"
    return out
