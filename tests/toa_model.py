"""The float64 model of the burst timing tap (include/vdl2hip.h, "Burst timing"; dumpvdl2_amd/csrc/toa.h) and its bounds.

design():            the template in float64, as the definition writes it (what vdl2hip_toa_template() is compared with)
correlate():         c64(tau), P64(tau), the bound b(tau) and the bound on |P - P64| for one burst, from the float32 template and y
derive():            everything from "Peak" down as exact arithmetic on a delivered float32 curve, E_y and the two half sums' phase
energy():            E_y at one lag
check_record():      one delivered record and curve against all of it (used by the host and the GPU tests alike)

The bounds' derivation.  u[n] carries the rounding of cosine and sine (2^-24 each) and of a product and a fused multiply-add; a tap's
product passes through at most two fused multiply-adds per earlier tap of its lane (three taps) and six additions of the tree: fewer
than 16 roundings in all, each at most 2^-24 of the sum of the magnitudes it has seen - the definition states (151 + 16) 2^-24
sum |s| |y|, which covers any order of the 151 taps.  P is a product and a fused multiply-add of c's components: 2^-22 P64 covers
their two roundings, the rest is |c|^2 - |c64|^2 <= 2 |c64| b + b^2.  A phase moves by at most asin(b / |c|) when c moves by b."""
import numpy as np

TAPS, LEAD, HALF = 151, 160, 75
EARLY, EDGE, FLAT, NO_CURVE = 1, 2, 4, 8
Q = np.array([0, 3, -3, 1, 1, 2, 0, 4, -3, 4, -2, 3, 1, -2, -3, 0], dtype=np.float64)      # demod.c:107-124, in units of pi / 4
EPS = 2.0 ** -24


def pulse(t):
    t = np.asarray(t, dtype=np.float64)
    return np.sinc(t) * np.cos(0.6 * np.pi * t) / (1.0 - (1.2 * t) ** 2)


def design():
    n = np.arange(TAPS, dtype=np.float64)
    s = np.zeros(TAPS, dtype=np.complex128)
    for i in range(16):
        s += np.exp(1j * Q[i] * np.pi / 4.0) * pulse((n - 10.0 * i) / 10.0)
    return s


def window(y_at, t0, W):
    """y_c[t0 - W .. t0 + W + 151) as complex128, zero before the stream's start.  y_at(first, count) -> complex array of samples first .. first + count - 1, first >= 0"""
    lo, n = t0 - W, TAPS + 2 * W
    out = np.zeros(n, dtype=np.complex128)
    a = max(lo, 0)
    if a < lo + n:
        out[a - lo:] = np.asarray(y_at(a, lo + n - a), dtype=np.complex128)
    return out


def correlate(s32, yw, dphi, W):
    """-> c64[nlags], P64, b, the bound on |P - P64|, and (c_a64, b_a, c_b64, b_b) per lag"""
    s = np.asarray(s32, dtype=np.complex64).astype(np.complex128)
    n = np.arange(TAPS, dtype=np.float64)
    u = np.conj(s) * np.exp(1j * (-float(np.float32(dphi)) * n / 10.0))
    nl = 2 * W + 1
    c = np.zeros(nl, dtype=np.complex128)
    b = np.zeros(nl)
    ca, cb = np.zeros(nl, dtype=np.complex128), np.zeros(nl, dtype=np.complex128)
    ba, bb = np.zeros(nl), np.zeros(nl)
    for k in range(nl):
        seg = yw[k:k + TAPS]
        prod, mag = u * seg, np.abs(s) * np.abs(seg)
        c[k], b[k] = prod.sum(), (TAPS + 16) * EPS * mag.sum()
        ca[k], ba[k] = prod[:HALF].sum(), (TAPS + 16) * EPS * mag[:HALF].sum()
        cb[k], bb[k] = prod[HALF:2 * HALF].sum(), (TAPS + 16) * EPS * mag[HALF:2 * HALF].sum()
    P = np.abs(c) ** 2
    return dict(c=c, P=P, b=b, Pbound=2.0 * np.abs(c) * b + b * b + 2.0 ** -22 * P, ca=ca, ba=ba, cb=cb, bb=bb)


def energy(yw, k):
    """E_y at lag index k: the float64 sum of the float32 re^2 + im^2"""
    seg = np.asarray(yw[k:k + TAPS]).astype(np.complex64)
    re, im = seg.real.astype(np.float64), seg.imag.astype(np.float64)
    return float((re * re + (im * im).astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64).sum())


def e_s(s32):
    s = np.asarray(s32, dtype=np.complex64)
    return float((s.real.astype(np.float64) ** 2 + s.imag.astype(np.float64) ** 2).sum())


def derive(P32, W, t0, dphi, E_y, E_s, resid32, kp=None):
    """the fields that are exact arithmetic on the delivered curve (float32), E_y and the narrowed resid (kp: the peak's index where
    the curve at hand is not the delivered one and cannot say which of two near-equal lags won)"""
    P = np.asarray(P32, dtype=np.float32)
    nl = 2 * W + 1
    assert P.size == nl
    if kp is None:
        kp = 0
        for k in range(1, nl):                              # the first of the largest: a float32 >
            if P[k] > P[kp]:
                kp = k
    a = float(P[kp - 1]) if kp > 0 else 0.0
    b = float(P[kp])
    c = float(P[kp + 1]) if kp + 1 < nl else 0.0
    den = (a - 2.0 * b) + c
    edge, flat = kp == 0 or kp == nl - 1, den >= 0.0
    frac = np.float32(0.0) if edge or flat else np.float32(0.5 * (a - c) / den)
    rho = np.float32(0.0) if E_y == 0.0 else np.float32(b / (E_s * E_y))
    cfo = np.float32((float(np.float32(dphi)) / 10.0 + float(np.float32(resid32))) * (105000.0 / (2.0 * np.pi)))
    return dict(kp=kp, peak_lag=kp - W, peak_sample=t0 + kp - W, toa_frac=frac, peak_power=P[kp], rho=rho, cfo_hz=cfo,
                flags=(EARLY if t0 - W < 0 else 0) | (EDGE if edge else 0) | (FLAT if flat else 0))


def angle_err(a, b):
    return abs((a - b + np.pi) % (2.0 * np.pi) - np.pi)


def asin_bound(b, c):
    return float(np.arcsin(min(1.0, b / abs(c)))) if abs(c) > 0.0 else np.pi


def check_record(rec, curve, s32, y_at, what=""):
    """One record (a mapping with vdl2hip_burst_toa's fields) and its curve (None: the record has none - then the model's own curve
    says which lags can have won) against the model on y.  Returns the largest curve error as a fraction
    of its bound."""
    nl = int(rec["nlags"])
    W = (nl - 1) // 2
    t0 = int(rec["first_symbol"]) - LEAD
    dphi = np.float32(rec["dphi"])
    yw = window(y_at, t0, W)
    m = correlate(s32, yw, dphi, W)
    worst = 0.0
    if curve is not None:
        curve = np.asarray(curve, dtype=np.float32)
        assert curve.size == nl, (what, curve.size, nl)
        err = np.abs(curve.astype(np.float64) - m["P"])
        assert np.all(err <= m["Pbound"]), (what, "curve", float((err - m["Pbound"]).max()))
        worst = float((err / np.maximum(m["Pbound"], 1e-300)).max()) if np.any(m["Pbound"] > 0) else 0.0
        assert not int(rec["flags"]) & NO_CURVE, what
        P32 = curve
    else:
        assert int(rec["flags"]) & NO_CURVE and int(rec["curve_off"]) == 0, what
        P32 = m["P"].astype(np.float32)
    kp = int(rec["peak_lag"]) + W
    assert 0 <= kp < nl, what
    if curve is None:                                       # the lag that won is one that can have: no other is larger by more than the bounds
        assert m["P"][kp] + m["Pbound"][kp] >= (m["P"] - m["Pbound"]).max(), (what, "peak_lag")
    E_y = energy(yw, kp)
    d = derive(P32, W, t0, dphi, E_y, e_s(s32), rec["resid"], kp=None if curve is not None else kp)
    assert int(rec["peak_lag"]) == d["peak_lag"] and int(rec["peak_sample"]) == d["peak_sample"], (what, rec["peak_lag"], d["peak_lag"])
    assert (int(rec["flags"]) & ~NO_CURVE) == d["flags"], (what, int(rec["flags"]), d["flags"])
    assert np.float32(rec["cfo_hz"]) == d["cfo_hz"], (what, rec["cfo_hz"], d["cfo_hz"])
    tol = 2.0 ** -22
    assert abs(float(rec["energy"]) - E_y) <= tol * E_y, (what, "energy", rec["energy"], E_y)
    if curve is not None:
        assert np.float32(rec["toa_frac"]) == d["toa_frac"] and np.float32(rec["peak_power"]) == d["peak_power"], (what, rec["toa_frac"], d["toa_frac"])
        assert abs(float(rec["rho"]) - float(d["rho"])) <= tol * float(d["rho"]), (what, "rho", rec["rho"], d["rho"])
    else:
        # no curve: the scalars are those of the model within what the curve's bound lets them move
        assert abs(float(rec["peak_power"]) - m["P"][kp]) <= m["Pbound"][kp], (what, "peak_power")
        if not d["flags"] & (EDGE | FLAT):
            a, b, c = m["P"][kp - 1], m["P"][kp], m["P"][kp + 1]
            den = a - 2 * b + c
            ea, eb, ec = m["Pbound"][kp - 1], m["Pbound"][kp], m["Pbound"][kp + 1]
            slack = 0.5 * (ea + ec) / abs(den) + 0.5 * abs(a - c) * (ea + 2 * eb + ec) / (den * den)
            assert abs(float(rec["toa_frac"]) - 0.5 * (a - c) / den) <= 2.0 * slack + 2.0 ** -23, (what, "toa_frac")
        assert abs(float(rec["rho"]) - m["P"][kp] / (e_s(s32) * E_y)) <= (m["Pbound"][kp] / m["P"][kp] + tol) * float(rec["rho"]) + 1e-30, (what, "rho")
    assert 0.0 <= float(rec["rho"]) <= 1.0 + 1e-6, (what, rec["rho"])
    if abs(m["c"][kp]) > 0.0:
        ulp = float(np.spacing(np.float32(np.pi)))
        assert angle_err(float(rec["carrier_phase"]), float(np.angle(m["c"][kp]))) <= asin_bound(m["b"][kp], m["c"][kp]) + ulp, (what, "carrier_phase")
        z = m["cb"][kp] * np.conj(m["ca"][kp])
        if abs(z) > 0.0:
            bound = (asin_bound(m["ba"][kp], m["ca"][kp]) + asin_bound(m["bb"][kp], m["cb"][kp])) / HALF
            want = float(np.angle(z)) / HALF
            assert min(abs(float(rec["resid"]) - want), 2.0 * np.pi / HALF - abs(float(rec["resid"]) - want)) <= bound + float(np.spacing(np.float32(np.pi / HALF))), (what, "resid", rec["resid"], want, bound)
    return worst
