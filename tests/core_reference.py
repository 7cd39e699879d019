"""The yardstick for the element-wise pieces of dumpvdl2_amd/csrc/vdl2_core.h that mix float and double the way the reference does
(src/demod.c:98-198, 256-264): plain numpy, no GPU, nothing compiled.

sync_metric()          got_sync() up to the threshold test: pherr and slope of n windows of 16 phases
slice_symbol()         one D8PSK decision: the phase-step index and whether the reference's index went negative
parabola_vertex()      calc_para_vertex(0, 3, y1, y2, y3)
ppm_of(), ppm_gate_threshold()   the --max-ppm gate

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
         "vertex": (6, 3, 1), "ppm": (7, 3, 2)}           # name -> (kind, 32-bit words in, words out) per element


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
