"""The yardstick for K1's decimated stream (k_chanfir, dumpvdl2_amd/csrc/kernels.h): plain numpy / scipy, no GPU.

exact_stream()      the channel filter of the reference (src/demod.c:302-329: table mixer, 2-pole IIR, decimation) with the
                    recursion in DOUBLE precision - what the stream is compared with;
block_form_model()  the recurrence K1 runs, restated in float32 with every product and every sum rounded (no FMA, sequential in
                    time): a model of the arithmetic, not of the kernel.  Its distance from exact_stream() on the same input is
                    what single precision costs, and the bound a kernel's stream is held to is a multiple of it (FACTOR_MAX,
                    FACTOR_RMS) - derived per input, never from what a kernel gave;
compare()           per-channel max and rms error of a candidate stream and of the model, in units of the WIDEBAND INPUT's peak:
                    the mix and the tap sums round at input level, so a quiet channel carries the same absolute error as a loud one.

Coefficients and NCO steps are the oracle's (Oracle.lpf(), Oracle.dphi(): pinned to the reference), the block-form constants and the
NCO table are design.h compiled for the CPU (hostsim_block_form, hostsim_nco_lut: pinned by tests/test_design.py) - nothing here is
taken from the receiver under test."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))

K_FIX = 128
K_MAXOS = 32
RUNUP = 256                 # blocks of run-up before a window of the model counts (P^128 < 1e-12: tests/test_design.py)
# A kernel differs from the model in legitimate ways only: FMA contraction (fewer roundings), the 64-lane scan composing states through
# powers of Q instead of sequentially, the fix-up add.  An equivalent but different rounding sequence has the same rms (factor 2 for its
# scatter) and, over 1e5..1e6 samples, an extreme value within a few times it (factor 4).
FACTOR_MAX = 4.0
FACTOR_RMS = 2.0
# The edges of the sample formats (constant inputs: the roundings of a block repeat block after block, nothing averages, and the
# recursion's DC gain multiplies them; an impulse into silence: nothing is left to compare) get one absolute bound instead of a derived one,
# in units of the input's peak: FACTOR_MAX times what the model itself is held to on those inputs (MODEL_EDGE_MAX; it reaches 6.1-6.3e-7
# on full-scale DC, ~10 roundings of 2^-24; tests/test_k1_reference.py::test_model_on_the_edges_of_the_formats).
MODEL_EDGE_MAX = 6.5e-7
ABS_BOUND = FACTOR_MAX * MODEL_EDGE_MAX
MAX_THREADS = 16


class BlockForm(C.Structure):           # design.h: struct BlockForm (size checked against the library's)
    _fields_ = [("os", C.c_int), ("run", C.c_int), ("g0", C.c_float * K_MAXOS), ("g1", C.c_float * K_MAXOS),
                ("P", C.c_float * 4), ("c0", C.c_float), ("c1", C.c_float), ("c2", C.c_float),
                ("cP", (C.c_float * 2) * K_FIX), ("Ppow", (C.c_float * 4) * (K_FIX + 1)), ("Q", (C.c_float * 4) * 6),
                ("Qpow", (C.c_float * 4) * 64), ("basis", C.c_float * 4)]


_hs = None


def _hostsim():
    global _hs
    if _hs is None:
        import pyhostsim
        L = C.CDLL(pyhostsim.build())
        L.hostsim_block_form.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(BlockForm)]
        assert L.hostsim_sizeof_blockform() == C.sizeof(BlockForm)
        _hs = L
    return _hs


def block_form_constants(A, B, os_, run=2):
    """design.h's derive_block_form() for the coefficients A, B (float32 [3] each, the oracle's)"""
    bf = BlockForm()
    a = (C.c_float * 3)(*[float(v) for v in A]); b = (C.c_float * 3)(*[float(v) for v in B])
    _hostsim().hostsim_block_form(a, b, int(os_), int(run), C.byref(bf))
    return bf


def nco_lut():
    """design.h's build_nco_lut(): float32 [256, 4] = sin, cos, (sin[i+1]-sin[i]) 2^-16, (cos[i+1]-cos[i]) 2^-16"""
    lut = np.zeros((256, 4), dtype=np.float32)
    _hostsim().hostsim_nco_lut(lut.ctypes.data_as(C.c_void_p))
    return lut


def to_float(raw, fmt):
    """raw IQ bytes -> float32 [n, 2] as process_buf_short() / process_buf_uchar() convert them (demod.c:349-363)"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    if fmt == 1:
        return raw.view(np.int16).reshape(-1, 2).astype(np.float32) / np.float32(32768.0)
    return (raw.reshape(-1, 2).astype(np.float32) - np.float32(127.5)) / np.float32(127.5)


def input_peak(raw, fmt):
    """peak magnitude of the wideband input: what every error here is normalised by"""
    v = to_float(raw, fmt).astype(np.float64)
    return float(np.sqrt((v * v).sum(axis=1).max()))


def _threads(n):
    return max(1, min(MAX_THREADS, n, os.cpu_count() or 1))


def _map(fn, n, nthreads):
    if nthreads <= 1 or n <= 1:
        return [fn(i) for i in range(n)]
    with ThreadPoolExecutor(_threads(min(n, nthreads))) as ex:
        return list(ex.map(fn, range(n)))


_CHUNK = 1 << 18


def exact_stream(cfg, raw, fmt, A, B, dphis, D, unrounded=False, n0=0, nthreads=1):
    """the channel filter of src/demod.c:302-329 in double precision: table mixer (sincosf_lut, entries float), 2-pole IIR, decimation.
    -> float32 [nchan, D, 2]; unrounded: the float64 result itself.  n0: absolute index of raw's first sample (the phase of a stretch
    cut out of a longer stream; the filter starts from rest).  nthreads: channels side by side."""
    from scipy.signal import lfilter
    os_ = cfg.oversample
    v = to_float(raw, fmt)
    n = D * os_
    x = v[:n, 0].astype(np.float64) + 1j * v[:n, 1].astype(np.float64)
    i = np.arange(257, dtype=np.float32)
    ang = (np.float32(2.0) * np.float32(np.pi) * (i % 256) / np.float32(256.0)).astype(np.float32)
    sl = np.sin(ang.astype(np.float64)).astype(np.float32).astype(np.float64); cl = np.cos(ang.astype(np.float64)).astype(np.float32).astype(np.float64)
    b = [float(A[0]), float(A[1]), float(A[2])]; a = [1.0, -float(B[1]), -float(B[2])]
    chunk = (_CHUNK // os_) * os_
    y = np.zeros((len(dphis), D, 2), dtype=np.float64 if unrounded else np.float32)

    def one(c):
        dphi = int(dphis[c]) & 0xffffff
        zi = np.zeros(2, dtype=np.complex128)
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            if dphi:
                idxn = np.arange(n0 + s, n0 + e, dtype=np.uint64)
                ph = ((idxn * np.uint64(dphi)) & np.uint64(0xffffff)).astype(np.int64)
                k = ph >> 16; f = (ph & 0xffff).astype(np.float64) / 65536.0
                xm = x[s:e] * ((cl[k] + (cl[k + 1] - cl[k]) * f) + 1j * (sl[k] + (sl[k + 1] - sl[k]) * f))
            else:
                xm = x[s:e]
            z, zi = lfilter(b, a, xm, zi=zi)
            z = z[os_ - 1::os_]
            y[c, s // os_:s // os_ + len(z), 0] = z.real; y[c, s // os_:s // os_ + len(z), 1] = z.imag

    _map(one, len(dphis), nthreads)
    return y


def _model_front(xr, xi, dphi, lut, g0, g1, os_, D, n0, phase_index, out):
    """mix and tap sums of one channel: out[0..5] <- the four tap sums and the last mixed sample (re, im) of every block"""
    f32 = np.float32
    n = D * os_
    chunk = (_CHUNK // os_) * os_
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        idx = phase_index[s:e] if phase_index is not None else np.arange(n0 + s, n0 + e, dtype=np.uint64)
        ph = (idx.astype(np.uint64) * np.uint64(dphi)) & np.uint64(0xffffff)
        F = (ph & np.uint64(0xffff)).astype(f32)
        ent = lut[(ph >> np.uint64(16)).astype(np.int64)]
        sn = ent[:, 2] * F + ent[:, 0]                    # sin/cos = e.zw * F + e.xy: product rounded, sum rounded
        cs = ent[:, 3] * F + ent[:, 1]
        x_r = xr[s:e]; x_i = xi[s:e]
        mr = (cs * x_r + sn * (-x_i)).reshape(-1, os_)    # m = cos * x + sin * (i x)
        mi = (cs * x_i + sn * x_r).reshape(-1, os_)
        k0, k1 = s // os_, e // os_
        t0r = np.zeros(k1 - k0, dtype=f32); t0i = np.zeros(k1 - k0, dtype=f32); t1r = np.zeros(k1 - k0, dtype=f32); t1i = np.zeros(k1 - k0, dtype=f32)
        for j in range(os_):                              # the two tap sums, sequentially in j
            t0r = t0r + g0[j] * mr[:, j]; t0i = t0i + g0[j] * mi[:, j]
            t1r = t1r + g1[j] * mr[:, j]; t1i = t1i + g1[j] * mi[:, j]
        out[0, k0:k1] = t0r; out[1, k0:k1] = t0i; out[2, k0:k1] = t1r; out[3, k0:k1] = t1i
        out[4, k0:k1] = mr[:, -1]; out[5, k0:k1] = mi[:, -1]


def block_form_model(cfg, raw, fmt, A, B, dphis, D, n0=0, nthreads=1, phase_index=None, run=2):
    """the recurrence K1 runs, in float32: sin/cos = e.zw F + e.xy from the 256-entry table, m = cos x + sin (i x), the two tap sums
    sequentially in j, t <- P t + acc, y = c0 t0 + c1 t1 + c2 m_last - every product and every sum rounded to float32.
    -> float32 [nchan, D, 2].  n0 as in exact_stream(); phase_index (uint64 [D * os], optional): the sample index the phase of each
    input sample is computed from, instead of n0 + i (for planting phase mistakes)."""
    f32 = np.float32
    os_ = cfg.oversample
    bf = block_form_constants(A, B, os_, run)
    lut = nco_lut()
    v = to_float(raw, fmt)
    n = D * os_
    xr = np.ascontiguousarray(v[:n, 0]); xi = np.ascontiguousarray(v[:n, 1])
    g0 = np.array(bf.g0[:os_], dtype=f32); g1 = np.array(bf.g1[:os_], dtype=f32)
    P = [f32(v) for v in bf.P]; c0, c1, c2 = f32(bf.c0), f32(bf.c1), f32(bf.c2)
    nch = len(dphis)
    # The state step is sequential in time.  It is evaluated on windows of W blocks side by side (and all channels at once), each from
    # rest RUNUP = W blocks ahead of its first output (a start state decays below double-precision resolution, let alone single,
    # within 128 blocks); blocks before the stream's start are zero input on a zero state, which is exactly the filter at rest.
    W = RUNUP
    nw = (D + W - 1) // W
    front = np.zeros((nch, 6, (nw + 1) * W), dtype=f32)          # [.., RUNUP + k]: block k

    def one(c):
        _model_front(xr, xi, int(dphis[c]) & 0xffffff, lut, g0, g1, os_, D, n0, phase_index, front[c, :, RUNUP:RUNUP + D])

    _map(one, nch, nthreads)
    fw = front.reshape(nch, 6, nw + 1, W)
    s0r = np.zeros((nch, nw), dtype=f32); s0i = np.zeros((nch, nw), dtype=f32); s1r = np.zeros((nch, nw), dtype=f32); s1i = np.zeros((nch, nw), dtype=f32)
    y = np.zeros((nch, nw, W, 2), dtype=f32)
    for s in range(2 * W):
        a = fw[:, :, :nw, s] if s < W else fw[:, :, 1:, s - W]  # window w, step s = block w W + s - RUNUP
        n0r = P[0] * s0r + (P[1] * s1r + a[:, 0]); n0i = P[0] * s0i + (P[1] * s1i + a[:, 1])
        n1r = P[2] * s0r + (P[3] * s1r + a[:, 2]); n1i = P[2] * s0i + (P[3] * s1i + a[:, 3])
        s0r, s0i, s1r, s1i = n0r, n0i, n1r, n1i
        if s >= W:
            y[:, :, s - W, 0] = c0 * n0r + (c1 * n1r + c2 * a[:, 4])
            y[:, :, s - W, 1] = c0 * n0i + (c1 * n1i + c2 * a[:, 5])
    return np.ascontiguousarray(y.reshape(nch, nw * W, 2)[:, :D])


def _err(y, y64, x_peak):
    d = np.asarray(y, dtype=np.float64) - y64
    m2 = (d * d).sum(axis=-1)
    return np.sqrt(m2.max(axis=-1)) / x_peak, np.sqrt(m2.mean(axis=-1)) / x_peak


def compare(candidate, y64, model, x_peak):
    """candidate, model: [nchan, D, 2] streams; y64: exact_stream(unrounded=True) of the same input; x_peak: input_peak().
    -> dict of float64 [nchan] arrays, all in units of the input's peak: max / rms (over time, of the complex error's magnitude) of
    the candidate and of the model against y64, and the bounds the candidate is held to: FACTOR_MAX, FACTOR_RMS times the model's."""
    cmax, crms = _err(candidate, y64, x_peak)
    mmax, mrms = _err(model, y64, x_peak)
    return {"max": cmax, "rms": crms, "model_max": mmax, "model_rms": mrms, "bound_max": FACTOR_MAX * mmax, "bound_rms": FACTOR_RMS * mrms}


def failures(r):
    """the channels of a compare() result that exceed a bound, as readable strings (empty: the candidate passes)"""
    out = []
    for c in range(len(r["max"])):
        if not (r["max"][c] <= r["bound_max"][c]) or not (r["rms"][c] <= r["bound_rms"][c]):
            out.append(f"channel {c}: max {r['max'][c]:.3e} (bound {r['bound_max'][c]:.3e}), rms {r['rms'][c]:.3e} (bound {r['bound_rms'][c]:.3e}) of the input's peak")
    return out


def stimulus(cf, freqs, os_, nsamples, fmt, seed, loud=None, noise=0.1, carrier=0.8):
    """a dense capture: white noise of `noise` of full scale on the whole band (every channel's output is ~1e-2 of the input's peak)
    and, on channel `loud`, an 8-PSK carrier at 10.5 kBd of `carrier` of full scale (that channel's peak ~ the input's).
    -> raw bytes (uint8 array) in format fmt (1: s16, 0: u8)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-noise, noise, nsamples) + 1j * rng.uniform(-noise, noise, nsamples)
    if loud is not None:
        fs = 105000 * os_
        sps = 10 * os_
        nsym = nsamples // sps + 1
        sym = np.exp(1j * np.pi / 4 * np.cumsum(rng.integers(0, 8, nsym)))
        base = np.repeat(sym, sps)[:nsamples]
        w = 2 * np.pi * (freqs[loud] - cf) / fs
        L = 4096
        q, r = np.divmod(np.arange(nsamples), L)
        x = x + carrier * base * np.exp(1j * w * r) * np.exp(1j * (w * L) * q)
    if fmt == 1:
        out = np.empty((nsamples, 2), dtype=np.int16)
        out[:, 0] = np.clip(np.rint(x.real * 32767.0), -32768, 32767); out[:, 1] = np.clip(np.rint(x.imag * 32767.0), -32768, 32767)
    else:
        out = np.empty((nsamples, 2), dtype=np.uint8)
        out[:, 0] = np.clip(np.rint(x.real * 127.5 + 127.5), 0, 255); out[:, 1] = np.clip(np.rint(x.imag * 127.5 + 127.5), 0, 255)
    return out.view(np.uint8).reshape(-1)


CF = 136975000              # a multiple of 8 Hz: exact in the float32 arithmetic of nco_step()


def channel_plan(os_, nch, variant=0):
    """channel frequencies for a receiver of nch channels at centre CF: the centre itself (step 0), the smallest non-zero step of either
    sign (8 Hz: nco_step() subtracts the frequencies in float32, which resolves 8 Hz at 137 MHz), an off-raster offset (100 008 Hz) of
    either sign, a channel near either band edge (0.45 fs), then a raster over the band.  Three channels cannot hold all of that: variant 0
    is (centre, +100 008, lower edge), variant 1 (+8 Hz, -100 008, upper edge).  -> (freqs, index of the 100 008 Hz channel)"""
    fs = 105000 * os_
    edge = int(0.45 * fs)
    if nch == 3:
        return ([CF, CF + 100008, CF - edge], 1) if variant == 0 else ([CF + 8, CF - 100008, CF + edge], 1)
    special = [CF, CF - 8, CF + 8, CF + 100008, CF - 100008, CF - edge, CF + edge, CF + 25000, CF - 250000]
    spacing = int(0.9 * fs / nch)
    return special + [CF + (c - nch // 2) * spacing + 777 for c in range(len(special), nch)], 3


EDGES = ("dc_full_scale", "most_negative", "nyquist_full_scale", "white_full_scale", "impulse_then_silence")


def edge_input(kind, fmt, nsamples, seed=1):
    """the inputs at the edges of the sample formats, raw bytes (uint8 array): full-scale DC; the most negative code on every sample
    (s16: -32768, u8: 0; u8's 255 is its full-scale DC); +-full scale alternating (a tone at the Nyquist frequency); white noise over every
    code; an impulse after 5 000 samples of silence followed by silence to the end (u8 has no zero: its silence is code 128)."""
    lo, hi, zero, dt = (-32768, 32767, 0, np.int16) if fmt == 1 else (0, 255, 128, np.uint8)
    x = np.empty((nsamples, 2), dtype=dt)
    if kind == "dc_full_scale":
        x[:] = hi
    elif kind == "most_negative":
        x[:] = lo
    elif kind == "nyquist_full_scale":
        x[0::2] = hi; x[1::2] = lo
    elif kind == "white_full_scale":
        x[:] = np.random.default_rng(seed).integers(lo, hi + 1, size=(nsamples, 2))
    elif kind == "impulse_then_silence":
        x[:] = zero; x[4999] = hi
    else:
        raise ValueError(kind)
    return x.view(np.uint8).reshape(-1)
