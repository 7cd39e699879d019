"""The spectrogram by its definition (include/vdl2hip.h, "Spectrogram"), numpy float64: lines, holds, the bounds a value is held to and
the channel rule.  The conversions and the transform are those of tests/test_gpu_spectrum.py's model: the format conversion in numpy
float32 arithmetic, the library's own window, np.fft.fft.

Bounds, against this float64 definition and never against the kernel: per segment the monitor's
  b_s[i] = (2 e |X[k]| ||X||_2 + e^2 ||X||_2^2 + 4 2^-24 |X[k]|^2) / (sum w)^2,   e = log2(N) 2^-24
line_mean within the mean of b_s over the line plus one float32 rounding of the result (2^-24 relative), line_max and max_hold within
the largest b_s[i] among the segments covered plus that rounding: |max a - max b| <= max |a - b|."""
import numpy as np

FMTS = {"u8": 0, "s16": 1, "cf32": 2, "s8": 4}
HALF_ULP = 2.0 ** -24


def to_float(raw, fmt):
    """x[i] as the header defines it, computed in float32 -> complex128"""
    if fmt == "u8":
        v = (raw.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    elif fmt == "s16":
        v = raw.astype(np.float32) / np.float32(32768.0)
    elif fmt == "s8":
        v = raw.astype(np.float32) / np.float32(128.0)
    else:
        v = raw.astype(np.float32)
    assert v.dtype == np.float32
    v = v.astype(np.float64).reshape(-1, 2)
    return v[:, 0] + 1j * v[:, 1]


def to_raw(x, fmt):
    """a complex stream in the caller's format (u8 / s8 / int16 pairs, float32 pairs)"""
    iq = np.stack([x.real, x.imag], axis=1)
    if fmt == "u8":
        return np.clip(np.rint(127.5 + 127.5 * iq), 0, 255).astype(np.uint8)
    if fmt == "s8":
        return np.clip(np.rint(128.0 * iq), -128, 127).astype(np.int8)
    if fmt == "s16":
        return np.clip(np.rint(32768.0 * iq), -32768, 32767).astype("<i2")
    return iq.astype(np.float32)


def make_stream(fmt, n, seed=1):
    """noise, a strong off-bin tone that comes and goes, and a weak one -> the stream in the caller's format"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    gate = 0.25 + 0.75 * (np.sin(2 * np.pi * t / (n / 3.3)) > 0)
    x = 0.5 * gate * np.exp(2j * np.pi * 0.12345 * t) + 0.5e-3 * np.exp(-2j * np.pi * 0.31 * t)
    x += 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return to_raw(x, fmt)


def segments(x, n, w, stride=1, skip=0):
    """(q, b): |X|^2 / (sum w)^2 and its bound per analysed segment, [segments, n] in ascending frequency.  The analysed segments are
    0, stride, 2 stride, ... of the stream x; the first `skip` of them are left out (a0 of a tap enabled later)"""
    nseg = x.size // n
    segs = x[:nseg * n].reshape(nseg, n)[::stride][skip:]
    wd = w.astype(np.float64)
    X = np.fft.fft(segs * wd, axis=1)
    sw2 = wd.sum() ** 2
    mag = np.abs(X)
    nrm = np.sqrt((mag ** 2).sum(axis=1, keepdims=True))
    eps = np.log2(n) * 2.0 ** -24
    b = (2 * eps * mag * nrm + eps ** 2 * nrm ** 2 + 4 * 2.0 ** -24 * mag ** 2) / sw2
    return np.fft.fftshift(mag ** 2 / sw2, axes=1), np.fft.fftshift(b, axes=1)


def model(q, b, R, hold_from_line=0, hold_from_segment=0):
    """the tap's results for the segments q (bounds b): dict of line_mean, line_max [lines, n] with their bounds mean_bound, max_bound,
    max_hold, floor_hold [n] with hold_bound, floor_bound, and the counts.  hold_from_*: the holds cover what came after a reset"""
    S, n = q.shape
    L = S // R
    ql, bl = q[:L * R].reshape(L, R, n), b[:L * R].reshape(L, R, n)
    line_mean, line_max = ql.mean(axis=1), ql.max(axis=1) if L else np.zeros((0, n))
    mean_bound = bl.mean(axis=1) + HALF_ULP * line_mean
    max_bound = (bl.max(axis=1) if L else np.zeros((0, n))) + HALF_ULP * line_max
    hs, hl = q[hold_from_segment:], line_mean[hold_from_line:]
    out = dict(lines=L, hold_segments=hs.shape[0], hold_lines=hl.shape[0], line_mean=line_mean, line_max=line_max,
               mean_bound=mean_bound, max_bound=max_bound)
    out["max_hold"] = hs.max(axis=0) if hs.shape[0] else np.zeros(n)
    out["hold_bound"] = (b[hold_from_segment:].max(axis=0) if hs.shape[0] else np.zeros(n)) + HALF_ULP * out["max_hold"]
    out["floor_hold"] = hl.min(axis=0) if hl.shape[0] else np.zeros(n)
    # |min a - min b| <= max |a - b| too
    out["floor_bound"] = mean_bound[hold_from_line:].max(axis=0) if hl.shape[0] else np.zeros(n)
    return out


def worst_ratio(got, want, bound):
    """max |got - want| / bound (0 for empty arrays; a zero bound with a zero error counts as 0)"""
    if want.size == 0:
        return 0.0
    err = np.abs(got.astype(np.float64) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def channel_rule(max_hold, floor_hold, freq_hz, enbw_bins, freqs):
    """(peak_dbfs, floor_dbfs) per channel: the strongest max_hold bin and the floor_hold power within 12.5 kHz (or of the nearest bin)"""
    peak, floor = [], []
    with np.errstate(divide="ignore"):
        for f in freqs:
            d = np.abs(freq_hz - f)
            sel = d <= 12500.0
            if not sel.any():
                sel = np.zeros_like(sel)
                sel[np.argmin(d)] = True
            p, s = float(max_hold[sel].astype(np.float64).max()), float(floor_hold[sel].astype(np.float64).sum())
            peak.append(10 * np.log10(p) if p > 0 else -np.inf)
            floor.append(10 * np.log10(s / enbw_bins) if s > 0 else -np.inf)
    return np.array(peak), np.array(floor)


def burst_stream(n=64, nseg=1000, seg=600, k=20, amp=0.03, sigma=0.01):
    """the stream of "the point of it": complex noise of sigma per component, a tone on bin centre k during one segment only"""
    rng = np.random.default_rng(1)
    x = sigma * (rng.standard_normal(nseg * n) + 1j * rng.standard_normal(nseg * n))
    t = np.arange(n, dtype=np.float64)
    x[seg * n:(seg + 1) * n] += amp * np.exp(2j * np.pi * k * t / n)
    return x
