"""The transmission capture's definition (include/vdl2hip.h, "Transmission capture") in numpy: the IQ window and its room, the
spectrum in float64, its error bound, and the four figures of vdl2hip_txcap_measure().  Nothing of the library's kernels is used: the
window comes from vdl2hip_spectrum_window(), everything else is written out here."""
import numpy as np

SPAN = 57344                      # the longest extent, the preamble search's
PARTIAL, CLIPPED, TRUNCATED, NO_ROOM, SHORT, NO_SPECTRUM = 1, 2, 4, 8, 16, 32     # VDL2HIP_TX_PARTIAL, VDL2HIP_TXC_*
IQ, SPECTRUM, UNDECODED_ONLY = 1, 2, 4                                            # VDL2HIP_TXCAP_*
ROOM_FLAGS = NO_ROOM | NO_SPECTRUM
DEF_N, DEF_POOL, DEF_SPECTRA = 256, 1 << 20, 1024
INT_FIELDS = ("chan", "freq", "first_bin", "win_first", "win_last", "iq_count", "flags", "segments", "nfft")


def window(first, last, pre, post):
    lo = max(0, first - pre)
    back = last - (SPAN - 1)
    return (max(lo, back), last + post, CLIPPED if back > lo else 0)


def extent(first, last):
    return max(first, last - (SPAN - 1)), last


def segments(length, n):
    return (length - n) // (n // 2) + 1 if length >= n else 0


def plan(tx, flags, pre=0, post=0, max_iq=0, nfft=0, pool_samples=0, pool_spectra=0):
    """tx: the log's records of ONE feed (rows with first_sample, last_sample, flags, chan, freq, first_bin) -> (a list of dicts with
    the integer fields of vdl2hip_tx_capture - iq_off in pairs of the feed's pool, spec index `spec` in the feed's spectra, None
    without one -, pairs of the pool in use)"""
    n = nfft or DEF_N
    pool, nspec = pool_samples or DEF_POOL, pool_spectra or DEF_SPECTRA
    out, off, used = [], 0, 0
    for i, t in enumerate(tx):
        first, last = int(t["first_sample"]), int(t["last_sample"])
        wf, wl, fl = window(first, last, pre, post)
        r = dict(chan=int(t["chan"]), freq=int(t["freq"]), first_bin=int(t["first_bin"]), win_first=wf, win_last=wl, iq_count=0, iq_off=0,
                 segments=0, nfft=0, spec=None)
        if flags & IQ:
            cnt = max(0, wl - wf + 1)
            if max_iq and cnt > max_iq:
                cnt, fl = max_iq, fl | TRUNCATED
            if off + cnt > pool:
                fl |= NO_ROOM
            else:
                r["iq_count"], r["iq_off"] = cnt, off
                used = max(used, off + cnt) if cnt else used
            off += cnt
        if flags & SPECTRUM:
            r["nfft"] = n
            if i < nspec:
                ef, el = extent(first, last)
                r["segments"] = segments(el - ef + 1, n)
                r["spec"] = i
                if r["segments"] == 0:
                    fl |= SHORT
            else:
                fl |= NO_SPECTRUM
        r["flags"] = fl | (int(t["flags"]) & PARTIAL)
        out.append(r)
    return out, used


def spectrum64(get, first, last, n, w):
    """-> (power float64 [n], bound float64 [n], S): the definition in float64 on the samples get(int64 indices) -> complex64, and the
    stated bound: the mean over the segments of b_s[i] = (2 e |X| ||X||_2 + e^2 ||X||_2^2 + 4 2^-24 |X|^2) norm, e = log2 n 2^-24, plus
    one float32 rounding of the result"""
    ef, el = extent(first, last)
    S = segments(el - ef + 1, n)
    if S == 0:
        return np.zeros(n), np.zeros(n), 0
    idx = ef + (n // 2) * np.arange(S, dtype=np.int64)[:, None] + np.arange(n, dtype=np.int64)[None, :]
    y = np.asarray(get(idx.reshape(-1)), dtype=np.complex64).astype(np.complex128).reshape(S, n)
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    X = np.fft.fftshift(np.fft.fft(y * w64[None, :], axis=1), axes=1)
    norm = 1.0 / w64.sum() ** 2
    a = np.abs(X)
    power = (a ** 2).sum(axis=0) * norm / S
    e = np.log2(n) * 2.0 ** -24
    l2 = np.sqrt((a ** 2).sum(axis=1))[:, None]
    b = (2 * e * a * l2 + e * e * l2 ** 2 + 4 * 2.0 ** -24 * a ** 2) * norm
    bound = b.sum(axis=0) / S
    return power, bound + 2.0 ** -24 * (power + bound), S


def check_spectrum(got, get, first, last, n, w, label=""):
    power, bound, S = spectrum64(get, first, last, n, w)
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == (n,), (label, got.shape)
    if S == 0:
        assert not got.any(), label
        return 0.0
    err = np.abs(got.astype(np.float64) - power)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), (label, S, worst, int(np.argmax(err / np.maximum(bound, 1e-300))))
    return worst


def measure(power, n=None):
    """vdl2hip_txcap_measure() in Python floats (IEEE double), ascending i"""
    p = [float(np.float32(v)) for v in power]
    n = n or len(p)
    step = 105000.0 / n
    total = 0.0
    for v in p:
        total += v
    out = dict(total=0.0, peak_hz=0.0, centroid_hz=0.0, obw_hz=0.0, peak_bin=0, obw_lo=0, obw_hi=0)
    if not total > 0.0:
        return out
    peak, moment, run, lo, hi = 0, 0.0, 0.0, None, None
    for i, v in enumerate(p):
        if v > p[peak]:
            peak = i
        moment += (float(i) - float(n // 2)) * step * v
        run += v
        if lo is None and run >= 0.005 * total:
            lo = i
        if hi is None and run >= 0.995 * total:
            hi = i
    return dict(total=total, peak_hz=(float(peak) - float(n // 2)) * step, centroid_hz=moment / total, obw_hz=float(hi - lo + 1) * step,
                peak_bin=peak, obw_lo=lo, obw_hi=hi)


def ring_get(y):
    """y: [ring, 2] float32 -> get(n) with the ring index masked per element"""
    c = np.ascontiguousarray(y, dtype=np.float32).view(np.complex64).reshape(-1)
    mask = c.size - 1
    return lambda n: c[n & mask]


def stream_get(y, base=0):
    """y: complex64 [N], sample n at y[n - base]"""
    c = np.asarray(y, dtype=np.complex64)
    return lambda n: c[n - base]
