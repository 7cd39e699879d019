"""The yardstick for the preamble search (include/vdl2hip.h, "Preamble search"; dumpvdl2_amd/csrc/txsearch.h): plain numpy on top of
tests/core_reference.py, no GPU, nothing compiled.

  Phi(n) = float32(arctan2(float64 im, float64 re)) for n >= 0, 0 for n < 0
  (p(n), s(n)) = core_reference.sync_metric over the 16 phases Phi(n - 150 + 10 i)
  and the definitions of the header, taken in ascending n.

tests/test_core_reference.py holds sync_metric() and ppm_of() bit for bit to the host build of the library's own source."""
import numpy as np

import core_reference as cr

F32 = np.float32
SPAN = 57344                      # kTxsSpan
CLIPPED, PARTIAL = 2, 1           # VDL2HIP_TXS_CLIPPED, VDL2HIP_TX_PARTIAL
DECODED, FRAMES_BAD, LOCK_NO_FRAME, NO_PREAMBLE = 0, 1, 2, 3
DEVICE_FIELDS = ("search_first", "search_last", "best_sample", "first_lock", "best_pherr", "best_slope", "best_ppm",
                 "lock_points", "below_thr", "lock_phases", "flags")


def phases(get, lo, hi):
    """Phi(lo .. hi) as float32; get(n: int64 array, all >= 0) -> complex64 samples"""
    n = np.arange(lo, hi + 1, dtype=np.int64)
    out = np.zeros(n.size, dtype=F32)
    ok = n >= 0
    if ok.any():
        v = np.asarray(get(n[ok]), dtype=np.complex64)
        out[ok] = np.arctan2(v.imag.astype(np.float64), v.real.astype(np.float64)).astype(F32)
    return out


def metric(get, lo, hi):
    """(p, s) float32 for n = lo .. hi"""
    ph = phases(get, lo - 150, hi)
    idx = np.arange(hi - lo + 1)[:, None] + 10 * np.arange(16)[None, :]
    with np.errstate(all="ignore"):
        return cr.sync_metric(ph[idx])


def search_range(first, last):
    lo = last - (SPAN - 1)
    return (first, 0) if first >= lo else (lo, CLIPPED)


def search(get, first, last, freq, txflags=0):
    """the device-written fields of the record of a transmission first_sample .. last_sample, as a dict (floats as float32)"""
    sf, flags = search_range(first, last)
    p3, s3 = metric(get, sf - 3, last)          # p(n - 3) beside p(n)
    p, s = p3[3:], s3[3:]
    best_p, best_n = F32(np.inf), -1
    finite = ~np.isnan(p)
    if finite.any():
        m = np.min(p[finite])
        if m < F32(np.inf):
            best_p = F32(m); best_n = int(np.flatnonzero(p == m)[0])      # the lowest n of the smallest p: what a strict < in ascending n keeps
    n = sf + np.arange(p.size, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        lock = (p3[:-3] < cr.SYNC_THR) & (p > p3[:-3]) & (n - 3 >= sf)
        below = int(np.count_nonzero(p < cr.SYNC_THR))
    ln = n[lock]
    slope = F32(s[best_n]) if best_n >= 0 else F32(0)
    return {
        "search_first": sf, "search_last": last, "best_sample": sf + best_n if best_n >= 0 else -1, "first_lock": int(ln[0]) if ln.size else -1,
        "best_pherr": best_p, "best_slope": slope, "best_ppm": F32(cr.ppm_of(slope, freq)) if best_n >= 0 else F32(0),
        "lock_points": int(ln.size), "below_thr": below, "lock_phases": int(np.bitwise_or.reduce(1 << (ln % 3))) if ln.size else 0,
        "flags": flags | (txflags & PARTIAL),
    }, (p, s)


def why(frames, frames_ok, lock_points):
    return DECODED if frames_ok else FRAMES_BAD if frames else LOCK_NO_FRAME if lock_points else NO_PREAMBLE


def same_bits(a, b):
    return np.asarray(a, dtype=F32).view(np.uint32) == np.asarray(b, dtype=F32).view(np.uint32)


def check(rec, want, label=""):
    """every device-written field of a record (a TXS_DTYPE row) against the model's dict: exact, floats by their bits"""
    for k in DEVICE_FIELDS:
        g, w = rec[k], want[k]
        if k in ("best_pherr", "best_slope", "best_ppm"):
            assert same_bits(g, w), (label, k, float(g), float(w))
        else:
            assert int(g) == int(w), (label, k, int(g), int(w))


def ring_get(y):
    """y: [ring, 2] float32 -> get(n) with the ring index masked per element"""
    c = np.ascontiguousarray(y, dtype=F32).view(np.complex64).reshape(-1)
    mask = c.size - 1
    return lambda n: c[n & mask]


def stream_get(y):
    """y: complex64 [N], sample n at y[n]"""
    c = np.asarray(y, dtype=np.complex64)
    return lambda n: c[n]
