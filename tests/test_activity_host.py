"""The activity monitor's kernels on the host (dumpvdl2_amd/csrc/activity.h).  Two pieces of their code are plain functions that the
library also builds for the CPU, behind test hooks that need no GPU:
  - the scan's step over a word of 64 busy flags (bit operations on a ballot mask), held here to the sequential rule of the header;
  - k_activity_power's four steps, run lane by lane and barrier by barrier with every staging array watched: its bins against a
    float64 sum, the order of additions against the grid (bins per workgroup), feeds against a carried partial sum, the ring's wrap."""
import ctypes as C

import numpy as np
import pytest

import activity_model as am
from dumpvdl2_amd import vdl2hip


@pytest.fixture(scope="module")
def lib():
    L = vdl2hip.load_library()
    L.vdl2hip_debug_activity_words.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.vdl2hip_debug_activity_power.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_float,
                                               C.c_void_p, C.c_uint32, C.c_void_p]
    return L


# ---------------------------------------------------------------- the scan's word step
def words_of(flags, cuts):
    """the flags cut into words of at most 64 at `cuts` (as feeds cut the bins), then into 64s"""
    busy, nbits = [], []
    for a, b in zip([0] + cuts, cuts + [len(flags)]):
        for k in range(a, b, 64):
            w = flags[k:min(k + 64, b)]
            busy.append(sum(1 << i for i, f in enumerate(w) if f))
            nbits.append(len(w))
    return np.array(busy, dtype=np.uint64), np.array(nbits, dtype=np.uint32)


def run_words(lib, flags, cuts, H):
    busy, nbits = words_of(list(flags), cuts)
    out = np.zeros(4, dtype=np.uint64)
    assert lib.vdl2hip_debug_activity_words(busy.ctypes.data, nbits.ctypes.data, busy.size, H, out.ctypes.data) == 0
    return [int(v) for v in out]


def model_words(flags, H):
    st = am.new_state()
    r = am.scan(np.where(flags, 1.0, 0.0).astype(np.float32), 0.5, H, st)
    return [r["transmissions"], r["longest_bins"], r["open"], st["first"] if st["open"] else 0]


@pytest.mark.parametrize("H", [0, 1, 2, 3, 7, 62, 63, 64, 65, 130, 255])
def test_scan_words_random(lib, H):
    rng = np.random.default_rng(100 + H)
    for trial in range(60):
        n = int(rng.integers(1, 700))
        density = [0.02, 0.2, 0.5, 0.9][trial % 4]
        flags = rng.random(n) < density
        if trial % 5 == 0:                                   # long runs: transmissions that span words
            flags = np.repeat(rng.random(n // 20 + 1) < 0.5, 20)[:n]
        cuts = sorted(set(int(c) for c in rng.integers(1, n, size=int(rng.integers(0, 6))))) if n > 1 else []
        assert run_words(lib, flags, cuts, H) == model_words(flags, H), (H, trial, n, cuts)


def test_scan_words_exhaustive_short(lib):
    """every pattern of 10 bins, cut in two at every place, H = 0 .. 3"""
    for H in range(4):
        for pat in range(1 << 10):
            flags = np.array([(pat >> i) & 1 for i in range(10)], dtype=bool)
            want = model_words(flags, H)
            for cut in (None, 1, 4, 9):
                assert run_words(lib, flags, [] if cut is None else [cut], H) == want, (H, pat, cut)


def test_scan_words_arguments(lib):
    out = np.zeros(4, dtype=np.uint64)
    one = np.array([3], dtype=np.uint64)
    assert lib.vdl2hip_debug_activity_words(one.ctypes.data, np.array([1], dtype=np.uint32).ctypes.data, 1, 0, out.ctypes.data) == -1   # a flag beyond the word
    assert lib.vdl2hip_debug_activity_words(one.ctypes.data, np.array([65], dtype=np.uint32).ctypes.data, 1, 0, out.ctypes.data) == -1
    assert lib.vdl2hip_debug_activity_words(one.ctypes.data, np.array([2], dtype=np.uint32).ctypes.data, 1, 256, out.ctypes.data) == -1


# ---------------------------------------------------------------- k_activity_power, lane by lane
CAP = 1 << 16


def ring_of(y, k_first):
    """a 16-byte aligned ring of CAP samples holding stream samples k_first ... at k & (CAP - 1); the rest is NaN: reading it shows"""
    buf = np.full(2 * CAP + 4, np.nan, dtype=np.float32)
    off = (-buf.ctypes.data // 4) % 4
    ring = buf[off:off + 2 * CAP].reshape(CAP, 2)
    assert ring.ctypes.data % 16 == 0
    idx = (k_first + np.arange(y.shape[0])) & (CAP - 1)
    ring[idx] = y
    return buf, ring


def run_power(lib, y, B, feeds, run, k_first=0, S=None):
    """the stream y (from k_on = k_first on) through the host build of the kernel, cut into `feeds` -> (series of the complete bins, carry)"""
    nb = y.shape[0] // B
    S = S or max(4, 1 << int(np.ceil(np.log2(nb + 2))))
    series = np.full(S, np.nan, dtype=np.float32)
    carry = np.zeros(1, dtype=np.float32)
    t0 = 0
    for d in feeds:
        if d == 0:
            continue
        # only this feed's samples are in the ring: a read behind its first or beyond its last sample meets a NaN
        keep, ring = ring_of(y[t0:t0 + d], k_first + t0)
        out = np.zeros(1, dtype=np.float32)
        r = lib.vdl2hip_debug_activity_power(ring.ctypes.data, CAP, k_first + t0, d, B, t0, run, float(carry[0]), series.ctypes.data, S, out.ctypes.data)
        assert r == 0, (r, B, d, t0, run)
        carry = out
        t0 += d
    assert t0 == y.shape[0]
    return series[:nb].copy() if nb <= S else series, carry[0]


def stream(n, seed):
    rng = np.random.default_rng(seed)
    lvl = np.repeat(10.0 ** rng.uniform(-4, -0.5, size=n // 97 + 1), 97)[:n]
    return (lvl[:, None] * rng.standard_normal((n, 2))).astype(np.float32)


def cut(n, sizes):
    out, k = [], 0
    while k < n:
        d = min(sizes[len(out) % len(sizes)], n - k)
        out.append(d)
        k += d
    return out


@pytest.mark.parametrize("B", [10, 11, 16, 17, 64, 105, 256, 257, 1000, 2047, 2048, 2049, 4100, 10500])
def test_power_definition_and_grid(lib, B):
    n = 3 * max(B, 2048) + 1234 + B // 2
    y = stream(n, B)
    ref = am.bin_powers(y, B)
    whole, carry = run_power(lib, y, B, [n], run=1 << 20)
    assert whole.size == ref.size == n // B
    ratio = np.abs(whole.astype(np.float64) - ref) / (am.bound(B) * ref)
    print(f"B={B}: worst ratio to the bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    tail = y[(n // B) * B:].astype(np.float64)
    assert abs(float(carry) - float((tail ** 2).sum())) <= am.bound(B) * float((tail ** 2).sum())
    # the order of additions belongs to the bin and the cut, not to the grid: any number of bins per workgroup gives the same bits
    for run in (1, 2, 3, 7, 100):
        got, c2 = run_power(lib, y, B, [n], run=run)
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)) and np.float32(c2).tobytes() == np.float32(carry).tobytes(), (B, run)


@pytest.mark.parametrize("B", [10, 105, 1000, 10500])
@pytest.mark.parametrize("k_first", [0, 1, CAP - 777, 3 * CAP - 1])
def test_power_cuts_and_wrap(lib, B, k_first):
    n = 2 * max(B, 2048) + 3001
    y = stream(n, 1000 + B)
    ref = am.bin_powers(y, B)
    whole, carry = run_power(lib, y, B, [n], run=5, k_first=k_first)
    for sizes in ([1], [B - 1, 1, 2 * B + 3], [5, 4000, 1, 1, 77], [B], [2048, 2049, 2047]):
        if sizes == [1] and n > 9000:
            continue                                             # (a sample per feed: the short streams are enough)
        got, c2 = run_power(lib, y, B, cut(n, sizes), run=3, k_first=k_first)
        r = np.abs(got.astype(np.float64) - ref) / (am.bound(B) * ref)
        assert r.max() <= 1.0, (B, sizes, r.max())
        assert np.all(np.abs(got.astype(np.float64) - whole) <= 2 * am.bound(B) * ref)
        assert abs(float(c2) - float(carry)) <= 2 * am.bound(B) * max(float(carry), 1e-30)


def test_power_series_ring(lib):
    """the series is a ring: bin m lands at m & (S - 1)"""
    B, n = 10, 10 * 70 + 3
    y = stream(n, 5)
    ref = am.bin_powers(y, B)
    series, _ = run_power(lib, y, B, cut(n, [250]), run=4, S=32)
    for m in range(70 - 32, 70):
        assert abs(float(series[m & 31]) - ref[m]) <= am.bound(B) * ref[m], m
