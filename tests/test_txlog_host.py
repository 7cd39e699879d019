"""The transmission log's word steps on the host (dumpvdl2_amd/csrc/txlog.h).  What k_txlog_plan and k_txlog_emit do to a word of 64
bins - the closes from bit operations on the busy mask, the segmented scan over the lanes, the record a closing lane builds, the state
the next word inherits - are plain functions the library also builds for the CPU.  The hook vdl2hip_debug_txlog_words runs them lane
by lane and level by level over one channel's bins; here its records are held to the sequential model (tests/txlog_model.py): integer
fields and peak_power exactly, mean_power to 2^-23 relative."""
import ctypes as C
import subprocess
import os

import numpy as np
import pytest

import txlog_model as tm
from dumpvdl2_amd import vdl2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = np.float32(0.01)


@pytest.fixture(scope="module")
def lib():
    L = vdl2hip.load_library()
    L.vdl2hip_debug_txlog_words.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_int64, C.c_uint64,
                                            C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def words_of(n, cuts):
    """n bins cut into feeds at `cuts`, every feed into words of 64 from its first bin"""
    nbits = []
    for a, b in zip([0] + cuts, cuts + [n]):
        nbits += [min(64, b - k) for k in range(a, b, 64)]
    return np.array(nbits, dtype=np.uint32)


def run_words(lib, p, cuts, H, B=105, k_on=0, base=0, init=None):
    p = np.ascontiguousarray(p, dtype=np.float32)
    nbits = words_of(p.size, list(cuts))
    assert int(nbits.sum()) == p.size
    recs = np.zeros(p.size // 2 + 2, dtype=vdl2hip.TX_DTYPE)
    out = np.zeros(4, dtype=np.uint64)
    ini = None if init is None else np.array(init, dtype=np.uint64)
    n = lib.vdl2hip_debug_txlog_words(p.ctypes.data, nbits.ctypes.data, nbits.size, float(THR), H, B, k_on, base,
                                      None if ini is None else ini.ctypes.data, recs.ctypes.data, recs.size, out.ctypes.data)
    assert n >= 0, (n, H, cuts)
    return recs[:n], [int(v) for v in out]


def check(lib, p, cuts, H, label, B=105, k_on=0, base=0, init=None):
    st = tm.new_state(base) if init is None else tm.new_state(base, *init)
    want = tm.log(p, THR, H, st, B, k_on)
    got, out = run_words(lib, p, cuts, H, B, k_on, base, init)
    tm.assert_records(got, want, label)
    assert np.all(got["frames"] == 0) and np.all(got["frames_ok"] == 0) and np.all(got["first_burst_ord"] == -1) and np.all(got["chan"] == 0)
    assert out == [int(st["open"]), st["idle"] if st["open"] else 0, st["first"] if st["open"] else 0, st["busy"] if st["open"] else 0], label
    return got


def powers(rng, flags, equal=False):
    """busy bins between 0.02 and 1, idle ones between 0 and 0.005 (equal: a handful of values, so that peaks tie)"""
    n = len(flags)
    hi = rng.choice(np.float32([0.25, 0.5, 0.5, 0.125]), size=n) if equal else rng.uniform(0.02, 1.0, size=n).astype(np.float32)
    lo = rng.uniform(0.0, 0.005, size=n).astype(np.float32)
    return np.where(flags, hi, lo).astype(np.float32)


def random_cuts(rng, n):
    return sorted(set(int(c) for c in rng.integers(1, n, size=int(rng.integers(0, 6))))) if n > 1 else []


@pytest.mark.parametrize("H", [0, 1, 2, 3, 7, 62, 63, 64, 65, 130, 255])
def test_words_random(lib, H):
    rng = np.random.default_rng(300 + H)
    nrec = 0
    for trial in range(60):
        n = int(rng.integers(1, 900))
        density = [0.02, 0.2, 0.5, 0.9][trial % 4]
        flags = rng.random(n) < density
        if trial % 5 == 0:                                       # long runs: transmissions that span 2 and 3 words
            flags = np.repeat(rng.random(n // 90 + 1) < 0.6, 90)[:n]
        if H >= 62 and trial % 3 == 0:                           # gaps long enough to close even with a long hang time
            flags[n // 3:n // 3 + H + int(rng.integers(0, 4))] = False
        p = powers(rng, flags, equal=trial % 6 == 1)
        nrec += len(check(lib, p, random_cuts(rng, n), H, (H, trial), B=int(rng.integers(10, 2000)), k_on=int(rng.integers(0, 1 << 40)),
                          base=int(rng.integers(0, 1 << 33))))
    assert nrec >= 10, nrec                                      # (the trials did close transmissions, whatever the hang time)


def test_words_exhaustive_short(lib):
    """every pattern of 10 bins, whole and cut in two at every place, H = 0 .. 3"""
    rng = np.random.default_rng(7)
    amp = rng.uniform(0.02, 1.0, size=10).astype(np.float32)
    for H in range(4):
        for pat in range(1 << 10):
            flags = np.array([(pat >> i) & 1 for i in range(10)], dtype=bool)
            p = np.where(flags, amp, np.float32(0.001)).astype(np.float32)
            for cut in [None] + list(range(1, 10)):
                check(lib, p, [] if cut is None else [cut], H, (H, pat, cut))


@pytest.mark.parametrize("H", [0, 1, 5, 63, 64, 70])
def test_close_on_word_boundaries(lib, H):
    """the close bin (last busy + H + 1) on the last bin of a word, on the first bin of the next, and either side of both; runs that
    span two and three words; one word after the other and cut into feeds at the boundary"""
    rng = np.random.default_rng(H)
    for close_at in (62, 63, 64, 65, 127, 128, 129, 191, 192):
        last = close_at - H - 1
        if last < 0:
            continue
        for length in (1, 2, 64, 65, 130, 190):
            first = last - length + 1
            if first < 0:
                continue
            n = 260
            flags = np.zeros(n, dtype=bool)
            flags[first:last + 1] = True
            flags[close_at + 1:close_at + 3] = True              # the next transmission starts right behind the close
            p = powers(rng, flags)
            for cuts in ([], [64], [128], [64, 128, 192], [close_at], [close_at + 1], [last + 1]):
                got = check(lib, p, [c for c in cuts if 0 < c < n], H, (H, close_at, length, cuts))
                assert got[0]["first_bin"] == first and got[0]["last_bin"] == last and got[0]["busy_bins"] == length


def test_equal_powers_lowest_peak_bin(lib):
    """of equal largest values the lowest bin is the peak bin - within a word, across words, across feeds"""
    for H in (0, 2):
        for n_busy, cuts in ((5, []), (64, []), (150, []), (150, [64]), (150, [70, 71]), (200, [1, 65, 130])):
            p = np.full(n_busy + H + 4, 0.001, dtype=np.float32)
            p[1:1 + n_busy] = 0.5
            got = check(lib, p, cuts, H, (H, n_busy, cuts))
            assert len(got) == 1 and got[0]["peak_bin"] == 1 and got[0]["peak_power"] == np.float32(0.5) and got[0]["mean_power"] == np.float32(0.5)
            # one larger value late, then ties again: the first of the largest
            p[n_busy - 2] = p[n_busy - 1] = 0.75
            got = check(lib, p, cuts, H, (H, n_busy, cuts, "late"))
            assert got[0]["peak_bin"] == n_busy - 2


@pytest.mark.parametrize("H", [0, 3, 64])
def test_partial_records(lib, H):
    """a transmission under way when the log takes effect: first_bin is the monitor's, the sums cover what the log saw"""
    rng = np.random.default_rng(50 + H)
    for idle in sorted({0, min(1, H), H}):
        base, first = 1000, 900
        # (a) it goes on for a while; (b) no busy bin follows: a record with busy_bins 0
        for tail in (7, 0):
            flags = np.zeros(tail + H + 80, dtype=bool)
            flags[H - idle:H - idle + tail] = True                # the first busy bin as late as the hang time still allows
            flags[-5:-2] = True
            p = powers(rng, flags)
            for cuts in ([], [1], [H - idle + 1]):
                got = check(lib, p, [c for c in cuts if 0 < c < p.size], H, (H, idle, tail, cuts), base=base, init=(1, idle, first))
                assert got[0]["flags"] == tm.TX_PARTIAL and got[0]["first_bin"] == first and got[0]["busy_bins"] == tail
                assert got[0]["last_bin"] == (base + H - idle + tail - 1 if tail else base - 1 - idle)
                assert np.all(got[1:]["flags"] == 0)
                if not tail:
                    assert got[0]["peak_power"] == 0 and got[0]["mean_power"] == 0 and got[0]["peak_bin"] == first


@pytest.mark.parametrize("nrec", [tm.MAIL_RECS, tm.MAIL_RECS + 1])
def test_mail_keys_on_a_clean_series(nrec):
    """the keying of the GPU tests' mailbox boundary (test_gpu_txlog.py, test_gpu_txsearch.py): on a clean series - a keyed bin busy,
    every other idle - and H = 0 every transmission is a record of its own, and all of them close within the stream"""
    keys = tm.mail_keys(nrec)
    total = 0
    for k in keys:
        p = np.full(tm.MAIL_BINS, 1e-7, dtype=np.float32)
        for s, e in k:
            assert e + 1 < tm.MAIL_BINS
            p[s:e + 1] = 0.01
        st = tm.new_state()
        recs = tm.log(p, 1e-4, 0, st)                            # (the GPU tests' threshold, -40 dBFS)
        assert [(r["first_bin"], r["last_bin"]) for r in recs] == k and not st["open"]
        total += len(recs)
    assert total == nrec and len(keys) == tm.MAIL_CHANS


def test_arguments(lib):
    p = np.full(4, 0.5, dtype=np.float32)
    out = np.zeros(4, dtype=np.uint64)
    recs = np.zeros(4, dtype=vdl2hip.TX_DTYPE)

    def call(nbits, H=0, B=105, init=None, cap=4):
        nb = np.array(nbits, dtype=np.uint32)
        ini = None if init is None else np.array(init, dtype=np.uint64)
        return lib.vdl2hip_debug_txlog_words(p.ctypes.data, nb.ctypes.data, nb.size, float(THR), H, B, 0, 0, None if ini is None else ini.ctypes.data,
                                             recs.ctypes.data, cap, out.ctypes.data)
    assert call([4]) == 0 and list(out) == [1, 0, 0, 4]
    assert call([0]) == -1 and call([65]) == -1 and call([4], H=256) == -1 and call([4], B=0) == -1
    assert call([4], H=2, init=[1, 3, 0]) == -1                   # more idle bins behind an open transmission than the hang time
    p[1] = 0.0
    assert call([4]) == 1 and call([4], cap=0) == -4              # VDL2HIP_E_TOOBIG


def test_structures_and_symbols(lib):
    assert C.sizeof(vdl2hip.TxlogCfg) == 16 and vdl2hip.TX_DTYPE.itemsize == 80 and C.sizeof(vdl2hip.TxlogInfo) == 64
    assert vdl2hip.TX_DTYPE.fields["frames"][1] == 64 and vdl2hip.TX_DTYPE.fields["first_burst_ord"][1] == 72
    for name in ("vdl2hip_txlog_enable", "vdl2hip_txlog_disable", "vdl2hip_txlog_info_get", "vdl2hip_txlog_read"):
        assert name in vdl2hip.EXPORTS and hasattr(lib, name)
    # the sizes and offsets the C compiler gives the header's structures
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vdl2hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",sizeof(vdl2hip_txlog_cfg),'
            'sizeof(vdl2hip_tx),sizeof(vdl2hip_txlog_info),offsetof(vdl2hip_tx,first_sample),offsetof(vdl2hip_tx,peak_power),offsetof(vdl2hip_tx,frames),'
            'offsetof(vdl2hip_txlog_info,kernel_ms));return 0;}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert got == [16, 80, 64, vdl2hip.TX_DTYPE.fields["first_sample"][1], vdl2hip.TX_DTYPE.fields["peak_power"][1], 64, 56]
    # without a receiver every entry point refuses
    assert lib.vdl2hip_txlog_enable(None, None) == -1 and lib.vdl2hip_txlog_disable(None) == -1
    assert lib.vdl2hip_txlog_info_get(None, None) == -1 and lib.vdl2hip_txlog_read(None, None, 0) == -1
