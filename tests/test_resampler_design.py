"""The resampler's design (vdl2hip_resampler_design, csrc/resample_design.h): host code, double precision, no GPU.

With fmin = min(input_rate, output_rate) the float32 taps must give: ripple <= 0.01 dB over |f| <= 0.40 fmin, >= 80 dB down for
|f| >= 0.60 fmin, every phase's DC gain within 3e-4 of 1 - measured here on an FFT of at least 64 times the tap count - and the ratios
the library does not take must be refused by the design call and by vdl2hip_create() alike, before a device is looked for."""
import ctypes as C
import math

import numpy as np
import pytest

CF = 136975000
E_INVAL, E_TOOBIG = -1, -4
# (input_rate, output_rate): the rates of the issue's table, 1.92 and 2.0 MS/s, and 10 -> 3.36 MS/s (oversample 32)
RATES = [(1250000, 1050000), (2500000, 2100000), (2400000, 2100000), (1000000, 1050000), (2048000, 2100000), (6000000, 2100000),
         (10000000, 2100000), (1920000, 2100000), (2000000, 2100000), (10000000, 3360000)]
REFUSED = [(2100001, 2100000), (17000000, 2100000), (500000, 2100000)]      # L > 1024; input_rate > 8 fout; 4 input_rate < fout


@pytest.fixture(scope="module")
def vh():
    from dumpvdl2_amd import build, vdl2hip
    build.build()
    vdl2hip.load_library()
    return vdl2hip


@pytest.mark.parametrize("fin,fout", RATES, ids=[f"{a}->{b}" for a, b in RATES])
def test_design_meets_its_specification(vh, fin, fout):
    L, M, T, taps = vh.resampler_design(fin, fout)
    g = math.gcd(fin, fout)
    assert (L, M) == (fout // g, fin // g) and math.gcd(L, M) == 1
    assert taps.shape == (T, L) and taps.dtype == np.float32
    h = taps.reshape(-1).astype(np.float64)                   # prototype order h[j L + p], at the rate L * fin
    nfft = 1 << int(math.ceil(math.log2(64 * h.size)))
    H = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(H.size) * (float(L) * fin / nfft)
    fmin = min(fin, fout)
    ripple = float(np.abs(20 * np.log10(H[f <= 0.40 * fmin])).max())
    stop = float(-20 * np.log10(H[f >= 0.60 * fmin].max()))
    dc = float(np.abs(taps.astype(np.float64).sum(axis=0) - 1.0).max())
    print(f"{fin} -> {fout}: L {L} M {M} T {T} ripple {ripple:.4f} dB stopband {stop:.2f} dB phase DC {dc:.2e}")
    assert ripple <= 0.01 and stop >= 80.0 and dc <= 3e-4, (ripple, stop, dc)


@pytest.mark.parametrize("fin,fout", REFUSED, ids=[f"{a}->{b}" for a, b in REFUSED])
def test_unsupported_ratios_are_refused(vh, fin, fout):
    lib = vh.load_library()
    L, M, T = C.c_uint32(), C.c_uint32(), C.c_uint32()
    buf = np.zeros(1 << 16, dtype=np.float32)
    assert lib.vdl2hip_resampler_design(fin, fout, C.byref(L), C.byref(M), C.byref(T), buf.ctypes.data, buf.size) == E_INVAL
    with pytest.raises(vh.Vdl2HipError, match="invalid argument"):
        vh.resampler_design(fin, fout)
    # vdl2hip_create(): refused while the arguments are checked - with or without a GPU (a supported rate gets past that: to a
    # receiver where there is a device, to VDL2HIP_E_DEVICE where there is none)
    assert fout == 2100000
    freqs = (C.c_uint32 * 1)(CF)
    cfg = vh.Cfg(C.sizeof(vh.Cfg), CF, 20, vh.FMT_S16LE, 1, freqs, 0.0, 0, 0, 0, 0, 0, fin, 0)
    h = C.c_void_p()
    assert lib.vdl2hip_create(C.byref(cfg), C.byref(h)) == E_INVAL


def test_reserved_word_must_be_zero(vh):
    lib = vh.load_library()
    assert C.sizeof(vh.Cfg) == 64 and vh.Cfg.input_rate.offset == 56
    freqs = (C.c_uint32 * 1)(CF)
    cfg = vh.Cfg(C.sizeof(vh.Cfg), CF, 20, vh.FMT_S16LE, 1, freqs, 0.0, 0, 0, 0, 0, 0, 0, 1)
    h = C.c_void_p()
    assert lib.vdl2hip_create(C.byref(cfg), C.byref(h)) == E_INVAL


def test_small_cap_still_reports_the_sizes(vh):
    lib = vh.load_library()
    L, M, T = C.c_uint32(), C.c_uint32(), C.c_uint32()
    buf = np.full(21 * 40, 7.0, dtype=np.float32)
    assert lib.vdl2hip_resampler_design(2500000, 2100000, C.byref(L), C.byref(M), C.byref(T), buf.ctypes.data, 100) == E_TOOBIG
    assert (L.value, M.value) == (21, 25) and 27 <= T.value <= 40
    assert np.all(buf == 7.0)                                  # nothing written beyond (or within) a buffer that is too small
    n = L.value * T.value
    assert lib.vdl2hip_resampler_design(2500000, 2100000, C.byref(L), C.byref(M), C.byref(T), buf.ctypes.data, n - 1) == E_TOOBIG
    assert lib.vdl2hip_resampler_design(2500000, 2100000, C.byref(L), C.byref(M), C.byref(T), buf.ctypes.data, n) == n
    assert np.all(buf[:n] != 7.0) and np.all(buf[n:] == 7.0)
    # symmetric (linear phase), peak in the middle
    assert np.allclose(buf[:n], buf[:n][::-1], rtol=0, atol=1e-7) and abs(int(np.argmax(buf[:n])) - n // 2) <= 1
