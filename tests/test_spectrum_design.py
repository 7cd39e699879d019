"""The input monitor's host side (include/vdl2hip.h, "Input monitor"): the analysis windows vdl2hip_spectrum_window() designs, what
the calls refuse, and the layout of the two structures.  Nothing here needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_TOOBIG = -1, -4
BH4 = (0.35875, 0.48829, 0.14128, 0.01168)


@pytest.fixture(scope="module")
def vh():
    from dumpvdl2_amd import build, vdl2hip
    build.build()
    vdl2hip.load_library()
    return vdl2hip


def window_formula(window, n):
    t = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    if window == 0:
        return np.ones(n)
    if window == 1:
        return 0.5 - 0.5 * np.cos(t)
    return BH4[0] - BH4[1] * np.cos(t) + BH4[2] * np.cos(2 * t) - BH4[3] * np.cos(3 * t)


@pytest.mark.parametrize("n", [64, 1024, 4096])
@pytest.mark.parametrize("window", [0, 1, 2])
def test_window_values(vh, n, window):
    w = vh.spectrum_window(n, window)
    assert w.dtype == np.float32 and w.shape == (n,)
    ref = window_formula(window, n)
    if window == 0:
        assert np.all(w == 1.0)
    # within 1 float32 ulp (of the value itself) of the double formula
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(w.astype(np.float64) - ref) <= ulp), np.max(np.abs(w.astype(np.float64) - ref) / ulp)
    wd = w.astype(np.float64)
    enbw = n * np.sum(wd * wd) / np.sum(wd) ** 2
    expect = [1.0, 1.5, (BH4[0] ** 2 + (BH4[1] ** 2 + BH4[2] ** 2 + BH4[3] ** 2) / 2) / BH4[0] ** 2][window]
    assert abs(expect - [1.0, 1.5, 2.00435][window]) < 1e-4
    assert abs(enbw - expect) < 1e-4


def test_refusals(vh):
    L = vh.load_library()
    buf = np.zeros(8192, dtype=np.float32)
    for nfft in (0, 32, 48, 96, 8192):
        assert L.vdl2hip_spectrum_window(nfft, vh.WIN_HANN, buf.ctypes.data, buf.size) == E_INVAL, nfft
    assert L.vdl2hip_spectrum_window(1024, 3, buf.ctypes.data, buf.size) == E_INVAL
    for nfft in (64, 1024, 4096):
        assert L.vdl2hip_spectrum_window(nfft, vh.WIN_BH4, buf.ctypes.data, nfft - 1) == E_TOOBIG
        assert L.vdl2hip_spectrum_window(nfft, vh.WIN_BH4, buf.ctypes.data, nfft) == nfft
    with pytest.raises(vh.Vdl2HipError):
        vh.spectrum_window(96)
    # the calls on a receiver refuse a missing one without looking for a device
    assert L.vdl2hip_spectrum_enable(None, None) == E_INVAL
    assert L.vdl2hip_spectrum_read(None, None, None, 0, 0) == E_INVAL
    assert L.vdl2hip_spectrum_channels(None, None, 0) == E_INVAL


def test_struct_sizes_and_exports(vh, tmp_path):
    prog = ('#include <stdio.h>\n#include "vdl2hip.h"\nint main(){printf("%zu %zu %d %d %d\\n",sizeof(vdl2hip_spectrum_cfg),'
            'sizeof(vdl2hip_spectrum_info),VDL2HIP_WIN_RECT,VDL2HIP_WIN_HANN,VDL2HIP_WIN_BH4);return 0;}\n')
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    a, b, r, h, k = map(int, subprocess.check_output([str(tmp_path / "t")]).split())
    assert (a, b) == (16, 88)
    assert (a, b) == (C.sizeof(vh.SpectrumCfg), C.sizeof(vh.SpectrumInfo))
    assert (r, h, k) == (vh.WIN_RECT, vh.WIN_HANN, vh.WIN_BH4) == (0, 1, 2)
    L = vh.load_library()
    for name in ("vdl2hip_spectrum_window", "vdl2hip_spectrum_enable", "vdl2hip_spectrum_read", "vdl2hip_spectrum_channels"):
        assert name in vh.EXPORTS and hasattr(L, name)
    assert L.vdl2hip_abi_version() == 6


def test_design_header_is_plain_cxx(tmp_path):
    """spectrum_design.h is host-only: it compiles without hipcc or any HIP header"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "spectrum_design.h"\nint main() { vdl2::SpectrumDesign d; return vdl2::design_spectrum(1024, 2, d) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "dumpvdl2_amd", "csrc"), str(src)])
