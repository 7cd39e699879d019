"""Signed 8-bit input (VDL2HIP_FMT_S8), the part that needs no GPU: the constant in the header and in the binding agree, the ABI
version and the structures are what they were, and vdl2hip_create() takes the value 4 while 3 and 5 stay refused - the format check
precedes the device look-up, so this shows without a device."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_DEVICE = -1, -3
CF = 136975000


def _header_values(tmp_path):
    # (a tiny C program, as tests/test_abi.py does for the structure sizes)
    prog = ('#include <stdio.h>\n#include "vdl2hip.h"\nint main(){printf("%d %d %zu\\n",VDL2HIP_FMT_S8,VDL2HIP_ABI_VERSION,sizeof(vdl2hip_cfg));return 0;}\n')
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    return list(map(int, subprocess.check_output([exe]).split()))


def test_constant_agrees_with_the_header_and_the_abi_stays(tmp_path):
    from dumpvdl2_amd import vdl2hip
    s8, abi, cfg_size = _header_values(tmp_path)
    assert vdl2hip.FMT_S8 == s8 == 4
    assert (vdl2hip.FMT_U8, vdl2hip.FMT_S16LE, vdl2hip.FMT_CF32) == (0, 1, 2)
    assert abi == vdl2hip.ABI_VERSION == 6
    assert cfg_size == C.sizeof(vdl2hip.Cfg) == 64


def test_the_conversion_is_the_s16_conversion_of_the_byte_shifted():
    """(float)b / 128.0f == (float)(256 b) / 32768.0f for all 256 bytes, in float32: what makes an S8 receiver an S16LE receiver fed b << 8"""
    b = np.arange(-128, 128, dtype=np.int8)
    a = b.astype(np.float32) / np.float32(128.0)
    k = (b.astype("<i2") * 256).astype(np.float32) / np.float32(32768.0)
    assert a.tobytes() == k.tobytes()
    assert a.min() == -1.0 and a.max() == 127 / 128 and np.array_equal(a.astype(np.float64) * 128, b.astype(np.float64))


def test_create_takes_4_and_refuses_3_and_5():
    from dumpvdl2_amd import build, vdl2hip
    build.build()
    L = vdl2hip.load_library()
    freqs = (C.c_uint32 * 1)(CF)
    got = {}
    for fmt in (3, 4, 5):
        cfg = vdl2hip.Cfg(C.sizeof(vdl2hip.Cfg), CF, 10, fmt, 1, freqs, 0.0, 0, 320000, 0, 0, 0, 0, 0)
        h = C.c_void_p()
        got[fmt] = L.vdl2hip_create(C.byref(cfg), C.byref(h))
        if h.value:
            L.vdl2hip_destroy(h)
    assert got[3] == E_INVAL and got[5] == E_INVAL, got
    assert got[4] != E_INVAL, got
    assert got[4] in (0, E_DEVICE), got                  # a receiver, or (no device on this machine) the device look-up's refusal
