"""Complex float32 input (VDL2HIP_FMT_CF32), the part that needs no GPU: the constant in the header and in the binding agree, the
ABI version and the structures are what they were, and the synthesiser hands out the waveform unquantised."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_values(tmp_path):
    # (a tiny C program, as tests/test_abi.py does for the structure sizes)
    prog = ('#include <stdio.h>\n#include "vdl2hip.h"\nint main(){printf("%d %d %d %d %zu\\n",VDL2HIP_FMT_U8,VDL2HIP_FMT_S16LE,VDL2HIP_FMT_CF32,'
            'VDL2HIP_ABI_VERSION,sizeof(vdl2hip_cfg));return 0;}\n')
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    return list(map(int, subprocess.check_output([exe]).split()))


def test_constant_agrees_with_the_header_and_the_abi_stays(tmp_path):
    from dumpvdl2_amd import vdl2hip
    u8, s16, cf32, abi, cfg_size = _header_values(tmp_path)
    assert (vdl2hip.FMT_U8, vdl2hip.FMT_S16LE, vdl2hip.FMT_CF32) == (u8, s16, cf32) == (0, 1, 2)
    assert abi == vdl2hip.ABI_VERSION == 6
    assert cfg_size == C.sizeof(vdl2hip.Cfg)


def test_library_reports_the_same_abi_version():
    from dumpvdl2_amd import build, vdl2hip
    build.build()
    assert vdl2hip.load_library().vdl2hip_abi_version() == 6


def test_synthesize_float32_is_the_unquantised_waveform():
    from dumpvdl2_amd import synth
    cfg = synth.SynthConfig(centerfreq=136975000, freqs=[136975000, 137015000], oversample=10, duration_s=0.05, seed=12, amplitude=0.3, noise_sigma=0.01)
    f, bursts_f = synth.synthesize(cfg, dtype=np.float32)
    assert f.dtype == np.float32 and f.size % 2 == 0
    # the other dtypes are what they were: the same waveform, quantised
    i16, bursts_i = synth.synthesize(cfg)
    u8, _ = synth.synthesize(cfg, dtype=np.uint8)
    assert i16.dtype == np.int16 and u8.dtype == np.uint8 and i16.size == u8.size == f.size
    assert np.array_equal(i16, np.clip(np.rint(f * 32768.0), -32768, 32767).astype(np.int16))
    assert np.array_equal(u8, np.clip(np.rint(f * 127.5 + 127.5), 0, 255).astype(np.uint8))
    assert len(bursts_f) == len(bursts_i)
    assert np.any(f * np.float32(32768.0) != np.rint(f * np.float32(32768.0))), "the float32 waveform is quantised"
    with pytest.raises(ValueError):
        synth.synthesize(cfg, dtype=np.float64)
