"""The activity monitor's host-only entry point (include/vdl2hip.h, "Activity monitor"): the 63 edges of the level histogram, and
that the library exports the monitor's five entry points.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

from dumpvdl2_amd import vdl2hip

E_TOOBIG = -4
SYMBOLS = ["vdl2hip_activity_edges", "vdl2hip_activity_enable", "vdl2hip_activity_disable", "vdl2hip_activity_read", "vdl2hip_activity_series"]


@pytest.fixture(scope="module")
def lib():
    return vdl2hip.load_library()


def test_edges(lib):
    e = vdl2hip.activity_edges()
    assert e.dtype == np.float32 and e.shape == (63,)
    assert np.all(np.diff(e.astype(np.float64)) > 0)
    for i in range(63):
        assert e[i] == np.float32(10.0 ** ((-120 + 2 * i) / 10)), i
    raw = np.zeros(64, dtype=np.float32)
    assert lib.vdl2hip_activity_edges(raw.ctypes.data, 64) == 63
    assert np.array_equal(raw[:63], e) and raw[63] == 0


def test_short_cap(lib):
    raw = np.full(63, -1, dtype=np.float32)
    assert lib.vdl2hip_activity_edges(raw.ctypes.data, 62) == E_TOOBIG
    assert lib.vdl2hip_activity_edges(None, 63) == E_TOOBIG
    assert np.all(raw == -1)


def test_symbols_exported(lib):
    for name in SYMBOLS:
        assert name in vdl2hip.EXPORTS
        assert getattr(lib, name) is not None


def test_structures():
    assert C.sizeof(vdl2hip.ActivityCfg) == 24 and C.sizeof(vdl2hip.ActivityInfo) == 48
    assert C.sizeof(vdl2hip.ActivityChan) == 568 == vdl2hip.ACTIVITY_CHAN_DTYPE.itemsize
    for name, _ in vdl2hip.ActivityChan._fields_:
        assert getattr(vdl2hip.ActivityChan, name).offset == vdl2hip.ACTIVITY_CHAN_DTYPE.fields[name][1], name
