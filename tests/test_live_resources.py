"""vdl2hip_debug_live_resources (not declared in vdl2hip.h): the library's count of the device buffers, page-locked buffers and events
it holds through its owning types (dumpvdl2_amd/csrc/hostmem.h).  Host only: it needs no receiver and no GPU.  What the count does
over a receiver's life is tests/test_gpu_lifecycle.py."""
import ctypes as C

from dumpvdl2_amd import vdl2hip

E_INVAL = -1


def test_nothing_is_held_before_a_receiver_exists():
    L = vdl2hip.load_library()
    out = (C.c_longlong * 3)(-1, -1, -1)
    assert L.vdl2hip_debug_live_resources(out) == 0
    assert list(out) == [0, 0, 0]
    assert vdl2hip.live_resources() == {"device": 0, "pinned": 0, "events": 0}
    assert L.vdl2hip_debug_live_resources(None) == E_INVAL
