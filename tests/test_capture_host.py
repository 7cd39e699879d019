"""The burst capture's kernels on the host (dumpvdl2_amd/csrc/capture.h).  Their per-burst steps - the clipped window, the copy with
its two alignment paths, the quality sums over runs of symbols and the fixed tree over 256 lanes, the offsets and the room decision -
are plain functions that the library also builds for the CPU, behind test hooks that need no GPU:
  - vdl2hip_debug_capture_burst: one burst over a ring of 4096 pairs -> window, copied pairs, record;
  - vdl2hip_debug_capture_plan: a feed's burst lists -> every burst's place in the pool, what has no room, the pool's fill.
The quality model and its bounds: tests/capture_model.py."""
import ctypes as C

import numpy as np
import pytest

import capture_model as cm
from dumpvdl2_amd import vdl2hip

RING = 4096
E_INVAL = -1


@pytest.fixture(scope="module")
def lib():
    L = vdl2hip.load_library()
    L.vdl2hip_debug_capture_burst.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2hip_debug_capture_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int64, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def aligned(n_pairs):
    raw = np.zeros(2 * n_pairs + 4, dtype=np.float32)
    o = (-raw.ctypes.data // 4) % 4
    return raw[o:o + 2 * n_pairs].reshape(n_pairs, 2)


@pytest.fixture(scope="module")
def ring():
    """D8PSK-like samples at every ring position: a phase of k pi / 4 plus up to +-0.21 pi / 4 of jitter each, so the step between
    any two of them is up to 0.42 pi / 4 off a constellation point - symbols land on both sides of |e| = 0.25 and none near 0.5 -
    under amplitudes of 0.01 .. 0.1"""
    rng = np.random.default_rng(20261019)
    y = aligned(RING)
    phase = (rng.integers(0, 8, RING) + rng.uniform(-0.21, 0.21, RING)) * (np.pi / 4)
    amp = rng.uniform(0.01, 0.1, RING)
    y[:, 0] = (amp * np.cos(phase)).astype(np.float32)
    y[:, 1] = (amp * np.sin(phase)).astype(np.float32)
    assert y.ctypes.data % 16 == 0
    return y


def burst(nsym, t_first, sync, ord_=7, prev_phi0=0.25, vdphi=0.01, ppm=1.5, prev_n=None, tl_bits=123):
    b = np.zeros(1, dtype=cm.BURST_DTYPE)
    b["nsym"] = nsym; b["tl_bits"] = tl_bits; b["t_first"] = t_first; b["sync_sample"] = sync
    b["end_sample"] = t_first + 10 * (nsym - 1); b["ord"] = ord_; b["prev_n"] = t_first - 10 if prev_n is None else prev_n
    b["prev_phi0"] = prev_phi0; b["vdphi"] = vdphi; b["ppm"] = ppm
    return b


def run_burst(lib, y, b, pre, post, k_end, off=0, chan=3, freq=136975000, expect=0):
    rec = np.zeros(1, dtype=vdl2hip.BURST_DTYPE)
    iq = np.full((70000, 2), np.nan, dtype=np.float32)
    r = lib.vdl2hip_debug_capture_burst(y.ctypes.data, y.shape[0], b.ctypes.data, pre, post, k_end, off, chan, freq, rec.ctypes.data, iq.ctypes.data, iq.shape[0])
    assert r == expect, r
    return rec[0], iq


def check_burst(lib, y, b, pre, post, k_end, off=0):
    rec, iq = run_burst(lib, y, b, pre, post, k_end, off)
    sync, end, t0, nsym = int(b["sync_sample"][0]), int(b["end_sample"][0]), int(b["t_first"][0]), int(b["nsym"][0])
    first, count = cm.window(sync, end, pre, post, k_end)
    assert (int(rec["iq_first"]), int(rec["iq_count"]), int(rec["iq_off"]), int(rec["flags"])) == (first, count, off, 0)
    idx = (first + np.arange(count)) & (RING - 1)
    assert np.array_equal(iq[:count].view(np.uint32), y[idx].view(np.uint32)), "the copied pairs are the ring's, bit for bit"
    assert np.all(np.isnan(iq[count:]))
    assert (int(rec["chan"]), int(rec["freq"]), int(rec["burst_ord"]), int(rec["sync_sample"]), int(rec["end_sample"]), int(rec["first_symbol"])) == (3, 136975000, 7, sync, end, t0)
    assert (int(rec["nsym"]), int(rec["tl_bits"]), int(rec["frames"]), int(rec["frames_ok"]), int(rec["fec_corrections"])) == (nsym, 123, 0, 0, -1)
    assert rec["ppm_error"] == b["ppm"][0] and rec["dphi"] == b["vdphi"][0] and rec["prev_phase"] == b["prev_phi0"][0]
    sym = y[(t0 + 10 * np.arange(nsym)) & (RING - 1)]
    q = cm.quality(sym, b["prev_phi0"][0], b["vdphi"][0])
    cm.check_quality(rec, q, label=f"nsym={nsym} first={first}")
    return rec, q


# ---------------------------------------------------------------- windows
@pytest.mark.parametrize("nsym", [1, 63, 64, 65, 5632])
def test_nsym(lib, ring, nsym):
    """a symbol per lane and fewer, one more than a wavefront's worth, the longest burst (22 symbols a lane, round the ring 13 times)"""
    t0 = 5000
    b = burst(nsym, t0, t0 - 170)
    rec, q = check_burst(lib, ring, b, 256, 32, t0 + 10 * nsym + 500)
    assert q["weak_hi"] > 0 or nsym < 63
    if nsym == 5632:
        assert rec["iq_count"] == 256 + 170 + 56310 + 32 + 1


@pytest.mark.parametrize("sync,off", [(4000, 0), (4001, 0), (4000, 1), (4001, 1), (4003, 5), (4002, 6)])
def test_alignment_paths(lib, ring, sync, off):
    """odd and even iq_first against an odd and even place in the pool: one 16-byte load per store, or two 8-byte ones, with and
    without a single pair in front"""
    for nsym in (20, 21):                                        # (an even and an odd number of pairs)
        b = burst(nsym, sync + 170, sync)
        rec, _ = check_burst(lib, ring, b, 256, 32 + (nsym & 1), 10000, off)
        assert rec["iq_first"] == sync - 256


def test_window_straddles_ring_end(lib, ring):
    sync = 3 * RING - 100                                        # the window begins 356 pairs before the ring's end and runs across it
    b = burst(40, sync + 170, sync)
    rec, _ = check_burst(lib, ring, b, 256, 32, 4 * RING)
    assert (rec["iq_first"] & (RING - 1)) + rec["iq_count"] > RING


def test_clipped_at_zero_and_at_k_end(lib, ring):
    b = burst(30, 200, 30, prev_n=-1, prev_phi0=0.0)             # before the stream: phase 0
    rec, _ = check_burst(lib, ring, b, 256, 32, 5000)
    assert rec["iq_first"] == 0 and rec["iq_count"] == 200 + 290 + 32 + 1
    end = 200 + 290
    for k_end, want_last in ((end + 1, end), (end + 10, end + 9), (end + 33, end + 32), (end + 34, end + 32)):
        rec, _ = check_burst(lib, ring, b, 256, 32, k_end)
        assert rec["iq_first"] + rec["iq_count"] - 1 == want_last
    rec, _ = check_burst(lib, ring, b, 0, 0, 5000)               # post = 0, pre = 0: from the sync to the last symbol
    assert rec["iq_first"] == 30 and rec["iq_count"] == end - 30 + 1
    rec, _ = check_burst(lib, ring, b, 4096, 1024, 1 << 20)      # the limits
    assert rec["iq_first"] == 0 and rec["iq_count"] == end + 1024 + 1


def test_phase_before_the_stream(lib, ring):
    """prev_n = -1: the decoder's phase before the stream is 0, and symbol 0 is judged against it"""
    b = burst(64, 0, 0, prev_n=-1, prev_phi0=0.0, vdphi=-0.02)
    rec, q = check_burst(lib, ring, b, 256, 0, 700)
    assert rec["prev_phase"] == 0.0 and rec["iq_first"] == 0


def test_refused_arguments(lib, ring):
    b = burst(10, 1000, 900)
    for kw in (dict(pre=4097), dict(post=1025), dict(k_end=1090)):
        a = dict(pre=256, post=32, k_end=5000)
        a.update(kw)
        run_burst(lib, ring, b, a["pre"], a["post"], a["k_end"], expect=E_INVAL)
    rec = np.zeros(1, dtype=vdl2hip.BURST_DTYPE)
    assert lib.vdl2hip_debug_capture_burst(ring.ctypes.data + 8, RING // 2, b.ctypes.data, 256, 32, 5000, 0, 0, 0, rec.ctypes.data, None, 0) == E_INVAL


def test_sums_do_not_depend_on_the_place(lib, ring):
    """the same burst placed elsewhere in the pool: the same record but for iq_off - the tree is fixed"""
    b = burst(700, 3000, 2830)
    a, _ = run_burst(lib, ring, b, 256, 32, 20000, off=0)
    c, _ = run_burst(lib, ring, b, 256, 32, 20000, off=12345)
    a, c = a.copy(), c.copy()
    c["iq_off"] = 0
    assert a.tobytes() == c.tobytes()


# ---------------------------------------------------------------- offsets and room
def plan(lib, lists, pre, post, k_end, pool, cap_bursts_chan=None):
    """lists: per channel [(sync, nsym)] -> (iq_off, iq_count, flags, records, pairs in use)"""
    nchan = len(lists)
    capb = cap_bursts_chan or max(1, max(len(l) for l in lists))
    bursts = np.zeros((nchan, capb), dtype=cm.BURST_DTYPE)
    for c, l in enumerate(lists):
        for i, (sync, nsym) in enumerate(l):
            bursts[c, i] = burst(nsym, sync + 170, sync)[0]
    nb = np.array([len(l) for l in lists], dtype=np.uint32)
    total = int(nb.sum())
    off = np.zeros(max(1, total), dtype=np.uint64); cnt = np.zeros(max(1, total), dtype=np.uint32); flags = np.zeros(max(1, total), dtype=np.uint32)
    hdr = np.zeros(2, dtype=np.uint64)
    r = lib.vdl2hip_debug_capture_plan(bursts.ctypes.data, nb.ctypes.data, nchan, capb, pre, post, k_end, pool, off.ctypes.data, cnt.ctypes.data, flags.ctypes.data, total, hdr.ctypes.data)
    assert r == total == int(hdr[0])
    return off[:total], cnt[:total], flags[:total], int(hdr[1])


def model_plan(lists, pre, post, k_end, pool):
    off, cnt, flags, at, used = [], [], [], 0, 0
    for l in lists:
        for sync, nsym in l:
            _, n = cm.window(sync, sync + 170 + 10 * (nsym - 1), pre, post, k_end)
            fits = at + n <= pool
            off.append(at if fits else 0); cnt.append(n if fits else 0); flags.append(0 if fits else 1)
            if fits:
                used = at + n
            at += n
    return np.array(off, dtype=np.uint64), np.array(cnt, dtype=np.uint32), np.array(flags, dtype=np.uint32), used


def seq(n, start=1000, nsym0=20):
    """n bursts one after the other, of nsym0, nsym0 + 1, ... symbols (cycling over 7 lengths)"""
    out, k = [], start
    for i in range(n):
        nsym = nsym0 + i % 7
        out.append((k, nsym))
        k += 170 + 10 * nsym + 300
    return out


def test_offsets_empty_channel_between(lib):
    lists = [seq(3), [], seq(2, 5000), [], [], seq(1, 200)]
    got = plan(lib, lists, 256, 32, 1 << 20, 1 << 20)
    want = model_plan(lists, 256, 32, 1 << 20, 1 << 20)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert got[3] == want[3] == int(got[0][-1] + got[1][-1]) and not got[2].any()
    assert got[0][0] == 0 and np.array_equal(got[0][1:], np.cumsum(got[1])[:-1])      # an exclusive prefix sum in record order


def test_offsets_130_bursts_on_one_channel(lib):
    """more than two rounds of the wave scan on the middle channel, one short of a round and exactly a round beside it"""
    lists = [seq(63), seq(130), seq(64), []]
    got = plan(lib, lists, 100, 0, 1 << 20, 1 << 22, cap_bursts_chan=131)
    want = model_plan(lists, 100, 0, 1 << 20, 1 << 22)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert got[3] == want[3] == int(np.sum(got[1]))


def test_room(lib):
    lists = [seq(2), [], seq(4, 3000)]
    full = plan(lib, lists, 256, 32, 1 << 20, 1 << 20)
    ends = full[0] + full[1]
    for pool in (int(ends[2]) - 1, int(ends[2]), int(ends[0]) - 1, 0, int(ends[4])):
        got = plan(lib, lists, 256, 32, 1 << 20, pool)
        want = model_plan(lists, 256, 32, 1 << 20, pool)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w), pool
        assert got[3] == want[3], pool
        fit = got[2] == 0
        assert np.array_equal(got[0][fit], full[0][fit]) and np.array_equal(got[1][fit], full[1][fit])      # those that fit stay where they were
    got = plan(lib, lists, 256, 32, 1 << 20, int(ends[2]) - 1)
    assert list(got[2]) == [0, 0, 1, 1, 1, 1] and got[3] == int(ends[1])


# ---------------------------------------------------------------- the structures of the header
def test_struct_layouts_match_header(tmp_path):
    """the sizes vdl2hip.h states, as the C compiler lays the structures out, and the offsets the bindings assume"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ("chan", "burst_ord", "nsym", "ppm_error", "flags", "iq_first", "iq_count", "iq_off", "frames", "fec_corrections", "weak_symbols", "mean_power", "phase_err_max")
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vdl2hip.h"\nint main(){printf("%zu %zu %zu %u %u", sizeof(vdl2hip_capture_cfg), sizeof(vdl2hip_burst), ' \
           'sizeof(vdl2hip_capture_info), VDL2HIP_CAPTURE_FAILED_ONLY, VDL2HIP_BURST_NO_ROOM);' + \
           "".join(f'printf(" %zu", offsetof(vdl2hip_burst, {f}));' for f in fields) + 'printf(" %zu %zu\\n", offsetof(vdl2hip_capture_info, bursts), offsetof(vdl2hip_capture_info, kernel_ms));return 0;}\n'
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    assert got[:5] == [24, 128, 56, vdl2hip.CAPTURE_FAILED_ONLY, vdl2hip.BURST_NO_ROOM]
    assert (C.sizeof(vdl2hip.CaptureCfg), vdl2hip.BURST_DTYPE.itemsize, C.sizeof(vdl2hip.CaptureInfo)) == (24, 128, 56)
    assert got[5:5 + len(fields)] == [vdl2hip.BURST_DTYPE.fields[f][1] for f in fields]
    assert got[-2:] == [vdl2hip.CaptureInfo.bursts.offset, vdl2hip.CaptureInfo.kernel_ms.offset]
    assert vdl2hip.load_library().vdl2hip_abi_version() == 6


def test_entry_points_refuse_null():
    L = vdl2hip.load_library()
    cfg = vdl2hip.CaptureCfg(C.sizeof(vdl2hip.CaptureCfg), 256, 32, 0, 0, 0)
    assert L.vdl2hip_capture_enable(None, C.byref(cfg)) == E_INVAL and L.vdl2hip_capture_disable(None) == E_INVAL
    assert L.vdl2hip_capture_info_get(None, None) == E_INVAL and L.vdl2hip_capture_read(None, None, 0, None, 0, None) == E_INVAL
