"""CPU side of the back end's piecewise checks (tests/burst_reference.py builds every case and its expected answer):
  * the oracle's bit-level entry pyoracle.decode_bits is pinned - to the transmitted frames of synthetic bursts, and to the full oracle on the
    modulated adversarial stream of tests/test_unstuff_adversarial.py;
  * every case then runs through the HOST build of the device code (tests/hostsim), with the lanes of a phase in either order, so that the
    inputs and expectations tests/test_gpu_burst_probe.py gives the device build are proven here first."""
import ctypes as C

import numpy as np
import pytest

import burst_reference as br
import pyhostsim
import test_unstuff_adversarial as adv
from dumpvdl2_amd import synth
from util import TOL_DB

CF = 136975000


@pytest.fixture(scope="module")
def po(oracle_mod):
    return oracle_mod


@pytest.fixture(scope="module")
def adv_bits():
    return adv.adversarial_bitstrings(np.random.default_rng(2024), 150)      # the 150 strings of tests/test_unstuff_adversarial.py


@pytest.fixture(scope="module")
def cases(po, adv_bits):
    return br.burst_cases(adversarial=adv_bits)


@pytest.fixture(scope="module", params=[False, True], ids=["lanes_up", "lanes_down"])
def H(request):
    L = C.CDLL(pyhostsim.build(reverse_lanes=request.param))
    assert L.hostsim_sizeof_burst() == br.BURST.itemsize and L.hostsim_sizeof_outframe() == br.OUTFRAME.itemsize and L.hostsim_sizeof_outctl() == br.OUTCTL.itemsize
    return L


# ---- the oracle's bit-level entry ----
def test_decode_bits_returns_the_transmitted_frames(po):
    rng = np.random.default_rng(8)
    for trial in range(40):
        frames = [synth.make_avlc_frame(rng.integers(0, 256, int(rng.integers(9, 300)), dtype=np.uint8).tobytes()) for _ in range(int(rng.integers(1, 5)))]
        bb = synth.build_burst(frames, rng, [int(rng.integers(0, 4)) for _ in range(9)])
        tx = synth.TxBurst(0, trial, frames, bb.tl_bits, bb.datalen_octets, bb.injected_byte_errors, 0, bb.decodable, 0.0)
        got, cnt = po.decode_bits(br.steps_to_bits(bb.symbols))
        assert all(f["datalen_octets"] == bb.datalen_octets for f in got)
        if bb.decodable:                                             # (a block pushed past its capacity may fail or be miscorrected)
            assert [(0, trial, f["idx"], f["octets"]) for f in got] == synth.expected_frames([tx])
            assert got[0]["num_fec_corrections"] == sum(bb.injected_byte_errors) and cnt[16] == len(frames) and cnt[14] == cnt[15] == bb.num_blocks


def test_decode_bits_matches_the_full_oracle_on_the_adversarial_stream(po, adv_bits):
    iq = adv.make_stream(adv_bits)
    o = po.Oracle(CF, [CF], oversample=10)
    o.process(iq.view(np.uint8), block_bytes=1 << 24)
    full = o.frames()
    c = list(o.counters(0).values())
    assert c[0] == len(adv_bits), "every burst of the stream must have synchronised for the bursts to be told apart by their ordinal"
    rng = np.random.default_rng(1)
    summed = [0] * br.NUM_COUNTERS
    for k, bits in enumerate(adv_bits):
        bb = synth.build_burst([], rng, raw_bits=bits)
        got, cnt = po.decode_bits(br.steps_to_bits(bb.symbols))
        want = [f for f in full if f["burst_ord"] == k]
        assert [(f["idx"], f["octets"], f["synd_weight"], f["datalen_octets"], f["num_fec_corrections"]) for f in got] \
            == [(f["idx"], f["octets"], f["synd_weight"], f["datalen_octets"], f["num_fec_corrections"]) for f in want], f"burst {k}"
        summed = [a + b for a, b in zip(summed, cnt)]
    assert summed[br.CNT_FIRST:br.CNT_LAST] == c[br.CNT_FIRST:br.CNT_LAST]           # (without the power-dependent good_loud)
    assert summed[1:6] == c[1:6]                                                      # the header's verdicts too


# ---- the references' own consistency ----
def test_header_tables_and_codewords(po):
    fix = br.header_fix_table()
    L = po.lib()
    for s, e in enumerate(fix):
        w = C.c_uint32(int(e))
        assert L.vdl2o_header_decode(C.byref(w)) == s and w.value == 0
    cw = br.header_codewords()
    assert (br.header_syndrome(cw) == 0).all() and len(np.unique(cw)) == 1 << 17
    e = br.header_expected(cw)
    tl = np.arange(1 << 17)
    assert (e[:, 1] == 0).all() and (e[tl <= br.MAX_TL, 2] == tl[tl <= br.MAX_TL]).all() and (e[tl > br.MAX_TL, 0] == 2).all()
    assert (e[(tl > 16) & (tl <= br.MAX_TL), 0] == 0).all() and (e[tl <= 16, 0] == 3).all()          # one or two octets carry no FEC


def test_rs_reference_populates_every_class(po):
    rows, nerr = br.rs_rows()
    ret, _ = br.rs_expected(rows)
    cl = br.rs_classes(rows, nerr, ret)
    print("rs classes:", cl, "rows:", len(rows))
    for k, floor in br.RS_FLOORS.items():
        assert cl[k] >= floor, (k, cl)


# ---- every case against the host build ----
def test_host_wave_primitives(H):
    v = br.wave_vectors()
    out = np.zeros((len(v), 68), np.uint32)
    H.hostsim_wave_prims.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    H.hostsim_wave_prims(v.ctypes.data, len(v), out.ctypes.data)
    assert 1500 <= len(v) <= 3000
    assert (out == br.wave_expected(v)).all()


def test_host_header(H):
    w, where = br.header_words()
    out = np.zeros((len(w), 4), np.uint32)
    H.hostsim_header_geometry.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    H.hostsim_header_geometry(w.ctypes.data, len(w), out.ctypes.data)
    exp = br.header_expected(w)
    bad = np.flatnonzero((out != exp).any(axis=1))
    assert bad.size == 0, f"{bad.size} header words, first {w[bad[0]]:#x}: {out[bad[0]]} != {exp[bad[0]]}"
    st = exp[:, 0]
    assert all((st[where["single"]] == k).any() for k in (0, 2, 3)) and all((st[where["random"]] == k).any() for k in (0, 1, 2))


def test_host_rs(H, po):
    rows, nerr = br.rs_rows()
    ret_ref, out_ref = br.rs_expected(rows)
    H.hostsim_rs_decode.restype = C.c_int
    H.hostsim_rs_decode.argtypes = [C.c_void_p, C.c_int]
    for order, label in ((np.arange(len(rows)), "forward"), (np.arange(len(rows))[::-1], "reversed")):
        ret = np.zeros(len(rows), np.int32); out = np.zeros((len(rows), 255), np.uint8)
        for i in order:                                              # (one BurstShared throughout: a row starts on what the row before left)
            d = (C.c_uint8 * 255)(*rows[i, :255].tolist())
            ret[i] = H.hostsim_rs_decode(d, int(rows[i, 255])); out[i] = np.frombuffer(bytes(d), np.uint8)
        br.rs_compare(rows, ret_ref, out_ref, ret, out, label)


def test_burst_cases_populate_what_they_are_for(cases):
    n = {c.name: c for c in cases}
    assert 300 <= len(cases) <= 480
    assert len(n["1000x1"].frames) == 1000 and len(n["65x12"].frames) == 65 and len(n["64x12"].frames) == 64
    assert [f["octets"] for f in n["2047flags"].frames] == [b""] and len(n["1x2000"].frames[0]["octets"]) == 2000
    assert min(c.nsym for c in cases) == 22 and max(c.tl_bits for c in cases) >= 8 * 2047 - 7
    assert {c.nsym % 64 for c in cases} >= {62, 1, 3}                        # (64 k - 1 and 64 k are no legal symbol counts)
    for i in range(12):
        c = n[f"bad_first{i}"].cnt
        assert c[14] == 1 and c[10] == 1 and c[15] == 0 and c[16] == 0 and not n[f"bad_first{i}"].frames       # only blocks.processed and fec_bad move
        c = n[f"bad_last{i}"].cnt
        assert c[10] == 1 and c[15] == c[14] - 1 >= 1 and not n[f"bad_last{i}"].frames
    assert sum(c.cnt[17] for c in cases) > 50 and sum(1 for c in cases if c.frames and not c.cnt[17]) > 50        # both sides of good_loud
    assert sum(1 for c in cases if c.frames and c.frames[0]["num_fec_corrections"] > 0) > 50
    assert sum(c.cnt[13] for c in cases) > 10 and sum(c.cnt[12] for c in cases) > 10                             # unstuff errors, truncated octets
    assert any(c.prev_n == -1 for c in cases) and any(c.t_first > 1 << 32 for c in cases)


@pytest.mark.parametrize("nwaves", [1, 4])
def test_host_bursts(H, cases, nwaves):
    for group in br.split_by_ring(cases):
        packed = br.pack_bursts(group)
        cap_f, cap_p = 8192, 1 << 18
        out = br.host_bursts(H, packed, nwaves, cap_f, cap_p)
        fig = br.check_bursts(group, out, nwaves, f"host, {nwaves} wavefronts, rings of {packed[2].shape[1]}", cap_f, cap_p, 64, 4096, TOL_DB)
        print(fig)


@pytest.mark.parametrize("name,cap_f,cap_p", br.CAPACITY)
def test_host_bursts_at_capacity(H, cases, name, cap_f, cap_p):
    group = br.capacity_group(cases, name)
    out = br.host_bursts(H, br.pack_bursts(group), 2, cap_f, cap_p)
    fig = br.check_bursts(group, out, 2, f"host, capacity {cap_f} / {cap_p}", cap_f, cap_p, 64, 4096, TOL_DB, expect_overflow=True)
    assert fig["missing"] > 0
    print(fig)


def test_host_finish_frame(H):
    """the frame finisher's cases, record by record, through the host build's finish_frame() (k_frame_finish itself exists on the device only)"""
    H.hostsim_finish_frame.restype = C.c_int
    H.hostsim_finish_frame.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_ulonglong)]
    lists = br.finish_lists()
    assert len(lists[0].expected) == 3000 and {len(e["octets"]) for e in lists[0].expected} >= set(br.FINISH_LENGTHS)
    assert {e["dir"] for e in lists[0].expected if e["status"] == 0} == {0, 1, 2, 3, 4, 5, 6} and {e["status"] for e in lists[0].expected} == {0, 1, 2}
    for fl in lists:
        acnt = [(C.c_ulonglong * 10)() for _ in range(fl.nchan)]
        for e in fl.expected:
            dst = C.c_uint32(); src = C.c_uint32()
            st = H.hostsim_finish_frame(e["octets"], len(e["octets"]), C.byref(dst), C.byref(src), acnt[int(e["rec"]["chan"])])
            assert (st, dst.value, src.value) == (e["status"], e["dst"], e["src"]), (fl.name, len(e["octets"]))
        assert [list(a) for a in acnt] == fl.acnt, fl.name


def test_hostsim_frames_with_an_empty_pool(po):
    """a feed whose only frames are zero-length (2 047 back-to-back flags: the most terminators a legal TL holds) has no octets at all"""
    iq = adv.make_stream([np.array(br.FLAG * 2047, dtype=np.uint8)])
    o = po.Oracle(CF, [CF], oversample=10)
    tr = o.trace_all(iq.size // 2 // 10 + 4)
    o.process(iq.view(np.uint8), block_bytes=1 << 24)
    D = o.decimated_count(0)
    hs = pyhostsim.HostSim([CF], 0.0, cap_log2=int(np.ceil(np.log2(D + 70000))))
    hs.feed(tr[:, :D, :])
    fo, fh = o.frames(), hs.frames()
    assert [f["octets"] for f in fo] == [b""] and [f["octets"] for f in fh] == [b""]
    assert list(o.counters(0).values()) == hs.counters(0)
