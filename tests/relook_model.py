"""The yardstick for the second look (include/vdl2hip.h, "Second look"; dumpvdl2_amd/csrc/relook.h): plain numpy and the CPU oracle, no
GPU, nothing of the library under test.

  anchors   from txsearch_model.metric (the dense p(n), s(n)) and the definition's local-minimum rule
  slicing   capture_model.slice_args (the float32 steps of slice_symbol()), rounded as C's roundf, C's % 8
  header    burst_reference.header_expected (held to the oracle's tables by tests/test_burst_reference.py)
  decoding  oracle.pyoracle.decode_bits: the reference's header and data state on the bit FIFO
  frame_pwr the reference's running mean (demod.c:266-268) in float32, symbol by symbol

Every integer field, pherr, slope, ppm_error, prev_phase and all octets are compared exactly; frame_pwr_dbfs within util.TOL_DB, the
tolerance tests/test_gpu_burst_probe.py applies to that figure (the decoder forms the mean of the same terms from 64 partial sums)."""
import numpy as np

import burst_reference as br
import capture_model as cm
import core_reference as cr
import txsearch_model as tm
from dumpvdl2_amd import synth
from oracle import pyoracle as po
from util import TOL_DB

F32 = np.float32
R = 160
PARTIAL, PPM_REJECT, TRUNCATED, NO_ROOM = 1, 2, 4, 8
DEF_THR, DEF_ANCHORS, DEF_FRAMES, DEF_OCTETS = F32(4.0), 4, 4096, 1 << 20
CNT = {n: i for i, n in enumerate(["SYNC_GOOD", "CRC_GOOD", "CRC_BAD", "ERR_NO_HEADER", "ERR_TOO_LONG", "ERR_NO_FEC", "ERR_DATA_TRUNCATED",
                                   "ERR_FEC_TRUNCATED", "ERR_DEINTERLEAVE_DATA", "ERR_DEINTERLEAVE_FEC", "ERR_FEC_BAD", "ERR_BITSTREAM",
                                   "ERR_TRUNCATED_OCTETS", "ERR_UNSTUFF", "BLOCKS_PROCESSED", "BLOCKS_FEC_OK", "MSG_GOOD", "MSG_GOOD_LOUD",
                                   "PPM_REJECT", "SLICER_NEG_IDX"])}
HDR_STOP = {1: CNT["CRC_BAD"], 2: CNT["ERR_TOO_LONG"], 3: CNT["ERR_NO_FEC"]}
FLOAT_FIELDS = ("pherr", "slope", "ppm_error", "prev_phase")
INT_FIELDS = ("anchor", "end_sample", "tl_bits", "nsym", "synd_weight", "stop", "frames", "frames_ok", "fec_corrections", "flags")


def anchors(p, thr):
    """indices into p (float32, the whole range in ascending n) that are anchors; a NaN is never one and never beats one"""
    q = np.where(np.isnan(p), F32(np.inf), np.asarray(p, dtype=F32))
    out = []
    for i in np.flatnonzero(q < F32(thr)):
        i = int(i)
        if np.all(q[max(0, i - R):i] > q[i]) and np.all(q[i + 1:i + R + 1] >= q[i]):
            out.append(i)
    return out


def select(idx, p, K):
    """the K best by (p ascending, n ascending), reported in ascending n"""
    return sorted(sorted(idx, key=lambda i: (float(p[i]), i))[:K])


def claim(tl_bits):
    octets = (tl_bits + 7) // 8
    f = octets // 2 + 1
    return f, (octets + 3 * f + 3) & ~3


def _samples(get, n):
    return np.asarray(get(np.asarray(n, dtype=np.int64)), dtype=np.complex64)


def _phase(v):
    return np.arctan2(v.imag.astype(np.float64), v.real.astype(np.float64)).astype(F32)


def _slice(ph, prev, slope):
    u = cm.slice_args(ph, prev, slope)
    r = cr._roundf(u).astype(np.int64)
    idx = np.where(r >= 0, r % 8, -((-r) % 8))               # C's %: the sign of the dividend
    neg = int(np.count_nonzero(idx < 0))
    g = synth.GRAY[idx & 7]
    bits = np.stack([(g >> 2) & 1, (g >> 1) & 1, g & 1], axis=1).reshape(-1).astype(np.uint8)
    return bits, neg


def _running_mean(v):
    re, im = v.real.astype(F32), v.imag.astype(F32)
    spwr = ((re * re).astype(F32) + (im * im).astype(F32)).astype(F32)
    fp = F32(0)
    for k in range(spwr.size):
        fp = F32(F32(F32(fp * F32(k)) + spwr[k]) / F32(k + 1))
    return fp


def attempt(get, a, p, s, freq, limit, max_ppm=0.0):
    """the attempt at anchor a with p(a), s(a) -> (record dict, frames): what decoding would give with all the room it wants"""
    phi0 = _phase(_samples(get, [a]))[0]
    ppm = F32(cr.ppm_of(F32(s), freq))
    r = dict(anchor=a, pherr=F32(p), slope=F32(s), ppm_error=ppm, prev_phase=phi0, tl_bits=0, nsym=0, synd_weight=0, end_sample=a + 90,
             stop=-1, counters=[0] * po.NUM_COUNTERS, frames=0, frames_ok=0, fec_corrections=-1, flags=0, claim=(0, 0))
    if max_ppm != 0.0 and abs(ppm) > F32(max_ppm):
        r["flags"] = PPM_REJECT
        return r, []
    if a + 90 > limit:
        r["flags"] = TRUNCATED
        return r, []
    hv = _samples(get, a + 10 * np.arange(1, 10))
    hbits, hneg = _slice(_phase(hv), phi0, s)
    d = hbits[:25] ^ synth._PRBS[:25]
    word = int(sum(int(b) << (24 - i) for i, b in enumerate(d)))
    status, synd, tl, want = (int(x) for x in br.header_expected(np.array([word], dtype=np.uint32))[0])
    if status != 0:
        c = r["counters"]
        if synd == 0:
            c[CNT["CRC_GOOD"]] += 1
        c[CNT["SLICER_NEG_IDX"]] += hneg
        c[HDR_STOP[status]] += 1
        r["stop"] = HDR_STOP[status]
        return r, []
    nsym = (want + 25 + 2) // 3
    r.update(tl_bits=tl, nsym=nsym, synd_weight=bin(int(br.header_fix_table()[synd])).count("1"), end_sample=a + 10 * nsym)
    if r["end_sample"] > limit:
        r["flags"] = TRUNCATED
        return r, []
    r["claim"] = claim(tl)
    v = _samples(get, a + 10 * np.arange(1, nsym + 1))
    bits, neg = _slice(_phase(v), phi0, s)
    frames, cnt = po.decode_bits(bits, float(_running_mean(v)))
    cnt[CNT["SLICER_NEG_IDX"]] += neg
    r["counters"] = cnt
    stops = [k for k in range(CNT["CRC_BAD"], CNT["ERR_UNSTUFF"] + 1) if cnt[k]]
    r["stop"] = stops[0] if stops else -1
    for f in frames:
        st, dst, src, _ = po.avlc_screen(f["octets"])
        f.update(avlc_status=st, dst_addr=dst if st == 0 else 0, src_addr=src if st == 0 else 0, sync_sample=a, end_sample=r["end_sample"], burst_ord=-1, ppm_error=ppm)
    r.update(frames=len(frames), frames_ok=sum(f["avlc_status"] == 0 for f in frames), fec_corrections=frames[-1]["num_fec_corrections"] if frames else -1)
    return r, frames


def second_look(get, first, last, limit, freq, threshold=0.0, max_anchors=0, max_ppm=0.0, pool_frames=0, pool_octets=0, txflags=0):
    """one transmission first_sample .. last_sample -> (attempts: list of (record dict, frames), anchors found)"""
    thr = F32(threshold) if threshold else DEF_THR
    K = max_anchors or DEF_ANCHORS
    pf, pc = pool_frames or DEF_FRAMES, pool_octets or DEF_OCTETS
    sf, _ = tm.search_range(first, last)
    p, s = tm.metric(get, sf, last)
    idx = anchors(p, thr)
    out = []
    off_f = off_p = 0
    for i in select(idx, p, K):
        r, frames = attempt(get, sf + i, p[i], s[i], freq, limit, max_ppm)
        cf, cp = r.pop("claim")
        if cf and (off_f + cf > pf or off_p + cp > pc):
            r.update(flags=r["flags"] | NO_ROOM, stop=-1, counters=[0] * po.NUM_COUNTERS, frames=0, frames_ok=0, fec_corrections=-1)
            frames = []
        off_f += cf; off_p += cp
        r["flags"] |= txflags & PARTIAL
        out.append((r, frames))
    return out, len(idx)


def check(rec, got_frames, want, want_frames, label=""):
    """a RELOOK_DTYPE row and its frames (dicts) against the model's attempt: exact, floats by their bits, frame_pwr_dbfs within TOL_DB"""
    for k in INT_FIELDS:
        assert int(rec[k]) == int(want[k]), (label, k, int(rec[k]), int(want[k]))
    for k in FLOAT_FIELDS:
        assert tm.same_bits(rec[k], want[k]), (label, k, float(rec[k]), float(want[k]))
    assert [int(x) for x in rec["counters"]] == [int(x) for x in want["counters"]], (label, "counters", list(rec["counters"]), want["counters"])
    assert len(got_frames) == len(want_frames), (label, "frames", len(got_frames), len(want_frames))
    for g, w in zip(got_frames, want_frames):
        assert g["octets"] == w["octets"], (label, "octets of frame", w["idx"])
        for k in ("idx", "synd_weight", "datalen_octets", "num_fec_corrections", "avlc_status", "dst_addr", "src_addr", "sync_sample", "end_sample", "burst_ord"):
            assert int(g[k]) == int(w[k]), (label, k, g[k], w[k])
        assert tm.same_bits(g["ppm_error"], w["ppm_error"]), (label, "ppm_error")
        assert np.isnan(g["nf_pwr_dbfs"]), (label, "nf_pwr_dbfs")
        d = abs(float(g["frame_pwr_dbfs"]) - float(w["frame_pwr_dbfs"]))
        print(f"{label} frame {w['idx']}: frame_pwr_dbfs {float(g['frame_pwr_dbfs']):.6f} model {float(w['frame_pwr_dbfs']):.6f} |diff| {d:.2e} (bound {TOL_DB})")
        assert d <= TOL_DB, (label, "frame_pwr_dbfs", g["frame_pwr_dbfs"], w["frame_pwr_dbfs"])
