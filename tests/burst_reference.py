"""Inputs and expected answers for the burst decoder's pieces and the frame finisher (vdl2_core.h: the wave primitives, header_to_geometry,
rs_decode_row, decode_burst, finish_frame; kernels.h: k_frame_finish) - the counterpart of tests/core_reference.py for the back end.  One
place builds every case and what it must give; tests/test_burst_reference.py runs the cases through the host build of the device code (both
lane orders), tests/test_gpu_burst_probe.py through the device build (vdl2hip_debug_burst_probe, vdl2hip_debug_frame_finish, PROBE_HEADER).

The references: numpy for the wave primitives; a numpy restatement of decode.c:209-258 over the tables tests/test_design.py pins for the
header; pyoracle.rs_decode (held to libfec by tests/test_oracle_rs.py); pyoracle.decode_bits - the oracle's own decode_vdl2_burst() on the
channel bits - for bursts; pyoracle.avlc_screen / crc16_x25 for the frame finisher; float64 for the two power figures.  The host build of the
device code is never a reference here: it is a second implementation under test."""
import ctypes as C

import numpy as np

from dumpvdl2_amd import synth
from oracle import pyoracle as po

U32 = np.uint32
K_BURST_WAVES = 2                  # kernels.h: kBurstWaves
K_RES_SLOTS, K_RES_POOL = 8, 1024  # vdl2_core.h: kResSlots, kResPool
K_MAIL_FRAMES, K_MAIL_POOL = 8, 2048
K_FRAME_BUF = 2112 + 64            # sizeof FrameShared::buf
NUM_COUNTERS, NUM_AVLC = 20, 10
CNT_FIRST, CNT_LAST = 6, 17        # CNT_ERR_DATA_TRUNCATED .. CNT_MSG_GOOD_LOUD: what decode_burst() owns
MAX_TL, MAX_TL_CORR = 0x3FFF, 0x1FFF

BURST = np.dtype([("chan", "<i4"), ("nsym", "<i4"), ("t_first", "<i8"), ("sync_sample", "<i8"), ("end_sample", "<i8"), ("ord", "<i8"),
                  ("prev_phi0", "<f4"), ("vdphi", "<f4"), ("ppm", "<f4"), ("vdphi_err", "<f4"), ("prev_n", "<i8"), ("tl_bits", "<u4"),
                  ("syndrome", "<u4"), ("nf_upd", "<i8"), ("sync_evals", "<i8")], align=True)
OUTFRAME = np.dtype([("chan", "<i4"), ("idx", "<i4"), ("len", "<u4"), ("pool_off", "<u4"), ("synd_weight", "<u4"), ("datalen_octets", "<u4"),
                     ("num_fec_corrections", "<i4"), ("frame_pwr_dbfs", "<f4"), ("nf_pwr_dbfs", "<f4"), ("ppm_error", "<f4"),
                     ("burst_ord", "<i8"), ("sync_sample", "<i8"), ("end_sample", "<i8"), ("nf_upd", "<i8"), ("avlc_status", "<u4"),
                     ("dst_addr", "<u4"), ("src_addr", "<u4"), ("pad_", "<u4")], align=True)
OUTCTL = np.dtype([("nbursts", "<u4"), ("nframes", "<u4"), ("pool_used", "<u4"), ("overflow", "<u4"), ("cap_bursts", "<u4"),
                   ("cap_frames", "<u4"), ("cap_pool", "<u4"), ("cap_log", "<u4"), ("nvalid", "<u4"), ("pool_out_used", "<u4"),
                   ("pad_", "<u4", (2,))], align=True)
OUTMAIL = np.dtype([("ctl", OUTCTL), ("frames", OUTFRAME, (K_MAIL_FRAMES,)), ("pool", "u1", (K_MAIL_POOL,))], align=True)
GUARD = 0xA5


# ------------------------------------------------------------------------------------------------------------------------------
# wave primitives
# ------------------------------------------------------------------------------------------------------------------------------
def wave_vectors(seed=11):
    """uint32 [n, 64]: a vector serves all four primitives - its non-zero entries are the flags, its values what is scanned and searched"""
    rng = np.random.default_rng(seed)
    v = [np.zeros((1, 64), U32)]
    one = np.zeros((64, 64), U32); one[np.arange(64), np.arange(64)] = rng.integers(1, 1 << 32, 64, dtype=np.uint64).astype(U32)
    v.append(one)                                                   # a single flag at each lane
    for lanes in ((31,), (32,), (63,), (31, 32), (32, 63), (31, 32, 63), (0, 63)):
        a = np.zeros((1, 64), U32); a[0, list(lanes)] = 1; v.append(a)
    v.append(np.ones((1, 64), U32)); v.append(np.full((1, 64), 0xffffffff, U32))      # all set; the scan wraps, the minimum is all ones
    for dens in (0.02, 0.1, 0.5, 0.9, 0.98):                        # random densities, small and full-range values
        m = rng.random((120, 64)) < dens
        v.append((m * rng.integers(1, 100, (120, 64))).astype(U32)); v.append((m * rng.integers(1, 1 << 32, (120, 64), dtype=np.uint64)).astype(U32))
    v.append(rng.integers(900, 1200, (60, 64)).astype(U32))         # totals past 2^16
    v.append(rng.integers(1 << 25, 1 << 26, (60, 64)).astype(U32))  # totals past 2^31
    v.append(rng.integers(1 << 31, 1 << 32, (60, 64), dtype=np.uint64).astype(U32))   # wrap
    mn = rng.integers(1000, 1 << 32, (64, 64), dtype=np.uint64).astype(U32); mn[np.arange(64), np.arange(64)] = rng.integers(0, 1000, 64).astype(U32)
    v.append(mn)                                                    # the minimum at each lane
    tie = rng.integers(500, 1 << 32, (64, 64), dtype=np.uint64).astype(U32)
    for i in range(64):
        tie[i, rng.choice(64, int(rng.integers(2, 9)), replace=False)] = 77
    v.append(tie)                                                   # ties
    hi = np.full((64, 64), 0xffffffff, U32); hi[np.arange(64), np.arange(64)] = 0xfffffffe; v.append(hi)
    return np.ascontiguousarray(np.concatenate(v))


def wave_expected(v):
    """[n, 68] uint32: wave_first_flag (-1: none), wave_count_flags, the exclusive scan mod 2^32, its total, the minimum"""
    n = len(v)
    out = np.zeros((n, 68), U32)
    nz = v != 0
    out[:, 0] = np.where(nz.any(axis=1), nz.argmax(axis=1), -1).astype(np.int64).astype(U32)
    out[:, 1] = nz.sum(axis=1)
    cs = np.cumsum(v.astype(np.uint64), axis=1)
    out[:, 2] = 0; out[:, 3:66] = (cs[:, :63] & 0xffffffff).astype(U32)
    out[:, 66] = (cs[:, 63] & 0xffffffff).astype(U32)
    out[:, 67] = v.min(axis=1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# header (decode.c:209-258)
# ------------------------------------------------------------------------------------------------------------------------------
HDR_H = np.array(synth.HDR_H, dtype=U32)                       # decode.c:55-61 (tests/test_design.py pins the device's and the oracle's to the reference's)


def _parity(x):
    x = x ^ (x >> 16); x = x ^ (x >> 8); x = x ^ (x >> 4); x = x ^ (x >> 2); x = x ^ (x >> 1)
    return x & U32(1)


def header_syndrome(w):
    w = np.asarray(w, dtype=U32)
    s = np.zeros(w.shape, U32)
    for i in range(5):
        s |= _parity(w & HDR_H[i]) << U32(4 - i)
    return s


def header_fix_table():
    """syndrome -> error pattern: decode.c:63-96 (every single-bit pattern owns its syndrome, six two-bit patterns take the rest)"""
    fix = np.zeros(32, U32)
    for bit in range(25):
        fix[int(header_syndrome(U32(1 << bit)))] = 1 << bit
    for a, b in ((23, 2), (23, 1), (24, 20), (23, 14), (23, 15), (24, 16)):
        e = (1 << a) | (1 << b)
        fix[int(header_syndrome(U32(e)))] = e
    return fix


def _rev17(x):
    r = np.zeros(x.shape, U32)
    for i in range(17):
        r |= ((x >> U32(i)) & U32(1)) << U32(16 - i)
    return r


def header_codewords():
    """all 2^17 codewords, index = TL: 3 reserved zeros, TL LSB first, 5 parity bits (vdl2o_header_parity)"""
    tl = np.arange(1 << 17, dtype=U32)
    up = _rev17(tl)
    L = po.lib()
    par = np.array([L.vdl2o_header_parity(int(u)) for u in up], dtype=U32)
    return (up << U32(5)) | par


def header_words(seed=3):
    rng = np.random.default_rng(seed)
    cw = header_codewords()
    parts = [("codewords", cw)]
    parts.append(("single", (cw[:, None] ^ (U32(1) << np.arange(25, dtype=U32))[None, :]).reshape(-1)))
    parts.append(("random", rng.integers(0, 1 << 25, 1 << 20, dtype=np.uint64).astype(U32)))
    edge_tl = np.array([t for c in (MAX_TL_CORR, MAX_TL) for t in range(c - 3, c + 4)] + [0, 1, 7, 8, 9, 16, 17, 23, 24, 25, (1 << 17) - 1], dtype=np.int64)
    e = cw[edge_tl]
    parts.append(("edges", np.concatenate([e, (e[:, None] ^ (U32(1) << np.arange(25, dtype=U32))[None, :]).reshape(-1)])))
    where = {}; k = 0
    for name, p in parts:
        where[name] = slice(k, k + len(p)); k += len(p)
    return np.ascontiguousarray(np.concatenate([p for _, p in parts])), where


def header_expected(words):
    """[n, 4] uint32: status (0 ok, 1 reserved bits set after correction, 2 too long, 3 no FEC), syndrome, tl_bits, want_bits"""
    fix = header_fix_table()
    keep = U32((1 << 22) - 1)
    h = np.asarray(words, dtype=U32) & keep
    s = header_syndrome(h)
    h = h ^ fix[s]
    bad = (h & keep) != h
    tl = _rev17(h >> U32(5))
    long_ = ~bad & (((s != 0) & (tl > MAX_TL_CORR)) | (tl > MAX_TL))
    octets = tl // 8 + (tl % 8 != 0)
    nblk = octets // 249; last = octets % 249
    fec = nblk * 6 + np.where(last < 3, 0, np.where(last < 31, 2, np.where(last < 68, 4, 6)))
    nofec = ~bad & ~long_ & (fec == 0)
    ok = ~bad & ~long_ & ~nofec
    out = np.zeros((len(h), 4), U32)
    out[:, 0] = np.where(bad, 1, np.where(long_, 2, np.where(nofec, 3, 0)))
    out[:, 1] = s
    out[:, 2] = np.where(bad, 0, tl)
    out[:, 3] = np.where(ok, 8 * (octets + fec), 0)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# Reed-Solomon rows
# ------------------------------------------------------------------------------------------------------------------------------
RS_EDGE_POS = (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 247, 248, 249, 250, 253, 254)


def rs_rows(seed=5, per_class=150, garbage=800):
    """(rows uint8 [n, 256]: 255 octets + npar; nerr [n]: errors put in, -1 for garbage rows).  Rows are made as
    tests/test_oracle_rs.py::test_decoder_matches_libfec makes them: a codeword, the parity a short block does not carry zero-filled, errors on
    the octets that are sent - half of their places from RS_EDGE_POS (the 64-lane stride of the syndrome and Chien phases, the parity), half
    random; a third of the rows end in zeros"""
    rng = np.random.default_rng(seed)
    rows, nerrs = [], []

    def codeword(npar, trailing):
        data = rng.integers(0, 256, 249, dtype=np.uint8)
        if trailing:
            data[int(rng.integers(1, 249)):] = 0
        par = list(po.rs_encode(data.tolist()))
        return list(data) + par[:npar] + [0] * (6 - npar)

    k = 0
    for npar in (6, 4, 2, 0):
        n = 249 + npar
        edge = [p for p in RS_EDGE_POS if p < n]
        for nerr in range(6):
            for _ in range(per_class):
                row = codeword(npar, k % 3 == 0); k += 1
                ne = (nerr + 1) // 2 if rng.random() < 0.5 else nerr // 2
                pos = set(int(p) for p in rng.choice(edge, size=min(ne, len(edge)), replace=False))
                while len(pos) < nerr:
                    pos.add(int(rng.integers(0, n)))
                for p in pos:
                    row[p] ^= int(rng.integers(1, 256))
                rows.append(row + [npar]); nerrs.append(nerr)
    for npar in (6, 4):                                             # every single-error position
        for p in range(255):
            row = codeword(npar, False)
            if p < 249 + npar:
                row[p] ^= int(rng.integers(1, 256))
            rows.append(row + [npar]); nerrs.append(1 if p < 249 + npar else 0)
    for _ in range(garbage):
        npar = int(rng.choice([6, 4, 2, 0]))
        row = rng.integers(0, 256, 255, dtype=np.uint8).tolist()
        for i in range(249 + npar, 255):
            row[i] = 0
        rows.append(row + [npar]); nerrs.append(-1)
    rows = np.array(rows, dtype=np.uint8); nerrs = np.array(nerrs)
    perm = rng.permutation(len(rows))                               # classes interleaved: a row follows any kind of row
    return np.ascontiguousarray(rows[perm]), nerrs[perm]


def rs_expected(rows):
    ret = np.zeros(len(rows), np.int32); out = np.zeros((len(rows), 255), np.uint8)
    for i, r in enumerate(rows):
        ret[i], o = po.rs_decode(r[:255].tolist(), int(r[255]))
        out[i] = np.frombuffer(o, np.uint8)
    return ret, out


def rs_classes(rows, nerr, ret):
    npar = rows[:, 255].astype(int)
    t = npar // 2
    return {"failed": int((ret < 0).sum()),
            "miscorrected": int(((nerr > t) & (ret >= 0) & (npar > 0)).sum()),
            "fixed1": int(((npar == 6) & (nerr == 1) & (ret == 1)).sum()), "fixed2": int(((npar == 6) & (nerr == 2) & (ret == 2)).sum()),
            "fixed3": int(((npar == 6) & (nerr == 3) & (ret == 3)).sum()),
            "short_early": int(((npar < 6) & (npar > 0) & (ret == 6 - npar)).sum())}


RS_FLOORS = {"failed": 100, "miscorrected": 40, "fixed1": 100, "fixed2": 100, "fixed3": 100, "short_early": 100}


def rs_compare(rows, ret_ref, out_ref, ret_got, out_got, label):
    """the rule of tests/test_oracle_rs.py::test_device_rs_stage_matches_libfec: the return value and the 249 data octets always, the whole row
    unless it is an error-free short block (recognised early; its erased parity octets, which nothing reads, are then not filled in)"""
    npar = rows[:, 255].astype(int)
    bad = np.flatnonzero(ret_got != ret_ref)
    assert bad.size == 0, f"{label}: {bad.size} return values differ, first row {bad[0]} (npar {npar[bad[0]]}): {ret_got[bad[0]]} != {ret_ref[bad[0]]}"
    bad = np.flatnonzero((out_got[:, :249] != out_ref[:, :249]).any(axis=1))
    assert bad.size == 0, f"{label}: data octets of {bad.size} rows differ, first row {bad[0]} (npar {npar[bad[0]]}, return {ret_ref[bad[0]]})"
    whole = ~((npar < 6) & (ret_ref == 6 - npar))
    bad = np.flatnonzero(whole & (out_got != out_ref).any(axis=1))
    assert bad.size == 0, f"{label}: parity octets of {bad.size} rows differ, first row {bad[0]} (npar {npar[bad[0]]}, return {ret_ref[bad[0]]})"


# ------------------------------------------------------------------------------------------------------------------------------
# bursts
# ------------------------------------------------------------------------------------------------------------------------------
def steps_to_bits(steps):
    """phase-step indices -> the three channel bits per symbol the slicer appends (demod.c:223, 270-274)"""
    g = synth.GRAY[np.asarray(steps, dtype=np.int64)]
    return ((g[:, None] >> np.array([2, 1, 0])) & 1).astype(np.uint8).reshape(-1)


def bits_to_steps(bits):
    t = np.asarray(bits, dtype=np.int64).reshape(-1, 3)
    return synth.GRAY_INV[t[:, 0] * 4 + t[:, 1] * 2 + t[:, 2]]


def geometry(tl_bits):
    octets = (tl_bits + 7) // 8
    nblk, last = divmod(octets, 249)
    fec = nblk * 6
    if last:
        nblk += 1
    fec += synth.fec_octets_for(last)
    if last == 0:
        last = 249
    return octets, nblk, last, fec


def octet_index(tl_bits, row, col):
    """place in the transmitted octet sequence (data, then FEC; both column-major over the rows: decode.c:135-163) of octet `col` (0..248 data,
    249.. parity) of RS row `row`"""
    octets, nblk, last, fec = geometry(tl_bits)
    if col < 249:
        assert col < (249 if row < nblk - 1 else last)
        return col * nblk + row if col < last else last * nblk + (col - last) * (nblk - 1) + row
    pc = col - 249
    npar_last = synth.fec_octets_for(last)
    assert pc < (6 if row < nblk - 1 else npar_last)
    if npar_last == 0:                                              # the last row carries no parity: the others' six columns over nblk - 1 rows
        return octets + pc * (nblk - 1) + row
    return octets + (pc * nblk + row if pc < npar_last else npar_last * nblk + (pc - npar_last) * (nblk - 1) + row)


def corrupt(bits, tl_bits, places, rng):
    """flip channel bits so that the octets at `places` ((row, col) pairs) are wrong"""
    bits = bits.copy()
    for row, col in places:
        i = 25 + 8 * octet_index(tl_bits, row, col)
        e = int(rng.integers(1, 256))
        for j in range(8):
            if (e >> j) & 1:
                bits[i + j] ^= 1
    return bits


class BurstCase:
    """one burst: its channel bits (header included, scrambled), how it is put on the air, what the oracle makes of the bits"""

    def __init__(self, name, bits, tl_bits, rng, amp=0.25, vdphi=0.0, prev_before_stream=False, far=False):
        self.name, self.bits, self.tl_bits = name, np.ascontiguousarray(bits, dtype=np.uint8), int(tl_bits)
        steps = bits_to_steps(self.bits)
        self.nsym = n = len(steps)
        octets, nblk, last, fec = geometry(self.tl_bits)
        assert n == (25 + 8 * (octets + fec) + 2) // 3
        # samples: A_m exp(j (phi0 + sum of steps pi/4 + (m + 1) vdphi + jitter)), the sample before the first symbol's at phase phi0
        phi0 = 0.0 if prev_before_stream else float(rng.uniform(-np.pi, np.pi))
        jit = rng.uniform(-0.9, 0.9, n + 1) * (np.pi / 16)
        if prev_before_stream:
            jit[0] = 0.0
        ph = phi0 + np.concatenate([[0.0], np.cumsum(steps) * (np.pi / 4) + np.arange(1, n + 1) * vdphi]) + jit
        a = amp * rng.uniform(0.8, 1.25, n + 1)
        y = (a * np.exp(1j * ph)).astype(np.complex64)
        self.t_first = int(rng.integers(1 << 33, 1 << 40)) if far else int(rng.integers(10, 3000))
        self.prev_n = -1 if prev_before_stream else self.t_first - 10
        self.y_prev, self.y = y[0], y[1:]
        self.prev_phi0 = np.float32(0.0) if prev_before_stream else np.float32(np.arctan2(np.float64(y[0].imag), np.float64(y[0].real)))
        self.vdphi = np.float32(vdphi)
        self.pwr = float(np.mean(self.y.real.astype(np.float64) ** 2 + self.y.imag.astype(np.float64) ** 2))
        assert abs(self.pwr - 1.0) > 0.2, "too close to the good_loud threshold for float rounding not to matter"
        self.ppm = np.float32(rng.uniform(-3, 3)); self.syndrome = int(rng.integers(0, 32)) | (int(rng.integers(0, 3)) << 8)
        self.ord = int(rng.integers(0, 1 << 40)); self.sync_sample = self.t_first - int(rng.integers(20, 40)); self.end_sample = self.t_first + 10 * (n - 1)
        self.nf_upd = int(rng.integers(0, 1 << 20))
        self.ring_len = 1 << int(np.ceil(np.log2(10 * n + 16)))
        fr, cnt = po.decode_bits(self.bits, np.float32(self.pwr))
        self.frames, self.cnt = fr, cnt

    def record(self, chan):
        b = np.zeros((), BURST)
        b["chan"], b["nsym"], b["t_first"], b["sync_sample"], b["end_sample"], b["ord"] = chan, self.nsym, self.t_first, self.sync_sample, self.end_sample, self.ord
        b["prev_phi0"], b["vdphi"], b["ppm"], b["vdphi_err"], b["prev_n"] = self.prev_phi0, self.vdphi, self.ppm, 0.0, self.prev_n
        b["tl_bits"], b["syndrome"], b["nf_upd"], b["sync_evals"] = self.tl_bits, self.syndrome, self.nf_upd, 1000 * self.nf_upd
        return b

    def fill_ring(self, ring):
        """ring: complex64 [ring_len] of zeros"""
        m = len(ring) - 1
        assert len(ring) >= 10 * self.nsym + 11
        ring[(self.t_first + 10 * np.arange(self.nsym)) & m] = self.y
        if self.prev_n >= 0:
            ring[self.prev_n & m] = self.y_prev


def burst_from_frames(name, frames, rng, raw_bits=None, places=None, want=None, **kw):
    """want: what the oracle's counters must say for the case to be the one meant (a row beyond repair may be miscorrected instead of
    failing): other errors are drawn until they do"""
    bb = synth.build_burst(frames, rng, raw_bits=raw_bits)
    clean = steps_to_bits(bb.symbols)
    for _ in range(50):
        bits = corrupt(clean, bb.tl_bits, places(bb.tl_bits) if callable(places) else places, rng) if places else clean
        c = BurstCase(name, bits, bb.tl_bits, rng, **kw)
        if want is None or want(c.cnt):
            return c
    return None                                                     # (e.g. a last row too short to fail: the caller draws other frames)


def random_frames_for_octets(total_bits_target, rng):
    """AVLC frames whose HDLC framing comes close to (and not past) total_bits_target bits"""
    frames = []
    while True:
        cur = synth.hdlc_bits(frames).size if frames else 8
        room = (total_bits_target - cur - 8) // 8
        if room < 14:
            break
        n = int(min(room * 5 // 6 - 2, rng.integers(12, 400)))       # stuffing adds at most a sixth
        if n < 9:
            break
        frames.append(synth.make_avlc_frame(rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    return frames


TL_OCTETS = (3, 4, 30, 31, 67, 68, 248, 249, 250, 252, 253, 498, 499, 747, 1992, 2047)


def raw_bits_of_length(tl_bits, rng):
    """an HDLC bit string of exactly tl_bits bits: flag, frames, flags, and stuffed random octets without a closing flag as the tail"""
    frames = random_frames_for_octets(tl_bits - 40, rng) if tl_bits > 200 else []
    hb = synth.hdlc_bits(frames).tolist() if frames else list(FLAG)
    tail = synth.hdlc_bits([rng.integers(0, 256, (tl_bits - len(hb)) // 8 + 2, dtype=np.uint8).tobytes()])[8:-8].tolist()
    out = (hb + tail)[:tl_bits]
    assert len(out) == tl_bits
    return np.array(out, dtype=np.uint8)


FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def burst_cases(seed=21, adversarial=None):
    """the list of BurstCase.  adversarial: the bit strings of tests/test_unstuff_adversarial.py"""
    rng = np.random.default_rng(seed)
    cases = []
    kws = [dict(), dict(amp=1.5), dict(vdphi=0.05), dict(vdphi=-0.05, amp=1.5)]
    k = 0
    # every geometry: TL in octets, and one TL beside each that is not a whole number of octets
    for no in TL_OCTETS:
        for tl in (8 * no, 8 * no - int(rng.integers(1, 8))):
            kw = dict(kws[k % 4]); k += 1
            if k % 5 == 0:
                kw["far"] = True
            if no == 30:
                kw["prev_before_stream"] = tl % 8 == 0
            cases.append(burst_from_frames(f"tl{tl}", [], rng, raw_bits=raw_bits_of_length(tl, rng), **kw))
    # symbol counts around a multiple of the 64 lanes.  nsym = (27 + 8 (octets + FEC)) // 3 is 1, 3 or 6 modulo 8 for every legal TL, so
    # 64 k - 1 and 64 k themselves cannot occur: 64 k - 2, 64 k + 1 and 64 k + 3 are the nearest, the smallest TL that gives each
    for res in (62, 1, 3):
        no = next(n for n in range(3, 2048) if (25 + 8 * (n + geometry(8 * n)[3]) + 2) // 3 % 64 == res)
        cases.append(burst_from_frames(f"nsym{res}", [], rng, raw_bits=raw_bits_of_length(8 * no - 3, rng), **kws[res % 4]))
    # random AVLC frames
    for i in range(40):
        fr = random_frames_for_octets(int(rng.integers(200, 6000)), rng) or [synth.make_avlc_frame(rng.integers(0, 256, 12, dtype=np.uint8).tobytes())]
        cases.append(burst_from_frames(f"avlc{i}", fr, rng, **kws[i % 4]))
    # malformed framing
    for i, bs in enumerate(adversarial or []):
        cases.append(burst_from_frames(f"adv{i}", [], rng, raw_bits=bs, **kws[i % 4]))
    # many frames, longest lists
    cases.append(burst_from_frames("1000x1", [bytes([int(x)]) for x in rng.integers(0, 256, 1000)], rng))
    cases.append(burst_from_frames("65x12", [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in range(65)], rng, amp=1.5))
    cases.append(burst_from_frames("64x12", [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in range(64)], rng))
    cases.append(burst_from_frames("2047flags", [], rng, raw_bits=np.array(FLAG * 2047, dtype=np.uint8)))
    cases.append(burst_from_frames("1x2000", [synth.make_avlc_frame(rng.integers(0, 256, 1998, dtype=np.uint8).tobytes())], rng, far=True))

    # octet errors: (row, col) places as a function of the geometry
    def some_in_every_row(tl):
        octets, nblk, last, fec = geometry(tl)
        out = []
        for r in range(nblk):
            width = (249 if r < nblk - 1 else last)
            npar = 6 if r < nblk - 1 else synth.fec_octets_for(last)
            ne = int(rng.integers(1, npar // 2 + 1)) if npar else 0
            cols = set()
            while len(cols) < ne:
                c = int(rng.choice([0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 247, 248, 249, 250, 254][:15] + [int(rng.integers(0, 255))]))
                if c < width or 249 <= c < 249 + npar:
                    cols.add(c)
            out += [(r, c) for c in cols]
        return out

    def in_row(r, ne, parity=None):
        def f(tl):
            octets, nblk, last, fec = geometry(tl)
            rr = r if r >= 0 else nblk + r
            width = 249 if rr < nblk - 1 else last
            npar = 6 if rr < nblk - 1 else synth.fec_octets_for(last)
            if parity is True:
                cols = 249 + rng.choice(npar, size=min(ne, npar), replace=False)
            else:
                cols = rng.choice(width, size=min(ne, width), replace=False)
            return [(rr, int(c)) for c in cols]
        return f

    def both(*fs):
        return lambda tl: [p for f in fs for p in f(tl)]

    sizes = (40, 120, 300, 700, 1200, 2000)
    for i in range(36):
        fr = random_frames_for_octets(8 * sizes[i % 6], rng)
        cases.append(burst_from_frames(f"fix_all{i}", fr, rng, places=some_in_every_row, **kws[i % 4]))
    for i in range(24):
        fr = random_frames_for_octets(8 * sizes[i % 6], rng)
        cases.append(burst_from_frames(f"fix_one{i}", fr, rng, places=in_row(int(rng.integers(0, 9)) % max(1, geometry(synth.hdlc_bits(fr).size)[1]), 1 + i % 3), **kws[i % 4]))
    for i in range(12):                                             # a first row beyond repair; a last row beyond repair after corrected ones
        for name, pl, want, kw in ((f"bad_first{i}", in_row(0, 4 + i % 3), lambda c: c[10] == 1 and c[14] == 1, kws[i % 4]),
                                   (f"bad_last{i}", both(in_row(0, 1 + i % 3), in_row(-1, 5)), lambda c: c[10] == 1 and c[14] > 1 and c[15] == c[14] - 1, kws[(i + 1) % 4])):
            c = None
            while c is None:
                c = burst_from_frames(name, random_frames_for_octets(8 * (300, 700, 1200, 2000)[i % 4], rng), rng, places=pl, want=want, **kw)
            cases.append(c)
    for i, no in enumerate((20, 29, 40, 60, 249 + 10, 249 + 50, 498 + 29)):   # short last blocks: errors in their data and in their parity
        fr = random_frames_for_octets(8 * no, rng)
        cases.append(burst_from_frames(f"short_data{i}", fr, rng, places=in_row(-1, 1), **kws[i % 4]))
        cases.append(burst_from_frames(f"short_par{i}", fr, rng, places=in_row(-1, 1, parity=True), **kws[(i + 2) % 4]))
        cases.append(burst_from_frames(f"short_over{i}", fr, rng, places=in_row(-1, 3), **kws[(i + 1) % 4]))
    return cases


# the many-frame bursts with room for records / octets that ends in the middle of a list: (burst, cap_frames, cap_pool)
CAPACITY = [("1000x1", 700, 1 << 16), ("1000x1", 4096, 1500), ("65x12", 40, 1 << 16), ("65x12", 4096, 1024 + 600), ("1000x1", 16, 1 << 16), ("65x12", 4096, 16)]


def capacity_group(cases, name):
    n = {c.name: c for c in cases}
    return [n["avlc0"], n[name], n["avlc1"], n["64x12"], n["avlc2"]]


def pack_bursts(cases):
    """(bursts BURST [n], freq uint32 [n], y complex64 [n, ring_len]) - burst i is channel i, so every burst has counters of its own"""
    ring_len = max(c.ring_len for c in cases)
    y = np.zeros((len(cases), ring_len), np.complex64)
    bursts = np.zeros(len(cases), BURST)
    for i, c in enumerate(cases):
        bursts[i] = c.record(i); c.fill_ring(y[i])
    freq = (136000000 + 25000 * np.arange(len(cases))).astype(U32)
    return bursts, freq, y


def split_by_ring(cases, short=4096):
    a = [c for c in cases if c.ring_len <= short]
    b = [c for c in cases if c.ring_len > short]
    return [g for g in (a, b) if g]


def check_bursts(cases, out, nwaves, label, cap_frames, cap_pool, guard_frames, guard_pool, tol_db, expect_overflow=False):
    """out: (frames OUTFRAME [cap + guard], pool uint8 [cap + guard], ctl OUTCTL scalar, cnt uint64 [n, 20]) of a probe run on pack_bursts(cases).
    Returns the figures worth printing."""
    frames, pool, ctl, cnt = out
    assert (frames[cap_frames:].view(np.uint8) == GUARD).all(), f"{label}: the guard behind the frame records was written to"
    assert (pool[cap_pool:] == GUARD).all(), f"{label}: the guard behind the octet pool was written to"
    assert int(ctl["cap_frames"]) == cap_frames and int(ctl["cap_pool"]) == cap_pool
    assert int(ctl["overflow"]) == (1 if expect_overflow else 0), f"{label}: overflow flag {int(ctl['overflow'])}"
    assert int(ctl["nframes"]) >= nwaves * K_RES_SLOTS and int(ctl["pool_used"]) >= nwaves * K_RES_POOL
    nrec = min(int(ctl["nframes"]), cap_frames)
    handed = frames[:nrec]
    untouched = frames[nrec:cap_frames]
    assert (untouched.view(np.uint8) == GUARD).all(), f"{label}: records past ctl.nframes were written to"
    valid = handed[handed["chan"] >= 0]
    others = handed[handed["chan"] < 0]
    assert (others["chan"] == -1).all() and (others["len"] == 0).all(), f"{label}: a record that was handed out is neither a frame nor a tombstone"
    # octet space: inside the pool, inside what the counters have handed out, no two frames share an octet
    order = np.argsort(valid["pool_off"], kind="stable")
    v = valid[order]
    nz = v[v["len"] > 0]
    ends = nz["pool_off"].astype(np.int64) + nz["len"]
    assert (ends <= min(int(ctl["pool_used"]), cap_pool)).all(), f"{label}: a frame's octets lie outside the pool"
    assert (nz["pool_off"][1:].astype(np.int64) >= ends[:-1]).all(), f"{label}: two frames share octets"
    by_chan = {}
    for f in valid:
        by_chan.setdefault(int(f["chan"]), []).append(f)
    worst_db, nframes, missing = 0.0, 0, 0
    for i, c in enumerate(cases):
        got = sorted(by_chan.pop(i, []), key=lambda f: int(f["idx"]))
        want = c.frames
        if expect_overflow:
            missing += len(want) - len(got)
            want = [want[int(f["idx"])] for f in got if 0 <= int(f["idx"]) < len(want)]
            assert len(set(int(f["idx"]) for f in got)) == len(got) == len(want), f"{label}: burst {c.name}: frame numbers {[int(f['idx']) for f in got]}"
        assert len(got) == len(want), f"{label}: burst {c.name}: {len(got)} frames, the oracle has {len(want)}"
        for f, w in zip(got, want):
            assert int(f["idx"]) == w["idx"], f"{label}: burst {c.name}: frame numbers"
            oc = pool[int(f["pool_off"]):int(f["pool_off"]) + int(f["len"])].tobytes()
            assert oc == w["octets"], f"{label}: burst {c.name} frame {w['idx']}: octets differ ({len(oc)} against {len(w['octets'])})"
            assert int(f["datalen_octets"]) == w["datalen_octets"] and int(f["num_fec_corrections"]) == w["num_fec_corrections"], \
                f"{label}: burst {c.name} frame {w['idx']}: datalen {int(f['datalen_octets'])} / corrections {int(f['num_fec_corrections'])}, oracle {w['datalen_octets']} / {w['num_fec_corrections']}"
            assert int(f["synd_weight"]) == c.syndrome >> 8 and int(f["burst_ord"]) == c.ord and int(f["sync_sample"]) == c.sync_sample
            assert int(f["end_sample"]) == c.end_sample and int(f["nf_upd"]) == c.nf_upd
            assert np.float32(f["ppm_error"]).view(U32) == np.float32(c.ppm).view(U32), f"{label}: burst {c.name}: ppm_error is not the burst's"
            d = abs(float(f["frame_pwr_dbfs"]) - 10.0 * np.log10(c.pwr))
            worst_db = max(worst_db, d)
            assert d <= tol_db, f"{label}: burst {c.name}: frame_pwr_dbfs {float(f['frame_pwr_dbfs'])} against {10.0 * np.log10(c.pwr)}"
            assert float(f["nf_pwr_dbfs"]) == 0.0
        nframes += len(got)
        # (overflow changes nothing in what the burst decoder counts: the counters move before the bounds checks)
        g = [int(x) for x in cnt[i]]
        assert g[CNT_FIRST:CNT_LAST + 1] == c.cnt[CNT_FIRST:CNT_LAST + 1], f"{label}: burst {c.name}: counters {g[CNT_FIRST:CNT_LAST + 1]}, oracle {c.cnt[CNT_FIRST:CNT_LAST + 1]}"
        assert g[:CNT_FIRST] == [0] * CNT_FIRST and g[CNT_LAST + 1:] == [0, 0], f"{label}: burst {c.name}: counters that are not the burst decoder's moved: {g}"
    assert not by_chan, f"{label}: frames of channels nobody sent: {sorted(by_chan)}"
    return {"frames": nframes, "records": nrec, "tombstones": int(len(others)), "worst_frame_pwr_db": worst_db, "missing": missing}


# ------------------------------------------------------------------------------------------------------------------------------
# frame finishing
# ------------------------------------------------------------------------------------------------------------------------------
def _rev28(v):
    return int(format(v & 0x0FFFFFFF, "028b")[::-1], 2)


def avlc_address(addr24, typ, status=0, low_bit=0):
    """four address octets that parse_dlc_addr() (avlc.c:158-161) turns into addr:24 | type:3 | status:1"""
    v = _rev28((addr24 & 0xFFFFFF) | ((typ & 7) << 24) | ((status & 1) << 27))
    return bytes([((v & 0x7f) << 1) | low_bit, ((v >> 7) & 0x7f) << 1, ((v >> 14) & 0x7f) << 1, (((v >> 21) & 0x7f) << 1) | 1])


def with_fcs(body):
    fcs = po.crc16_x25(body) ^ 0xFFFF
    return body + bytes([fcs & 0xFF, fcs >> 8])


FINISH_LENGTHS = (0, 1, 10, 11, 12, 13, 14, 15, 2111, K_FRAME_BUF, K_FRAME_BUF + 1, 2300)


def finish_frames(seed=31, n=3000, nchan=5):
    """[(chan, octets, nf_upd)] in list order - tombstones are put in by finish_lists()"""
    rng = np.random.default_rng(seed)
    out = []

    def add(octets, chan=None):
        out.append((int(rng.integers(0, nchan)) if chan is None else chan, bytes(octets), 0))

    for ln in FINISH_LENGTHS:
        for good in (True, False):
            if ln >= 11 and good:
                add(with_fcs(avlc_address(int(rng.integers(0, 1 << 24)), 4) + avlc_address(int(rng.integers(0, 1 << 24)), 1) + rng.integers(0, 256, ln - 10, dtype=np.uint8).tobytes()))
            else:
                add(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
    for st in range(8):                                              # every pair of address types
        for dt in range(8):
            body = avlc_address(int(rng.integers(0, 1 << 24)), dt, int(rng.integers(0, 2)), int(rng.integers(0, 2))) \
                + avlc_address(int(rng.integers(0, 1 << 24)), st, int(rng.integers(0, 2)), int(rng.integers(0, 2))) + rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            add(with_fcs(body))
    while len(out) < n:
        ln = int(rng.integers(0, 60)) if rng.random() < 0.8 else int(rng.integers(60, 600))
        u = rng.random()
        if ln >= 11 and u < 0.6:
            add(with_fcs(rng.integers(0, 256, ln - 2, dtype=np.uint8).tobytes()))
        elif ln >= 11 and u < 0.7:                                   # FCS wrong in one bit
            b = bytearray(with_fcs(rng.integers(0, 256, ln - 2, dtype=np.uint8).tobytes())); b[int(rng.integers(0, ln))] ^= 1 << int(rng.integers(0, 8)); add(b)
        else:
            add(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
    return out


class FinishList:
    """one launch of k_frame_finish: records (tombstones among them) + pool + control block + rings, and what must come out"""

    def __init__(self, name, items, tomb_at, rng, nchan=5, ring_len=64, cap_frames=None, nframes=None):
        """items: [(chan, octets)] of the real records in list order; tomb_at: positions of the final list that are tombstones"""
        self.name, self.nchan, self.ring_len = name, nchan, ring_len
        total = len(items) + len(tomb_at)
        tomb = set(tomb_at)
        assert all(0 <= t < total for t in tomb)
        rec = np.zeros(total, OUTFRAME)
        pool = bytearray()
        self.ring = rng.uniform(0.0005, 2.0, (nchan, ring_len)).astype(np.float32)
        it = iter(items)
        self.expected = []
        self.acnt = [[0] * NUM_AVLC for _ in range(nchan)]
        for i in range(total):
            if i in tomb:
                rec[i]["chan"] = -1
                continue
            chan, octets = next(it)
            pool += rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8).tobytes()        # holes, as the burst decoder's reserves leave them
            r = rec[i]
            r["chan"], r["idx"], r["len"], r["pool_off"] = chan, i % 7, len(octets), len(pool)
            pool += octets
            r["synd_weight"], r["datalen_octets"], r["num_fec_corrections"] = i % 3, len(octets) + 5, i % 5
            r["frame_pwr_dbfs"], r["ppm_error"] = -12.5 + i, 0.25 * i
            r["burst_ord"], r["sync_sample"], r["end_sample"] = i, 1000 * i, 1000 * i + 500
            # nf_upd on both sides of the ring's wrap
            r["nf_upd"] = (ring_len - 1, ring_len, ring_len + 1, 5 * ring_len - 1, 5 * ring_len, 3, 0)[i % 7] if i % 2 else int(rng.integers(0, 1 << 30))
            r["avlc_status"], r["dst_addr"], r["src_addr"], r["pad_"] = 0xdeadbeef, 0xdeadbeef, 0xdeadbeef, 0xdeadbeef
        self.records, self.pool = rec, np.frombuffer(bytes(pool), np.uint8) if pool else np.zeros(0, np.uint8)
        ctl = np.zeros((), OUTCTL)
        ctl["nframes"] = total if nframes is None else nframes
        ctl["cap_frames"] = total if cap_frames is None else cap_frames
        ctl["pool_used"], ctl["cap_pool"] = len(pool), len(pool)
        self.ctl = ctl
        self.nlist = min(int(ctl["nframes"]), int(ctl["cap_frames"]))
        for i in range(self.nlist):
            r = rec[i]
            if r["chan"] < 0:
                continue
            octets = bytes(pool[int(r["pool_off"]):int(r["pool_off"]) + int(r["len"])])
            st, dst, src, d = po.avlc_screen(octets)
            c = self.acnt[int(r["chan"])]
            c[0] += 1
            if st == 1:
                c[1] += 1
            elif st == 2:
                c[3] += 1
            else:
                c[2] += 1
                if d:
                    c[3 + d] += 1
            nf = 20.0 * np.log10(np.float64(self.ring[int(r["chan"]), int(r["nf_upd"]) & (ring_len - 1)]) + 0.001)
            self.expected.append(dict(rec=r.copy(), octets=octets, status=st, dst=dst if st == 0 else 0, src=src if st == 0 else 0, nf=nf, dir=d))
        self.pool_out_used = sum((len(e["octets"]) + 3) & ~3 for e in self.expected)


def finish_lists(seed=33):
    rng = np.random.default_rng(seed)
    frames = finish_frames()
    small = [(c, o) for c, o, _ in frames if len(o) < 200]
    lists = []
    lists.append(FinishList("all3000", [(c, o) for c, o, _ in frames], sorted(rng.choice(3600, 600, replace=False).tolist()), rng))
    for n in (0, 1, 8, 9, 16, 17):
        pick = [small[int(j)] for j in rng.choice(len(small), n, replace=False)] if n else []
        lists.append(FinishList(f"list{n}", pick, [], rng))
    for pos in range(16):                                            # a tombstone at every position of a 16-record chunk
        pick = [small[int(j)] for j in rng.choice(len(small), 31, replace=False)]
        lists.append(FinishList(f"tomb_at{pos}", pick, [16 + pos], rng))
    pick = [small[int(j)] for j in rng.choice(len(small), 40, replace=False)]
    lists.append(FinishList("tomb_chunks", pick, list(range(16, 32)) + list(range(48, 64)) + [70], rng))
    lists.append(FinishList("only_tombs", [], list(range(37)), rng))
    # mail limits: eight records whose octets just fit / just do not fit kMailPool
    for extra in (0, 1):
        pick = [(i % 5, rng.integers(0, 256, 256 if i < 7 else 256 - 3 + 4 * extra, dtype=np.uint8).tobytes()) for i in range(8)]
        lists.append(FinishList(f"mail_pool{extra}", pick, [], rng))
    pick = [small[int(j)] for j in rng.choice(len(small), 40, replace=False)]
    lists.append(FinishList("cap_frames", pick, [3], rng, cap_frames=29, nframes=41))       # the list is cut at cap_frames
    return lists


def check_finish(fl, out, label, tol_db):
    """out: (frames_out OUTFRAME [nrec], pool_out uint8, mail OUTMAIL scalar, acnt uint64 [nchan, 10])"""
    fo, po_, mail, acnt = out
    ctl = mail["ctl"]
    exp = fl.expected
    assert int(ctl["nvalid"]) == len(exp), f"{label} {fl.name}: nvalid {int(ctl['nvalid'])}, {len(exp)} records are frames"
    assert int(ctl["pool_out_used"]) == fl.pool_out_used, f"{label} {fl.name}: pool_out_used {int(ctl['pool_out_used'])} != {fl.pool_out_used}"
    for k in ("nframes", "cap_frames", "pool_used", "cap_pool", "overflow", "nbursts"):
        assert int(ctl[k]) == int(fl.ctl[k]), f"{label} {fl.name}: ctl.{k} changed"
    assert [[int(x) for x in r] for r in acnt] == fl.acnt, f"{label} {fl.name}: AVLC counters {acnt.tolist()} != {fl.acnt}"
    got = fo[:len(exp)]
    assert (fo[len(exp):].view(np.uint8) == GUARD).all(), f"{label} {fl.name}: records written past nvalid"
    assert (po_[fl.pool_out_used:] == GUARD).all(), f"{label} {fl.name}: octets written past pool_out_used"
    # the order across wavefronts is not defined: a multiset, each record with its own octets at its own place
    def key_exp(e):
        return (int(e["rec"]["burst_ord"]),)
    byord = {int(e["rec"]["burst_ord"]): e for e in exp}
    assert len(byord) == len(exp)
    seen = set()
    spans = []
    worst = 0.0
    for g in got:
        o = int(g["burst_ord"])
        assert o in byord and o not in seen, f"{label} {fl.name}: record {o} delivered twice or never sent"
        seen.add(o)
        e = byord[o]; r = e["rec"]
        for k in ("chan", "idx", "len", "synd_weight", "datalen_octets", "num_fec_corrections", "sync_sample", "end_sample", "nf_upd"):
            assert int(g[k]) == int(r[k]), f"{label} {fl.name}: record {o} field {k}"
        assert g["frame_pwr_dbfs"] == r["frame_pwr_dbfs"] and g["ppm_error"] == r["ppm_error"]
        assert (int(g["avlc_status"]), int(g["dst_addr"]), int(g["src_addr"]), int(g["pad_"])) == (e["status"], e["dst"], e["src"], 0), \
            f"{label} {fl.name}: record {o} (len {int(r['len'])}): status/dst/src {int(g['avlc_status'])}/{int(g['dst_addr']):x}/{int(g['src_addr']):x}, oracle {e['status']}/{e['dst']:x}/{e['src']:x}"
        d = abs(float(g["nf_pwr_dbfs"]) - e["nf"]); worst = max(worst, d)
        assert d <= tol_db, f"{label} {fl.name}: record {o}: nf_pwr_dbfs {float(g['nf_pwr_dbfs'])} against {e['nf']}"
        off, ln = int(g["pool_off"]), int(g["len"])
        assert off % 4 == 0 and off + ln <= fl.pool_out_used
        assert po_[off:off + ln].tobytes() == e["octets"], f"{label} {fl.name}: record {o}: delivered octets differ"
        spans.append((off, (ln + 3) & ~3))
    spans.sort()
    assert all(a + l <= b for (a, l), (b, _) in zip(spans, spans[1:])), f"{label} {fl.name}: delivered frames share octet space"
    # the mail copy: the first kMailFrames delivered records, and the octets of those that lie within kMailPool
    for s in range(min(len(exp), K_MAIL_FRAMES)):
        assert mail["frames"][s].tobytes() == got[s].tobytes(), f"{label} {fl.name}: mail record {s} is not the delivered one"
        off, ln = int(got[s]["pool_off"]), int(got[s]["len"])
        if off + ln <= K_MAIL_POOL:
            assert mail["pool"][off:off + ln].tobytes() == po_[off:off + ln].tobytes(), f"{label} {fl.name}: mail octets of record {s}"
    return worst


# ------------------------------------------------------------------------------------------------------------------------------
# the device builds (vdl2hip_debug_burst_probe, vdl2hip_debug_frame_finish, vdl2hip_debug_core_probe kind 8), for the GPU tests
# ------------------------------------------------------------------------------------------------------------------------------
_BP_ARGS = [C.c_int, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def device_wave(L, v, grid=2):
    out = np.full((len(v), 68), 0x5a5a5a5a, U32)
    L.vdl2hip_debug_burst_probe.argtypes = _BP_ARGS
    rc = L.vdl2hip_debug_burst_probe(0, v.ctypes.data, len(v), grid, out.ctypes.data, None, 0, None, 0, 0, 0, 0, 0, None, None, None, None)
    assert rc == 0, f"vdl2hip_debug_burst_probe(wave) = {rc}"
    return out


def device_rs(L, rows, grid=2):
    n = len(rows)
    rows = np.ascontiguousarray(rows)
    buf = np.zeros(n * 256 + n * 4, np.uint8)
    L.vdl2hip_debug_burst_probe.argtypes = _BP_ARGS
    rc = L.vdl2hip_debug_burst_probe(1, rows.ctypes.data, n, grid, buf.ctypes.data, None, 0, None, 0, 0, 0, 0, 0, None, None, None, None)
    assert rc == 0, f"vdl2hip_debug_burst_probe(rs) = {rc}"
    return buf[n * 256:].view(np.int32).copy(), buf[:n * 256].reshape(n, 256)[:, :255].copy()


def device_header(L, words):
    w = np.ascontiguousarray(words, dtype=U32).reshape(-1, 1)
    out = np.full((len(w), 4), 0x5a5a5a5a, U32)
    L.vdl2hip_debug_core_probe.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    rc = L.vdl2hip_debug_core_probe(8, w.ctypes.data, len(w), out.ctypes.data)
    assert rc == 0, f"vdl2hip_debug_core_probe(header) = {rc}"
    return out


def _burst_outputs(n, cap_frames, cap_pool, guard_frames, guard_pool):
    return (np.zeros(cap_frames + guard_frames, OUTFRAME), np.zeros(cap_pool + guard_pool, np.uint8), np.zeros((), OUTCTL), np.zeros((n, NUM_COUNTERS), np.uint64))


def device_bursts(L, packed, grid, cap_frames, cap_pool, guard_frames=64, guard_pool=4096):
    bursts, freq, y = packed
    n = len(bursts)
    fr, pool, ctl, cnt = _burst_outputs(n, cap_frames, cap_pool, guard_frames, guard_pool)
    L.vdl2hip_debug_burst_probe.argtypes = _BP_ARGS
    rc = L.vdl2hip_debug_burst_probe(2, bursts.ctypes.data, n, grid, None, freq.ctypes.data, n, y.ctypes.data, y.shape[1], cap_frames, cap_pool, guard_frames, guard_pool,
                                     fr.ctypes.data, pool.ctypes.data, ctl.ctypes.data, cnt.ctypes.data)
    assert rc == 0, f"vdl2hip_debug_burst_probe(burst) = {rc}"
    return fr, pool, ctl, cnt


def host_bursts(H, packed, nwaves, cap_frames, cap_pool, guard_frames=64, guard_pool=4096):
    """the host build of the same code on the same inputs (tests/hostsim: hostsim_decode_burst)"""
    bursts, freq, y = packed
    n = len(bursts)
    fr, pool, ctl, cnt = _burst_outputs(n, cap_frames, cap_pool, guard_frames, guard_pool)
    H.hostsim_decode_burst.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = H.hostsim_decode_burst(bursts.ctypes.data, n, nwaves, freq.ctypes.data, n, y.ctypes.data, y.shape[1], cap_frames, cap_pool, guard_frames, guard_pool,
                                fr.ctypes.data, pool.ctypes.data, ctl.ctypes.data, cnt.ctypes.data)
    assert rc == 0, f"hostsim_decode_burst = {rc}"
    return fr, pool, ctl, cnt


def device_finish(L, fl, grid):
    nrec = len(fl.records)
    cap = fl.pool_out_used + 64
    fo = np.zeros(max(nrec, 1), OUTFRAME); pout = np.zeros(cap, np.uint8); mail = np.zeros((), OUTMAIL); acnt = np.zeros((fl.nchan, NUM_AVLC), np.uint64)
    assert L.vdl2hip_debug_sizeof_outmail() == OUTMAIL.itemsize
    L.vdl2hip_debug_frame_finish.argtypes = [C.c_uint, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.c_void_p, C.c_void_p]
    rc = L.vdl2hip_debug_frame_finish(grid, fl.records.ctypes.data if nrec else None, nrec, fl.pool.ctypes.data if len(fl.pool) else None, len(fl.pool), fl.ctl.ctypes.data,
                                      fl.ring.ctypes.data, fl.ring_len, fl.nchan, fo.ctypes.data, pout.ctypes.data, cap, mail.ctypes.data, acnt.ctypes.data)
    assert rc == 0, f"vdl2hip_debug_frame_finish({fl.name}) = {rc}"
    return fo[:nrec], pout, mail, acnt
