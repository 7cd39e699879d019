"""The yardstick for K4, the walker (vdl2_core.h: walk_run, spec_walk, stitch_try_accept, stitch_materialize, stitch_channel; kernels.h: k_walk,
k_walk_spec, k_walk_stitch): the reference program's per-sample state machine - demod() and got_sync(), demod.c:105-286, as
oracle/vdl2_oracle.c states them at chan_demod and chan_try_sync - restated in plain Python over the numpy pieces of tests/core_reference.py
(sync_metric, parabola_vertex, ppm_of, slice_symbol) and tests/burst_reference.py (the header code).  RefChannel visits EVERY sample: it keeps
the 160-entry phase ring, counts v->sclk up to 3 in the search state and up to 10 in the locked state, and knows nothing of candidates, zones,
hops or segments.  Phases are float32(np.arctan2) of float64 arguments.  tests/test_walk_reference.py holds it to the oracle's event trace
(vdl2o_trace_sync_events), event for event, on the oracle's own decimated streams cut into feeds.

One place builds every probe case and what it must give; tests/test_walk_reference.py runs the cases through the host build of the device
code (hostsim_walk_probe: a second witness for the mapping below, not a reference), tests/test_gpu_walk_probe.py through the device build
(vdl2hip_debug_walk_probe).

Two things are done in batches, for speed, and change no value: the phases of a feed are taken for all its samples at once, and got_sync()'s
metric of an evaluation whose 16 ring taps are the contiguous samples n - 150, n - 140 .. n is looked up in a table of cr.sync_metric over
every contiguous window of the stream (check_table=True works every one of them out from the ring as well and compares; the CPU test does).
The data symbols of a burst are sliced at its end, all at once.

THE MAPPING  reference program (vdl2_channel_t, after sample k_end - 1)  ->  WalkState
  mode        0: dstate DM_INIT; 1: DM_SYNC and the header (nine symbols) not yet decoded; 2: DM_SYNC, header good, burst not over.  (A burst
              that ends - or a header that is refused - AT sample k_end - 1 leaves decoder state DEC_IDLE, and demod_reset() runs at the top of
              the next demod() call: the reset touches nothing that call reads before, so it counts as done: mode 0.)
  a           the sample of the first demod() call after the last demod_reset() (0 at the start): the current DM_INIT interval's first sample
  e           the sample of the next got_sync() evaluation: (k_end - 1) + max(1, 3 - sclk)
  e0          the first evaluation since pherr[1], pherr[2] were last set to PHERR_MAX: a + 2 after a reset; n + max(1, 3 - sclk) after a
              got_sync() success at n that --max-ppm dropped (v->sclk keeps the vertex value: demod.c:179, 233)
  bursts      got_sync() successes that locked; evals: got_sync() calls (1000 * mag_nf updates + nfcnt)
  pherr1, pherr2, prev_dphi   v->pherr[1], v->pherr[2], v->prev_slope
  iva, ivb    earlier DM_INIT intervals [first sample, sync sample], most recent first: together with [a, k_end) they say which sample every
              entry of the phase ring holds.  The ring is the meaning: ring_samples() lists the samples of the ring's 160 entries, newest
              first (-1: never written, phase 0), from either side.  k_walk keeps every interval (the newest 32); a stitched walk that adopted
              a speculative segment keeps that segment's own intervals only (stitch_materialize: the oldest of them is longer than 320
              samples and no look-back of 160 gets past it), so niv and the entries beyond what the ring reaches differ between launch
              shapes, legitimately.  The comparison: the 160 ring samples, every shape; iva/ivb entry for entry up to niv = min(syncs, 32), k_walk.
  pb          mode != 0: chan, ord (bursts before it), sync_sample, t_first = sync + max(1, 10 - sclk), prev_phi0 = v->prev_phi at the sync
              (ring[ring_idx - sclk]), prev_n = the sample that ring entry holds, vdphi = v->slope, ppm = v->ppm_error, vdphi_err 0 (no
              referee), sync_evals = evals at the sync, nf_upd = sync_evals / 1000; mode 1: nsym, end_sample, tl_bits, syndrome 0; mode 2:
              tl_bits, syndrome (| weight of the corrected pattern << 8), nsym = ceil((want_bits + 25) / 3), end_sample = t_first + 10 (nsym - 1)
  Fields nothing reads again are left out of the comparison: e in mode != 0 (the burst's end sets it; the walker keeps the place its search
  had reached, the reference program has no such thing while it is locked); prev_dphi - v->prev_slope - in mode != 0 and in mode 0 with
  pherr1 = PHERR_MAX (a success reads it only after an evaluation of the same run has written it: the walker does not keep the slope of the
  evaluation before a success, the reference program does; measured: they differ at every feed end inside a burst); pb in mode 0; iva/ivb
  beyond niv.  Everything else - a, e0, pherr1, pherr2 inside a burst too - is compared in every mode.
A Burst descriptor is pb of mode 2 at the burst's last symbol.  Counters the walker owns: demod.sync.good, decoder.crc.good, decoder.crc.bad,
decoder.errors.too_long, decoder.errors.no_fec, demod.ppm_reject, and demod.slicer_neg_idx of the nine symbols of a refused header (a good
header's are counted by the burst decoder with the rest of the burst).  The evaluation log of a feed: the evaluated samples of [k0, k_end)
in maximal runs of stride 3."""
import ctypes as C

import numpy as np

import burst_reference as br
import core_reference as cr
from dumpvdl2_amd import synth
from nf_reference import ieee_subnormals      # (a process that has loaded a -ffast-math library flushes subnormals, numpy and the host build included)

F32 = np.float32
I64 = np.int64
PHERR_BIG = F32(1000.0)
K_RING, K_SPS, K_SKIP, K_HDR_SYMS, K_HDR_BITS = 160, 10, 3, 9, 25
NUM_IV, MAX_SEG, SPEC_LOG, SPEC_BURSTS, SPEC_REQ, SPEC_BACK, CLEAN_AFTER, FRESH_AFTER = 32, 32, 128, 48, 8, 4096, 320, 156      # vdl2_core.h
NUM_COUNTERS = 20
CNT_SYNC_GOOD, CNT_CRC_GOOD, CNT_CRC_BAD, CNT_TOO_LONG, CNT_NO_FEC, CNT_PPM_REJECT, CNT_NEG_IDX = 0, 1, 2, 4, 5, 18, 19
WALKER_COUNTERS = (CNT_SYNC_GOOD, CNT_CRC_GOOD, CNT_CRC_BAD, CNT_TOO_LONG, CNT_NO_FEC, CNT_PPM_REJECT, CNT_NEG_IDX)
GUARD = 0xA5

BURST = br.BURST
OUTCTL = br.OUTCTL
CHUNK = np.dtype([("first", "<i8"), ("count", "<i8")])
WALKSTATE = np.dtype([("a", "<i8"), ("e", "<i8"), ("e0", "<i8"), ("bursts", "<i8"), ("pherr1", "<f4"), ("pherr2", "<f4"), ("prev_dphi", "<f4"), ("evals", "<i8"),
                      ("mode", "<i4"), ("niv", "<i4"), ("pad_", "<i4"), ("iva", "<i8", (NUM_IV,)), ("ivb", "<i8", (NUM_IV,)), ("pb", BURST)], align=True)
SPECHEAD = np.dtype([("n_first", "<i8"), ("a", "<i8"), ("e", "<i8"), ("e0", "<i8"), ("evals", "<i8"), ("bursts", "<i8"), ("pherr1", "<f4"), ("pherr2", "<f4"),
                     ("prev_dphi", "<f4"), ("mode", "<i4"), ("niv", "<i4"), ("nb", "<u4"), ("nlog", "<u4"), ("ok", "<u4"), ("nreq", "<u4"), ("pad_", "<u4"),
                     ("c_first", CHUNK), ("c_last", CHUNK)], align=True)
REFREQ = np.dtype([("chan", "<i4"), ("kind", "<i4"), ("n", "<i8"), ("t_first", "<i8"), ("prev_n", "<i8"), ("vdphi", "<f4"), ("vdphi_err", "<f4"), ("prev_phi0", "<f4"),
                   ("pad_", "<f4"), ("code", "<u4"), ("pad2_", "<u4")], align=True)
SPECOUT = np.dtype([("h", SPECHEAD), ("st", WALKSTATE), ("cnt", "<u8", (NUM_COUNTERS,)), ("ctl", OUTCTL), ("nlog", "<u4"), ("pad_", "<u4"), ("bursts", BURST, (SPEC_BURSTS,)),
                    ("chunks", CHUNK, (SPEC_LOG,)), ("req", REFREQ, (SPEC_REQ,)), ("nreq", "<u4"), ("pad2_", "<u4")], align=True)

_PRBS25 = np.asarray(synth.scramble_sequence(K_HDR_BITS), dtype=np.uint8)
_GRAY = np.array([0, 1, 3, 2, 6, 7, 5, 4], dtype=np.int64)            # demod.c:223
_FIX = None


def _fix_weight(s):
    global _FIX
    if _FIX is None:
        _FIX = br.header_fix_table()
    return bin(int(_FIX[s])).count("1")


def phases(y):
    """float32 [n]: (float)atan2((double)im, (double)re) - demod.c:232, 256"""
    y = np.asarray(y, dtype=F32)
    return np.arctan2(y[:, 1].astype(np.float64), y[:, 0].astype(np.float64)).astype(F32)


def sync_tables(ph):
    """ChanView's pf and cand for a whole stream from its phases: pf[n] = cr.sync_metric of the contiguous window at n (taps before sample 0
    are phase 0), cand[n] = pf[n - 3].p < 4 && pf[n].p > pf[n - 3].p (n >= 3).  -> (pf float32 [N, 2], cand bool [N])"""
    n = len(ph)
    padded = np.concatenate([np.zeros(150, F32), np.asarray(ph, F32)])
    idx = np.arange(n)[:, None] + 10 * np.arange(16)[None, :]
    pf = np.empty((n, 2), F32)
    for k in range(0, n, 1 << 16):
        p, f = cr.sync_metric(padded[idx[k:k + (1 << 16)]])
        pf[k:k + (1 << 16), 0] = p; pf[k:k + (1 << 16), 1] = f
    cand = np.zeros(n, bool)
    cand[3:] = (pf[:-3, 0] < cr.SYNC_THR) & (pf[3:, 0] > pf[:-3, 0])
    return pf, cand


# ------------------------------------------------------------------------------------------------------------------------------
# the reference: one channel of the reference program, sample by sample
# ------------------------------------------------------------------------------------------------------------------------------
class RefChannel:
    """demod() / got_sync() on one channel's decimated stream y (float32 [N, 2], the whole stream; feeds are stretches of it)"""

    def __init__(self, chan, freq, max_ppm, y, pf=None, check_table=False):
        self.chan, self.freq, self.max_ppm = int(chan), int(freq), F32(max_ppm)
        self.y = np.asarray(y, dtype=F32)
        self.ph = phases(self.y)
        self.pf = pf if pf is not None else sync_tables(self.ph)[0]
        self.check_table = check_table
        # vdl2_channel_t (calloc'ed: vdl2_channel_init(), demod.c:379-392) - the ring as Python floats (a float32 is one exactly)
        self.ring = [0.0] * K_RING
        self.ring_n = [-1] * K_RING                 # bookkeeping: which sample each ring entry holds
        self.ring_idx = 0
        self.sclk = 0
        self.locked = False
        self.pherr1 = self.pherr2 = PHERR_BIG
        self.prev_slope = F32(0)
        self.prev_phi = F32(0); self.slope = F32(0); self.ppm_error = F32(0)
        self.nsym = 0; self.want_bits = K_HDR_BITS; self.header_done = False
        # bookkeeping that is not in the reference program
        self.n = 0                                  # the next sample
        self.evals = 0; self.bursts = 0
        self.a = 0; self.e0 = 2
        self.history = []                           # (first sample, sync sample) of earlier DM_INIT intervals, most recent first
        self.pb = None
        self.counters = np.zeros(NUM_COUNTERS, np.uint64)
        self.neg_all = 0                            # demod.slicer_neg_idx as the reference program counts it: every symbol
        self.events = []                            # dicts: sample, evals, accepted, ppm_error, hdr_status, end_sample
        self.table_checked = 0
        # after every sample: the next evaluation (-1 while locked) and whether the state is "clean" (vdl2_core.h: walk_clean) - what the
        # stitcher's decisions are replayed from (stitch_plan)
        self.t_e = []; self.t_clean = []

    # got_sync()'s metric at sample n from the ring as it stands (demod.c:126-171)
    def _metric(self, n):
        taps = [(self.ring_idx + (i + 1) * K_SPS) % K_RING for i in range(16)]
        contiguous = all(self.ring_n[t] == n - 150 + 10 * i for i, t in enumerate(taps)) if n >= 150 else \
            all(self.ring_n[t] == (n - 150 + 10 * i if n - 150 + 10 * i >= 0 else -1) for i, t in enumerate(taps))
        if contiguous and not self.check_table:
            return self.pf[n, 0], self.pf[n, 1]
        p, f = cr.sync_metric(np.array([[self.ring[t] for t in taps]], dtype=F32))
        if contiguous:
            assert p[0].tobytes() == self.pf[n, 0].tobytes() and f[0].tobytes() == self.pf[n, 1].tobytes(), f"sample {n}: the table of contiguous windows differs from the ring"
            self.table_checked += 1
        return p[0], f[0]

    def _demod_reset(self, a):
        self.sclk = 0; self.locked = False
        self.pherr1 = self.pherr2 = PHERR_BIG
        self.nsym = 0; self.want_bits = K_HDR_BITS; self.header_done = False
        self.a = a; self.e0 = a + 2; self.pb = None

    def _symbols(self, first, count):
        """slice symbols first .. first + count - 1 of the burst in progress -> (index, neg)"""
        t = self.pb["t_first"] + K_SPS * np.arange(first, first + count)
        phi = self.ph[t]
        prev = np.concatenate([[self.pb["prev_phi0"] if first == 0 else self.ph[t[0] - K_SPS]], phi[:-1]]).astype(F32)
        return cr.slice_symbol(phi, prev, np.full(count, self.slope, F32))

    def feed(self, k0, k_end):
        """samples [k0, k_end) -> dict: bursts (BURST [m]), evaluated (int64 [n]: the samples of the got_sync() calls, in order)"""
        assert k0 == self.n and k_end <= len(self.y)
        out_bursts = []; evaluated = []
        for n in range(k0, k_end):
            self._step(n, out_bursts, evaluated)
            e = -1 if self.locked else n + max(1, K_SKIP - self.sclk)
            self.t_e.append(e); self.t_clean.append(e >= self.a + CLEAN_AFTER and e >= self.e0 + 6)
        self.n = k_end
        b = np.zeros(len(out_bursts), BURST)
        for i, d in enumerate(out_bursts):
            for k, v in d.items():
                b[k][i] = v
        return dict(bursts=b, evaluated=np.asarray(evaluated, I64))

    def _step(self, n, out_bursts, evaluated):
        """one demod() call"""
        ph = self.ph
        if not self.locked:
            # demod.c:229-236
            self.ring_idx = (self.ring_idx + 1) % K_RING
            self.ring[self.ring_idx] = float(ph[n]); self.ring_n[self.ring_idx] = n
            self.sclk += 1
            if self.sclk < K_SKIP:
                return
            self.sclk = 0
            self.evals += 1; evaluated.append(n)
            p0, slope = self._metric(n)
            if self.pherr1 < cr.SYNC_THR and p0 > self.pherr1:
                # demod.c:173-193
                vx = cr.parabola_vertex(self.pherr2, self.pherr1, p0)
                assert np.isfinite(vx), f"sample {n}: calc_para_vertex() is not finite (the C program's int conversion would be undefined)"
                self.sclk = int(-cr._roundf(vx))
                assert 0 <= self.sclk < K_RING, (n, self.sclk)
                sp = self.ring_idx - self.sclk
                if sp < 0:
                    sp += K_RING
                self.prev_phi = F32(self.ring[sp]); prev_n = self.ring_n[sp]
                self.slope = self.prev_slope
                self.ppm_error = cr.ppm_of(self.slope, self.freq)[()]
                self.pherr1 = self.pherr2 = PHERR_BIG
                ev = dict(sample=n, evals=self.evals, accepted=0, ppm_error=self.ppm_error, hdr_status=-1, end_sample=-1)
                self.events.append(ev)
                if self.max_ppm != 0 and abs(self.ppm_error) > self.max_ppm:
                    self.counters[CNT_PPM_REJECT] += 1
                    self.e0 = n + max(1, K_SKIP - self.sclk)
                    return
                ev["accepted"] = 1
                self.counters[CNT_SYNC_GOOD] += 1
                self.locked = True
                self.history.insert(0, (self.a, n))
                self.pb = dict(chan=self.chan, nsym=0, t_first=n + max(1, K_SPS - self.sclk), sync_sample=n, end_sample=0, ord=self.bursts, prev_phi0=self.prev_phi,
                               vdphi=self.slope, ppm=self.ppm_error, vdphi_err=F32(0), prev_n=prev_n, tl_bits=0, syndrome=0, nf_upd=self.evals // 1000, sync_evals=self.evals)
                self.bursts += 1
                return
            self.pherr2 = self.pherr1; self.pherr1 = p0; self.prev_slope = slope
            return
        # DM_SYNC: demod.c:252-285
        self.sclk += 1
        if self.sclk < K_SPS:
            return
        self.sclk = 0
        assert n == self.pb["t_first"] + K_SPS * self.nsym
        self.nsym += 1
        if 3 * self.nsym < self.want_bits + (K_HDR_BITS if self.header_done else 0):
            return
        ev = self.events[-1]
        if not self.header_done:
            # decode_vdl2_burst(), decoder state DEC_HEADER: decode.c:198-258
            idx, neg = self._symbols(0, K_HDR_SYMS)
            bits = ((_GRAY[idx][:, None] >> np.array([2, 1, 0])) & 1).reshape(-1)[:K_HDR_BITS].astype(np.uint8) ^ _PRBS25
            word = int(sum(int(b) << (K_HDR_BITS - 1 - i) for i, b in enumerate(bits)))
            status, synd, tl, want = (int(v) for v in br.header_expected(np.array([word], np.uint32))[0])
            self.neg_all += int(neg.sum())
            if synd == 0:
                self.counters[CNT_CRC_GOOD] += 1
            ev["hdr_status"] = status
            if status != 0:
                self.counters[{1: CNT_CRC_BAD, 2: CNT_TOO_LONG, 3: CNT_NO_FEC}[status]] += 1
                self.counters[CNT_NEG_IDX] += int(neg.sum())
                ev["end_sample"] = n
                self._demod_reset(n + 1)
                return
            self.header_done = True; self.want_bits = want
            nsym = (want + K_HDR_BITS + 2) // 3
            self.pb.update(tl_bits=tl, syndrome=synd | (_fix_weight(synd) << 8), nsym=nsym, end_sample=self.pb["t_first"] + K_SPS * (nsym - 1))
            return
        # the burst is over: decoder state DEC_DATA has its want_bits
        assert self.nsym == self.pb["nsym"] and n == self.pb["end_sample"]
        self.neg_all += int(self._symbols(K_HDR_SYMS, self.nsym - K_HDR_SYMS)[1].sum())
        ev["end_sample"] = n
        out_bursts.append(dict(self.pb))
        self._demod_reset(n + 1)

    def state(self):
        """the mapping onto WalkState (one WALKSTATE record) after the samples fed so far"""
        s = np.zeros((), WALKSTATE)
        s["mode"] = 0 if not self.locked else 2 if self.header_done else 1
        s["a"] = self.a; s["e0"] = self.e0; s["e"] = (self.n - 1) + max(1, K_SKIP - self.sclk)
        s["bursts"] = self.bursts; s["evals"] = self.evals
        s["pherr1"] = self.pherr1; s["pherr2"] = self.pherr2; s["prev_dphi"] = self.prev_slope
        h = self.history[:NUM_IV]
        s["niv"] = len(h)
        for i, (ia, ib) in enumerate(h):
            s["iva"][i] = ia; s["ivb"][i] = ib
        if self.locked:
            for k, v in self.pb.items():
                s["pb"][k] = v
        return s

    def ring_samples(self):
        """the samples the ring's 160 entries hold, newest first (-1: never written)"""
        return np.array([self.ring_n[(self.ring_idx - d) % K_RING] for d in range(K_RING)], I64)


def chunks_of(evaluated):
    """the evaluation log of a feed: maximal runs of stride 3 -> int64 [m, 2] = (first, count)"""
    ev = np.asarray(evaluated, I64)
    if len(ev) == 0:
        return np.zeros((0, 2), I64)
    cut = np.flatnonzero(np.diff(ev) != 3) + 1
    starts = np.concatenate([[0], cut]); ends = np.concatenate([cut, [len(ev)]])
    return np.stack([ev[starts], ends - starts], axis=1).astype(I64)


def ring_samples(ws, k_end):
    """the same list from a WalkState record: [a, k_end) of the current interval (mode 0), then the interval history"""
    out = []
    if int(ws["mode"]) == 0:
        out.extend(range(k_end - 1, int(ws["a"]) - 1, -1)[:K_RING])
    for i in range(int(ws["niv"])):
        if len(out) >= K_RING:
            break
        out.extend(range(int(ws["ivb"][i]), int(ws["iva"][i]) - 1, -1)[:K_RING - len(out)])
    out = out[:K_RING] + [-1] * (K_RING - len(out))
    return np.array(out, I64)


STATE_ALWAYS = ("bursts", "evals", "mode", "a", "e0", "pherr1", "pherr2")
STATE_SEARCH = ("e",)


def state_differences(ref, ref_ring, got, k_end, history_entries):
    """names of the fields in which a WalkState record differs from the reference's, by the meaning the mapping above gives (bit patterns for
    the floats).  history_entries: compare niv, iva and ivb entry for entry as well (k_walk)"""
    bad = [k for k in STATE_ALWAYS if ref[k].tobytes() != got[k].tobytes()]
    if int(ref["mode"]) == 0:
        bad += [k for k in STATE_SEARCH if ref[k].tobytes() != got[k].tobytes()]
        if ref["pherr1"] < PHERR_BIG and ref["prev_dphi"].tobytes() != got["prev_dphi"].tobytes():
            bad.append("prev_dphi")
    elif ref["pb"].tobytes() != got["pb"].tobytes():
        bad += ["pb." + k for k in BURST.names if ref["pb"][k].tobytes() != got["pb"][k].tobytes()]
    if not np.array_equal(ref_ring, ring_samples(got, k_end)):
        bad.append("ring")
    if history_entries:
        n = int(ref["niv"])
        if int(got["niv"]) != n or not np.array_equal(ref["iva"][:n], got["iva"][:n]) or not np.array_equal(ref["ivb"][:n], got["ivb"][:n]):
            bad.append("history")
    return bad


def canonical_state(ws, k_end):
    """the bytes of a WalkState record as far as anything that follows can depend on it: what two launch shapes must agree in (field by
    field: the record's alignment holes are nobody's)"""
    live = list(STATE_ALWAYS)
    if int(ws["mode"]) == 0:
        live += list(STATE_SEARCH) + (["prev_dphi"] if ws["pherr1"] < PHERR_BIG else [])
    out = [ws[k].tobytes() for k in live]
    if int(ws["mode"]) != 0:
        out += [ws["pb"][k].tobytes() for k in BURST.names]
    return b"".join(out) + ring_samples(ws, k_end).tobytes()


# ------------------------------------------------------------------------------------------------------------------------------
# launch shapes, and the stitcher's decisions replayed from the reference's own trajectory
# ------------------------------------------------------------------------------------------------------------------------------
def launch_of(shape, D):
    """How a feed of D samples is launched in a shape -> (mode, nseg, seglen).  shape None: k_walk.  ("segments", seg_max, seg_min): what
    launch_back() makes of a receiver with those two settings - k_walk for a feed of fewer than two segments' worth of samples.
    ("seglen", L): segments of exactly L samples (k_walk where that gives fewer than 2 or more than kMaxSeg of them)"""
    if shape is None or D <= 0:
        return 0, 1, D
    if shape[0] == "segments":
        nseg = min(shape[1], D // shape[2])
        if nseg < 2:
            return 0, 1, D
        seglen = (D + nseg - 1) // nseg
        return 1, (D + seglen - 1) // seglen, seglen
    seglen = shape[1]
    nseg = (D + seglen - 1) // seglen
    return (1, nseg, seglen) if 2 <= nseg <= MAX_SEG else (0, 1, D)


def stitch_plan(t_e, t_clean, k0, seglen, nseg, k_end, heads):
    """stitch_channel()'s decisions for one channel and feed, from the reference's trajectory (RefChannel.t_e, t_clean: the state after every
    sample) and the SpecHeads the speculative walks delivered: which segments are adopted (stitch_try_accept's conditions, at the boundary
    or at the first clean state inside the segment) and which are walked.  -> dict of counts"""
    st = dict(adopted=0, walked=0, pre=0, pending=0, history=0, refused_first=0, refused_chunk=0, refused_overflow=0)
    njobs = 0
    for s in range(1, nseg):
        b = k0 + s * seglen
        kn = b + seglen if s + 1 < nseg else k_end

        def attempt(k):                          # the real state is the reference's after sample k - 1
            nonlocal njobs
            if not t_clean[k - 1] or not b <= t_e[k - 1] < kn:
                return False
            e = int(t_e[k - 1]); r = (e - b) % 3; pre = (e - (b + r)) // 3
            H = heads[(s - 1) * 3 + r]
            if not H["ok"]:
                st["refused_overflow"] += 1; return False
            if H["n_first"] < e:
                st["refused_first"] += 1; return False
            if njobs >= MAX_SEG:
                return False
            if H["nlog"] != 0 and H["c_first"]["count"] <= pre:
                st["refused_chunk"] += 1; return False
            njobs += 1
            st["adopted"] += 1; st["pre"] += pre > 0; st["pending"] += H["mode"] != 0; st["history"] += H["niv"] > 0
            return True

        if attempt(b):
            continue
        if not t_clean[b - 1]:
            idx = np.flatnonzero(t_clean[b:kn])
            if len(idx) and attempt(b + int(idx[0]) + 1):
                continue
        st["walked"] += 1
    return st


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """nchan <= len(y) channels (channel c on stream y[c], float32 [N, 2]), fed in the stretches bounds[i] .. bounds[i + 1]"""

    def __init__(self, name, freqs, max_ppm, y, bounds, ring_len=1 << 16, cap_bursts_chan=64, cap_log=8192, note=""):
        self.name, self.freqs, self.max_ppm, self.ring_len, self.cap_bursts_chan, self.cap_log, self.note = name, [int(f) for f in freqs], float(max_ppm), ring_len, cap_bursts_chan, cap_log, note
        self.y = [np.ascontiguousarray(v, dtype=F32) for v in y]
        self.bounds = [int(b) for b in bounds]
        assert self.bounds[0] == 0 and all(b1 >= b0 for b0, b1 in zip(self.bounds, self.bounds[1:])) and all(self.bounds[-1] <= len(v) for v in self.y)
        self._exp = {}

    def feeds(self):
        return list(zip(self.bounds[:-1], self.bounds[1:]))

    @ieee_subnormals()
    def expected(self, c):
        """the reference's answers for channel c: per feed the descriptors, the chunk list, the walker's counters so far, the mapped state and
        the ring's samples; the trajectory; the sync tables (the walker's inputs)"""
        if c not in self._exp:
            ph = phases(self.y[c])
            pf, cand = sync_tables(ph)
            r = RefChannel(c, self.freqs[c], self.max_ppm, self.y[c], pf=pf)
            per_feed = []
            for k0, k1 in self.feeds():
                oldest = min([n for n in r.ring_n if n >= 0] + [k0])
                res = r.feed(k0, k1)
                if r.pb is not None:
                    oldest = min(oldest, r.pb["sync_sample"] - 160)
                assert k1 - oldest <= self.ring_len - 64 - 160, f"{self.name} channel {c} feed [{k0}, {k1}): reaches back to sample {oldest}, the ring holds {self.ring_len}"
                per_feed.append(dict(bursts=res["bursts"], chunks=chunks_of(res["evaluated"]), counters=r.counters.copy(), state=r.state(), ring=r.ring_samples()))
            self._exp[c] = dict(feeds=per_feed, t_e=np.asarray(r.t_e, I64), t_clean=np.asarray(r.t_clean, bool), pf=pf, cand=cand, events=r.events, ref=r)
        return self._exp[c]


def initial_states(nchan):
    ws = np.zeros(nchan, WALKSTATE)
    ws["e"] = 2; ws["e0"] = 2; ws["pherr1"] = PHERR_BIG; ws["pherr2"] = PHERR_BIG
    return ws


class Rings:
    """y, pf and cand as the product keeps them: rings addressed by the sample index, a feed writing its own samples (and, as the sync stage
    does, the metric of whole 64-sample words: beyond the feed's end PHERR_MAX and no candidate).  What no feed has written is poison: NaN
    samples, a metric of (12345, 54321) as tests/hostsim leaves where K3 stores nothing, candidate words of all ones"""

    def __init__(self, nchan, ring_len):
        self.mask = ring_len - 1
        self.y = np.full((nchan, ring_len, 2), np.nan, F32)
        self.pf = np.empty((nchan, ring_len, 2), F32); self.pf[:, :, 0] = 12345.0; self.pf[:, :, 1] = 54321.0
        self.cand = np.full((nchan, ring_len // 64), 0xFFFFFFFFFFFFFFFF, np.uint64)

    def write(self, c, y, pf, cand, k0, k1):
        n = np.arange(k0, k1)
        self.y[c, n & self.mask] = y[k0:k1]
        lo, hi = k0 & ~63, (k1 + 63) & ~63
        n = np.arange(lo, hi)
        v = np.empty((hi - lo, 2), F32); v[:, 0] = PHERR_BIG; v[:, 1] = 0
        v[:max(0, k1 - lo)] = pf[lo:k1]
        self.pf[c, n & self.mask] = v
        bits = np.zeros(hi - lo, np.uint8); bits[:max(0, k1 - lo)] = cand[lo:k1]
        if hi > lo:
            words = np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
            self.cand[c, np.arange(lo >> 6, hi >> 6) & (self.mask >> 6)] = words


_PROBE_ARGS = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
               C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def probe(fn, mode, rings, freqs, max_ppm, k0, k1, nseg, seglen, ws, cnt, cap_bursts_chan, cap_log):
    """one call of vdl2hip_debug_walk_probe / hostsim_walk_probe (the same arguments); ws and cnt are updated in place -> (status, outputs)"""
    nchan = len(ws)
    fn.argtypes = _PROBE_ARGS; fn.restype = C.c_int
    fr = np.asarray(freqs[:nchan], np.uint32)
    out = dict(bursts=np.zeros((nchan, cap_bursts_chan), BURST), nb=np.zeros(nchan, np.uint32), log=np.zeros((nchan, cap_log), CHUNK), nlog=np.zeros(nchan, np.uint32),
               ctl=np.zeros((), OUTCTL), seg=np.zeros((nchan, 2), np.uint32), spec=np.zeros((nchan, 3 * (nseg - 1)), SPECOUT) if mode == 1 else None)
    rc = fn(mode, nchan, rings.y.ctypes.data, rings.pf.ctypes.data, rings.cand.ctypes.data, rings.mask + 1, fr.ctypes.data, max_ppm, k0, k1, nseg, seglen, ws.ctypes.data, cnt.ctypes.data,
            cap_bursts_chan, cap_log, out["bursts"].ctypes.data, out["nb"].ctypes.data, out["log"].ctypes.data, out["nlog"].ctypes.data, out["ctl"].ctypes.data,
            out["seg"].ctypes.data if mode == 1 else None, out["spec"].ctypes.data if mode == 1 else None)
    return rc, out


def device_fn(L):
    assert L.vdl2hip_debug_sizeof_walkstate() == WALKSTATE.itemsize and L.vdl2hip_debug_sizeof_burst() == BURST.itemsize and L.vdl2hip_debug_sizeof_specout() == SPECOUT.itemsize
    return L.vdl2hip_debug_walk_probe


def host_fn(H):
    assert H.hostsim_sizeof_walkstate() == WALKSTATE.itemsize and H.hostsim_sizeof_burst() == BURST.itemsize and H.hostsim_sizeof_specout() == SPECOUT.itemsize
    return H.hostsim_walk_probe


PLAN_KEYS = ("adopted", "walked", "pre", "pending", "history", "refused_first", "refused_chunk", "refused_overflow")


@ieee_subnormals()
def run_case(fn, case, nchan, shape, label):
    """The case's feeds, one probe call each, the state and the counters carried from call to call.  Everything that comes back is held to the
    reference bit for bit: the descriptors (and 0xA5 behind them), the chunk list (the same), nb_chan, nlog, the control block, the counters,
    the end state by its meaning (state_differences), and in stitched feeds seg_stats against stitch_plan().
    -> (the bytes two launch shapes must agree in, stitch statistics summed over channels and feeds)"""
    exp = [case.expected(c) for c in range(nchan)]
    rings = Rings(nchan, case.ring_len)
    ws = initial_states(nchan); cnt = np.zeros((nchan, NUM_COUNTERS), np.uint64)
    blob = []; stats = dict.fromkeys(PLAN_KEYS, 0); stats["stitched_feeds"] = 0
    for i, (k0, k1) in enumerate(case.feeds()):
        where = f"{label} {case.name} feed {i} [{k0}, {k1})"
        for c in range(nchan):
            rings.write(c, case.y[c], exp[c]["pf"], exp[c]["cand"], k0, k1)
        mode, nseg, seglen = launch_of(shape, k1 - k0)
        rc, out = probe(fn, mode, rings, case.freqs, case.max_ppm, k0, k1, nseg, seglen, ws, cnt, case.cap_bursts_chan, case.cap_log)
        assert rc == 0, f"{where}: the probe returned {rc}"
        over = 0
        for c in range(nchan):
            e = exp[c]["feeds"][i]; w = f"{where} channel {c}"
            nb = min(len(e["bursts"]), case.cap_bursts_chan); nl = min(len(e["chunks"]), case.cap_log)
            over |= int(len(e["bursts"]) > case.cap_bursts_chan or len(e["chunks"]) > case.cap_log)
            assert out["nb"][c] == nb, f"{w}: {out['nb'][c]} bursts, the reference {len(e['bursts'])} (room for {case.cap_bursts_chan})"
            got = out["bursts"][c]
            for j in range(nb):
                assert got[j].tobytes() == e["bursts"][j].tobytes(), f"{w} burst {j}: {got[j]} != {e['bursts'][j]}"
            assert got[nb:].tobytes() == bytes([GUARD]) * (got[nb:].nbytes), f"{w}: something was written behind the {nb} descriptors"
            assert out["nlog"][c] == nl, f"{w}: {out['nlog'][c]} chunks, the reference {len(e['chunks'])} (room for {case.cap_log})"
            lg = np.stack([out["log"][c]["first"][:nl], out["log"][c]["count"][:nl]], axis=1)
            assert np.array_equal(lg, e["chunks"][:nl]), f"{w}: chunk list {lg[:8].tolist()} ..., the reference {e['chunks'][:8].tolist()} ..."
            assert out["log"][c][nl:].tobytes() == bytes([GUARD]) * (out["log"][c][nl:].nbytes), f"{w}: something was written behind the {nl} chunks"
            assert np.array_equal(cnt[c], e["counters"]), f"{w}: counters {cnt[c].tolist()}, the reference {e['counters'].tolist()}"
            bad = state_differences(e["state"], e["ring"], ws[c], k1, history_entries=shape is None)
            assert not bad, f"{w}: end state differs in {bad}: {ws[c]} != {e['state']}"
            if mode == 1:
                plan = stitch_plan(exp[c]["t_e"], exp[c]["t_clean"], k0, seglen, nseg, k1, out["spec"][c]["h"])
                assert (int(out["seg"][c, 0]), int(out["seg"][c, 1])) == (plan["adopted"], plan["walked"]), f"{w}: seg_stats {out['seg'][c].tolist()}, from the reference's trajectory {plan}"
                for k in PLAN_KEYS:
                    stats[k] += int(plan[k])
        stats["stitched_feeds"] += mode
        ctl = np.zeros((), OUTCTL); ctl["cap_bursts"] = nchan * case.cap_bursts_chan; ctl["cap_log"] = case.cap_log; ctl["overflow"] = over
        assert out["ctl"].tobytes() == ctl.tobytes(), f"{where}: control block {out['ctl']}, expected {ctl}"
        blob += [out["bursts"].tobytes(), out["nb"].tobytes(), out["log"].tobytes(), out["nlog"].tobytes(), out["ctl"].tobytes(), cnt.tobytes()] + [canonical_state(ws[c], k1) for c in range(nchan)]
    return b"".join(blob), stats


# ------------------------------------------------------------------------------------------------------------------------------
# streams synthesised at the decimated rate: D8PSK symbols, 10 samples each
# ------------------------------------------------------------------------------------------------------------------------------
FREQ = 136975000
STEPS_PER_PPM = 2 * np.pi * FREQ * 1e-6 / 10500           # carrier offset of 1 ppm in radians per symbol


def transmission_length(nsteps):
    return (5 + 16 + nsteps + 8) * K_SPS + 1                # synth.modulate(): ramp, unique word, payload, the pulse's tails


def synth_stream(n, txs, seed, noise=0.002, amp=0.1):
    """float32 [n, 2]: white noise plus the transmissions txs = (first sample, phase steps after the unique word, carrier offset in radians per
    symbol, start phase[, "rect"]), each synth.modulate() at 10 samples per symbol - or, with "rect", the unique word and the steps as
    rectangular symbols: the phase held for 10 samples, so that got_sync()'s metric stays low for several samples around every unique word"""
    rng = np.random.default_rng(seed)
    y = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for start, steps, cfo, ph0, *pulse in txs:
        if pulse:
            assert pulse == ["rect"]
            w = np.repeat(np.exp(1j * (ph0 + np.cumsum(np.concatenate([synth.PREAMBLE_STEPS, np.asarray(steps, dtype=np.int64)])) * (np.pi / 4))), K_SPS)
        else:
            w = synth.modulate(np.asarray(steps, dtype=np.int64), K_SPS, start_phase=ph0)
        assert start >= 0 and start + len(w) <= n, (start, len(w), n)
        y[start:start + len(w)] += amp * w * np.exp(1j * (cfo / K_SPS) * np.arange(len(w)))
    return np.stack([y.real, y.imag], axis=1).astype(F32)


_REFUSED_PAIRS = []


def header_steps(tl, rng, flips=0, refused=False):
    """the nine symbols of a header that says tl bits: 3 reserved bits, TL LSB first, 5 parity bits (decode.c:209-222), scrambled, and two
    bits of whatever follows; flips: that many of the 22 code bits inverted; refused: two code bits inverted whose syndrome the decoder
    takes for a pattern with a reserved bit in it - the corrected word has that bit set (decoder.crc.bad)"""
    rev = sum(1 << (16 - i) for i in range(17) if tl & (1 << i))
    word = rev << 5
    for i in range(5):
        if bin(word & synth.HDR_H[i] & ~0x1F).count("1") & 1:
            word |= 1 << (4 - i)
    if refused:
        if not _REFUSED_PAIRS:                   # (the code is linear: which error patterns are taken for one with a reserved bit does not depend on the word)
            pat = np.array([(1 << a) | (1 << b) for a in range(22) for b in range(a)], np.uint32)
            _REFUSED_PAIRS.extend(int(v) for v in pat[br.header_expected(pat ^ np.uint32(word))[:, 0] == 1])
        word ^= _REFUSED_PAIRS[int(rng.integers(len(_REFUSED_PAIRS)))]
        assert br.header_expected(np.array([word], np.uint32))[0, 0] == 1
    bits = np.array([(word >> (24 - i)) & 1 for i in range(25)], np.uint8)
    for p in rng.choice(np.arange(3, 25), size=flips, replace=False):
        bits[p] ^= 1
    bits = np.concatenate([bits ^ _PRBS25, rng.integers(0, 2, 2).astype(np.uint8)])
    tri = bits.reshape(-1, 3).astype(np.int64)
    return synth.GRAY_INV[tri[:, 0] * 4 + tri[:, 1] * 2 + tri[:, 2]]


def burst_steps(tl, rng):
    """a whole burst of tl random bits (header, data, FEC): it decodes to a descriptor, whatever the burst decoder makes of the bits"""
    return synth.build_burst([], raw_bits=rng.integers(0, 2, tl).astype(np.uint8)).symbols


def _layout(n, items, rng, first=400, gap=(40, 400)):
    """place transmissions one behind the other: items = (steps, cfo) -> txs"""
    txs = []; t = first
    for steps, cfo in items:
        ln = transmission_length(len(steps))
        if t + ln >= n:
            break
        txs.append((t, steps, cfo, float(rng.uniform(0, 2 * np.pi))))
        t += ln + int(rng.integers(*gap))
    return txs


def _bounded(bounds, most=40000):
    out = [0]
    for b in sorted(bounds):
        while b - out[-1] > most:
            out.append(out[-1] + most)
        out.append(b)
    return out


def _ends(case_y, freqs, max_ppm, c=0):
    """the reference's events on stream c fed whole: where the bursts end decides where some cases cut their feeds"""
    r = RefChannel(c, freqs[c], max_ppm, case_y[c])
    r.feed(0, len(case_y[c]))
    return r.events


def make_gate_storm():
    """Unique words back to back, 16 symbols apart, at 11 to 19 ppm under a gate of 5, as rectangular symbols (channel 4: shaped ones): every
    unique word is a cluster of got_sync() successes the gate drops, every drop shifts the evaluation grid and begins a chunk - some 200 chunks
    in 20 000 samples.  The speculative walks of a segment that long run out of their kSpecLog chunks (H.ok == 0: the segment is walked for
    real); with cap_log = 100 the feed's own log overflows."""
    ys = []
    for c in range(5):
        rng = np.random.default_rng(100 + c)
        steps = np.tile(synth.PREAMBLE_STEPS, 245 - 3 * c)
        off = (11 + 2 * c) * STEPS_PER_PPM * (1 if c % 2 == 0 else -1)
        ys.append(synth_stream(40600, [(300 + 7 * c, steps, off, float(rng.uniform(0, 6))) + (("rect",) if c < 4 else ())], seed=200 + c, noise=(0.002, 0.01, 0.03, 0.002, 0.002)[c]))
    return Case("gate_storm", [FREQ] * 5, 5.0, ys, [0, 40000, 40600])


def make_headers():
    """Refused headers of each kind (reserved bits set, too long, no FEC, whatever nine random symbols say) between short bursts whose headers
    are good, some with one bit corrected, 40 to 400 samples apart.  Feeds of 1, 2 and 3 samples and an empty one in the middle.  With
    cap_bursts_chan of 1 and 2 the feeds' burst lists overflow."""
    ys = []
    for c in range(5):
        rng = np.random.default_rng(300 + c)
        items = []
        for k in range(40):
            kind = (k + c) % 8
            junk = rng.integers(0, 8, 12)
            if kind in (0, 3, 6):
                st = burst_steps(int(rng.integers(24, 600)), rng)
            elif kind == 1:
                st = np.concatenate([header_steps(int(rng.integers(0x4000, 0x1FFFF)), rng), junk])               # too long
            elif kind == 2:
                st = np.concatenate([header_steps(int(rng.integers(1, 17)), rng), junk])                         # no FEC
            elif kind == 4:
                st = np.concatenate([header_steps(800, rng, refused=True), junk])             # reserved bits set
            elif kind == 5:
                tl = int(rng.integers(24, 300))
                st = burst_steps(tl, rng).copy(); st[:K_HDR_SYMS] = header_steps(tl, rng, flips=1)                  # one bit corrected
            else:
                st = rng.integers(0, 8, 30)
            items.append((st, float(rng.uniform(-2, 2)) * STEPS_PER_PPM))
        ys.append(synth_stream(40000, _layout(40000, items, rng), seed=400 + c))
    return Case("headers", [FREQ] * 5, 0.0, ys, [0, 13000, 13001, 13003, 13006, 13006, 27000, 40000])


def make_dense():
    """DM_INIT intervals shorter than the phase ring.  Rectangular symbols, one unbroken stream: a unique word, then again and again a locked
    stretch (nine symbols of a header that is refused, or a short burst) followed by 14 symbols that CONTINUE the unique word's last two
    symbols: the ring does not see the locked stretch, so 140 samples after the reset it holds a unique word - two symbols from before the
    stretch, 14 from after - and got_sync() fires.  Every such evaluation reads its taps through the interval history (seq_index), every sync
    takes prev_phi0 and the carrier slope from there, and the ring of a fresh interval reaches back over two or three earlier ones."""
    ps = synth.PREAMBLE_STEPS
    assert ps[15] == ps[1]                                   # symbols 14 -> 15 step like symbols 0 -> 1: why two symbols can be re-used
    ys = []
    for c in range(5):
        rng = np.random.default_rng(500 + c)
        steps = []
        for k in range(60):
            if (k + c) % 4 == 3:
                locked = burst_steps(int(rng.integers(24, 120)), rng)
            elif (k + c) % 4 == 1:
                locked = header_steps(int(rng.integers(0x4000, 0x1FFFF)), rng)
            elif (k + c) % 4 == 2:
                locked = header_steps(int(rng.integers(1, 17)), rng)
            else:
                locked = header_steps(int(rng.integers(24, 800)), rng, refused=True)
            steps += list(locked) + [int((ps[2] - locked.sum()) % 8)] + list(ps[3:])
        steps += list(rng.integers(0, 8, 20))
        n = 600 + transmission_length(len(steps))
        ys.append(synth_stream(n, [(300 + 3 * c, steps, float(rng.uniform(-1, 1)) * STEPS_PER_PPM, float(rng.uniform(0, 6)), "rect")], seed=600 + c, noise=0.003))
    n = min(len(v) for v in ys)
    return Case("dense", [FREQ] * 5, 0.0, ys, _bounded([n // 3, n // 3 + 77, 2 * n // 3, n]))


def make_burst_end():
    """Short bursts; channel 0's feeds end ON a burst's last symbol (end_sample = k_end - 1: the burst is delivered in this feed), one sample
    before it (end_sample = k_end) and two before (k_end + 1), inside a unique word, inside the nine header symbols, inside a burst's data,
    and 100 and 250 samples after a burst's end (inside the stretch whose evaluations read the ring through the history, and inside the 320
    samples after which the search counts as clean).  The other channels' bursts lie elsewhere: their feeds end wherever."""
    ys = []
    for c in range(5):
        rng = np.random.default_rng(700 + c)
        items = [(burst_steps(int(rng.integers(24, 900)), rng), float(rng.uniform(-2, 2)) * STEPS_PER_PPM) for _ in range(30)]
        ys.append(synth_stream(36000, _layout(36000, items, rng, first=200 + 130 * c, gap=(200, 900)), seed=800 + c))
    ev = [e for e in _ends(ys, [FREQ] * 5, 0.0) if e["accepted"] and e["hdr_status"] == 0 and e["end_sample"] > 0]
    assert len(ev) >= 9, len(ev)
    cut = [ev[0]["end_sample"] + 1, ev[1]["end_sample"], ev[2]["end_sample"] - 1, ev[3]["sample"] - 70, ev[4]["sample"] + 45, (ev[5]["sample"] + ev[5]["end_sample"]) // 2,
           ev[6]["end_sample"] + 100, ev[7]["end_sample"] + 250, ev[8]["end_sample"] + 2]
    return Case("burst_end", [FREQ] * 5, 0.0, ys, _bounded(cut + [36000]))


def make_silence():
    """Exact zeros (both signs), samples in the subnormal range, a step from silence into a burst and back: the phases of zeros are 0 or
    +-pi, got_sync()'s metric on them is a constant (nothing fires: it must RISE), and the subnormal samples have phases like any others"""
    ys = []
    for c in range(5):
        rng = np.random.default_rng(900 + c)
        items = [(burst_steps(int(rng.integers(24, 400)), rng), float(rng.uniform(-2, 2)) * STEPS_PER_PPM) for _ in range(8)]
        y = synth_stream(16000, _layout(16000, items, rng, first=5200 + 50 * c, gap=(300, 600)), seed=1000 + c)
        y[:1500] = 0.0; y[700:1500, c % 2] = -0.0
        y[1500:3000] = (rng.standard_normal((1500, 2)) * 1e-41).astype(F32)
        y[3000:4000] = (rng.standard_normal((1000, 2)) * 3e-39).astype(F32)
        y[4000:5000] *= F32(1e-30)
        k = 9000 + 100 * c
        y[k:k + 1200] = 0.0
        y[15000:] = 0.0
        ys.append(y)
    return Case("silence", [FREQ] * 5, 0.0, ys, [0, 1000, 2200, 3500, 9500, 16000])


def make_ring_wrap():
    """A ring of 4096 samples under short bursts: the ring wraps inside bursts (their header and first symbols are read from before the
    wrap), inside the 156 samples after a burst's end (the ring's entries from the interval before lie on the other side) and inside
    unique words.  Feeds of at most 2000 samples, so that what a feed reaches back to is still in the ring."""
    ys = []
    for c in range(5):
        rng = np.random.default_rng(1100 + c)
        txs = []
        for m in range(1, 7):
            st = burst_steps(int(rng.integers(24, 160)), rng)
            ln = transmission_length(len(st))
            # burst m straddles the wrap at 4096 m, its end a few samples before it, or its unique word on it
            start = 4096 * m - (ln // 2 if m % 3 == 1 else ln - 40 - 17 * c if m % 3 == 2 else 120 + 11 * c)
            txs.append((start, st, float(rng.uniform(-2, 2)) * STEPS_PER_PPM, float(rng.uniform(0, 6))))
        ys.append(synth_stream(27000, txs, seed=1200 + c))
    return Case("ring_wrap", [FREQ] * 5, 0.0, ys, _bounded([4090, 4100, 8150, 8200, 27000], most=1900), ring_len=4096)


def make_sweep():
    """2000 samples in one feed, a short burst in the middle: the case whose segment length is swept (SWEEP_SEGLEN), so that a segment
    boundary falls on every sample of the unique word, the header, the burst and the stretch after it"""
    ys = []
    for c in range(5):
        rng = np.random.default_rng(1300 + c)
        st = burst_steps(24 + 16 * c, rng)
        ys.append(synth_stream(2000, [(250 + 60 * c, st, float(rng.uniform(-2, 2)) * STEPS_PER_PPM, float(rng.uniform(0, 6)))], seed=1400 + c))
    return Case("sweep", [FREQ] * 5, 0.0, ys, [0, 2000])


SWEEP_SEGLEN = range(64, 464)


def make_trace_case(name, oracle_mod):
    """The oracle's own decimated streams of a small capture (its five busiest channels), cut where the reference's events say something is
    going on: inside a unique word, inside the nine header symbols, inside a burst, 100 and 250 samples after a burst's end; feeds of 1, 2
    and 3 samples and an empty one; the stream's first feed has taps before sample 0"""
    import cases
    cfg, iq, _, _ = cases.load(name)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
    D = iq.size // 2 // cfg.oversample
    tr = o.trace_all(D)
    o.trace_sync_events(4096)
    o.process(np.ascontiguousarray(iq).view(np.uint8).reshape(-1), block_bytes=1 << 24, nthreads=8)
    ev = [o.sync_events(c) for c in range(len(cfg.freqs))]
    score = [10 * min(int(e["accepted"].sum()), 3) + min(int((e["accepted"] == 0).sum()), 5) + len(e) / 1000 for e in ev]
    chans = sorted(np.argsort(score, kind="stable")[::-1][:5].tolist())
    chans = (chans * 5)[:5]                                 # (a capture of fewer than five channels: its channels again)
    ys = [tr[c].copy() for c in chans]
    freqs = [cfg.freqs[c] for c in chans]
    cut = []
    kinds = 0
    for c in sorted(set(chans)):
        for e in ev[c]:
            n, end = int(e["sample"]), int(e["end_sample"])
            if not e["accepted"]:
                cut.append(n - 40 if kinds % 2 else n + 2)
            elif end > 0:
                k = kinds % 6
                cut.append((n - 70, n + 45, (n + end) // 2, end + 100, end + 250, end + 1)[k])
                if k == 3:
                    cut += [cut[-1] + 1, cut[-1] + 3, cut[-1] + 6, cut[-1] + 6]
            kinds += 1
    cut = [k for k in cut if 0 < k < D]
    case = Case("cut_" + name, freqs, cfg.rx_max_ppm, ys, _bounded(cut + [D]))
    case.oracle_events = [o.sync_events(c).copy() for c in chans]
    case.oracle_counters = [list(o.counters(c).values()) for c in chans]
    case.oracle_evals = [o.sync_evals(c) for c in chans]
    return case


TRACE_CAPTURES = ("config2_1s", "dirty25k_1s", "os10_noisy_1s", "config4_0p4s")
def _variant(base, name, **room):
    """a case's streams and feeds again with other capacities: the reference's answers are the same ones"""
    b = get_case(base)
    c = Case(name, b.freqs, b.max_ppm, b.y, b.bounds, ring_len=b.ring_len, **room)
    c._exp = b._exp
    return c


SYNTH_CASES = {"gate_storm": make_gate_storm, "gate_storm_log100": lambda: _variant("gate_storm", "gate_storm_log100", cap_log=100), "headers": make_headers,
               "headers_cap1": lambda: _variant("headers", "headers_cap1", cap_bursts_chan=1), "headers_cap2": lambda: _variant("headers", "headers_cap2", cap_bursts_chan=2), "dense": make_dense,
               "burst_end": make_burst_end, "silence": make_silence, "ring_wrap": make_ring_wrap, "sweep": make_sweep}
CASE_NAMES = ["cut_" + n for n in TRACE_CAPTURES] + list(SYNTH_CASES)
_cases = {}


@ieee_subnormals()
def get_case(name, oracle_mod=None):
    if name not in _cases:
        _cases[name] = make_trace_case(name[4:], oracle_mod) if name.startswith("cut_") else SYNTH_CASES[name]()
    return _cases[name]


SHAPES = [None, ("segments", 2, 64), ("segments", 3, 64), ("segments", 5, 64), ("segments", 32, 64), ("segments", 32, 1000)]


def adoption_floors(fn, label):
    tot = dict.fromkeys(PLAN_KEYS, 0)
    for name in ("headers", "dense", "gate_storm"):
        for shape in (("segments", 2, 64), ("segments", 5, 64), ("segments", 32, 64)):
            st = run_case(fn, get_case(name), 5, shape, label)[1]
            for k in PLAN_KEYS:
                tot[k] += st[k]
    assert tot["adopted"] >= 500 and tot["walked"] >= 300 and tot["pre"] >= 100 and tot["pending"] >= 100 and tot["history"] >= 100, tot
    assert tot["refused_first"] >= 10 and tot["refused_overflow"] >= 4, tot
    assert tot["refused_chunk"] == 0, tot      # (Pinned: H.n_first >= st.e implies H.c_first.count > pre)
    return tot
