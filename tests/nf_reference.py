"""A plain reference of the noise floor (K4b: vdl2_core.h "Noise floor"), and the cases the host build (tests/test_nf_reference.py) and the
device build (tests/test_gpu_nf_probe.py, through vdl2hip_debug_nf_probe) are held to.  numpy only; nothing of vdl2_core.h is used here.

The reference program keeps, per channel, a low-passed magnitude and a noise floor (demod.c:238-243), in float32:

    mag    = hypot(re, im)                                        for every got_sync() evaluation
    mag_lp = mag_lp * 0.9f + mag * (1.0f - 0.9f)                  from mag_lp = 0 at the start of the stream
    mag_nf = 0.85f * mag_nf + (1.0f - 0.85f) * fminf(mag_lp, mag_nf) + 0.0001f      at every 1000th evaluation, from mag_nf = 2.0f

sequential() is exactly that, operation by operation.  windowed() is the definition the kernel states: mag_lp at an update is the same
recurrence started from 0 over the last kLpTerms = 256 evaluations the chunk list still reaches.  Both take one channel's ring `y`
([ring_len, 2] float32, ring_len a power of two; sample n is read at n & (ring_len - 1), as the kernel reads it) and the evaluated samples as
chunks [(first, count)], samples first, first + 3, ...

Where the two agree bit for bit - tests/test_nf_reference.py asserts it for every case below but the one whose tail is too short - the
kernel, held to windowed(), is held to the reference program.  They do NOT agree on every input, and the inputs below are chosen with that
in mind (none of this is a property of the kernel; it is float32):
  * 256 or more evaluations of exactly 0 after anything else: sequential() stalls a few subnormal steps above 0 (x * 0.9f rounds back to x
    for x below 5 * 2^-149), windowed() gives 0.  The same holds for a stretch in which mag_lp itself stays subnormal.  Exact zeros and
    subnormals therefore stand at the start of a stream, where mag_lp is 0 in both, or one by one among ordinary samples.
  * a step down by more than some 60 dB less than 256 evaluations before an update, or float32's largest magnitudes less than some 1050
    evaluations before the next update's window: what the window leaves out (0.9^256 = 2e-12 of the loud part) is then no longer far
    below half an ulp of what it holds.  The steps below are 40 dB, and the one sample near the top of the range is followed by 2300
    evaluations of a level of 1000.
A window of 256 evaluations touches at most 256 chunks; where the issue's list of chunk spans says 300, the span of a GROUP of updates
(two of them) is meant, which is what the kernel stages."""
import contextlib
import ctypes as C
import ctypes.util

import numpy as np

LP_TERMS = 256           # kLpTerms
NF_TAIL = 64             # kNfTail
NF_SLICE = 191           # kNfSlice: chunks of the list a group of updates stages
RING_LEN = 4096          # the y ring of every case
F32 = np.float32
I64 = np.int64

C9 = F32(0.9)
C1 = F32(1.0) - F32(0.9)
C85 = F32(0.85)
C15 = F32(1.0) - F32(0.85)
CADD = F32(0.0001)

CHUNK = np.dtype([("first", "<i8"), ("count", "<i8")])
NFSTATE = np.dtype([("mag_nf", "<f4"), ("ntail", "<i4"), ("evals", "<i8"), ("tail_ord", "<i8"), ("tail", CHUNK, (NF_TAIL,))])
NFFEED = np.dtype([("ev0", "<i8"), ("ev1", "<i8"), ("u0", "<i8"), ("u1", "<i8"), ("begin_ord", "<i8"), ("ncomb", "<u4"), ("pad_", "<u4")])
GUARD_F32 = np.frombuffer(b"\xa5\xa5\xa5\xa5", "<f4")[0]
RING_FILL = F32(-7777.0)                 # what a history-ring entry holds before anything has written it


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def ieee_subnormals():
    """The arithmetic below must keep subnormals.  A process that has loaded a library built with -ffast-math (the oracle's "fast" flavour,
    tests/test_golden_fixtures.py) runs with flush-to-zero set in the thread's floating-point environment, numpy included: inside this
    block the default environment holds, and the thread's own comes back afterwards.  This is glibc's: FE_DFL_ENV is (fenv_t *) -1 there and
    256 octets hold its fenv_t with room to spare.  Elsewhere the call may do nothing - then the check below fails, as it does wherever
    subnormals still do not survive."""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    env = C.create_string_buffer(256)
    libm.fegetenv.argtypes = [C.c_void_p]; libm.fesetenv.argtypes = [C.c_void_p]
    assert libm.fegetenv(env) == 0
    try:
        assert libm.fesetenv(C.c_void_p(-1)) == 0                         # FE_DFL_ENV
        t = np.array([1e-40, 0.5], F32)
        assert (t[:1] * t[1:])[0] > 0 and float(t[0]) > 0, "subnormals are flushed: the reference cannot be computed here"
        yield
    finally:
        libm.fesetenv(env)


def positions(chunks):
    """sample numbers of the evaluations, in order"""
    ch = np.asarray(chunks, I64).reshape(-1, 2)
    if len(ch) == 0:
        return np.zeros(0, I64)
    cnt = ch[:, 1]
    start = np.cumsum(cnt) - cnt
    idx = np.arange(int(cnt.sum()), dtype=I64)
    which = np.repeat(np.arange(len(ch)), cnt)
    return ch[which, 0] + 3 * (idx - start[which])


def magnitudes(y, chunks):
    """mag of every evaluation: float32(hypot(double re, double im))"""
    y = np.asarray(y, F32)
    p = positions(chunks) & (len(y) - 1)
    with ieee_subnormals():
        return np.hypot(y[p, 0].astype(np.float64), y[p, 1].astype(np.float64)).astype(F32)


def nf_chain(lp, nf0=F32(2.0)):
    """mag_nf after each update, from mag_lp at each update"""
    out = np.zeros(len(lp), F32)
    nf = F32(nf0)
    with ieee_subnormals(), np.errstate(over="ignore"):
        for i, v in enumerate(lp):
            nf = C85 * nf + C15 * (v if v < nf else nf) + CADD
            out[i] = nf
    return out


def sequential(y, chunks):
    """(mag_lp at each update, mag_nf after each update): the reference program's own arithmetic, one evaluation after the other"""
    mags = magnitudes(y, chunks)
    nupd = len(mags) // 1000
    lps = np.zeros(nupd, F32)
    lp = F32(0.0)
    ml = list(mags[:1000 * nupd])
    with ieee_subnormals(), np.errstate(over="ignore", under="ignore"):
        for u in range(nupd):
            for m in ml[1000 * u:1000 * u + 1000]:
                lp = lp * C9 + m * C1
            lps[u] = lp
    return lps, nf_chain(lps)


def windowed(y, chunks, reach=None):
    """the same from 0 over the last LP_TERMS evaluations before (and with) the one that triggers the update.  reach: per update, the
    ordinal of the oldest evaluation the chunk list still holds (None: everything)"""
    mags = magnitudes(y, chunks)
    nupd = len(mags) // 1000
    o = 1000 * np.arange(1, nupd + 1, dtype=I64) - 1
    lo = np.maximum(o - (LP_TERMS - 1), 0)
    if reach is not None:
        lo = np.maximum(lo, np.asarray(reach, I64)[:nupd])
    lp = np.zeros(nupd, F32)
    with ieee_subnormals(), np.errstate(over="ignore", under="ignore"):
        for t in range(LP_TERMS - 1, -1, -1):
            i = o - t
            ok = i >= lo
            m = mags[np.where(ok, i, 0)] if nupd else mags[:0]
            lp = np.where(ok, lp * C9 + m * C1, lp).astype(F32)
    return lp, nf_chain(lp)


def same_bits(a, b):
    return np.asarray(a, F32).view(np.uint32) == np.asarray(b, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------
# the state a channel carries from feed to feed, stated plainly: the newest chunks, at most NF_TAIL of them, as many as it takes to
# hold LP_TERMS evaluations; a feed whose first evaluation continues the last remembered chunk lengthens that chunk
# ------------------------------------------------------------------------------------------------------------------------------
class TailModel:
    def __init__(self):
        self.tail = []                      # [(first, count)]
        self.tail_ord = 0
        self.evals = 0

    def feed(self, chunks):
        """-> the record of this feed (ev0, ev1, u0, u1, begin_ord, ncomb)"""
        new = [(int(f), int(c)) for f, c in chunks]
        comb = list(self.tail)
        if comb and new and new[0][0] == comb[-1][0] + 3 * comb[-1][1]:    # the feed goes on where the one before stopped: one chunk
            comb[-1] = (comb[-1][0], comb[-1][1] + new[0][1]); new = new[1:]
        comb += new
        ev0 = self.evals
        begin = self.tail_ord if comb else ev0
        ev1 = begin + sum(c for _, c in comb)
        rec = dict(ev0=ev0, ev1=ev1, u0=ev0 // 1000, u1=ev1 // 1000, begin_ord=begin, ncomb=len(comb))
        keep, held = 0, 0
        while keep < len(comb) and keep < NF_TAIL and held < LP_TERMS:
            keep += 1
            held += comb[-keep][1]
        self.tail = comb[len(comb) - keep:]
        self.tail_ord = ev1 - held
        self.evals = ev1
        return rec


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name; y [nchan, RING_LEN, 2]; feeds[f][c] = int64 [n, 2] chunks of channel c in feed f; cap_log, cap_hist, nf_ring; short_tail: the
    remembered tail is meant to hold fewer than LP_TERMS evaluations somewhere (windowed() != sequential() is expected there)"""

    def __init__(self, name, y, feeds, cap_log=512, cap_hist=80, nf_ring=128, short_tail=False):
        self.name, self.y, self.feeds, self.cap_log, self.cap_hist, self.nf_ring, self.short_tail = name, np.ascontiguousarray(y, F32), feeds, cap_log, cap_hist, nf_ring, short_tail
        self.nchan = len(self.y)
        self._exp = {}

    def all_chunks(self, c):
        parts = [np.asarray(f[c], I64).reshape(-1, 2) for f in self.feeds]
        return np.concatenate(parts) if parts else np.zeros((0, 2), I64)

    def expected(self, c):
        """per channel, once: feed records, reach per update, windowed (what both builds are held to), and the remembered tails"""
        if c not in self._exp:
            tm = TailModel()
            recs, tails = [], []
            for f in self.feeds:
                recs.append(tm.feed(np.asarray(f[c], I64).reshape(-1, 2)))
                tails.append((list(tm.tail), tm.tail_ord))
            nupd = tm.evals // 1000
            reach = np.zeros(nupd, I64)
            for r in recs:
                reach[r["u0"]:r["u1"]] = r["begin_ord"]
            lp, nf = windowed(self.y[c], self.all_chunks(c), reach)
            lp.setflags(write=False); nf.setflags(write=False)
            self._exp[c] = dict(recs=recs, tails=tails, reach=reach, lp=lp, nf=nf)
        return self._exp[c]


def _noise(rng, kind):
    """a ring of one of the three kinds of magnitudes the definition was first tried on"""
    z = rng.uniform(-1.0, 1.0, (RING_LEN, 2))
    if kind == "small":
        z *= 1e-3
    elif kind == "bursty":                                 # loud and quiet stretches 40 dB apart
        lvl = np.where((np.arange(RING_LEN) // 300) % 3 == 0, 1.0, 0.01)
        z *= lvl[:, None]
    elif kind == "gauss":
        z = rng.normal(0.0, 0.2, (RING_LEN, 2))
    return z.astype(F32)


_KINDS = ["uniform", "small", "bursty", "gauss", "uniform"]


def _rings(rng):
    return np.stack([_noise(rng, k) for k in _KINDS])


def chunks_from_counts(counts, rng, start=None, gap_max=5000):
    """chunks of the given lengths, one behind the other with the gaps a shift of the evaluation grid leaves (any number of samples)"""
    out = np.zeros((len(counts), 2), I64)
    p = int(rng.integers(0, 1 << 20)) if start is None else int(start)
    for i, n in enumerate(counts):
        out[i] = (p, n)
        p += 3 * int(n) + int(rng.integers(1, gap_max + 1))
        if rng.integers(0, 4) == 0:
            p += 1                                           # (never a multiple of 3 for long: the grid really shifts)
    return out, p


def _split_total(total, rng, lo=1, hi=5000):
    """random lengths lo..hi that add up to total"""
    out = []
    while total > 0:
        n = int(min(total, rng.integers(lo, hi + 1)))
        out.append(n); total -= n
    return out


def _storm(total, rng, hi=5):
    """lengths 1..hi adding up to total"""
    return _split_total(total, rng, 1, hi)


class _Chan:
    """builds one channel's feeds while keeping count of its evaluations"""

    def __init__(self, rng):
        self.rng, self.evals, self.pos, self.feeds, self.cur = rng, 0, int(rng.integers(0, 1 << 20)), [], []

    def add(self, counts, gap_max=5000):
        ch, self.pos = chunks_from_counts(counts, self.rng, self.pos, gap_max)
        self.cur.append(ch); self.evals += int(sum(counts))

    def to(self, total, **kw):
        """one chunk up to `total` evaluations in all"""
        assert total > self.evals
        self.add([total - self.evals], **kw)

    def end_feed(self):
        self.feeds.append(np.concatenate(self.cur) if self.cur else np.zeros((0, 2), I64)); self.cur = []


def _assemble(name, y, chans, **kw):
    nf = max(len(c.feeds) for c in chans)
    for c in chans:
        while len(c.feeds) < nf:
            c.end_feed()                                     # (a channel with fewer feeds idles: no evaluations, the tail is kept)
    return Case(name, y, [[c.feeds[f] for c in chans] for f in range(nf)], **kw)


def case_boundaries(seed=1):
    """one long chunk per feed; the feeds end one evaluation before, at, and one behind an update.  With them: the first feed of a stream, feeds
    without an update, feeds without evaluations"""
    rng = np.random.default_rng(seed)
    targets = [[999, 1000, 1001, 2999, None, 4000, 6001, 6002, 9000],
               [1000, 1999, 2001, None, 5000, 5999, 6000, 6001, 8999],
               [1001, 3000, 3999, 4000, 4001, None, 4500, 7000, 9001],
               [None, 1, 2, 999, 1000, 1256, 2000, 2255, 3000],
               [5, None, 260, 1000, None, 2000, 2001, 32999, 33000]]
    chans = []
    for t in targets:
        ch = _Chan(rng)
        for x in t:
            if x is not None:
                ch.to(x)
            ch.end_feed()
        chans.append(ch)
    return _assemble("boundaries", _rings(rng), chans)


def case_groups(seed=2):
    """feeds of 31, 32, 33, 64 and 65 updates, each channel in an order of its own and from a count of its own"""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        ch.add([int(rng.integers(1, 999))]); ch.end_feed()
        order = np.roll([31, 32, 33, 64, 65], c)
        for n in order:
            tgt = (ch.evals // 1000 + int(n)) * 1000 + int(rng.choice([0, 0, 1, 500, 999]))
            ch.add(_split_total(tgt - ch.evals, rng, 200, 20000)); ch.end_feed()
        chans.append(ch)
    return _assemble("groups", _rings(rng), chans, cap_hist=66, nf_ring=128)


def case_batch(seed=3):
    """pass 3's batch of 2048: 2047, 2048 and 2049 updates in one feed (cap_hist is the largest of them + 1)"""
    rng = np.random.default_rng(seed)
    chans = []
    for n, pre in [(2047, 0), (2048, 700), (2049, 999), (33, 1500), (1, 0)]:
        ch = _Chan(rng)
        if pre:
            ch.add([pre])
        ch.end_feed()
        ch.add(_split_total((ch.evals // 1000 + n) * 1000 + int(rng.integers(0, 999)) - ch.evals, rng, 20000, 400000)); ch.end_feed()
        ch.add([1500]); ch.end_feed()
        chans.append(ch)
    return _assemble("batch", _rings(rng), chans, cap_hist=2050, nf_ring=4096)


def case_random_chunks(seed=4):
    """chunk lengths 1 to 5000 with the gaps a grid shift leaves"""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        for f in range(4):
            ch.add([int(x) for x in rng.integers(1, 5001, int(rng.integers(5, 30)))]); ch.end_feed()
        chans.append(ch)
    return _assemble("random_chunks", _rings(rng), chans, cap_hist=128, nf_ring=128)


def _span_feed(ch, nspan, rng, follow):
    """a feed with one update whose 256 evaluations touch exactly nspan chunks: the end of a long one, nspan - 2 of 1 to 5 evaluations, and
    the one the trigger lies in.  follow: chunks behind it (none: the list, and with it the staged slice, ends with the trigger's chunk)"""
    small = [1] * (nspan - 2)
    for _ in range(max(250 - len(small), 0)):
        i = int(rng.integers(0, max(len(small), 1)))
        if small and small[i] < 5 and rng.integers(0, 2):
            small[i] += 1
    S = sum(small)
    j = int(rng.integers(0, 254 - S + 1))                    # evaluations of the trigger's chunk before the trigger
    o = (ch.evals // 1000 + 1) * 1000 - 1                     # the trigger's ordinal (the next update but one where the next is too near)
    if o - S - j - ch.evals < 1:
        o += 1000
    ch.add([o - S - j - ch.evals] + small + [j + 1 + (int(rng.integers(0, 4)) if follow else 0)], gap_max=40)
    if follow:
        ch.add(_storm(int(rng.integers(30, 200)), rng), gap_max=40)
        ch.add([int(rng.integers(300, 600))])
    assert (ch.evals // 1000) * 1000 - 1 == o
    ch.end_feed()


def case_storms(seed=5):
    """storms of chunks of 1 to 5 evaluations: one update's window over 2, 64, 190, 191, 192 and 256 chunks (the staged slice of 191 just not
    full, full, and one short: the list in memory), with chunks behind the trigger and with the list ending there; then groups of two
    updates over 300 and more chunks, and whole feeds of nothing else"""
    rng = np.random.default_rng(seed)
    spans = [[2, 190, 191, 192, 64, 256], [191, 192, 2, 64, 256, 190], [192, 191, 190, 256, 2, 64], [64, 256, 192, 191, 190, 2], [190, 64, 191, 2, 192, 256]]
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        for k, n in enumerate(spans[c]):
            _span_feed(ch, n, rng, follow=(k + c) % 2 == 0 and n != NF_SLICE)      # a full slice that ends with the list, in every channel ...
        _span_feed(ch, NF_SLICE, rng, follow=True)                              # ... and one with chunks behind it
        # a group of two updates whose span (1256 evaluations) is 300 chunks and more
        tgt = (ch.evals // 1000 + 2) * 1000 + 3
        lead = tgt - 1300 - ch.evals
        if lead > 0:
            ch.add([lead])
        ch.add(_storm(tgt - ch.evals, rng), gap_max=40); ch.end_feed()
        # a feed of 3 updates of nothing but storm, and its successor starting inside the tail
        ch.add(_storm(3000 + int(rng.integers(0, 900)), rng), gap_max=40)
        ch.add([300]); ch.end_feed()
        ch.add([2000]); ch.end_feed()
        chans.append(ch)
    return _assemble("storms", _rings(rng), chans, cap_log=2048)


def case_tail_cross(seed=6):
    """windows that reach back across one and across two feed boundaries through the remembered tail, and a tail of exactly 64 chunks that
    still holds 256 evaluations"""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        # across one boundary: the feed ends 1 .. 255 evaluations before the update
        ch.to(3000 - [1, 100, 255, 17, 200][c]); ch.end_feed()
        ch.to(3000 + c); ch.end_feed()
        # across two: a feed of a few evaluations in between
        ch.to(6000 - 180); ch.end_feed()
        ch.add([20 + c, 30]); ch.end_feed()
        ch.to(6000 + 40 * c); ch.end_feed()
        # 64 chunks of 4 evaluations end the feed: all of them are kept, and the next feed's first update needs every one
        ch.to(9000 - 256 - 1 - c)
        ch.add([4] * 64, gap_max=40); ch.end_feed()
        ch.add([1 + c, 700]); ch.end_feed()
        # 63 chunks of 4 and one of 5: 257 evaluations in 64 chunks
        ch.to(12000 - 257 - 2)
        ch.add([5] + [4] * 63, gap_max=40); ch.end_feed()
        ch.add([2, 1, 900]); ch.end_feed()
        # an empty feed between the tail and its use
        ch.to(15000 - 60); ch.end_feed()
        ch.end_feed()
        ch.to(15000 + 500); ch.end_feed()
        chans.append(ch)
    return _assemble("tail_cross", _rings(rng), chans)


def case_tail_short(seed=7):
    """more than 64 chunks of at most 3 evaluations end a feed: the remembered 64 hold fewer than 256 evaluations, and the next feed's first
    update replays fewer than 256"""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        ch.to(2000 - 400)
        ch.add(_split_total(400 - 1 - 3 * c, rng, 1, 3), gap_max=40); ch.end_feed()
        ch.add([1 + 3 * c + int(rng.integers(1, 30)), 800]); ch.end_feed()
        ch.to(5000 - 300)
        ch.add([1 + c % 3] * 90, gap_max=40); ch.end_feed()
        ch.to(5000 + 10); ch.end_feed()
        chans.append(ch)
    return _assemble("tail_short", _rings(rng), chans, short_tail=True)


def case_ring_wraps(seed=8):
    """the y ring wraps inside a window (the trigger a few samples behind a multiple of the ring's length), and the history ring of 64 entries
    wraps several times over the run"""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        for f in range(14):
            nu = int(rng.integers(1, 32))
            o = (ch.evals // 1000 + nu) * 1000 - 1             # the feed's last trigger: at sample k * RING_LEN + a little
            lead = int(rng.integers(1, 400))
            ch.add([lead])
            n = o - ch.evals + 1 + int(rng.integers(0, 700))
            first = RING_LEN * int(rng.integers(1, 1000)) + int(rng.integers(0, 300)) - 3 * (o - ch.evals)
            if first < 0:
                first += RING_LEN * (-first // RING_LEN + 1)
            ch.cur.append(np.array([[first, n]], I64)); ch.evals += n; ch.pos = first + 3 * n + 7
            ch.end_feed()
        chans.append(ch)
    return _assemble("ring_wraps", _rings(rng), chans, cap_hist=33, nf_ring=64)


def case_tiny_feeds(seed=11):
    """feeds of a few samples: 70 to 200 feeds in a row of 0 to 3 evaluations each, every one continuing the grid of the one before, then an
    update.  A feed's log begins a chunk of its own; were those kept apart, the 64 remembered chunks would hold 64 to 192 evaluations.
    Among them a grid shift inside the run (a chunk that does NOT continue), and a run that follows a storm"""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        for rnd in range(3):
            nfeeds = [70, 130, 200, 65, 90][(c + rnd) % 5]
            counts = [int(rng.integers(0, 4)) if c != 1 else 1 for _ in range(nfeeds)]      # channel 1: one evaluation per feed
            tgt = (ch.evals // 1000 + 1) * 1000 - 1 - sum(counts) + int(rng.integers(1, 40))  # the trigger lies in the run's last feeds
            if tgt - ch.evals < 1:
                tgt += 1000
            if rnd == 1:
                ch.add(_storm(tgt - ch.evals, rng), gap_max=40)
            else:
                ch.to(tgt)
            ch.end_feed()
            pos = int(ch.cur[-1][-1, 0] + 3 * ch.cur[-1][-1, 1]) if ch.cur else int(ch.feeds[-1][-1, 0] + 3 * ch.feeds[-1][-1, 1])
            for i, n in enumerate(counts):
                if rnd == 2 and i == nfeeds // 2:
                    pos += 5                                   # the grid shifts once
                if n:
                    ch.cur.append(np.array([[pos, n]], I64)); ch.evals += n; pos += 3 * n
                ch.end_feed()
            ch.pos = pos + 11
            ch.add([400]); ch.end_feed()
        chans.append(ch)
    return _assemble("tiny_feeds", _rings(rng), chans)


TOP = F32(3.0e38)


def _level_settling_at(target):
    """the constant magnitude at which mag_lp settles on `target` exactly (the recurrence's rounding leaves it a few ulps off the level)"""
    m = F32(target)
    for _ in range(64):
        lp = F32(0.0)
        for _ in range(600):
            lp = lp * C9 + m * C1
        if lp == target:
            return m
        m = np.nextafter(m, F32(np.inf) if lp < target else F32(-np.inf))
    raise AssertionError("no level settles there")


def case_magnitudes(seed=9):
    """exact zeros, subnormals, one sample near the top of float32's range, steps of 40 dB from loud to silent (fminf takes either side), and
    mag_lp == mag_nf.  Every channel's ring is cut into 8 regions of 512 samples; a chunk stays inside one region (170 evaluations at most)"""
    rng = np.random.default_rng(seed)
    R = 512
    per = R // 3                                             # evaluations of a chunk that starts with its region

    def ring():
        y = np.zeros((RING_LEN, 2), np.float64)
        y[1 * R:2 * R] = rng.uniform(-1, 1, (R, 2)) * 1e-40                      # subnormal
        y[2 * R:3 * R] = rng.uniform(-1, 1, (R, 2)) * 1e3
        y[3 * R:4 * R] = rng.uniform(-1, 1, (R, 2)) * 10
        y[4 * R:5 * R] = rng.uniform(-1, 1, (R, 2)) * 0.1
        y[5 * R:6 * R] = rng.uniform(-1, 1, (R, 2)) * 1e-3
        y[5 * R + 9:6 * R:37] = 0.0                                            # exact zeros and subnormals one by one among them
        y[5 * R + 20:6 * R:41] = rng.uniform(-1, 1, (len(range(5 * R + 20, 6 * R, 41)), 2)) * 1e-41
        y[6 * R:7 * R] = (_level_settling_at(F32(2.0)), 0.0)
        y[7 * R:8 * R] = rng.uniform(-1, 1, (R, 2)) * 0.5
        with ieee_subnormals():
            y = y.astype(F32)
        y[7 * R + 100] = (TOP, F32(-1.5e30))                                   # read by one chunk of one evaluation only (never at a chunk's stride from a region's start)
        return y

    def stay(ch, region, n):
        """n evaluations inside a region, in chunks that start with it"""
        while n > 0:
            k = min(n, per if region != 7 else 33)            # (region 7: short of the top sample)
            ch.cur.append(np.array([[region * R + RING_LEN * int(rng.integers(0, 50)), k]], I64)); ch.evals += k; n -= k

    ys, chans = [], []
    for c in range(5):
        ch = _Chan(rng)
        if c == 4:                                            # mag_lp == mag_nf: a level of 2.0 from the first evaluation on
            stay(ch, 6, 2500); ch.end_feed()
            stay(ch, 5, 2500); ch.end_feed()
        else:
            stay(ch, 0, 744 + 10 * c); stay(ch, 1, 256 - 10 * c)      # update 1: zeros, then subnormals - mag_lp is subnormal
            if c % 2:
                ch.end_feed()
            stay(ch, 2, 1980 - 7 * c)
            ch.cur.append(np.array([[7 * R + 100 + RING_LEN * 3, 1]], I64)); ch.evals += 1     # the sample near the top, 19 evaluations before update 3
            stay(ch, 2, 2300 + 7 * c); ch.end_feed()
            for region, n in [(3, 1000), (4, 1000 + 50 * c), (5, 3000), (7, 1200), (5, 2000 - 50 * c), (2, 900), (5, 1100)]:
                stay(ch, region, n)
                if region != 4:
                    ch.end_feed()
        ys.append(ring()); chans.append(ch)
    return _assemble("magnitudes", np.stack(ys), chans, cap_log=512)


def case_random_run(seed=10):
    """40 random feeds over all of the above, the state carried from feed to feed; the history ring of 64 wraps"""
    rng = np.random.default_rng(seed)
    chans = []
    for c in range(5):
        ch = _Chan(rng)
        for f in range(40):
            kind = int(rng.integers(0, 8))
            if kind == 0:
                pass                                            # no evaluations
            elif kind == 1:
                ch.add([int(rng.integers(1, 999))])
            elif kind == 2:
                ch.to((ch.evals // 1000 + int(rng.integers(1, 34))) * 1000 + int(rng.choice([-1, 0, 1])))
            elif kind == 3:
                ch.add([int(x) for x in rng.integers(1, 5001, int(rng.integers(1, 12)))])
            elif kind == 4:
                ch.add(_storm(int(rng.integers(100, 2500)), rng), gap_max=40); ch.add([int(rng.integers(256, 900))])
            elif kind == 5:
                ch.add([int(rng.integers(1, 300))] * int(rng.integers(1, 60)), gap_max=400); ch.add([int(rng.integers(256, 600))])
            elif kind == 6:
                ch.add([4] * 64, gap_max=40)                  # a tail of 64 chunks that just holds 256
            else:
                ch.add(_split_total(int(rng.integers(1000, 40000)), rng, 1, 5000))
            ch.end_feed()
        chans.append(ch)
    return _assemble("random_run", _rings(rng), chans, cap_log=1024, cap_hist=48, nf_ring=64)


CASE_MAKERS = [case_boundaries, case_groups, case_batch, case_random_chunks, case_storms, case_tail_cross, case_tail_short, case_ring_wraps, case_magnitudes, case_random_run, case_tiny_feeds]
_CASES = {}


def get_case(name):
    """every case is built once per process, and its expectations with it"""
    if name not in _CASES:
        mk = {m.__name__[5:]: m for m in CASE_MAKERS}[name]
        _CASES[name] = mk()
    return _CASES[name]


CASE_NAMES = [m.__name__[5:] for m in CASE_MAKERS]


# ------------------------------------------------------------------------------------------------------------------------------
# a build under test: run(nchan, y, chunks [nchan, cap_log] CHUNK, nlog, cap_log, nf NFSTATE [nchan], ring [nchan, nf_ring], nf_ring, cap_hist)
#   -> (lpbuf [nchan, cap_hist], feeds NFFEED [nchan]); nf and ring are updated in place
# ------------------------------------------------------------------------------------------------------------------------------
_DEV_ARGS = [C.c_int, C.c_uint, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]


def device_runner(L, mode, grid):
    assert L.vdl2hip_debug_sizeof_nfstate() == NFSTATE.itemsize and L.vdl2hip_debug_sizeof_nffeed() == NFFEED.itemsize
    L.vdl2hip_debug_nf_probe.argtypes = _DEV_ARGS

    def run(nchan, y, chunks, nlog, cap_log, nf, ring, nf_ring, cap_hist):
        lp = np.zeros((nchan, cap_hist), F32); fd = np.zeros(nchan, NFFEED)
        rc = L.vdl2hip_debug_nf_probe(mode, grid, nchan, y.ctypes.data, y.shape[1], chunks.ctypes.data, nlog.ctypes.data, cap_log, nf.ctypes.data, ring.ctypes.data, nf_ring, cap_hist,
                                      lp.ctypes.data, fd.ctypes.data)
        assert rc == 0, f"vdl2hip_debug_nf_probe(mode {mode}, grid {grid}) = {rc}"
        return lp, fd
    return run


def host_runner(H):
    import pyhostsim
    assert H.hostsim_sizeof_nfstate() == NFSTATE.itemsize and H.hostsim_sizeof_nffeed() == NFFEED.itemsize

    def run(nchan, y, chunks, nlog, cap_log, nf, ring, nf_ring, cap_hist):
        lp = np.zeros((nchan, cap_hist), F32); fd = np.zeros(nchan, NFFEED)
        with ieee_subnormals():                                  # (the host build runs in this thread's floating-point environment)
            rc = pyhostsim.nf_feed(H, nchan, y, chunks, nlog, cap_log, nf, ring, nf_ring, cap_hist, lp, fd)
        assert rc == 0, f"hostsim_nf_feed = {rc}"
        return lp, fd
    return run


def initial_state(nchan):
    nf = np.zeros(nchan, NFSTATE)
    nf["mag_nf"] = 2.0
    return nf


def run_case(run, case, nchan, label):
    """the case's feeds through a build, everything compared after every feed.  Returns every byte the build gave back (for comparing two
    builds or two launch shapes with each other) and the number of values compared"""
    y = np.ascontiguousarray(case.y[:nchan])
    nf = initial_state(nchan)
    ring = np.full((nchan, case.nf_ring), RING_FILL, F32)
    ring_exp = ring.copy()
    mask = case.nf_ring - 1
    exps = [case.expected(c) for c in range(nchan)]
    blob, ncmp = [], 0
    for f, feed in enumerate(case.feeds):
        chunks = np.zeros((nchan, case.cap_log), CHUNK); nlog = np.zeros(nchan, np.uint32)
        for c in range(nchan):
            ch = np.asarray(feed[c], I64).reshape(-1, 2)
            assert len(ch) <= case.cap_log
            chunks["first"][c, :len(ch)] = ch[:, 0]; chunks["count"][c, :len(ch)] = ch[:, 1]; nlog[c] = len(ch)
        lp, fd = run(nchan, y, chunks, nlog, case.cap_log, nf, ring, case.nf_ring, case.cap_hist)
        blob += [lp.tobytes(), fd.tobytes(), nf.tobytes(), ring.tobytes()]
        for c in range(nchan):
            e = exps[c]; r = e["recs"][f]; where = f"{label} {case.name} feed {f} channel {c}"
            got = {k: int(fd[c][k]) for k in ("ev0", "ev1", "u0", "u1", "begin_ord", "ncomb")}
            assert got == r, f"{where}: feed record {got}, expected {r}"
            u0, u1 = r["u0"], r["u1"]
            n = u1 - u0
            assert n + 1 <= case.cap_hist
            bad = np.flatnonzero(~same_bits(lp[c, 1:n + 1], e["lp"][u0:u1]))
            assert bad.size == 0, (f"{where}: mag_lp of {bad.size} of {n} updates differs, first update {u0 + 1 + bad[0]} (the {bad[0] + 1}th of the feed): "
                                   f"{lp[c, 1 + bad[0]]!r} against {e['lp'][u0 + bad[0]]!r}")
            assert same_bits(lp[c, 0], GUARD_F32) and same_bits(lp[c, n + 1:], GUARD_F32).all(), f"{where}: lpbuf written outside entries 1 .. {n}"
            ring_exp[c, u0 & mask] = e["nf"][u0 - 1] if u0 > 0 else F32(2.0)
            for u in range(u0 + 1, u1 + 1):
                ring_exp[c, u & mask] = e["nf"][u - 1]
            bad = np.flatnonzero(~same_bits(ring[c], ring_exp[c]))
            assert bad.size == 0, f"{where}: history ring entry {bad[0]} is {ring[c, bad[0]]!r}, expected {ring_exp[c, bad[0]]!r} ({bad.size} entries differ; updates {u0} .. {u1})"
            nf_exp = e["nf"][u1 - 1] if u1 > 0 else F32(2.0)
            assert same_bits(nf[c]["mag_nf"], nf_exp), f"{where}: NfState.mag_nf {nf[c]['mag_nf']!r}, expected {nf_exp!r}"
            assert int(nf[c]["evals"]) == r["ev1"], f"{where}: NfState.evals {int(nf[c]['evals'])}, expected {r['ev1']}"
            tail, tail_ord = e["tails"][f]
            got_tail = [(int(t["first"]), int(t["count"])) for t in nf[c]["tail"][:int(nf[c]["ntail"])]]
            assert (got_tail, int(nf[c]["tail_ord"])) == (tail, tail_ord), f"{where}: remembered tail of {len(got_tail)} chunks from ordinal {int(nf[c]['tail_ord'])}, expected {len(tail)} from {tail_ord}"
            ncmp += 2 * n + 3
    return b"".join(blob), ncmp
