"""K1's own output - the decimated stream with the referee off - against the channel filter in double precision
(tests/k1_reference.py), over every build of k_chanfir the library dispatches, every feed geometry, both look-back paths and the
edges of the sample formats.  The bound of a cell is derived in the cell from the float32 model of K1's recurrence on the same
input (max error <= 4 x the model's, rms <= 2 x: k1_reference.FACTOR_MAX / FACTOR_RMS say why), in units of the wideband input's
peak; tests/test_k1_reference.py shows on the CPU what that bound passes and what it fails.  Every checked channel is compared over
the whole stream the ring still holds.  K1_STREAM_MATRIX=<file> in the environment appends one row per cell (model, kernel,
ratio): profiles/k1_stream_matrix.txt is such a run."""
import os
import time
import types

import numpy as np
import pytest

import k1_reference as k1

pytestmark = pytest.mark.gpu
S16, U8 = 1, 0
FMT = {"s16": S16, "u8": U8}
D_SMALL = 30000                     # outputs per channel of a small cell: 235 tiles, as many segments
RUNUP64 = 2048                      # blocks of run-up where the reference is evaluated on the stream's tail only (0.74^2048: nothing)


@pytest.fixture(scope="module")
def vh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    vdl2hip.load_library()          # raises if the HIP library is missing: no fallback
    return vdl2hip


def _record(label, r, nout, seconds, note=""):
    path = os.environ.get("K1_STREAM_MATRIX")
    line = (f"{label:<44} ch {len(r['max']):>3} out {nout:>7}  model max {r['model_max'].max():.2e} rms {r['model_rms'].max():.2e}  "
            f"kernel max {r['max'].max():.2e} rms {r['rms'].max():.2e}  kernel/model max {np.max(r['max'] / np.maximum(r['model_max'], 1e-300)):5.2f} "
            f"rms {np.max(r['rms'] / np.maximum(r['model_rms'], 1e-300)):5.2f}  {seconds:5.1f} s {note}")
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _readable_from(rx, total):
    """index of the oldest decimated output the ring still holds (read_decimated() refuses what lies further back)"""
    from dumpvdl2_amd.vdl2hip import Vdl2HipError
    try:
        rx.read_decimated(rx.chan_first, 0, 1)
        return 0
    except Vdl2HipError:
        pass
    for k in range(30, 9, -1):                      # the ring's size is a power of two
        if total - (1 << k) > 0:
            try:
                rx.read_decimated(rx.chan_first, total - (1 << k), 1)
                return total - (1 << k)
            except Vdl2HipError:
                continue
    raise AssertionError("nothing readable")


def run_cell(vh, oracle_mod, label, os_, freqs, fmt, raw, feed, debug=None, max_block=None, checked=None, tail=None, absolute=False, note=""):
    """raw through a receiver without referee in the pieces `feed` yields -> compare() of what the ring holds (or its last `tail`
    outputs) on the `checked` channels (default: all), asserted against the derived bound (absolute: k1.ABS_BOUND instead)"""
    t0 = time.time()
    sb = 4 if fmt == S16 else 2
    nch = len(freqs)
    checked = list(range(nch)) if checked is None else checked
    o = oracle_mod.Oracle(k1.CF, freqs, oversample=os_, sample_fmt=fmt)      # coefficients and NCO steps: the oracle's, never the receiver's
    A, B = o.lpf()
    dphi = [o.dphi(c) for c in range(nch)]
    o.close()
    pieces = list(feed(raw.size // sb))
    assert sum(pieces) == raw.size // sb
    rx = vh.Receiver(k1.CF, freqs, os_, fmt, 0.0, max_block_bytes=max_block or max(pieces) * sb)
    rx.debug_option("referee", 0)                   # what read_decimated() returns is K1's own output, nowhere the referee's scan
    for k, v in (debug or {}).items():
        rx.debug_option(k, v)
    pinned = None
    off = 0
    for i, m in enumerate(pieces):
        blk = raw[off * sb:(off + m) * sb]
        if i == 0 and note == "cold":              # a large page-locked block into an idle receiver: copied and channelised in pieces
            import torch
            pinned = torch.from_numpy(blk.copy()).pin_memory()
            rx.feed_pinned_tensor(pinned)
        else:
            rx.feed(blk)
        off += m
    rx.sync()
    D = (raw.size // sb) // os_
    first = _readable_from(rx, D)
    if tail is not None:
        first = max(first, D - tail)
    got = np.stack([rx.read_decimated(c, first, D - first) for c in checked])
    st = rx.stats()
    steps = [rx.nco_step(c) & 0xFFFFFF for c in range(nch)]
    rx.close()
    assert got.shape == (len(checked), D - first, 2)
    assert steps == [d & 0xFFFFFF for d in dphi]
    if note == "cold":
        assert st["cold_start_feeds"] == 1
    if (debug or {}).get("force_timeout"):
        assert st["front_sync_timeouts"] > 0
    else:
        assert st["front_sync_timeouts"] == 0
    # the reference from rest RUNUP64 blocks ahead of the first output compared (from the stream's start where that is nearer)
    w0 = max(0, first - RUNUP64)
    cfg = types.SimpleNamespace(oversample=os_)
    sub = raw[w0 * os_ * sb:]
    dsel = [dphi[c] for c in checked]
    y64 = k1.exact_stream(cfg, sub, fmt, A, B, dsel, D - w0, unrounded=True, n0=w0 * os_, nthreads=k1.MAX_THREADS)[:, first - w0:]
    model = k1.block_form_model(cfg, sub, fmt, A, B, dsel, D - w0, n0=w0 * os_, nthreads=k1.MAX_THREADS)[:, first - w0:]
    r = k1.compare(got, y64, model, k1.input_peak(raw, fmt))
    r["y64"], r["model"], r["got"] = y64, model, got
    _record(label, r, D - first, time.time() - t0, note)
    if absolute:
        assert r["max"].max() <= k1.ABS_BOUND, f"{label}: {r['max'].max():.3e} of the input's peak (bound {k1.ABS_BOUND:.3e})"
    else:
        rms = np.sqrt((y64 ** 2).sum(-1).mean(-1)) / k1.input_peak(raw, fmt)
        assert rms.min() >= 1e-3, f"{label}: the stimulus leaves a checked channel quiet: {rms.min():.1e} of the input's peak"
        bad = k1.failures(r)
        assert not bad, f"{label}: " + "; ".join(f"[{checked[int(b.split()[1][:-1])]}] {b}" for b in bad)
    return r


def whole(n):
    yield n


def dense(os_, freqs, loud, fmt, nsamples, seed, period=None):
    """k1.stimulus() of nsamples; period: that many samples generated, then repeated (long streams)"""
    if period is None or period >= nsamples:
        return k1.stimulus(k1.CF, freqs, os_, nsamples, fmt, seed, loud=loud)
    sb = 4 if fmt == S16 else 2
    base = k1.stimulus(k1.CF, freqs, os_, period, fmt, seed, loud=loud)
    return np.tile(base, nsamples // period + 1)[:nsamples * sb]


# ---- builds: k_chanfir<OS, R, CR, FMT> over OS in {20, 13, 10, generic}, CR in {1, 2, 4}, the unsigned-byte prefetch build (FMT = kFmtU8: OS 20 / 10 with CR 4)
# and the staging path everywhere else.  3, 9 and 21 channels = CR 1, 2, 4, each with a partly filled last group; 21 leaves a wave inactive.

@pytest.mark.parametrize("fmt", ["s16", "u8"])
@pytest.mark.parametrize("nch", [3, 9, 21])
@pytest.mark.parametrize("os_", [20, 13, 10, 7, 16], ids=lambda o: f"os{o}")
def test_builds(vh, oracle_mod, os_, nch, fmt):
    freqs, loud = k1.channel_plan(os_, nch, variant=FMT[fmt] ^ 1)         # (three channels: the two formats share the plan's items between them)
    raw = dense(os_, freqs, loud, FMT[fmt], D_SMALL * os_ + 3, seed=os_ * 100 + nch)
    run_cell(vh, oracle_mod, f"build os{os_} {nch}ch {fmt}", os_, freqs, FMT[fmt], raw, whole)


# ---- segment length: 256 channels (gy = 16), feeds whose tiles-per-segment come out as 8, 1 and 2 (feed_common: ntile gy / 6144); the
# first one page-locked into the idle receiver (a cold start in pieces).  32 of the 256 channels are compared: the first and the last
# channel group row (gy 0 and 15), in them every (wave, position) slot - channels 0..15 and 240..255.

BIG_FEEDS = (420000, 60000, 120000)          # (the first: 8 MiB or more in either format at oversample 10, what a cold start in pieces takes)


@pytest.mark.parametrize("fmt", ["s16", "u8"])
@pytest.mark.parametrize("os_", [20, 10], ids=lambda o: f"os{o}")
def test_256_channels_segment_lengths(vh, oracle_mod, os_, fmt):
    tiles = [min(8, max(1, ((d + 127) // 128) * 16 // 6144)) for d in BIG_FEEDS]
    assert tiles == [8, 1, 2]
    freqs, loud = k1.channel_plan(os_, 256)
    n = [BIG_FEEDS[0] * os_ + 3, BIG_FEEDS[1] * os_ + 5, BIG_FEEDS[2] * os_ - 8 + 1]      # carries of 3, 8, 1 samples between them
    raw = dense(os_, freqs, loud, FMT[fmt], sum(n), seed=256 + os_, period=1 << 20)
    run_cell(vh, oracle_mod, f"256ch os{os_} {fmt} tiles 8,1,2", os_, freqs, FMT[fmt], raw, lambda total: iter(n),
             checked=list(range(16)) + list(range(240, 256)), note="cold")


# ---- feed geometry, on one CR 4 s16 build, the unsigned-byte prefetch build, one CR 2 build and the generic CR 1 build

GEOMETRY_BUILDS = {"cr4-s16": (20, 21, "s16"), "u8-prefetch": (10, 21, "u8"), "cr2": (13, 9, "s16"), "generic-cr1": (7, 3, "u8")}


def blocks_320k(sb):
    def feed(n):
        step = 320000 // sb
        for k in range(0, n, step):
            yield min(step, n - k)
    return feed


def random_pieces(seed, hi=3000):
    def feed(n):
        rng = np.random.default_rng(seed); k = 0
        while k < n:
            m = min(n - k, int(rng.integers(1, hi + 1)))
            yield m; k += m
    return feed


def tile_edge_sizes(os_):
    """feeds of D < 128, D = 128 k, D = 128 k + 1 outputs, a single output, none at all (the samples wait in the carry)"""
    def feed(n):
        cyc = [100 * os_, 384 * os_, 257 * os_, 128 * os_, os_, 129 * os_, 3, os_ - 3]; k = i = 0
        while k < n:
            m = min(n - k, cyc[i % len(cyc)])
            yield m; k += m; i += 1
    return feed


@pytest.mark.parametrize("geometry", ["whole", "blocks320k", "pieces1to3000", "tile_edges", "ring_wraps", "past_2pow24"])
@pytest.mark.parametrize("build", list(GEOMETRY_BUILDS))
def test_feed_geometry(vh, oracle_mod, build, geometry):
    os_, nch, fmt = GEOMETRY_BUILDS[build]
    f = FMT[fmt]; sb = 4 if f == S16 else 2
    freqs, loud = k1.channel_plan(os_, nch)
    kw = {}
    n = D_SMALL * os_ + 3
    if geometry == "whole":
        feed = whole
    elif geometry == "blocks320k":
        feed = blocks_320k(sb)
    elif geometry == "pieces1to3000":
        feed = random_pieces(7); kw["max_block"] = 3000 * sb
    elif geometry == "tile_edges":
        feed = tile_edge_sizes(os_)
    elif geometry == "ring_wraps":
        # blocks of at most 40 000 bytes: the ring is 2^17 outputs, the stream 3.4 of them; odd piece lengths put feeds on odd ring slots
        n = 450000 * os_ + 1
        feed = random_pieces(11, hi=40000 // sb); kw["max_block"] = 40000
    else:
        # the absolute sample index passes 2^24 (the phase is its low 24 bits times the step): four blocks, the last 50 000 outputs compared
        n = (1 << 24) + 30000 * os_ + 7
        feed = lambda total: iter([total // 4 + 1] * 3 + [total - 3 * (total // 4 + 1)])
        kw["tail"] = 50000
    raw = dense(os_, freqs, loud, f, n, seed=os_ + nch, period=1 << 20)
    run_cell(vh, oracle_mod, f"feed {build} {geometry}", os_, freqs, f, raw, feed, **kw)


# ---- look-back paths: the separate fix-up kernel (no_fuse) and the fall-back every consumer takes when its producer's state does not
# arrive (force_timeout), documented as differing from the fused look-back "in rounding only": the same bound

@pytest.mark.parametrize("build,path", [("cr4-s16", "no_fuse"), ("generic-cr1", "no_fuse"), ("u8-prefetch", "force_timeout"), ("cr2", "force_timeout")])
def test_look_back_paths(vh, oracle_mod, build, path):
    os_, nch, fmt = GEOMETRY_BUILDS[build]
    freqs, loud = k1.channel_plan(os_, nch)
    raw = dense(os_, freqs, loud, FMT[fmt], D_SMALL * os_ + 3, seed=os_ + nch + 1)
    half = (D_SMALL // 2 + 13) * os_ + 5                                 # two feeds: the state a feed hands to the next takes the path too
    run_cell(vh, oracle_mod, f"path {build} {path}", os_, freqs, FMT[fmt], raw, lambda total: iter([half, total - half]), debug={path: 1})


# ---- the edges of the sample formats

SUBNORMAL = 1.1754944e-38           # below this a float32 is subnormal


def _subnormals(y):
    a = np.abs(y)
    return int(((a > 0) & (a < SUBNORMAL)).sum())


def _note(text):
    print(text)
    path = os.environ.get("K1_STREAM_MATRIX")
    if path:
        with open(path, "a") as f:
            f.write("    " + text + "\n")


@pytest.mark.parametrize("fmt", ["s16", "u8"])
@pytest.mark.parametrize("kind", k1.EDGES)
def test_input_edges(vh, oracle_mod, kind, fmt):
    """Full-scale DC, the most negative code, a full-scale Nyquist tone, white noise over every code, an impulse followed by 200 000
    samples of silence.  On constant inputs nothing averages and after the impulse nothing is left, so the model's own error is no
    scale here: the bound is absolute, k1.ABS_BOUND = 2.6e-6 of the input's peak (four times what the model is held to on these inputs).
    In these receivers a segment is one tile long, and what a segment hands to the next reaches 128 outputs into it (by then a state
    has decayed by 1e-17 at oversample 20): the impulse's tail ends there, twenty orders of magnitude above the subnormal range -
    test_impulse_decays_through_subnormals is the cell where the tail gets that far."""
    build = "cr4-s16" if fmt == "s16" else "u8-prefetch"
    os_, nch, _ = GEOMETRY_BUILDS[build]
    freqs, _ = k1.channel_plan(os_, nch)
    raw = k1.edge_input(kind, FMT[fmt], 205000 + 3)
    r = run_cell(vh, oracle_mod, f"edge {kind} {fmt}", os_, freqs, FMT[fmt], raw, blocks_320k(4 if fmt == "s16" else 2), absolute=True)
    if kind == "impulse_then_silence" and fmt == "s16":
        nz = np.nonzero(np.abs(r["got"][0]).sum(-1))[0]
        _note(f"impulse s16, centre channel: last non-zero output {int(nz[-1]) - 4999 // os_} outputs after the impulse, {np.abs(r['got'][0][nz[-1]]).max():.1e} of full scale")


def test_impulse_decays_through_subnormals(vh, oracle_mod):
    """One full-scale impulse at the first sample of an 8-tile segment of a 256-channel receiver, then silence: inside a segment the
    state is carried from tile to tile in registers, 1 024 outputs without a cut, and at oversample 20 it decays by 0.74 per output -
    through the subnormal range (1e-38 .. 1e-45) some 290 to 345 outputs after the impulse.  The hardware KEEPS subnormals: the
    code objects are built with float_denorm_mode_32 = 3 (hipcc's default for gfx950, no flush-to-zero flag in build.py), and the
    kernel's stream holds subnormal outputs where the model's (numpy on the CPU, IEEE) does (3 378 and 3 435 of them on the 32 checked
    channels, profiles/k1_stream_matrix.txt).  The row notes both counts; the bound is
    the absolute one, against which a tail flushed to zero (an error of 1e-38) would show in the note and not fail."""
    os_ = 20
    freqs, _ = k1.channel_plan(os_, 256)
    D = BIG_FEEDS[0]
    raw = k1.edge_input("impulse_then_silence", S16, D * os_)
    x = raw.view(np.int16).reshape(-1, 2)
    x[4999] = 0; x[3 * 1024 * os_] = 32767                                   # segment 3 = outputs 3 072 .. 4 095
    checked = list(range(16)) + list(range(240, 256))
    r = run_cell(vh, oracle_mod, "edge impulse at a segment start, 256ch os20 s16", os_, freqs, S16, raw, whole, checked=checked, absolute=True)
    _note(f"impulse, 8-tile segment: subnormal outputs in the kernel's stream {_subnormals(r['got'])}, in the model's {_subnormals(r['model'])}")
