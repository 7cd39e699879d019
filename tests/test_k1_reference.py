"""The yardstick of tests/test_gpu_k1_stream.py, tested on the CPU (tests/k1_reference.py): the bound derived from the float32 model of
K1's recurrence must pass what is right - the model itself, the double-precision stream rounded once - and fail what is subtly wrong:
the oracle's sequential float32 scan (right, but 30-100 times noisier: why it cannot be the yardstick) and the mistakes a channeliser
kernel can make without a decoded frame changing."""
import types

import numpy as np
import pytest

import k1_reference as k1

D = 26250                   # 0.25 s of decimated stream
OVERSAMPLES = (7, 10, 13, 16, 20)
MARGIN = 5.0                # what is wrong must exceed the bound by this factor


class Case:
    def __init__(self, oracle_mod, os_, with_oracle=True):
        self.os = os_
        self.cfg = types.SimpleNamespace(oversample=os_)
        self.freqs, self.loud = k1.channel_plan(os_, 9)
        self.raw = k1.stimulus(k1.CF, self.freqs, os_, D * os_, 1, 100 + os_, loud=self.loud)
        o = oracle_mod.Oracle(k1.CF, self.freqs, oversample=os_, sample_fmt=1)
        self.A, self.B = o.lpf()
        self.dphi = [o.dphi(c) for c in range(len(self.freqs))]
        self.oracle = None
        if with_oracle:
            tr = o.trace_all(D + 4)
            o.process(self.raw, block_bytes=1 << 24, nthreads=2)
            assert o.decimated_count(0) == D
            self.oracle = tr[:, :D].copy()
        o.close()
        self.y64 = k1.exact_stream(self.cfg, self.raw, 1, self.A, self.B, self.dphi, D, unrounded=True, nthreads=k1.MAX_THREADS)
        self.model = k1.block_form_model(self.cfg, self.raw, 1, self.A, self.B, self.dphi, D, nthreads=k1.MAX_THREADS)
        self.peak = k1.input_peak(self.raw, 1)

    def compare(self, cand):
        return k1.compare(cand, self.y64, self.model, self.peak)

    def model_of(self, chan, first_block, nblocks, phase_index=None):
        """the model of one channel over blocks first_block .. +nblocks, started from rest at first_block"""
        s = first_block * self.os
        return k1.block_form_model(self.cfg, self.raw[4 * s:], 1, self.A, self.B, [self.dphi[chan]], nblocks, n0=s, phase_index=phase_index)[0]


_cases = {}


@pytest.fixture
def case(oracle_mod, request):
    os_ = request.param
    if os_ not in _cases:
        _cases[os_] = Case(oracle_mod, os_)
    return _cases[os_]


@pytest.mark.parametrize("case", OVERSAMPLES, indirect=True, ids=lambda o: f"os{o}")
def test_what_is_right_passes(case):
    """the model against its own bound; the double-precision stream rounded to float32 (the best a float32 stream can be); and the stimulus
    is dense: every channel's output rms is at least 1e-3 of the input's peak, the loud channel's peak is most of it"""
    r = case.compare(case.model)
    assert not k1.failures(r)
    assert r["model_max"].max() < 1e-6 and r["model_max"].min() > 0          # the scale the issue measured: 2-4e-7 on the loud channel
    r = case.compare(case.y64.astype(np.float32))
    assert not k1.failures(r), k1.failures(r)
    rms = np.sqrt((case.y64 ** 2).sum(-1).mean(-1)) / case.peak
    assert rms.min() >= 1e-3, rms
    assert np.sqrt((case.y64[case.loud] ** 2).sum(-1).max()) >= 0.8 * case.peak


@pytest.mark.parametrize("case", OVERSAMPLES, indirect=True, ids=lambda o: f"os{o}")
def test_the_oracles_float32_scan_fails(case):
    """the reference's sequential float32 recursion is 30-100 times the model's error on the loud channel: held to this bound it fails by
    more than MARGIN at every oversample - which is why it is not what K1 is compared with"""
    r = case.compare(case.oracle)
    c = case.loud
    print(f"os {case.os}: oracle max {r['max'][c]:.2e} rms {r['rms'][c]:.2e}, model max {r['model_max'][c]:.2e} rms {r['model_rms'][c]:.2e} of the input's peak")
    assert r["max"][c] >= MARGIN * r["bound_max"][c] and r["rms"][c] >= MARGIN * r["bound_rms"][c]
    # ... and it is the same filter: nothing but rounding noise separates the two
    assert r["max"].max() < 1e-4


def test_windowed_model_is_the_sequential_recurrence(oracle_mod):
    """block_form_model() evaluates the state step on windows with RUNUP blocks of run-up: against the same float32 recurrence run
    sequentially from the stream's start, block by block"""
    f32 = np.float32
    os_, nblk = 13, 1500
    cs = Case(oracle_mod, os_, with_oracle=False)
    bf = k1.block_form_constants(cs.A, cs.B, os_)
    lut = k1.nco_lut()
    v = k1.to_float(cs.raw, 1)
    g0 = np.array(bf.g0[:os_], dtype=f32); g1 = np.array(bf.g1[:os_], dtype=f32)
    P = [f32(p) for p in bf.P]; c0, c1, c2 = f32(bf.c0), f32(bf.c1), f32(bf.c2)
    for c in (0, 3, 5):
        dphi = cs.dphi[c] & 0xffffff
        t0 = np.zeros(2, dtype=f32); t1 = np.zeros(2, dtype=f32)
        got = np.zeros((nblk, 2), dtype=f32)
        for k in range(nblk):
            a0 = np.zeros(2, dtype=f32); a1 = np.zeros(2, dtype=f32)
            for j in range(os_):
                n = k * os_ + j
                ph = (n * dphi) & 0xffffff
                e = lut[ph >> 16]; F = f32(ph & 0xffff)
                sn = e[2] * F + e[0]; cn = e[3] * F + e[1]
                x = v[n]
                m = np.array([cn * x[0] + sn * (-x[1]), cn * x[1] + sn * x[0]], dtype=f32)
                a0 = a0 + g0[j] * m; a1 = a1 + g1[j] * m
            t0, t1 = P[0] * t0 + (P[1] * t1 + a0), P[2] * t0 + (P[3] * t1 + a1)
            got[k] = c0 * t0 + (c1 * t1 + c2 * m)
        assert np.array_equal(got, cs.model[c, :nblk]), c


SEG = 128 * 37              # a segment boundary: a whole number of tiles (128 blocks) into the stream
PLANTED = ("start_state_dropped", "fixup_row_off_by_one", "phase_one_step_ahead", "odd_slot_pair_swapped", "neighbour_channel")


@pytest.mark.parametrize("case", [20, 10], indirect=True, ids=lambda o: f"os{o}")
@pytest.mark.parametrize("what", PLANTED)
def test_planted_mistakes_fail(case, what):
    """mistakes planted in a copy of the model's output - each confined to a few outputs of one channel, none of which changes a decoded
    frame - exceed the bound, the smallest of them by more than MARGIN (a condition on these inputs, checked here)"""
    y = case.model.copy()
    c = 4                                               # CF - 100 008 Hz: an offset channel off the raster, one of the quiet ones
    if what == "start_state_dropped":
        # the outputs of one segment's first tile without the state the segment before leaves behind
        y[c, SEG:SEG + 128] = case.model_of(c, SEG, 128)
    elif what == "fixup_row_off_by_one":
        # ... with the fix-up's row i + 1, (c0, c1) P^(i+2) t, added to output i
        zs = case.model_of(c, SEG, 128)
        fix = case.model[c, SEG:SEG + 128] - zs
        y[c, SEG:SEG + 127] = zs[:127] + fix[1:]
    elif what == "phase_one_step_ahead":
        # the NCO one sample ahead from one tile on (the state before it is right: RUNUP blocks of the true phase lead in)
        n0 = (SEG - k1.RUNUP) * case.os
        idx = np.arange(n0, n0 + (k1.RUNUP + 256) * case.os, dtype=np.uint64)
        idx[k1.RUNUP * case.os:] += np.uint64(1)
        y[c, SEG:SEG + 256] = case.model_of(c, SEG - k1.RUNUP, k1.RUNUP + 256, phase_index=idx)[k1.RUNUP:]
    elif what == "odd_slot_pair_swapped":
        y[c, [SEG + 1, SEG + 2]] = y[c, [SEG + 2, SEG + 1]]
    elif what == "neighbour_channel":
        y[c, SEG:SEG + 128] = y[c + 1, SEG:SEG + 128]
    r = case.compare(y)
    assert len(k1.failures(r)) == 1, k1.failures(r)
    print(f"os {case.os} {what}: max {r['max'][c]:.2e} = {r['max'][c] / r['bound_max'][c]:.0f} x the bound")
    assert r["max"][c] >= MARGIN * r["bound_max"][c]


@pytest.mark.parametrize("os_,nch,fmt", [(20, 21, 1), (10, 21, 0)], ids=["os20-s16", "os10-u8"])
@pytest.mark.parametrize("kind", k1.EDGES)
def test_model_on_the_edges_of_the_formats(oracle_mod, kind, os_, nch, fmt):
    """the absolute bound of the GPU suite's edge cells is FACTOR_MAX times what the model is held to here, on the same inputs"""
    freqs, _ = k1.channel_plan(os_, nch)
    raw = k1.edge_input(kind, fmt, 205003)
    o = oracle_mod.Oracle(k1.CF, freqs, oversample=os_, sample_fmt=fmt)
    A, B = o.lpf(); dphi = [o.dphi(c) for c in range(nch)]
    o.close()
    cfg = types.SimpleNamespace(oversample=os_)
    n = 205003 // os_
    y64 = k1.exact_stream(cfg, raw, fmt, A, B, dphi, n, unrounded=True, nthreads=k1.MAX_THREADS)
    model = k1.block_form_model(cfg, raw, fmt, A, B, dphi, n, nthreads=k1.MAX_THREADS)
    r = k1.compare(model, y64, model, k1.input_peak(raw, fmt))
    print(f"{kind}: model max {r['model_max'].max():.2e} of the input's peak")
    assert r["model_max"].max() <= k1.MODEL_EDGE_MAX
    assert k1.ABS_BOUND == k1.FACTOR_MAX * k1.MODEL_EDGE_MAX
