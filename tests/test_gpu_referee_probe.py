"""The DEVICE build of the referee's margin arithmetic (vdl2_core.h: sync_metric_ref in both forms - with sync_metric_flipped,
sync_metric_two and sync_metric_unwrap_alts behind it -, ref_pherr_range, ref_candidate_verdict, ref_vertex_marginal, ref_symbol_dist,
ref_symbol_marginal) through the test hook vdl2hip_debug_core_probe (kernels.h: k_core_probe, kinds 9 .. 13), element by element, against
tests/core_reference.py's numpy restatements on that file's own input sets - the references and inputs tests/test_core_reference_referee.py
has held to the host build here on the CPU.

  pherr, slope, the ranges, the verdict's bits and the boolean results: bit for bit.
  E = sqrtf(the sum of 16 figures): the sum is taken in the source's order by both (nothing may reorder it: no fast-math), sqrtf is
      correctly rounded in numpy and good to 1 ulp at worst on the device - 1 ulp allowed.
  alo, ahi: the pherr they start from is bit-equal; the short cut (sync_metric_unwrap_alts) adds at most five terms to it, each a product
      of at most five factors one of which holds a division - a term is off by 1 ulp of itself at the most if the device's division were
      1 ulp instead of half of one, a term is at most 2 (2 pi)^2 16 = 1 263, the running value as much again: 10 ulps of 1 263 = 1.2e-3
      allowed.  The re-run forms (sync_metric_flipped, sync_metric_two) are sync_metric's own operations: equal whenever that one is.
How many values are NOT bit-equal is printed beside the allowance.

Then, without the restatement: the metric run again in float64 with each listed decision - and both - taken the other way lies in the
device's [alo, ahi], and the device's E is kRefBig exactly when a tap is zero or more than two decisions hang on the stream's error
(core_reference.check_alternatives_and_E)."""
import numpy as np
import pytest

import core_reference as cr

pytestmark = pytest.mark.gpu
F32 = np.float32
ALT_ALLOWANCE = 10 * float(np.spacing(F32(1263.0)))


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    return vdl2hip.load_library()


@pytest.fixture(scope="module")
def windows():
    ph, eps2, where = cr.ref_windows()
    ph.setflags(write=False); eps2.setflags(write=False)
    return ph, eps2, where


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("full", [True, False], ids=["full", "plain"])
def test_sync_metric_ref(L, windows, full):
    ph, eps2, where = windows
    dev = cr.device_probe(L, "ref_full" if full else "ref_plain", np.concatenate([ph, eps2], axis=1))
    ref = np.stack(cr.sync_metric_ref(ph, eps2, full), axis=1)
    d = np.flatnonzero((bits(dev[:, :2]) != bits(ref[:, :2])).any(axis=1))
    assert d.size == 0, f"pherr / slope: {d.size} of {len(ph)} windows differ, first {d[:5]}: {dev[d[:3]]} / {ref[d[:3]]}"
    nE = int((bits(dev[:, 2]) != bits(ref[:, 2])).sum()); nA = int((bits(dev[:, 3:]) != bits(ref[:, 3:])).any(axis=1).sum())
    print(f"device sync_metric_ref full={full}: E not bit-equal at {nE} of {len(ph)} windows, alo / ahi at {nA}")
    big = ref[:, 2] == cr.REF_BIG
    assert np.array_equal(dev[:, 2] == cr.REF_BIG, big)
    dE = np.abs(dev[~big, 2].astype(np.float64) - ref[~big, 2]) / np.spacing(ref[~big, 2])
    assert dE.max() <= 1.0, f"E: {dE.max()} ulps"
    unknown = ref[:, 4] == cr.REF_BIG                     # ("cannot tell": [0, kRefBig])
    assert np.array_equal(dev[:, 4] == cr.REF_BIG, unknown) and np.all(dev[unknown, 3] == ref[unknown, 3])
    dA = np.abs(dev[~unknown, 3:].astype(np.float64) - ref[~unknown, 3:])
    print(f"    largest |alo, ahi - reference| {dA.max():.3e} (allowed {ALT_ALLOWANCE:.3e})")
    assert dA.max() <= ALT_ALLOWANCE
    n = cr.check_alternatives_and_E(ph, eps2, dev, full, f"device build, full={full}")
    assert n >= 20000


def test_ranges_and_verdict(L):
    a = cr.verdict_inputs()
    dev = cr.device_probe(L, "verdict", a)
    r0 = cr.ref_pherr_range(a[:, 0], a[:, 1], a[:, 2], a[:, 3]); r3 = cr.ref_pherr_range(a[:, 4], a[:, 5], a[:, 6], a[:, 7])
    r6 = cr.ref_pherr_range(a[:, 9], a[:, 10], a[:, 11], a[:, 12])
    rr = np.stack([r0[0], r0[1], r3[0], r3[1], r6[0], r6[1]], axis=1)
    d = np.flatnonzero((bits(dev[:, 1:]) != bits(rr)).any(axis=1))
    assert d.size == 0, f"ref_pherr_range: {d.size} of {len(a)} differ, first {a[d[:2]]}: {dev[d[:2], 1:]} / {rr[d[:2]]}"
    vd = cr.ref_candidate_verdict(r0, r3, a[:, 8], a[:, 7], r6, a[:, 13], a[:, 14])
    got = dev[:, 0].copy().view(np.int32)
    d = np.flatnonzero(got != vd)
    assert d.size == 0, f"ref_candidate_verdict: {d.size} of {len(a)} differ, first {a[d[:2]]}: {got[d[:3]]} / {vd[d[:3]]}"
    assert all((vd == v).sum() > 2000 for v in (0, 1, 3))


def test_vertex_marginal(L):
    a = cr.vertex_boxes()
    got = cr.device_probe(L, "vertex_marginal", a).view(np.int32)[:, 0]
    ref = cr.ref_vertex_marginal(*[a[:, k] for k in range(6)]).astype(np.int32)
    d = np.flatnonzero(got != ref)
    assert d.size == 0, f"{d.size} of {len(a)} differ, first {a[d[:3]]}: {got[d[:3]]} / {ref[d[:3]]}"
    assert 0.1 < ref.mean() < 0.9


def test_symbol_margin(L):
    a = cr.symbol_inputs()
    dev = cr.device_probe(L, "symbol", a)
    dist = cr.ref_symbol_dist(a[:, 0], a[:, 1], a[:, 2]); marg = cr.ref_symbol_marginal(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    d = np.flatnonzero((bits(dev[:, 0]) != bits(dist)) | (dev[:, 1].copy().view(np.int32) != marg.astype(np.int32)))
    assert d.size == 0, f"{d.size} of {len(a)} differ, first {a[d[:3]]}: {dev[d[:3]]} / {dist[d[:3]]} {marg[d[:3]]}"
    assert 0.2 < marg.mean() < 0.8
