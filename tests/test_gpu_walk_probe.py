"""The DEVICE build of K4, the walker (kernels.h: k_walk, k_walk_spec, k_walk_stitch; vdl2_core.h: walk_run, spec_walk, stitch_try_accept,
stitch_materialize, stitch_channel), through the test hook vdl2hip_debug_walk_probe, against tests/walk_reference.py: the reference program's
demod() / got_sync() restated sample by sample in Python.  tests/test_walk_reference.py proves on the CPU that the restatement IS the oracle's
state machine, event for event, that every probe stream has one phase (libm's atan2 and the product's atan2_f64 agree on every sample), and runs
the same cases through the host build; the host build is no reference here.

One call is one feed of 1, 3 or 5 channels on inputs the test controls: y, the sync metric pf (cr.sync_metric of every contiguous window) and
the candidate bits from numpy, the WalkState and the counters carried from call to call.  Everything that comes back is compared bit for bit:
every field of every Burst descriptor (prev_n, vdphi_err, sync_evals and nf_upd, which no frame shows, among them; the descriptors of
bursts that will deliver no frame too), 0xA5 behind the last descriptor, the evaluation-log chunk list (the maximal runs of stride 3 of the
evaluated samples) and 0xA5 behind it, nb_chan, nlog, the control block with its overflow flag, the walker's counters, and the end state by
the meaning walk_reference.py writes down (the 160 samples of the phase ring instead of the interval list, which legitimately differs
between launch shapes).  seg_stats must be what the reference's own trajectory and the SpecHeads say the stitcher has to decide.

Launch shapes: k_walk; k_walk_spec + k_walk_stitch as a receiver with seg_max 2, 3, 5 and 32 and seg_min 64 and 1000 launches them (four
walks per workgroup, the last workgroup partly idle; two channels per stitch workgroup on dynamic LDS, the last one half empty with 1, 3 and 5
channels); segment lengths of 64 .. 463 samples on one small case.  Every shape must give the same bytes as k_walk.

Case counts, adoption figures, wall time and the deliberate breakages these tests catch: profiles/walk_probe_device.txt."""
import numpy as np
import pytest

import walk_reference as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    return wr.device_fn(vdl2hip.load_library())


@pytest.mark.parametrize("name", wr.CASE_NAMES)
def test_walk(fn, oracle_mod, name):
    case = wr.get_case(name, oracle_mod)
    tot = dict.fromkeys(wr.PLAN_KEYS, 0)
    for nchan in (5, 3, 1):
        blobs = {}
        for shape in wr.SHAPES:
            blobs[shape], st = wr.run_case(fn, case, nchan, shape, "device")
            for k in wr.PLAN_KEYS:
                tot[k] += st[k]
        same = [b == blobs[None] for b in blobs.values()]
        assert all(same), f"{name}, {nchan} channels: launch shapes differ in their bytes: {same}"
    print(f"{name}: {len(case.feeds())} feeds x {len(wr.SHAPES)} launch shapes x 5, 3, 1 channels equal the reference bit for bit and each other byte for byte; stitcher: {tot}")


def test_segment_length_sweep(fn):
    case = wr.get_case("sweep")
    ref, _ = wr.run_case(fn, case, 3, None, "device")
    tot = dict.fromkeys(wr.PLAN_KEYS, 0)
    for L in wr.SWEEP_SEGLEN:
        b, st = wr.run_case(fn, case, 3, ("seglen", L), f"device seglen {L}")
        assert b == ref, f"segments of {L} samples: bytes differ from k_walk's"
        for k in wr.PLAN_KEYS:
            tot[k] += st[k]
    print(f"sweep: segments of {wr.SWEEP_SEGLEN[0]} .. {wr.SWEEP_SEGLEN[-1]} samples, 3 channels: {tot}")
    assert tot["adopted"] > 1000 and tot["walked"] > 1000 and tot["pre"] > 100 and tot["pending"] > 100 and tot["history"] > 100


def test_adoption_floors(fn):
    """seg_stats shows adopted and walked segments; the SpecHeads show adoptions with pre > 0, with H.mode != 0 (a burst in progress taken from
    a SpecOut), with H.niv > 0, and refusals by H.n_first < st.e and by H.ok == 0 (more than kSpecLog chunks)"""
    print("stitcher on headers, dense and gate_storm, 5 channels, seg_max 2, 5 and 32:", wr.adoption_floors(fn, "device"))


def test_sizes_the_product_cannot_have_are_refused(fn):
    case = wr.get_case("sweep")
    rings = wr.Rings(1, 4096)
    e = case.expected(0)
    rings.write(0, case.y[0], e["pf"], e["cand"], 0, 2000)
    INVAL = -1
    def rc(k0=0, k1=2000, mode=1, nseg=4, seglen=500, ws=None, cap_b=8, cap_l=64):
        ws = wr.initial_states(1) if ws is None else ws
        return wr.probe(fn, mode, rings, case.freqs, 0.0, k0, k1, nseg, seglen, ws, np.zeros((1, wr.NUM_COUNTERS), np.uint64), cap_b, cap_l)[0]
    assert rc() == 0
    assert rc(seglen=63, nseg=32) == INVAL and rc(nseg=1, seglen=2000) == INVAL and rc(nseg=33, seglen=64) == INVAL
    assert rc(nseg=5, seglen=500) == INVAL and rc(nseg=3, seglen=500) == INVAL        # not the feed's length over seglen, rounded up
    assert rc(k1=5000) == INVAL                                                       # longer than the ring
    assert rc(mode=2) == INVAL and rc(cap_b=0) == INVAL and rc(cap_l=0) == INVAL
    bad = wr.initial_states(1); bad["mode"] = 3
    assert rc(ws=bad) == INVAL
    bad = wr.initial_states(1); bad["e"] = 7                                          # a search that is not where the feed begins
    assert rc(ws=bad) == INVAL
    bad = wr.initial_states(1); bad["mode"] = 2; bad["pb"]["sync_sample"] = 100; bad["pb"]["t_first"] = 107; bad["pb"]["nsym"] = 30; bad["pb"]["end_sample"] = 400
    assert rc(k0=200, k1=2000, nseg=4, seglen=450, ws=bad) == INVAL                   # end_sample is not t_first + 10 (nsym - 1)
