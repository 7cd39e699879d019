"""The shared device logic (vdl2_core.h: walker, stitcher, noise-floor replay, burst decoder, frame finisher) in its CPU build, on a
stream that begins hours in: every index it keeps is an absolute 64-bit sample number, narrowed in places that are right only
because of a mask or a bounded difference.  The simulator is started at decimated position K (hostsim_set_position) and fed the
decimated stream of the oracle started at the same position; frames, timing, the reference counters and the AVLC counters must be
the oracle's.  K just below 2^31 and 2^32 puts each boundary inside the capture."""
import zlib

import numpy as np
import pytest

import cases
import position
import pyhostsim
from util import assert_frames_equal

CASES3 = ["dirty25k_1s", "os10_noisy_1s", "config4_0p4s"]
POSITIONS = {"below_2^31": lambda D: 2**31 - D // 2, "below_2^32": lambda D: 2**32 - D // 2, "2^40+7": lambda D: 2**40 + 7}


def run_at(name, K, chunks=None, segments=None, two_tier=False, referee=False, seed=1):
    cfg, iq, _, _ = cases.load(name)
    C = len(cfg.freqs)
    want = position.oracle_at(name, K * cfg.oversample)
    tr, D = want["trace"], want["D"]
    hs = pyhostsim.HostSim(list(cfg.freqs), cfg.rx_max_ppm, cap_log2=17 if chunks else int(np.ceil(np.log2(D + 70000))))
    hs.set_position(K)
    if segments:
        hs.set_segments(*segments)
    if two_tier:
        hs.set_two_tier(True)
    if referee:
        hs.set_exact(tr)
    if chunks is None:
        hs.feed(tr)
    else:
        rng = np.random.default_rng(seed); k = 0
        while k < D:
            m = min(D - k, int(rng.integers(*chunks))); hs.feed(tr[:, k:k + m, :]); k += m
    got = dict(frames=hs.frames(), counters=[hs.counters(c) for c in range(C)], avlc=[hs.avlc_counters(c) for c in range(C)])
    hs.close()
    return want, got


def check(want, got, K, D, label):
    assert len(want["frames"]) > 0
    assert_frames_equal(want["frames"], got["frames"], exact_samples=True, label=label)
    assert all(K <= f["sync_sample"] < f["end_sample"] < K + D for f in got["frames"]), label
    assert [c[:cases.N_REFERENCE_COUNTERS] for c in want["counters"]] == [c[:cases.N_REFERENCE_COUNTERS] for c in got["counters"]], label
    assert want["counters"] == got["counters"], label          # on identical input the two diagnostics agree too
    assert want["avlc"] == got["avlc"], label
    key = lambda f: (f["chan"], f["burst_ord"], f["idx"])
    a, b = sorted(want["frames"], key=key), sorted(got["frames"], key=key)
    assert [f["nf_pwr_dbfs"] for f in a] == [f["nf_pwr_dbfs"] for f in b], label       # the reference's arithmetic, on identical input
    assert [f["ppm_error"] for f in a] == [f["ppm_error"] for f in b], label


@pytest.mark.parametrize("where", list(POSITIONS))
@pytest.mark.parametrize("name", CASES3)
@pytest.mark.parametrize("pieces", ["whole", "pieces"])
def test_device_logic_at_a_position(oracle_mod, name, where, pieces):
    cfg, iq, _, _ = cases.load(name)
    D = iq.size // 2 // cfg.oversample
    K = POSITIONS[where](D)
    chunks = None if pieces == "whole" else {"dirty25k_1s": (500, 20000), "os10_noisy_1s": (64, 5000), "config4_0p4s": (3000, 50000)}[name]
    want, got = run_at(name, K, chunks, seed=zlib.crc32(f"{name} {where}".encode()))
    if where != "2^40+7":
        b = 2**31 if where == "below_2^31" else 2**32
        assert K < b < K + D and any(f["sync_sample"] < b for f in want["frames"]) and any(f["end_sample"] >= b for f in want["frames"])
    check(want, got, K, D, f"{name} at K={K} {pieces}")


@pytest.mark.parametrize("name,chunks,segments,two_tier,referee", [
    ("dirty25k_1s", (3000, 40000), (450, 5), True, False), ("os10_noisy_1s", None, (64, 32), True, False),
    ("config4_0p4s", None, (4000, 7), False, False), ("config4_0p4s", (3000, 50000), None, True, True)])
@pytest.mark.parametrize("where", ["below_2^31", "below_2^32"])
def test_segmented_walk_and_screening_rule_at_a_position(oracle_mod, name, where, chunks, segments, two_tier, referee):
    """the speculative segments (spec_walk / stitch_channel), K3's two-tier rule and the referee's plumbing across each boundary"""
    cfg, iq, _, _ = cases.load(name)
    D = iq.size // 2 // cfg.oversample
    K = POSITIONS[where](D)
    want, got = run_at(name, K, chunks, segments, two_tier, referee)
    check(want, got, K, D, f"{name} at K={K} chunks={chunks} segments={segments} two_tier={two_tier} referee={referee}")


def test_position_is_refused_after_a_feed(oracle_mod):
    cfg, iq, _, _ = cases.load("os10_noisy_1s")
    hs = pyhostsim.HostSim(list(cfg.freqs), cfg.rx_max_ppm, cap_log2=12)
    hs.feed(np.zeros((len(cfg.freqs), 100, 2), dtype=np.float32))
    with pytest.raises(ValueError):
        hs.set_position(2**32)
    hs.close()
