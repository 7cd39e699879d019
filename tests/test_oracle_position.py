"""The oracle started at a stream position (Oracle.set_position): a stream that begins at input sample n, at rest.

Aligned positions (every NCO phase 0 again) must give the committed golden answers with the burst timing shifted - an expectation
that owes nothing to set_position itself.  Unaligned positions pin the phase rule (n * nco_dphi) & 0xffffff: zeros in front of a
capture leave the filter at rest and only advance the NCO, so the oracle at 0 on zeros(n) + capture and the oracle at n on the
capture produce the same decimated stream, bit for bit."""
import numpy as np
import pytest

import cases
import position

CASES3 = ["dirty25k_1s", "os10_noisy_1s", "config4_0p4s"]


@pytest.mark.parametrize("name", CASES3)
def test_aligned_position_gives_the_golden_answers_shifted(oracle_mod, name):
    cfg, iq, _, gold = cases.load(name)
    n = position.ALIGNED
    assert n > 2**32 and n % cfg.oversample == 0 and n % (1 << 24) == 0
    got = position.oracle_at(name, n)
    assert got["K"] == n // cfg.oversample
    cases.check_against_golden(got["frames"], got["counters"], position.shifted_golden(gold, got["K"]), label=f"{name} at {n}")
    # and the decimated stream itself is the one at position 0: same phases, same rest
    assert np.array_equal(got["trace"].view(np.uint32), position.oracle_at(name, 0)["trace"].view(np.uint32))


@pytest.mark.parametrize("name", CASES3)
@pytest.mark.parametrize("periods", [0, 257])
def test_unaligned_position_continues_the_phase_of_a_silent_lead_in(oracle_mod, name, periods):
    """periods = 0: the lead-in of zeros is what the run at 0 is really fed.  A lead-in past 2^32 cannot be fed; there the phase
    rule is held to the same run through the NCO's period: positions that differ by a multiple of 2^24 input samples have the
    same phases."""
    cfg, iq, _, _ = cases.load(name)
    os_ = cfg.oversample
    n = 12340 * os_ + periods * os_ * (1 << 24)
    assert periods == 0 or n > 2**32
    at_n = position.oracle_run(oracle_mod, cfg, iq, n)
    lead = np.concatenate([np.zeros(2 * 12340 * os_, dtype=np.int16), np.asarray(iq, dtype=np.int16).reshape(-1)])
    at_0 = position.oracle_run(oracle_mod, cfg, lead, 0)
    assert at_0["D"] == 12340 + at_n["D"] and at_n["D"] == iq.size // 2 // os_
    a, b = at_0["trace"][:, 12340:, :], at_n["trace"]
    assert not np.any(at_0["trace"][:, :12340, :])           # zeros leave the filter at rest
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.any(b)
    assert any(cfg.centerfreq != f for f in cfg.freqs)       # at least one channel is mixed, or nothing here depends on the phase


def test_set_position_refusals(oracle_mod):
    cfg, iq, _, _ = cases.load("os10_noisy_1s")
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample)
    with pytest.raises(ValueError):
        o.set_position(10 * 2**32 + 3)                       # not a multiple of the oversampling
    o.set_position(10 * 2**32)
    o.process(np.zeros(400, dtype=np.int16).view(np.uint8))
    assert o.decimated_count(0) == 20
    with pytest.raises(ValueError):
        o.set_position(0)                                    # only before the first block


def test_sync_events_are_absolute_and_counted_from_the_start(oracle_mod):
    cfg, iq, _, _ = cases.load("os10_noisy_1s")
    ev = []
    for pos in (0, position.ALIGNED):
        o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
        if pos:
            o.set_position(pos)
        o.trace_sync_events(4096)
        o.process(np.asarray(iq).view(np.uint8), block_bytes=1 << 24)
        ev.append([o.sync_events(c).copy() for c in range(len(cfg.freqs))])
    Ka = position.ALIGNED // cfg.oversample
    for a, b in zip(*ev):
        assert len(a) == len(b) and len(a) > 0
        assert np.array_equal(a["sample"] + Ka, b["sample"]) and np.array_equal(a["evals"], b["evals"])
        ended = a["end_sample"] >= 0
        assert np.array_equal(ended, b["end_sample"] >= 0)
        assert np.array_equal(a["end_sample"][ended] + Ka, b["end_sample"][ended])
