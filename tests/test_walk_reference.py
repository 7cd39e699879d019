"""tests/walk_reference.py - the per-sample restatement of demod() / got_sync() that the walker's device build is held to
(tests/test_gpu_walk_probe.py) - against the oracle, and the probe cases on the CPU.

  * The reference IS the reference program's state machine: on the oracle's own decimated streams of four small captures (the last with
    the --max-ppm gate on), cut into feeds, every got_sync() success - its sample, the evaluation count, dropped or accepted, ppm_error,
    the header's verdict, the sample at which the burst ended - the counters and the evaluation count are the oracle's
    (vdl2o_trace_sync_events), identically.
  * Every probe stream gives the same float32 phase from libm's atan2 (the reference) and from atan2_f64 (the product): no sample is left out.
  * The cases hold what they were built for (feed ends inside unique words, headers and bursts, interval starts within the ring's reach of
    older intervals, segments with more chunks than a speculative walk may log, ...): floors, so that a change to a generator cannot
    quietly empty a case.
  * The host build of the device code (hostsim_walk_probe: same arguments as the device hook) gives the reference's descriptors, chunk
    lists, counters and end states in every launch shape, and the same bytes in all of them.  It is a second witness for the mapping
    written down in walk_reference.py, not a reference."""
import ctypes as C

import numpy as np
import pytest

import pyhostsim
import walk_reference as wr


@pytest.fixture(scope="module")
def H():
    return C.CDLL(pyhostsim.build())


@pytest.mark.parametrize("name", wr.TRACE_CAPTURES)
def test_reference_is_the_oracles_state_machine(oracle_mod, name):
    case = wr.get_case("cut_" + name, oracle_mod)
    nev = 0
    for c in range(5):
        e = case.expected(c)
        mine, ev = e["events"], case.oracle_events[c]
        assert len(mine) == len(ev), f"{name} stream {c}: {len(mine)} got_sync() successes, the oracle {len(ev)}"
        for m, o in zip(mine, ev):
            got = (m["sample"], m["evals"], m["accepted"], np.float32(m["ppm_error"]).tobytes(), m["hdr_status"], m["end_sample"])
            want = (int(o["sample"]), int(o["evals"]), int(o["accepted"]), o["ppm_error"].tobytes(), int(o["hdr_status"]), int(o["end_sample"]))
            assert got == want, f"{name} stream {c}: event {m} != the oracle's {o}"
        r = e["ref"]
        assert r.n == len(case.y[c]) and r.evals == case.oracle_evals[c], f"{name} stream {c}: {r.evals} evaluations, the oracle {case.oracle_evals[c]}"
        for k in wr.WALKER_COUNTERS[:-1]:
            assert int(r.counters[k]) == case.oracle_counters[c][k], f"{name} stream {c}: counter {k}: {int(r.counters[k])}, the oracle {case.oracle_counters[c][k]}"
        assert r.neg_all == case.oracle_counters[c][wr.CNT_NEG_IDX]
        # the evaluated samples, feed by feed, are what the chunk lists say, and their count is the oracle's
        assert sum(int(f["chunks"][:, 1].sum()) for f in e["feeds"]) == case.oracle_evals[c]
        nev += len(ev)
    assert nev >= 5
    print(f"{name}: {len(case.feeds())} feeds, 5 streams, {nev} got_sync() successes, counters and evaluation counts equal the oracle's")


def test_metric_table_is_the_ring(oracle_mod):
    """The reference looks the metric of an evaluation on a contiguous ring up in a table; here it works every one out from the ring too"""
    case = wr.get_case("cut_os10_noisy_1s", oracle_mod)
    n = 30000
    r = wr.RefChannel(0, case.freqs[0], case.max_ppm, case.y[0][:n], check_table=True)
    for k in range(0, n, 7001):
        r.feed(k, min(n, k + 7001))
    want = [o for o in case.oracle_events[0] if o["sample"] < n]
    assert [m["sample"] for m in r.events] == [int(o["sample"]) for o in want] and r.table_checked > 2000
    print(f"{r.table_checked} of {r.evals} evaluations read a contiguous ring: the table holds the ring's own value for every one")


@pytest.mark.parametrize("name", wr.CASE_NAMES)
def test_probe_streams_have_one_phase(H, oracle_mod, name):
    """libm's atan2 and the product's atan2_f64 give the same float32 for every sample of every probe stream (they differ on about one
    sample in 10^8): a stream that fails here gets another seed, no sample is left out of any comparison"""
    case = wr.get_case(name, oracle_mod)
    H.hostsim_phase.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for c, y in enumerate(case.y):
        out = np.empty(len(y), np.float32)
        with wr.ieee_subnormals():
            H.hostsim_phase(y.ctypes.data, out.ctypes.data, len(y))
            ref = wr.phases(y)
        bad = np.flatnonzero(out.view(np.uint32) != ref.view(np.uint32))
        assert len(bad) == 0, f"{name} stream {c}: samples {bad[:5].tolist()} have two phases"


def test_cases_hold_what_they_are_for(oracle_mod):
    sit = dict.fromkeys(("in_word", "mode1", "mode2", "within156", "within320", "tiny", "empty"), 0)
    for name in ("cut_" + n for n in wr.TRACE_CAPTURES):
        case = wr.get_case(name, oracle_mod)
        assert case.feeds()[0][0] == 0 and max(k1 - k0 for k0, k1 in case.feeds()) <= 40000
        sit["tiny"] += sum(1 for k0, k1 in case.feeds() if 1 <= k1 - k0 <= 3); sit["empty"] += sum(1 for k0, k1 in case.feeds() if k1 == k0)
        for c in range(5):
            e = case.expected(c)
            syncs = np.array([v["sample"] for v in e["events"]])
            for (k0, k1), f in zip(case.feeds(), e["feeds"]):
                st = f["state"]
                sit["in_word"] += int(np.any((syncs - 150 < k1) & (k1 <= syncs)))
                sit["mode1"] += int(st["mode"] == 1); sit["mode2"] += int(st["mode"] == 2)
                if st["mode"] == 0 and st["niv"] > 0:
                    sit["within156"] += int(k1 - st["a"] < wr.FRESH_AFTER); sit["within320"] += int(wr.FRESH_AFTER <= k1 - st["a"] < wr.CLEAN_AFTER)
    print("feed ends of the cases cut from the oracle's traces:", sit)
    assert sit["in_word"] >= 8 and sit["mode1"] >= 8 and sit["mode2"] >= 20 and sit["within156"] >= 8 and sit["within320"] >= 4 and sit["tiny"] >= 12 and sit["empty"] >= 4
    # gate_storm: a feed's log overflows cap_log = 100; half and a third of the long feed hold more chunks than kSpecLog
    g = wr.get_case("gate_storm")
    for c in range(5):
        e = g.expected(c)
        ch = e["feeds"][0]["chunks"]
        assert len(ch) > 100 and all(v["accepted"] == 0 for v in e["events"])
        if c < 4:
            for lo, hi in ((20000, 40000), (13334, 26668)):
                assert ((ch[:, 0] >= lo) & (ch[:, 0] < hi)).sum() > wr.SPEC_LOG + 2, (c, lo, hi)
    # dense: the ring of a fresh interval reaches over two earlier ones; syncs fire less than 150 samples into an interval (their taps and
    # prev_phi0 come through the history)
    d = wr.get_case("dense")
    reach = 0; early = 0; kinds = set()
    for c in range(5):
        e = d.expected(c)
        reach = max([reach] + [int((np.diff(f["ring"][f["ring"] >= 0]) < -1).sum()) for f in e["feeds"]])
        hist = e["ref"].history
        early += sum(1 for a, b in hist if b - a < 150)
        kinds |= {v["hdr_status"] for v in e["events"]}
    assert reach >= 2 and early >= 40 and kinds >= {0, 1, 2, 3}, (reach, early, kinds)
    h = wr.get_case("headers")
    assert {v["hdr_status"] for c in range(5) for v in h.expected(c)["events"]} >= {0, 1, 2, 3}
    assert max(len(f["bursts"]) for c in range(5) for f in h.expected(c)["feeds"]) >= 3            # cap_bursts_chan of 1 and 2 overflow
    assert any(int(b["syndrome"]) >> 8 == 1 for c in range(5) for f in h.expected(c)["feeds"] for b in f["bursts"])      # a corrected header
    # burst_end: stream 0's bursts end at k_end - 1, k_end and k_end + 1
    b = wr.get_case("burst_end")
    ends = [int(x["end_sample"]) for f in b.expected(0)["feeds"] for x in f["bursts"]]
    k_ends = [k1 for _, k1 in b.feeds()]
    assert any(x + 1 in k_ends for x in ends) and any(x in k_ends for x in ends) and any(x - 1 in k_ends for x in ends)
    # ring_wrap: a burst in progress, and an interval less than 156 samples old, at a feed end just behind a multiple of the ring's length
    w = wr.get_case("ring_wrap")
    inb = sum(1 for c in range(5) for (k0, k1), f in zip(w.feeds(), w.expected(c)["feeds"]) if f["state"]["mode"] != 0 and (k1 - 1) // 4096 != int(f["state"]["pb"]["sync_sample"]) // 4096)
    stale = sum(1 for c in range(5) for (k0, k1), f in zip(w.feeds(), w.expected(c)["feeds"]) if f["state"]["mode"] == 0 and f["state"]["niv"] > 0
                and k1 - f["state"]["a"] < wr.FRESH_AFTER and int(f["state"]["ivb"][0]) // 4096 != (k1 - 1) // 4096)
    print(f"ring_wrap: {inb} feed ends inside a burst that began before the wrap, {stale} inside the 156 samples after a burst with the wrap between")
    assert inb >= 2 and stale >= 1
    s = wr.get_case("silence")
    mag = [s.y[c].view(np.uint32) & 0x7fffffff for c in range(5)]            # (by their bits: a flushed environment compares a subnormal as 0)
    assert all(not np.any(m[:1500]) and np.all(m[1500:4000] < 0x00800000) and np.count_nonzero(m[1500:4000]) > 4000 for m in mag)


TOTAL = dict.fromkeys(wr.PLAN_KEYS, 0)


@pytest.mark.parametrize("name", wr.CASE_NAMES)
def test_host_build_gives_the_reference(H, oracle_mod, name):
    case = wr.get_case(name, oracle_mod)
    fn = wr.host_fn(H)
    for nchan in (5, 3, 1):
        blobs = {}
        for shape in wr.SHAPES:
            blobs[shape], st = wr.run_case(fn, case, nchan, shape, "host build")
            for k in wr.PLAN_KEYS:
                TOTAL[k] += st[k]
        assert all(b == blobs[None] for b in blobs.values()), f"{name}, {nchan} channels: launch shapes differ in their bytes: {[b == blobs[None] for b in blobs.values()]}"
    print(f"{name}: {len(case.feeds())} feeds x {len(wr.SHAPES)} launch shapes x 1, 3, 5 channels equal the reference; so far {TOTAL}")


def test_host_build_segment_length_sweep(H):
    case = wr.get_case("sweep")
    fn = wr.host_fn(H)
    ref, _ = wr.run_case(fn, case, 3, None, "host build")
    tot = dict.fromkeys(wr.PLAN_KEYS, 0)
    for L in wr.SWEEP_SEGLEN:
        b, st = wr.run_case(fn, case, 3, ("seglen", L), f"host build seglen {L}")
        assert b == ref, f"segments of {L} samples: bytes differ from the plain walk's"
        for k in wr.PLAN_KEYS:
            tot[k] += st[k]
    print(f"sweep: segments of {wr.SWEEP_SEGLEN[0]} .. {wr.SWEEP_SEGLEN[-1]} samples: {tot}")
    assert tot["adopted"] > 1000 and tot["walked"] > 1000 and tot["pre"] > 100 and tot["pending"] > 100 and tot["history"] > 100


def test_host_build_adoption_floors(H):
    """The stitcher's paths are all taken: segments adopted and walked; adoptions that join behind the segment's start (pre > 0), that bring a
    burst in progress (H.mode != 0), that bring interval history (H.niv > 0); speculative walks refused because they fired before the join
    (H.n_first < st.e) and because they ran out of room (H.ok == 0: kSpecLog in gate_storm)"""
    print(wr.adoption_floors(wr.host_fn(H), "host build"))


def test_host_probe_refuses_what_the_product_cannot_have(H):
    case = wr.get_case("sweep")
    fn = wr.host_fn(H)
    rings = wr.Rings(1, 4096)
    e = case.expected(0)
    rings.write(0, case.y[0], e["pf"], e["cand"], 0, 2000)
    def rc(k0=0, k1=2000, mode=1, nseg=4, seglen=500, ws=None, cap_b=8, cap_l=64):
        ws = wr.initial_states(1) if ws is None else ws
        return wr.probe(fn, mode, rings, case.freqs, 0.0, k0, k1, nseg, seglen, ws, np.zeros((1, wr.NUM_COUNTERS), np.uint64), cap_b, cap_l)[0]
    assert rc() == 0
    assert rc(seglen=63, nseg=32) == -1 and rc(nseg=1, seglen=2000) == -1 and rc(nseg=33, seglen=64) == -1
    assert rc(nseg=5, seglen=500) == -1 and rc(nseg=3, seglen=500) == -1            # not the feed's length over seglen, rounded up
    assert rc(k1=5000) == -1                                                        # longer than the ring
    assert rc(mode=2) == -1 and rc(cap_b=0) == -1 and rc(cap_l=0) == -1
    bad = wr.initial_states(1); bad["mode"] = 3
    assert rc(ws=bad) == -1
    bad = wr.initial_states(1); bad["e"] = 7                                        # a search that is not where the feed begins
    assert rc(ws=bad) == -1
    bad = wr.initial_states(1); bad["mode"] = 2; bad["pb"]["sync_sample"] = 100; bad["pb"]["t_first"] = 107; bad["pb"]["nsym"] = 30; bad["pb"]["end_sample"] = 400
    assert rc(k0=200, k1=2000, nseg=4, seglen=450, ws=bad) == -1                      # end_sample is not t_first + 10 (nsym - 1)
