"""CPU side of the noise-floor replay's checks (tests/nf_reference.py builds every case and its expectation):
  * the definition the kernel states - mag_lp at an update is the recurrence from 0 over the last 256 evaluations (windowed) - equals the
    reference program's own recurrence over the whole stream (sequential) BIT FOR BIT on every case the device is given.  That is a condition on
    the inputs, not a tolerance: an input that broke it would be printed and has to be replaced (nf_reference's docstring names the kinds that
    do).  The one exception is meant: the case whose remembered tail holds fewer than 256 evaluations, which has its own expectation;
  * every case then runs through the HOST build of the kernel's source (tests/hostsim: hostsim_nf_feed), with the lanes of a phase in either
    order, and is held to what tests/test_gpu_nf_probe.py holds the device build to."""
import ctypes as C

import numpy as np
import pytest

import nf_reference as nr
import pyhostsim


@pytest.fixture(scope="module", params=[False, True], ids=["lanes_up", "lanes_down"])
def H(request):
    return C.CDLL(pyhostsim.build(reverse_lanes=request.param))


@pytest.mark.parametrize("name", nr.CASE_NAMES)
def test_windowed_is_the_recurrence(name):
    case = nr.get_case(name)
    total = differ = 0
    worst = 0.0
    for c in range(case.nchan):
        e = case.expected(c)
        chunks = case.all_chunks(c)
        lp_s, nf_s = nr.sequential(case.y[c], chunks)
        lp_w, nf_w = nr.windowed(case.y[c], chunks)                       # the whole list within reach
        assert len(lp_s) == len(lp_w) == len(e["lp"])
        o = 1000 * np.arange(1, len(lp_s) + 1, dtype=np.int64) - 1
        short = e["reach"] > np.maximum(o - (nr.LP_TERMS - 1), 0)          # updates whose window the remembered tail cuts short
        if not case.short_tail:
            assert not short.any(), f"{name} channel {c}: the tail is too short at updates {1 + np.flatnonzero(short)}: replace the input"
        bad = np.flatnonzero(~nr.same_bits(lp_s, lp_w) | ~nr.same_bits(nf_s, nf_w))
        for u in bad[:10]:
            print(f"{name} channel {c} update {u + 1}: sequential mag_lp {lp_s[u]!r} mag_nf {nf_s[u]!r}, windowed {lp_w[u]!r} {nf_w[u]!r}")
        total += len(lp_s); differ += bad.size
        assert bad.size == 0, f"{name} channel {c}: windowed != sequential at {bad.size} of {len(lp_s)} updates, first {bad[0] + 1}: replace the input"
        # what the builds are held to: the window as far as the chunk list reaches
        full = ~short
        assert nr.same_bits(e["lp"][full], lp_s[full]).all()
        if case.short_tail:
            assert short.any(), f"{name} channel {c}: no update's window is cut short"
            mags = nr.magnitudes(case.y[c], chunks)
            for u in np.flatnonzero(short):
                k = int(o[u] - e["reach"][u] + 1)                         # evaluations the window still holds
                assert 0 < k < nr.LP_TERMS
                d = abs(float(e["lp"][u]) - float(lp_s[u])); bound = 0.9 ** k * float(mags[:o[u] + 1].max())
                dn = abs(float(e["nf"][u]) - float(nf_s[u]))
                db = abs(20 * np.log10(float(e["nf"][u]) + 0.001) - 20 * np.log10(float(nf_s[u]) + 0.001))
                worst = max(worst, d)
                print(f"{name} channel {c} update {u + 1}: the tail holds {k} evaluations: |mag_lp - sequential| = {d:.3e} (bound 0.9^k max mag = {bound:.3e}), "
                      f"|mag_nf - sequential| = {dn:.3e} = {db:.2e} dB")
                assert d <= bound
        else:
            assert nr.same_bits(e["nf"], nf_s).all()
    print(f"{name}: {total} updates, {differ} differ between windowed and sequential; largest deviation of a short tail {worst:.3e}")
    assert total > 0


def test_the_cases_are_what_they_claim():
    """the properties the cases are there for are properties of the inputs: checked here, so that a changed generator cannot lose them silently"""
    def spans(case, c):
        """chunks the window of each update touches"""
        ch = case.all_chunks(c)
        cum = np.concatenate([[0], np.cumsum(ch[:, 1])])
        o = 1000 * np.arange(1, cum[-1] // 1000 + 1) - 1
        return np.searchsorted(cum, o, "right") - np.searchsorted(cum, np.maximum(o - 255, 0), "right") + 1
    st = nr.get_case("storms")
    for c in range(st.nchan):
        s = set(spans(st, c).tolist())
        assert {2, 64, 190, 191, 192, 256} <= s, sorted(s)
        # a group of two updates over 300 chunks and more; a staged slice of exactly kNfSlice chunks that ends with the list (ncomb)
        ch = st.all_chunks(c)
        cum = np.concatenate([[0], np.cumsum(ch[:, 1])])
        chunk_of = lambda o: int(np.searchsorted(cum, o, "right")) - 1
        recs = st.expected(c)["recs"]
        assert any(r["u1"] - r["u0"] == 2 and chunk_of(1000 * r["u1"] - 1) - chunk_of(1000 * (r["u0"] + 1) - 256) + 1 >= 300 for r in recs), f"channel {c}"
        assert any(r["u1"] - r["u0"] == 1 and chunk_of(1000 * r["u1"] - 1) == chunk_of(r["ev1"] - 1)
                   and chunk_of(1000 * r["u1"] - 1) - chunk_of(1000 * r["u1"] - 256) + 1 == nr.NF_SLICE for r in recs), f"channel {c}"
    upd = lambda case, c: [r["u1"] - r["u0"] for r in case.expected(c)["recs"]]
    assert all({31, 32, 33, 64, 65} <= set(upd(nr.get_case("groups"), c)) for c in range(5))
    assert [max(upd(nr.get_case("batch"), c)) for c in range(3)] == [2047, 2048, 2049]
    b = nr.get_case("boundaries")
    ends = {r["ev1"] % 1000 for c in range(5) for r in b.expected(c)["recs"]}
    assert {999, 0, 1} <= ends
    assert any(r["ncomb"] > 0 and r["ev1"] == r["ev0"] for c in range(5) for r in b.expected(c)["recs"])      # no evaluations, the tail kept
    tc = nr.get_case("tail_cross")
    assert any(len(t) == nr.NF_TAIL and sum(n for _, n in t) == nr.LP_TERMS for c in range(5) for t, _ in tc.expected(c)["tails"])
    rw = nr.get_case("ring_wraps")
    assert all(rw.expected(c)["recs"][-1]["u1"] > 3 * rw.nf_ring for c in range(5))
    for c in range(5):                                                     # a window, all in one chunk, that goes round the y ring's end
        pos = nr.positions(rw.all_chunks(c))
        o = 1000 * np.arange(1, len(pos) // 1000 + 1) - 1
        assert ((pos[o] - pos[o - 255] == 3 * 255) & (pos[o] // nr.RING_LEN != pos[o - 255] // nr.RING_LEN)).any(), f"channel {c}"
    tf = nr.get_case("tiny_feeds")
    for c in range(5):                                                     # an update whose window lies in more than 64 feeds
        ev = np.array([r["ev1"] for r in tf.expected(c)["recs"]])
        assert any(np.searchsorted(ev, 1000 * u - 1, "right") - np.searchsorted(ev, 1000 * u - 256, "right") > nr.NF_TAIL for u in range(1, ev[-1] // 1000 + 1)), f"channel {c}"
    rr = nr.get_case("random_run")
    assert len(rr.feeds) == 40 and all(rr.expected(c)["recs"][-1]["u1"] > rr.nf_ring for c in range(5))
    # magnitudes: fminf takes either side, and once both are equal; update 1 of channel 0 is subnormal; the top of the range shows in update 3
    m = nr.get_case("magnitudes")
    e = m.expected(0)
    assert 0 < int(e["lp"][:1].view(np.uint32)[0]) < 0x00800000 and e["lp"][2] > 1e36      # (by its bits: a flushed environment compares a subnormal as 0)
    nf_before = np.concatenate([[np.float32(2.0)], e["nf"][:-1]])
    assert (e["lp"] < nf_before).any() and (e["lp"] > nf_before).any()
    e4 = m.expected(4)
    assert e4["lp"][0] == np.float32(2.0), repr(e4["lp"][0])               # mag_lp == mag_nf at the first update


@pytest.mark.parametrize("name", nr.CASE_NAMES)
def test_host_build(H, name):
    case = nr.get_case(name)
    run = nr.host_runner(H)
    blob5, n5 = nr.run_case(run, case, 5, "host")
    blob1, n1 = nr.run_case(run, case, 1, "host")
    print(f"host {name}: {len(case.feeds)} feeds, {n5} + {n1} values compared bit for bit")
    assert n5 > 0


def test_the_walkers_log_keeps_256_evaluations_in_a_few_chunks(oracle_mod):
    """What the walker hands the replay, on a synthetic capture with the --max-ppm gate on (config3_0p6s: 64 channels 25 kHz apart, 5 ppm;
    the host build on the oracle's decimated stream, one feed).  A chunk ends where the evaluation grid shifts - a sync, or a preamble the gate
    drops - and after either the next fire is two evaluations away at the least.  So chunks are few and long: here never two of fewer than 4
    evaluations in a row, and the last 256 evaluations before any chunk's end in 2 chunks at the most, where the replay remembers 64
    (kNfTail).  (The other way a chunk ends, a feed's end, is joined again by nf_prepare: case tiny_feeds.)"""
    import cases
    cfg, iq, _, _ = cases.load("config3_0p6s")
    assert cfg.rx_max_ppm > 0
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
    tr = o.trace_all(iq.size // 2 // cfg.oversample + 4)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=4)
    D = o.decimated_count(0)
    hs = pyhostsim.HostSim(list(cfg.freqs), cfg.rx_max_ppm, cap_log2=int(np.ceil(np.log2(D + 70000))))
    hs.feed(tr[:, :D, :])
    dropped = sum(hs.counters(c)[18] for c in range(len(cfg.freqs)))
    chunks = shortest = 0
    worst_run = worst_need = 0
    for c in range(len(cfg.freqs)):
        cnt = hs.eval_log(c)[:, 1]
        assert len(cnt) and cnt.min() >= 2, f"channel {c}: a chunk of {cnt.min() if len(cnt) else 0} evaluations"
        chunks += len(cnt); shortest = int(cnt.min()) if not shortest else min(shortest, int(cnt.min()))
        run = 0
        for n in cnt:
            run = run + 1 if n < 4 else 0
            worst_run = max(worst_run, run)
        cum = np.concatenate([[0], np.cumsum(cnt)])
        need = np.arange(1, len(cum)) - (np.searchsorted(cum, cum[1:] - nr.LP_TERMS, "right") - 1)     # chunks that hold the 256 evaluations before a chunk's end
        worst_need = max(worst_need, int(need[cum[1:] >= nr.LP_TERMS].max()))
    hs.close()
    print(f"config3_0p6s: {dropped} preambles dropped by the gate, {chunks} chunks, shortest {shortest} evaluations, longest run of chunks under 4 evaluations {worst_run}, "
          f"most chunks holding the last 256 evaluations {worst_need}")
    assert dropped > 0 and worst_run <= 1 and worst_need <= 2
