"""The marking step of the burst decoder, shared by decode_burst() and k_burst_mark (vdl2_core.h: burst_mark), on the CPU.

tests/mark_ahead/mark_ahead_host.cpp - a stand-alone program - walks the oracle's decimated stream with the host build of the walker and
gives every burst descriptor to the burst decoder's first pass and to the marking step on its own: the pieces the first pass lists
and the pieces of the step's mask must be the same, burst for burst, and both must be what the first pass listed before the step was
factored out (tests/golden/mark_ahead_*.txt, recorded with the program's -DMARK_AHEAD_BASELINE build against that older source).
The streams hold bursts whose slope is worked out again (redo_slope) and bursts whose first symbol's predecessor lies in the feed
before (prev_n); a `wide` request - a stretch of 128 pieces or more - is longer than a burst can be (kMaxSyms symbols are 55 pieces),
so the program makes one up: a real descriptor with prev_n moved back into the silence that the test puts in front of the capture.
config3's 0.6 s hold no marked symbol on the oracle's own stream and the no-gate 0.6 s four bursts with one; a third capture - the
same without the gate, 2.4 s, eight channels - gives the comparison 31 bursts and 148 pieces."""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mark_ahead", "mark_ahead_host.cpp")
WIDE_BACK = 135168        # 132 pieces of 1 024 samples


def streams(name):
    """-> (cfg, iq): the two captures of the issue.  config4 without its --max-ppm gate, 0.6 s, three channels: the busiest one of
    the capture's first 0.6 s and its two neighbours 8 kHz away, which lock on to its leakage (weak bursts, many marked symbols) -
    behind 1.4 s of silence, so that the made-up wide burst's prev_n is a sample of the stream"""
    if name == "config3_0p6s":
        cfg, iq, _, _ = cases.load(name)
        return cfg, iq, 0
    from dumpvdl2_amd import workloads, synth
    long = name == "config4_nogate_2p4s"      # (more bursts for the comparison to stand on: 2.4 s, the eight channels around the busiest)
    cfg = dataclasses.replace(workloads.config4(2.4 if long else 0.6), rx_max_ppm=0.0)
    iq, bursts = synth.synthesize(cfg)
    per = np.bincount([b.chan for b in bursts], minlength=len(cfg.freqs))
    if long:
        c = int(np.argmax(per[4:-4])) + 4
        return dataclasses.replace(cfg, freqs=tuple(cfg.freqs[c - 4:c + 4])), iq.reshape(-1), 0
    c = int(np.argmax(per[1:-1])) + 1
    cfg = dataclasses.replace(cfg, freqs=tuple(cfg.freqs[c - 1:c + 2]))
    pad = np.zeros(2 * 140000 * cfg.oversample, dtype=iq.dtype)
    return cfg, np.concatenate([pad, iq.reshape(-1)]), WIDE_BACK


def write_input(path, oracle_mod, name):
    cfg, iq, wide_back = streams(name)
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, max_ppm=cfg.rx_max_ppm)
    D = iq.size // 2 // cfg.oversample
    tr = o.trace_all(D + 4)
    o.process(iq.view(np.uint8), block_bytes=1 << 24, nthreads=4)
    D = o.decimated_count(0)
    tr = np.ascontiguousarray(tr[:, :D, :], dtype=np.float32)
    # feeds: pieces of 2 500 - 9 000 samples (config4's bursts are up to 8 500 long: most begin in the feed before the one that
    # hands them over), the longer ones walked in segments of >= 2 500
    rng = np.random.default_rng(7); lens = []; k = 0
    while k < D:
        m = min(D - k, int(rng.integers(2500, 9000))); lens.append(m); k += m
    with open(path, "wb") as f:
        f.write(struct.pack("<4i f i q", len(cfg.freqs), len(lens), 2500, 8, float(cfg.rx_max_ppm), wide_back, D))
        f.write(np.asarray(cfg.freqs, dtype=np.uint32).tobytes()); f.write(np.asarray(lens, dtype=np.int64).tobytes()); f.write(tr.tobytes())
    return path


def build_program(out, extra=(), hostsim_dir=None):
    hostsim_dir = hostsim_dir or os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", hostsim_dir, *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(str(tmp_path_factory.mktemp("mark_ahead") / "mark_ahead_host"))


@pytest.mark.parametrize("name", ["config3_0p6s", "config4_nogate_0p6s", "config4_nogate_2p4s"])
def test_marking_step_lists_what_the_first_pass_lists(oracle_mod, program, tmp_path, name):
    inp = write_input(str(tmp_path / "in.bin"), oracle_mod, name)
    p = subprocess.run([program, inp], capture_output=True, text=True, timeout=300)
    lines = p.stdout.splitlines()
    assert p.returncode == 0, "\n".join(l for l in lines if not l.startswith("B "))[-2000:] + p.stderr[-2000:]
    summary = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    print(name, summary)
    assert lines[-1].startswith("SUMMARY") and summary["bad"] == 0
    if name == "config4_nogate_0p6s":      # (config3's carriers are strong and 100 kHz apart: on the oracle's own stream none of its symbols is within the margin)
        assert summary["redo_slope"] >= 1 and summary["prev_n_in_previous_feed"] >= 1 and summary["wide"] == 1, summary
    with open(os.path.join(ROOT, "tests", "golden", f"mark_ahead_{name}.txt")) as f:
        want = [l for l in f.read().splitlines() if l]
    assert [l for l in lines if l.startswith("B ")] == want
