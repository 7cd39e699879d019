"""What the spectrogram tap costs, on ONE GPU box: config4 (256 channels, 16 s) is synthesised once, then every case runs in a process
of its own, under a time limit, and reports ms per step with the block resident in HBM (vdl2hip_feed_device) and fed from
page-locked host memory (vdl2hip_feed_pinned), six feeds in flight, profiling off, the input monitor on at nfft 1024 in all of them:

  (a) parent        the parent commit's library (parent=path/to/lib.so): the monitor as it was
  (b) tap off       this build, monitor on, spectrogram off: the same kernels as (a)
  (c) R=16          spectrogram on, 16 segments a line
  (d) R=<small>     spectrogram on with the shortest lines the ring limit takes at this block size (--small-r; R = 1 needs
                    ring_lines * nfft <= 2^25 for the lines of one feed, which a 134 MB block at nfft 1024 does not meet)

The four cases run interleaved, --rounds times each (a fresh process every time), and their medians are reported with every run
beside them: (b) has to lie within the spread of (a); (c) and (d) are reported.  (c) and (d) also give kernel_ms per feed: the summed
HIP-event time of the monitor's launches with the tap's among them, from a pass of their own at profiling level 2.  With --ratios
FILE the worst share of the error bounds reached in tests/test_gpu_specgram.py (the lines that file prints) is quoted underneath.

  python dev/gpu_specgram_rate.py parent=lib.so [--out profiles/specgram_rate.txt] [--ratios test_output.txt]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPTURE = "/tmp/vdl2_spectrum_rate_config4"
NFFT = 1024


def run(rx, feed, steps, repeats, lag):
    times = []
    for _ in range(repeats):
        rx.set_drain_lag(lag)
        t0 = time.perf_counter()
        for _ in range(steps):
            feed()
            rx.drain_packed()
        rx.set_drain_lag(0)
        rx.drain_packed()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    return round(statistics.median(times), 3)


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    cfg = workloads.config4(args.duration)
    host = torch.from_numpy(np.load(CAPTURE + f"_{args.duration:g}.npy"))
    nbytes = host.numel() * host.element_size()
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vdl2hip.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=nbytes)
    rx.spectrum_enable(NFFT, vdl2hip.WIN_HANN, 1)
    res = {"name": args.name, "R": args.R, "MB_per_step": round(nbytes / 1e6, 1)}
    if args.R:
        try:
            rx.specgram_enable(args.R)
        except vdl2hip.Vdl2HipError as e:
            res["refused"] = str(e)
            rx.close()
            print(json.dumps(res), flush=True)
            return
        res["ring_lines"] = rx.specgram()["ring_lines"]
    dev = host.to("cuda:0")
    pin = host.pin_memory()
    del host
    for _ in range(3):                              # (the clocks come up; the first block of an idle receiver is not timed)
        rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed()
    res["hbm_ms"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    res["pinned_ms"] = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    rx.sync()
    rx.set_profiling(2)
    rx.spectrum(reset=True)
    k0 = rx.spectrum(power=False)["kernel_ms"]
    for _ in range(args.steps):
        rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed()
    rx.sync()
    sp = rx.spectrum(power=False)
    res["kernel_ms"] = round((sp["kernel_ms"] - k0) / args.steps, 4)
    res["segments_per_step"] = sp["segments"] // args.steps
    rx.set_profiling(0)
    if args.R:
        res["lines"] = rx.specgram()["lines"]
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specgram_rate.txt"))
    ap.add_argument("--ratios", default=None, help="output of tests/test_gpu_specgram.py run with -s: its 'specgram bound ratio' lines")
    ap.add_argument("--duration", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small-r", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--name", default="in-tree")
    ap.add_argument("--R", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import numpy as np
    from dumpvdl2_amd import synth, workloads
    path = CAPTURE + f"_{args.duration:g}.npy"
    if not os.path.exists(path):
        t0 = time.time()
        iq, _ = synth.synthesize(workloads.config4(args.duration), workers=8)
        np.save(path, iq)
        print(f"# capture ready ({time.time() - t0:.0f} s)", flush=True)
    libs = dict(s.partition("=")[::2] for s in args.libs)
    parent = libs.pop("parent", None)
    if not parent or not os.path.exists(parent):
        # (b) against (a) is what the record is for: without the parent's library only a scratch file is written
        print("WARNING: no parent=path/to/lib.so (or it does not exist): case (a) cannot run, and (b) has nothing to be held against", flush=True)
        if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "specgram_rate.txt"):
            sys.exit("refusing to write the record profiles/specgram_rate.txt without case (a): name the parent commit's build, or another --out")
        parent = None
    cases = ([("(a) parent, monitor on", "parent", parent, 0)] if parent else []) + [("(b) tap off", "in-tree", "", 0), ("(c) tap on, R = 16", "in-tree", "", 16),
                                                                                   (f"(d) tap on, R = {args.small_r}", "in-tree", "", args.small_r)]
    plan = [("R = 1", "in-tree", "", 1)] + cases * args.rounds        # (R = 1 first: whether the ring limit takes it at this block size)
    rows, stopped = [], False
    for label, name, lib, R in plan:
        env = dict(os.environ)
        if lib:
            env["VDL2HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--name", name, "--R", str(R), "--duration", str(args.duration),
               "--steps", str(args.steps), "--repeats", str(args.repeats)]
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{label}: TIMEOUT - nothing more is started", flush=True)
            stopped = True
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            print(f"{label}: FAILED rc={p.returncode} - nothing more is started\n{p.stderr[-1500:]}", flush=True)
            stopped = True
            break
        rows.append(dict(json.loads(line[-1]), label=label))
        print(line[-1], flush=True)
    lines = [f"config4: 256 channels, {args.duration:g} s per step (int16), profiling off, six feeds in flight, input monitor on at nfft {NFFT}; "
             f"a fresh process per run, the cases interleaved, median of {args.repeats} x {args.steps} steps in each run, {time.strftime('%Y-%m-%d')}",
             f"{'case':<24} {'runs':>5} {'MB/step':>8} {'ms/step HBM':>12} {'ms/step pinned':>15} {'monitor kernel ms/feed':>23} {'segments/feed':>14} {'ring_lines':>11}"]
    for label, _, _, _ in cases:
        sel = [r for r in rows if r["label"] == label and "hbm_ms" in r]
        if not sel:
            continue
        hbm, pin = [r["hbm_ms"] for r in sel], [r["pinned_ms"] for r in sel]
        lines.append(f"{label:<24} {len(sel):>5} {sel[0]['MB_per_step']:>8} {statistics.median(hbm):>12.3f} {statistics.median(pin):>15.3f} "
                     f"{statistics.median(r['kernel_ms'] for r in sel):>23.4f} {sel[0]['segments_per_step']:>14} {sel[0].get('ring_lines', ''):>11}")
        lines.append(f"{'':<24} each run, HBM: {' '.join(str(v) for v in hbm)} (spread {max(hbm) - min(hbm):.3f}); pinned: {' '.join(str(v) for v in pin)} (spread {max(pin) - min(pin):.3f})")
    for r in rows:
        if "refused" in r:
            lines.append(f"{r['label']}: refused at this block size ({r['refused']}): the lines one feed completes, plus one, times nfft exceed 2^25")
        elif r["label"] == "R = 1":
            lines.append(f"R = 1, one run: {r['hbm_ms']} ms/step HBM, {r['pinned_ms']} pinned, kernel {r['kernel_ms']} ms/feed, ring_lines {r.get('ring_lines')}")
    if stopped:
        lines.append("(a run failed or ran into its time limit: the table is incomplete)")
    if args.ratios and os.path.exists(args.ratios):
        found = re.findall(r"specgram bound ratios? (.*?): (.*)", open(args.ratios, errors="replace").read())
        worst = (0.0, "")
        for label, rest in found:
            for v in re.findall(r"([0-9]+\.[0-9]+)", rest):
                worst = max(worst, (float(v), label))
        if found:
            lines.append("")
            lines.append(f"error bounds of tests/test_gpu_specgram.py: worst share reached over {len(found)} checks {worst[0]:.4f} ({worst[1]})")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
