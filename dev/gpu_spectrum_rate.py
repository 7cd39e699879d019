"""What the input monitor costs, on ONE GPU box: config4 (256 channels, 16 s) is synthesised once, then every case runs in a process
of its own, under a time limit, and reports ms per step with the block resident in HBM (vdl2hip_feed_device) and fed from
page-locked host memory (vdl2hip_feed_pinned), six feeds in flight, profiling off:

  (a) parent        the parent commit's library, where one is named (parent=path/to/lib.so): it has no monitor
  (b) off           this build, monitor off
  (c) 1024/1        monitor on, nfft 1024, every segment
  (d) 4096/1        nfft 4096, every segment
  (e) 1024/16       nfft 1024, every 16th segment

(a) and (b) run interleaved, --pairs times each (a fresh process every time), and their medians are reported: (b) against (a) shows
what "off" costs.  (c) - (e) also report kernel_ms per feed: the summed HIP-event time of the monitor's two launches, from a pass of
their own at profiling level 2.  Any other name=path/to/lib.so is a variant build of this tree: it runs (c) - (e) right after the
in-tree library and gets rows of its own.  With --ratios FILE the worst share of the float32 error bound the kernel reached in
tests/test_gpu_spectrum.py (the lines that file prints) is quoted underneath.

  python dev/gpu_spectrum_rate.py [--out profiles/spectrum_rate.txt] [parent=lib.so] [name=variant.so ...]"""
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
CASES = {"off": None, "1024/1": (1024, 1), "4096/1": (4096, 1), "1024/16": (1024, 16)}


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
    mon = CASES[args.case]
    if mon:
        rx.spectrum_enable(mon[0], vdl2hip.WIN_HANN, mon[1])
    dev = host.to("cuda:0")
    pin = host.pin_memory()
    del host
    for _ in range(3):                              # (the clocks come up; the first block of an idle receiver is not timed)
        rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed()
    res = {"name": args.name, "case": args.case, "MB_per_step": round(nbytes / 1e6, 1)}
    res["hbm_ms"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    res["pinned_ms"] = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    if mon:
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
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a); name=path: a variant build, for (c) - (e)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_rate.txt"))
    ap.add_argument("--ratios", default=None, help="output of tests/test_gpu_spectrum.py run with -s: its 'spectrum bound ratio' lines")
    ap.add_argument("--duration", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--name", default="in-tree")
    ap.add_argument("--case", default="off", choices=list(CASES))
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
    missing = [v for v in libs.values() if not os.path.exists(v)]
    if missing:
        sys.exit(f"no such library: {missing}")
    if not parent or not os.path.exists(parent):
        # (b) against (a) is what the record is for: without the parent's library only a scratch file is written
        print("WARNING: no parent=path/to/lib.so (or it does not exist): case (a) cannot run, and (b) has nothing to be held against", flush=True)
        if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "spectrum_rate.txt"):
            sys.exit("refusing to write the record profiles/spectrum_rate.txt without case (a): name the parent commit's build, or another --out")
        parent = None
    plan = []
    for _ in range(args.pairs):
        if parent:
            plan.append(("parent", parent, "off"))
        plan.append(("in-tree", "", "off"))
    for c in CASES:
        if c != "off":
            plan += [("in-tree", "", c)] + [(name, lib, c) for name, lib in libs.items()]
    rows = []
    for name, lib, case in plan:
        env = dict(os.environ)
        if lib:
            env["VDL2HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--name", name, "--case", case, "--duration", str(args.duration),
               "--steps", str(args.steps), "--repeats", str(args.repeats)]
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{name} {case}: TIMEOUT - nothing more is started", flush=True)
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            print(f"{name} {case}: FAILED rc={p.returncode} - nothing more is started\n{p.stderr[-1500:]}", flush=True)
            break
        rows.append(json.loads(line[-1]))
        print(line[-1], flush=True)
    lines = [f"config4: 256 channels, {args.duration:g} s per step (int16), profiling off, six feeds in flight; a fresh process per run, "
             f"median of {args.repeats} x {args.steps} steps in each",
             f"{'case':<22} {'runs':>5} {'MB/step':>8} {'ms/step HBM':>12} {'ms/step pinned':>15} {'monitor kernel ms/feed':>23} {'segments/feed':>14}"]
    table = [("(a) parent", "parent", "off"), ("(b) monitor off", "in-tree", "off")]
    for tag, text, case in (("(c)", "nfft 1024 stride 1", "1024/1"), ("(d)", "nfft 4096 stride 1", "4096/1"), ("(e)", "nfft 1024 stride 16", "1024/16")):
        table += [(f"{tag} {text}", "in-tree", case)] + [(f"{tag} {name}", name, case) for name in libs]
    for label, name, case in table:
        sel = [r for r in rows if r["name"] == name and r["case"] == case]
        if not sel:
            continue
        hbm, pin = statistics.median(r["hbm_ms"] for r in sel), statistics.median(r["pinned_ms"] for r in sel)
        km = sel[0].get("kernel_ms", "")
        lines.append(f"{label:<22} {len(sel):>5} {sel[0]['MB_per_step']:>8} {hbm:>12.3f} {pin:>15.3f} {km:>23} {sel[0].get('segments_per_step', ''):>14}")
        if len(sel) > 1:
            lines.append(f"{'':<22} each run, HBM: {' '.join(str(r['hbm_ms']) for r in sel)}; pinned: {' '.join(str(r['pinned_ms']) for r in sel)}")
    if args.ratios and os.path.exists(args.ratios):
        found = re.findall(r"spectrum bound ratio (.*?) nfft=(\d+): ([0-9.]+)", open(args.ratios, errors="replace").read())
        if found:
            worst = max(found, key=lambda m: float(m[2]))
            lines.append("")
            lines.append(f"float32 error bound of tests/test_gpu_spectrum.py (eps = log2(N) 2^-24): worst share reached over {len(found)} checks "
                         f"{float(worst[2]):.4f} ({worst[0]}, nfft {worst[1]})")
            byn = {}
            for lab, n, v in found:
                if lab.startswith("definition"):
                    byn[int(n)] = max(byn.get(int(n), 0.0), float(v))
            lines.append("  the definition test, by nfft: " + ", ".join(f"{n}: {v:.4f}" for n, v in sorted(byn.items())))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
