"""What the transmission log costs, on ONE GPU box, in the style of dev/gpu_activity_rate.py (whose capture and timing loop it uses):
config4 (256 channels, 16 s: the bench workload's step) is synthesised once, then every case runs in a process of its own, under a
time limit, and reports ms per step with the block resident in HBM and fed from page-locked host memory, six feeds in flight,
profiling off:

  (a) parent        the parent commit's library (parent=path/to/lib.so): it has no log; activity monitor on (bins of 105, -40 dBFS)
  (b) off           this build, activity monitor on, log off
  (c) on            activity monitor and log on
  (d) on, -60 dBFS  the same with the threshold near the noise: many more transmissions close per feed
  (e) off/32        this build, the first 32 channels of the plan as a shard, activity monitor on, log off
  (f) on/32         the same shard, log on

(a) and (b) run interleaved, --pairs times each (a fresh process every time): (b) against (a) shows what "off" costs, the spread of
(a) against itself what a difference means.  The cases with the monitor on also report kernel_ms per feed of the activity monitor's
two launches and, beside it, of the log's two, from a pass of their own at profiling level 2, and the records logged per feed.

  python dev/gpu_txlog_rate.py parent=lib.so [--out profiles/txlog_rate.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_activity_rate import CAPTURE, capture, run  # noqa: E402

# case -> (channels, log on, threshold dBFS)
CASES = {"off": (256, False, -40.0), "on": (256, True, -40.0), "on-60": (256, True, -60.0), "off/32": (32, False, -40.0), "on/32": (32, True, -40.0)}


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    capture(args.duration)
    cfg = workloads.config4(args.duration)
    host = torch.from_numpy(np.load(CAPTURE + f"_{args.duration:g}.npy"))
    nbytes = host.numel() * host.element_size()
    nchan, log, thr = CASES[args.case]
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vdl2hip.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=nbytes,
                          chan_first=0, chan_count=0 if nchan == len(cfg.freqs) else nchan)
    rx.activity_enable(105, thr)
    if log:
        rx.txlog_enable()
    dev = host.to("cuda:0")
    pin = host.pin_memory()
    del host

    def drop():
        rx.drain_packed()
        if log:
            rx.txlog_read()
    for _ in range(3):                              # (the clocks come up; the first block of an idle receiver is not timed)
        rx.feed_device(dev.data_ptr(), nbytes); drop()
    res = {"name": args.name, "case": args.case, "MB_per_step": round(nbytes / 1e6, 1)}
    res["hbm_ms"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    if log:
        rx.txlog_read()
    res["pinned_ms"] = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    rx.sync()
    rx.set_profiling(2)
    a0 = rx.activity()
    t0 = rx.txlog_info() if log else None
    for _ in range(args.steps):
        rx.feed_device(dev.data_ptr(), nbytes); drop()
    rx.sync()
    a1 = rx.activity()
    res["activity_kernel_ms"] = round((a1["kernel_ms"] - a0["kernel_ms"]) / args.steps, 4)
    if log:
        t1 = rx.txlog_info()
        res["txlog_kernel_ms"] = round((t1["kernel_ms"] - t0["kernel_ms"]) / args.steps, 4)
        res["records_per_step"] = round((t1["transmissions"] - t0["transmissions"]) / args.steps, 1)
        res["dropped"] = int(t1["dropped"])
        res["frames_matched"], res["frames_unmatched"] = int(t1["frames_matched"]), int(t1["frames_unmatched"])
    rx.set_profiling(0)
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txlog_rate.txt"))
    ap.add_argument("--duration", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--name", default="in-tree")
    ap.add_argument("--case", default="off", choices=list(CASES))
    args = ap.parse_args()
    if args.child:
        return child(args)
    capture(args.duration)
    libs = dict(s.partition("=")[::2] for s in args.libs)
    parent = libs.pop("parent", None)
    if not parent or not os.path.exists(parent):
        print("WARNING: no parent=path/to/lib.so (or it does not exist): case (a) cannot run, and (b) has nothing to be held against", flush=True)
        if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "txlog_rate.txt"):
            sys.exit("refusing to write the record profiles/txlog_rate.txt without case (a): name the parent commit's build, or another --out")
        parent = None
    plan = []
    for _ in range(args.pairs):
        if parent:
            plan.append(("parent", parent, "off"))
        plan.append(("in-tree", "", "off"))
    plan += [("in-tree", "", c) for c in CASES if c != "off"]
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
             f"median of {args.repeats} x {args.steps} steps in each; activity monitor on in every case (bins of 105 samples)",
             f"{'case':<34} {'runs':>5} {'ms/step HBM':>12} {'ms/step pinned':>15} {'activity kernel ms/feed':>24} {'log kernel ms/feed':>19} {'records/feed':>13}"]
    table = [("(a) parent", "parent", "off"), ("(b) log off", "in-tree", "off"), ("(c) log on, -40 dBFS", "in-tree", "on"),
             ("(d) log on, -60 dBFS", "in-tree", "on-60"), ("(e) 32-channel shard, log off", "in-tree", "off/32"), ("(f) 32-channel shard, log on", "in-tree", "on/32")]
    for label, name, case in table:
        sel = [r for r in rows if r["name"] == name and r["case"] == case]
        if not sel:
            continue
        hbm, pin = statistics.median(r["hbm_ms"] for r in sel), statistics.median(r["pinned_ms"] for r in sel)
        lines.append(f"{label:<34} {len(sel):>5} {hbm:>12.3f} {pin:>15.3f} {sel[0]['activity_kernel_ms']:>24} {sel[0].get('txlog_kernel_ms', ''):>19} {sel[0].get('records_per_step', ''):>13}")
        if len(sel) > 1:
            h, q = [r["hbm_ms"] for r in sel], [r["pinned_ms"] for r in sel]
            lines.append(f"{'':<34} each run, HBM: {' '.join(map(str, h))} (spread {max(h) - min(h):.3f}); pinned: {' '.join(map(str, q))} (spread {max(q) - min(q):.3f})")
        if "dropped" in sel[0]:
            lines.append(f"{'':<34} records without room {sel[0]['dropped']}, frames matched {sel[0]['frames_matched']}, unmatched {sel[0]['frames_unmatched']}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
