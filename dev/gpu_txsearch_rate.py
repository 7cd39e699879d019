"""What the preamble search costs, on ONE GPU box, in the style of dev/gpu_txlog_rate.py (whose capture and timing loop it uses):
config4 (256 channels, 16 s: the bench workload's step) is synthesised once, then every case runs in a process of its own, under a
time limit, and reports ms per step with the block resident in HBM and fed from page-locked host memory, six feeds in flight,
profiling off:

  (a) parent        the parent commit's library (parent=path/to/lib.so): it has no search; nothing enabled
  (b) off           this build, nothing enabled: the search off, and the log and the activity monitor with it
  (c) log           activity monitor (bins of 105, -50 dBFS, hang 2) and transmission log on
  (d) search        the same with the search on
  (e) search/32     (d) on the first 32 channels of the plan as a shard

(a) and (b) run interleaved, --pairs times each (a fresh process every time): (b) against (a) shows what "off" costs, the spread of
(a) against itself what a difference means.  (c) .. (e) also report kernel_ms per feed of the log's two launches and of the search's
three, from a pass of their own at profiling level 2, the records per feed and the samples searched per feed.

  python dev/gpu_txsearch_rate.py parent=lib.so [--out profiles/txsearch_rate.txt]"""
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

THR, HANG = -50.0, 2
# case -> (channels, log on, search on)
CASES = {"off": (256, False, False), "log": (256, True, False), "search": (256, True, True), "search/32": (32, True, True)}


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    capture(args.duration)
    cfg = workloads.config4(args.duration)
    host = torch.from_numpy(np.load(CAPTURE + f"_{args.duration:g}.npy"))
    nbytes = host.numel() * host.element_size()
    nchan, log, search = CASES[args.case]
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vdl2hip.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=nbytes,
                          chan_first=0, chan_count=0 if nchan == len(cfg.freqs) else nchan)
    if log:
        rx.activity_enable(105, THR, HANG)
        rx.txlog_enable()
    if search:
        rx.txsearch_enable()
    dev = host.to("cuda:0")
    pin = host.pin_memory()
    del host

    why = [0, 0, 0, 0]

    def drop():
        rx.drain_packed()
        if log:
            rx.txlog_read()
        if search:
            recs = rx.txsearch_read()
            for w in range(4):
                why[w] += int(np.count_nonzero(recs["why"] == w))
    for _ in range(3):                              # (the clocks come up; the first block of an idle receiver is not timed)
        rx.feed_device(dev.data_ptr(), nbytes); drop()
    res = {"name": args.name, "case": args.case, "MB_per_step": round(nbytes / 1e6, 1)}
    res["hbm_ms"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    drop()
    res["pinned_ms"] = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    rx.sync()
    drop()
    if log:
        rx.set_profiling(2)
        t0, s0 = rx.txlog_info(), rx.txsearch_info() if search else None
        why[:] = [0, 0, 0, 0]
        for _ in range(args.steps):
            rx.feed_device(dev.data_ptr(), nbytes); drop()
        rx.sync()
        t1 = rx.txlog_info()
        res["txlog_kernel_ms"] = round((t1["kernel_ms"] - t0["kernel_ms"]) / args.steps, 4)
        res["records_per_step"] = round((t1["transmissions"] - t0["transmissions"]) / args.steps, 1)
        res["decoded_per_step"] = round((t1["decoded"] - t0["decoded"]) / args.steps, 1)
        res["dropped"] = int(t1["dropped"])
        if search:
            s1 = rx.txsearch_info()
            drop()
            res["txsearch_kernel_ms"] = round((s1["kernel_ms"] - s0["kernel_ms"]) / args.steps, 4)
            res["samples_per_step"] = round((s1["samples_searched"] - s0["samples_searched"]) / args.steps)
            res["clipped"] = int(s1["clipped"])
            res["why"] = [round(w / args.steps, 1) for w in why]
        rx.set_profiling(0)
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txsearch_rate.txt"))
    ap.add_argument("--duration", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=3)
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
        if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "txsearch_rate.txt"):
            sys.exit("refusing to write the record profiles/txsearch_rate.txt without case (a): name the parent commit's build, or another --out")
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
             f"median of {args.repeats} x {args.steps} steps in each; (c) .. (e): activity monitor with bins of 105 samples, {THR:g} dBFS, hang {HANG}",
             f"{'case':<34} {'runs':>5} {'ms/step HBM':>12} {'ms/step pinned':>15} {'log kernel ms/feed':>19} {'search kernel ms/feed':>22} {'records/feed':>13} {'samples searched/feed':>22}"]
    table = [("(a) parent", "parent", "off"), ("(b) search off (nothing enabled)", "in-tree", "off"), ("(c) monitor and log on", "in-tree", "log"),
             ("(d) monitor, log and search on", "in-tree", "search"), ("(e) 32-channel shard, all three on", "in-tree", "search/32")]
    for label, name, case in table:
        sel = [r for r in rows if r["name"] == name and r["case"] == case]
        if not sel:
            continue
        hbm, pin = statistics.median(r["hbm_ms"] for r in sel), statistics.median(r["pinned_ms"] for r in sel)
        lines.append(f"{label:<34} {len(sel):>5} {hbm:>12.3f} {pin:>15.3f} {sel[0].get('txlog_kernel_ms', ''):>19} {sel[0].get('txsearch_kernel_ms', ''):>22} "
                     f"{sel[0].get('records_per_step', ''):>13} {sel[0].get('samples_per_step', ''):>22}")
        if len(sel) > 1:
            h, q = [r["hbm_ms"] for r in sel], [r["pinned_ms"] for r in sel]
            lines.append(f"{'':<34} each run, HBM: {' '.join(map(str, h))} (spread {max(h) - min(h):.3f}); pinned: {' '.join(map(str, q))} (spread {max(q) - min(q):.3f})")
        if "dropped" in sel[0]:
            lines.append(f"{'':<34} records without room {sel[0]['dropped']}, decoded per feed {sel[0]['decoded_per_step']}"
                         + (f", clipped {sel[0]['clipped']}; records per feed by why (decoded, frames bad, lock no frame, no preamble): {sel[0]['why']}" if "why" in sel[0] else ""))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
