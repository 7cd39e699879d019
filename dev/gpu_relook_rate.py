"""What the second look costs, on ONE GPU box, after dev/gpu_txsearch_rate.py (whose capture and timing loop it shares):
config4 (256 channels; --duration seconds a step, 16 by default: the bench workload's step; the record in profiles/ names its own) is synthesised once, then every case runs in a process of its own, under a
time limit, and reports ms per step with the block resident in HBM and fed from page-locked host memory, six feeds in flight,
profiling off:

  (a) parent        the parent commit's library (parent=path/to/lib.so): it has no second look; nothing enabled
  (b) off           this build, nothing enabled: the tap off, and the search, the log and the activity monitor with it
  (c) search        activity monitor (bins of 105, -50 dBFS, hang 2), transmission log and preamble search on
  (d) relook        the same with the second look on (threshold 4, 4 anchors, the default pools)
  (e) relook/room   (d) with pools in which every attempt finds room (pool_frames 2^20, pool_octets 2^24): every attempt is decoded

(a) and (b) run interleaved, --pairs times each (a fresh process every time): (b) against (a) shows what "off" costs, the spread of
(a) against itself what a difference means.  (c) and (d) also report kernel_ms per feed of the search's three launches and of the
second look's three, from a pass of their own at profiling level 2, the records, anchors, attempts and frames per feed.  No cost is
fixed in advance; the condition is only that (b) is (a) within (a)'s own run-to-run spread.

  python dev/gpu_relook_rate.py parent=lib.so [--out profiles/relook_rate.txt]"""
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
# case -> (channels, log and search on, second look on)
CASES = {"off": (256, False, False), "search": (256, True, False), "relook": (256, True, True), "relook/room": (256, True, True)}


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    capture(args.duration)
    cfg = workloads.config4(args.duration)
    host = torch.from_numpy(np.load(CAPTURE + f"_{args.duration:g}.npy"))
    nbytes = host.numel() * host.element_size()
    nchan, log, relook = CASES[args.case]
    search = log
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vdl2hip.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=nbytes,
                          chan_first=0, chan_count=0 if nchan == len(cfg.freqs) else nchan)
    if log:
        rx.activity_enable(105, THR, HANG)
        rx.txlog_enable()
    if search:
        rx.txsearch_enable()
    if relook:
        rx.relook_enable(**(dict(pool_frames=1 << 20, pool_octets=1 << 24) if args.case == "relook/room" else {}))
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
        if relook:
            rx.relook_read()
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
        r0 = rx.relook_info() if relook else None
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
        if relook:
            r1 = rx.relook_info()
            res["relook_kernel_ms"] = round((r1["kernel_ms"] - r0["kernel_ms"]) / args.steps, 4)
            for k in ("anchors_found", "attempts", "frames", "frames_ok", "frames_new", "dropped"):
                res["rl_" + k] = round((r1[k] - r0[k]) / args.steps, 1)
        rx.set_profiling(0)
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relook_rate.txt"))
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
        if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "relook_rate.txt"):
            sys.exit("refusing to write the record profiles/relook_rate.txt without case (a): name the parent commit's build, or another --out")
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
            sys.exit(f"{name} {case}: TIMEOUT - nothing more is started, nothing is written")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            sys.exit(f"{name} {case}: FAILED rc={p.returncode} - nothing more is started, nothing is written\n{p.stderr[-1500:]}")
        rows.append(json.loads(line[-1]))
        print(line[-1], flush=True)
    lines = [f"config4: 256 channels, {args.duration:g} s per step (int16), profiling off, six feeds in flight; a fresh process per run, "
             f"median of {args.repeats} x {args.steps} steps in each; (c), (d): activity monitor with bins of 105 samples, {THR:g} dBFS, hang {HANG}",
             f"{'case':<34} {'runs':>5} {'ms/step HBM':>12} {'ms/step pinned':>15} {'search kernel ms/feed':>22} {'second look kernel ms/feed':>27} {'records/feed':>13}"]
    table = [("(a) parent", "parent", "off"), ("(b) tap off (nothing enabled)", "in-tree", "off"), ("(c) monitor, log and search on", "in-tree", "search"),
             ("(d) the same with the second look", "in-tree", "relook"), ("(e) (d) with room for every attempt", "in-tree", "relook/room")]
    for label, name, case in table:
        sel = [r for r in rows if r["name"] == name and r["case"] == case]
        if not sel:
            continue
        hbm, pin = statistics.median(r["hbm_ms"] for r in sel), statistics.median(r["pinned_ms"] for r in sel)
        lines.append(f"{label:<34} {len(sel):>5} {hbm:>12.3f} {pin:>15.3f} {sel[0].get('txsearch_kernel_ms', ''):>22} {sel[0].get('relook_kernel_ms', ''):>27} "
                     f"{sel[0].get('records_per_step', ''):>13}")
        if "rl_attempts" in sel[0]:
            lines.append(f"{'':<34} per feed: anchors {sel[0]['rl_anchors_found']}, attempts {sel[0]['rl_attempts']}, frames {sel[0]['rl_frames']}, good {sel[0]['rl_frames_ok']}, "
                         f"new {sel[0]['rl_frames_new']}, without room {sel[0]['rl_dropped']}")
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
