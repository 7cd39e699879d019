"""What the transmission capture costs, on ONE GPU box, in the style of dev/gpu_txsearch_rate.py (whose capture and timing loop it
shares through dev/gpu_activity_rate.py): config4 (256 channels, 16 s: the bench workload's step) is synthesised once, then every case
runs in a process of its own, under a time limit, and reports ms per step with the block resident in HBM and fed from page-locked
host memory, six feeds in flight, profiling off:

  (a) parent        the parent commit's library (parent=path/to/lib.so): it has no capture; nothing enabled
  (b) off           this build, nothing enabled: the capture off, and the log and the activity monitor with it
  (c) log           activity monitor (bins of 105, -50 dBFS, hang 2) and transmission log on
  (d) iq            the same with the capture on, IQ only (pre 256, post 105)
  (e) spectrum      ... spectrum only (256 bins, Hann)
  (f) both          ... both

(a) and (b) run interleaved, --pairs times each (a fresh process every time): (b) against (a) shows what "off" costs, the spread of
(a) against itself what a difference means.  (d) .. (f) also report vdl2hip_txcap_info.kernel_ms per feed, from a pass of their own
at profiling level 2, the records, the pairs and the spectra per feed and what found no room.

  python dev/gpu_txcap_rate.py parent=lib.so [--out profiles/txcap_rate.txt]"""
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
# case -> (log on, capture: None or (iq, spectrum))
CASES = {"off": (False, None), "log": (True, None), "iq": (True, (True, False)), "spectrum": (True, (False, True)), "both": (True, (True, True))}


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    capture(args.duration)
    cfg = workloads.config4(args.duration)
    host = torch.from_numpy(np.load(CAPTURE + f"_{args.duration:g}.npy"))
    nbytes = host.numel() * host.element_size()
    log, cap = CASES[args.case]
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vdl2hip.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=nbytes)
    if log:
        rx.activity_enable(105, THR, HANG)
        rx.txlog_enable()
    if cap:
        rx.txcap_enable(iq=cap[0], spectrum=cap[1], pre=256, post=105)
    dev = host.to("cuda:0")
    pin = host.pin_memory()
    del host
    recs = np.zeros(1 << 16, dtype=vdl2hip.TXC_DTYPE) if cap else None
    iq = np.zeros((1 << 22, 2), dtype=np.float32) if cap else None
    sp = np.zeros(1 << 20, dtype=np.float32) if cap else None

    def drop():
        rx.drain_packed()
        if log:
            rx.txlog_read()
        while cap and rx.L.vdl2hip_txcap_read(rx.h, recs.ctypes.data, recs.size, iq.ctypes.data, iq.shape[0], None, sp.ctypes.data, sp.size, None) > 0:
            pass
    for _ in range(3):                              # (the clocks come up; the first block of an idle receiver is not timed)
        rx.feed_device(dev.data_ptr(), nbytes); drop()
    res = {"name": args.name, "case": args.case, "MB_per_step": round(nbytes / 1e6, 1)}
    res["hbm_ms"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    drop()
    res["pinned_ms"] = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
    rx.sync()
    drop()
    if cap:
        rx.set_profiling(2)
        t0, s0 = rx.txlog_info(), rx.txcap_info()
        for _ in range(args.steps):
            rx.feed_device(dev.data_ptr(), nbytes); drop()
        rx.sync()
        t1, s1 = rx.txlog_info(), rx.txcap_info()
        drop()
        per = lambda a, b, k: round((b[k] - a[k]) / args.steps, 1)
        res["txlog_kernel_ms"] = round((t1["kernel_ms"] - t0["kernel_ms"]) / args.steps, 4)
        res["txcap_kernel_ms"] = round((s1["kernel_ms"] - s0["kernel_ms"]) / args.steps, 4)
        res["records_per_step"] = per(s0, s1, "records")
        res["pairs_per_step"] = per(s0, s1, "iq_samples")
        res["spectra_per_step"] = per(s0, s1, "spectra")
        res["iq_dropped_per_step"] = per(s0, s1, "iq_dropped")
        res["spectra_dropped_per_step"] = per(s0, s1, "spectra_dropped")
        rx.set_profiling(0)
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txcap_rate.txt"))
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
        if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "txcap_rate.txt"):
            sys.exit("refusing to write the record profiles/txcap_rate.txt without case (a): name the parent commit's build, or another --out")
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
             f"median of {args.repeats} x {args.steps} steps in each; (c) .. (f): activity monitor with bins of 105 samples, {THR:g} dBFS, hang {HANG}; "
             "capture: pre 256, post 105, 256 bins, pools at their defaults",
             f"{'case':<34} {'runs':>5} {'ms/step HBM':>12} {'ms/step pinned':>15} {'log kernel ms/feed':>19} {'capture kernel ms/feed':>23} {'records/feed':>13} {'pairs/feed':>12} {'spectra/feed':>13}"]
    table = [("(a) parent", "parent", "off"), ("(b) capture off (nothing enabled)", "in-tree", "off"), ("(c) monitor and log on", "in-tree", "log"),
             ("(d) ... and capture, IQ only", "in-tree", "iq"), ("(e) ... and capture, spectrum only", "in-tree", "spectrum"), ("(f) ... and capture, both", "in-tree", "both")]
    for label, name, case in table:
        sel = [r for r in rows if r["name"] == name and r["case"] == case]
        if not sel:
            continue
        hbm, pin = statistics.median(r["hbm_ms"] for r in sel), statistics.median(r["pinned_ms"] for r in sel)
        lines.append(f"{label:<34} {len(sel):>5} {hbm:>12.3f} {pin:>15.3f} {sel[0].get('txlog_kernel_ms', ''):>19} {sel[0].get('txcap_kernel_ms', ''):>23} "
                     f"{sel[0].get('records_per_step', ''):>13} {sel[0].get('pairs_per_step', ''):>12} {sel[0].get('spectra_per_step', ''):>13}")
        if len(sel) > 1:
            h, q = [r["hbm_ms"] for r in sel], [r["pinned_ms"] for r in sel]
            lines.append(f"{'':<34} each run, HBM: {' '.join(map(str, h))} (spread {max(h) - min(h):.3f}); pinned: {' '.join(map(str, q))} (spread {max(q) - min(q):.3f})")
        if "iq_dropped_per_step" in sel[0]:
            lines.append(f"{'':<34} per feed without room: windows {sel[0]['iq_dropped_per_step']}, spectra {sel[0]['spectra_dropped_per_step']}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
