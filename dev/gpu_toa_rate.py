"""What burst timing costs, on ONE GPU box: config4 (256 channels, 16 s: the bench workload's step) is synthesised once, then every
case runs in a process of its own, under a time limit, and reports ms per step with the block resident in HBM (vdl2hip_feed_device)
and fed from page-locked host memory (vdl2hip_feed_pinned), six feeds in flight, profiling off:

  (a) parent     the parent commit's library (parent=path/to/lib.so): it has no such tap - optional
  (b) off        this build, the tap off
  (c) on         the tap on, max_lag 8, the default pool of curves
  (d) on, W=32   the tap on, max_lag 32

(a), (b) and (c) alternate, --pairs times each (a fresh process every time); their medians and every run are reported: the spread of
a case against itself says what a difference means.  (c) and (d) also report kernel_ms per feed - the summed HIP-event time of k_toa,
from a pass of their own at profiling level 2 - the bursts per feed, and the resulting time per burst.  In the timed loops the records
are read and dropped after every drain, as a consumer would.

  python dev/gpu_toa_rate.py [parent=lib.so] [--out profiles/toa_rate.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPTURE = "/tmp/vdl2_spectrum_rate_config4"          # (the input monitor's rate script synthesises the same capture)
CASES = {"off": None, "on": 8, "on32": 32}


def run(rx, feed, steps, repeats, lag, take=None):
    times = []
    for _ in range(repeats):
        rx.set_drain_lag(lag)
        t0 = time.perf_counter()
        for _ in range(steps):
            feed()
            rx.drain_packed()
            if take:
                take()
        rx.set_drain_lag(0)
        rx.drain_packed()
        if take:
            take()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    return round(statistics.median(times), 3)


def capture(duration):
    """the synthesised block, made once and kept"""
    import numpy as np
    from dumpvdl2_amd import synth, workloads
    path = CAPTURE + f"_{duration:g}.npy"
    if not os.path.exists(path):
        t0 = time.time()
        iq, _ = synth.synthesize(workloads.config4(duration), workers=8)
        np.save(path, iq)
        print(f"# capture ready ({time.time() - t0:.0f} s)", flush=True)


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    capture(args.duration)                          # (a child run on its own, under a profiler for instance)
    cfg = workloads.config4(args.duration)
    host = torch.from_numpy(np.load(CAPTURE + f"_{args.duration:g}.npy"))
    nbytes = host.numel() * host.element_size()
    W = CASES[args.case]
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vdl2hip.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=nbytes)
    take = None
    if W:
        import ctypes as C
        rx.toa_enable(max_lag=W)
        recs = np.zeros(1 << 14, dtype=vdl2hip.BURST_TOA_DTYPE)
        cv = np.zeros(1 << 20, dtype=np.float32)

        def take():                                 # (the records and their curves handed over and dropped: no Python per record)
            while rx.L.vdl2hip_toa_read(rx.h, recs.ctypes.data, recs.size, cv.ctypes.data, cv.size, C.byref(C.c_size_t(0))) > 0:
                pass
    dev = host.to("cuda:0")
    pin = host.pin_memory()
    del host
    for _ in range(3):                              # (the clocks come up; the first block of an idle receiver is not timed)
        rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed()
    res = {"name": args.name, "case": args.case, "MB_per_step": round(nbytes / 1e6, 1)}
    res["hbm_ms"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG, take)
    res["pinned_ms"] = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG, take)
    if W:
        rx.sync(); take()
        rx.set_profiling(2)
        a0 = rx.toa_info()
        for _ in range(args.steps):
            rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed(); take()
        rx.sync(); take()
        a1 = rx.toa_info()
        res["kernel_ms"] = round((a1["kernel_ms"] - a0["kernel_ms"]) / args.steps, 4)
        res["bursts_per_step"] = int(a1["bursts"] - a0["bursts"]) // args.steps
        res["curves_per_step"] = int(a1["curves"] - a0["curves"]) // args.steps
        res["edge_per_step"] = int(a1["edge"] - a0["edge"]) // args.steps
        rx.set_profiling(0)
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "toa_rate.txt"))
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
    if parent and not os.path.exists(parent):
        sys.exit(f"{parent}: no such library")
    plan = []
    for _ in range(args.pairs):
        if parent:
            plan.append(("parent", parent, "off"))
        plan.append(("in-tree", "", "off"))
        plan.append(("in-tree", "", "on"))
    plan.append(("in-tree", "", "on32"))
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
             f"{'case':<24} {'runs':>5} {'MB/step':>8} {'ms/step HBM':>12} {'ms/step pinned':>15} {'k_toa ms/feed':>14} {'bursts/feed':>12} {'us/burst':>9}"]
    table = [("(a) parent", "parent", "off"), ("(b) tap off", "in-tree", "off"), ("(c) on, max_lag 8", "in-tree", "on"), ("(d) on, max_lag 32", "in-tree", "on32")]
    for label, name, case in table:
        sel = [r for r in rows if r["name"] == name and r["case"] == case]
        if not sel:
            continue
        hbm, pin = statistics.median(r["hbm_ms"] for r in sel), statistics.median(r["pinned_ms"] for r in sel)
        km, nb, per = sel[0].get("kernel_ms", ""), sel[0].get("bursts_per_step", ""), ""
        if km and nb:
            per = round(km * 1e3 / nb, 3)
        lines.append(f"{label:<24} {len(sel):>5} {sel[0]['MB_per_step']:>8} {hbm:>12.3f} {pin:>15.3f} {km:>14} {nb:>12} {per:>9}")
        if len(sel) > 1:
            h, q = [r["hbm_ms"] for r in sel], [r["pinned_ms"] for r in sel]
            lines.append(f"{'':<24} each run, HBM: {' '.join(map(str, h))} (spread {max(h) - min(h):.3f}); pinned: {' '.join(map(str, q))} (spread {max(q) - min(q):.3f})")
        if km:
            lines.append(f"{'':<24} curves per feed {sel[0]['curves_per_step']}, records with the peak at the edge per feed {sel[0]['edge_per_step']}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
