"""What the burst capture costs, on ONE GPU box: config4 (256 channels, 16 s: the bench workload's step) is synthesised once, then
every case runs in a process of its own, under a time limit, and reports ms per step with the block resident in HBM
(vdl2hip_feed_device) and fed from page-locked host memory (vdl2hip_feed_pinned), six feeds in flight, profiling off:

  (a) parent        the parent commit's library (parent=path/to/lib.so): it has no capture
  (b) off           this build, capture off
  (c) on            capture on, pre 256, post 32, the default pool
  (d) off/32        this build, the first 32 channels of the plan as a shard, capture off
  (e) on/32         the same shard, capture on

(a) and (b) run interleaved, --pairs times each (a fresh process every time); their medians and every run are reported: (b) against (a)
shows what "off" costs, the spread of (a) against itself what a difference means.  (c) and (e) also report kernel_ms per feed - the
summed HIP-event time of the capture's two launches, from a pass of their own at profiling level 2 -, the bursts and IQ pairs per
feed, the bytes the copy must move (8 read and 8 written per pair, 128 per record) and the resulting rate as a share of the 6.3 TB/s
a copy kernel reaches.  In the timed loops the records are read and dropped after every drain, as a consumer would.

  python dev/gpu_capture_rate.py parent=lib.so [--out profiles/capture_rate.txt]"""
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
CASES = {"off": (256, False), "on": (256, True), "off/32": (32, False), "on/32": (32, True)}
HBM_ACHIEVABLE = 6.3e12


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
    nchan, on = CASES[args.case]
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, vdl2hip.FMT_S16LE, cfg.rx_max_ppm, max_block_bytes=nbytes,
                          chan_first=0, chan_count=0 if nchan == len(cfg.freqs) else nchan)
    take = None
    if on:
        import ctypes as C
        rx.capture_enable()
        recs = np.zeros(1 << 14, dtype=vdl2hip.BURST_DTYPE)
        iq = np.zeros((1 << 21, 2), dtype=np.float32)

        def take():                                 # (the records and their IQ handed over and dropped: no Python per record)
            while rx.L.vdl2hip_capture_read(rx.h, recs.ctypes.data, recs.size, iq.ctypes.data, iq.shape[0], C.byref(C.c_size_t(0))) > 0:
                pass
    dev = host.to("cuda:0")
    pin = host.pin_memory()
    del host
    for _ in range(3):                              # (the clocks come up; the first block of an idle receiver is not timed)
        rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed()
    res = {"name": args.name, "case": args.case, "MB_per_step": round(nbytes / 1e6, 1)}
    res["hbm_ms"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG, take)
    res["pinned_ms"] = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG, take)
    if on:
        rx.sync(); take()
        rx.set_profiling(2)
        a0 = rx.capture_info()
        for _ in range(args.steps):
            rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed(); take()
        rx.sync(); take()
        a1 = rx.capture_info()
        res["kernel_ms"] = round((a1["kernel_ms"] - a0["kernel_ms"]) / args.steps, 4)
        res["bursts_per_step"] = int(a1["bursts"] - a0["bursts"]) // args.steps
        res["pairs_per_step"] = int(a1["iq_samples"] - a0["iq_samples"]) // args.steps
        res["dropped_per_step"] = int(a1["iq_dropped"] - a0["iq_dropped"]) // args.steps
        res["bytes_per_step"] = 16 * res["pairs_per_step"] + 128 * res["bursts_per_step"]
        rx.set_profiling(0)
    res["fallbacks"] = rx.stats()["front_sync_timeouts"]
    rx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="parent=path/to/lib.so: the parent commit's build, for case (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_rate.txt"))
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
    capture(args.duration)
    libs = dict(s.partition("=")[::2] for s in args.libs)
    parent = libs.pop("parent", None)
    if not parent or not os.path.exists(parent):
        # (b) against (a) is what the record is for: without the parent's library only a scratch file is written
        print("WARNING: no parent=path/to/lib.so (or it does not exist): case (a) cannot run, and (b) has nothing to be held against", flush=True)
        if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "capture_rate.txt"):
            sys.exit("refusing to write the record profiles/capture_rate.txt without case (a): name the parent commit's build, or another --out")
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
             f"median of {args.repeats} x {args.steps} steps in each",
             f"{'case':<28} {'runs':>5} {'MB/step':>8} {'ms/step HBM':>12} {'ms/step pinned':>15} {'capture kernel ms/feed':>23} {'MB moved/feed':>14} {'share of 6.3 TB/s':>18}"]
    table = [("(a) parent", "parent", "off"), ("(b) capture off", "in-tree", "off"), ("(c) on, pre 256 post 32", "in-tree", "on"),
             ("(d) 32-channel shard, off", "in-tree", "off/32"), ("(e) 32-channel shard, on", "in-tree", "on/32")]
    for label, name, case in table:
        sel = [r for r in rows if r["name"] == name and r["case"] == case]
        if not sel:
            continue
        hbm, pin = statistics.median(r["hbm_ms"] for r in sel), statistics.median(r["pinned_ms"] for r in sel)
        km, mb, share = sel[0].get("kernel_ms", ""), "", ""
        if km:
            mb = round(sel[0]["bytes_per_step"] / 1e6, 2)
            share = round(sel[0]["bytes_per_step"] / (km * 1e-3) / HBM_ACHIEVABLE, 3)
        lines.append(f"{label:<28} {len(sel):>5} {sel[0]['MB_per_step']:>8} {hbm:>12.3f} {pin:>15.3f} {km:>23} {mb:>14} {share:>18}")
        if len(sel) > 1:
            h, q = [r["hbm_ms"] for r in sel], [r["pinned_ms"] for r in sel]
            lines.append(f"{'':<28} each run, HBM: {' '.join(map(str, h))} (spread {max(h) - min(h):.3f}); pinned: {' '.join(map(str, q))} (spread {max(q) - min(q):.3f})")
        if km:
            lines.append(f"{'':<28} bursts per feed {sel[0]['bursts_per_step']}, IQ pairs per feed {sel[0]['pairs_per_step']}, windows without room per feed {sel[0]['dropped_per_step']}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
