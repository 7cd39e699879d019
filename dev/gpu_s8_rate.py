"""What signed-byte input costs beside unsigned bytes and int16, on ONE GPU box: config4 (256 channels, 16 s) is synthesised once as
int16, raised by GAIN (the capture's amplitude is 0.01 of full scale: eight bits would be +-1 LSB - dev/gpu_u8_rate.py) and rendered as
S16 (k), U8 (k / 256 + 127.5, rounded) and S8 (k / 256, rounded), then every library named - the in-tree build by
default - runs in a process of its own, under a time limit, over the three renderings with profiling level 1 and reports side by side:

  k1      the channeliser's own time per launch (chanfir_ms / chanfir_launches): the median of the repeats, and their range - the
          spread the U8 build shows between repeats is what the S8 build's figure is read against
  hbm     ms per step with the block resident in HBM (vdl2hip_feed_device)
  pinned  ms per step fed from page-locked host memory (vdl2hip_feed_pinned)
  frames  per step, HBM-resident (the byte renderings are coarser samples than the int16 ones: their frames need not be the same)

  python dev/gpu_s8_rate.py [--out profiles/s8_rate.txt] [name=lib.so ...]

A library without the format (the parent commit's, to show that the U8 and S16 paths have not moved) reports its U8 and S16 figures alone."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPTURE = "/tmp/vdl2_s8_rate_config4"
FORMATS = (("u8", 0), ("s16", 1), ("s8", 4))
GAIN = 12.0


def run(rx, feed, steps, repeats, lag):
    times, k1, frames = [], [], 0
    for _ in range(repeats):
        rx.set_drain_lag(lag)
        s0 = rx.stats()
        t0 = time.perf_counter()
        n = 0
        for _ in range(steps):
            feed()
            n += rx.drain_packed()[0]
        rx.set_drain_lag(0)
        n += rx.drain_packed()[0]
        times.append((time.perf_counter() - t0) / steps * 1e3)
        s1 = rx.stats()
        k1.append((s1["chanfir_ms"] - s0["chanfir_ms"]) / max(1, s1["chanfir_launches"] - s0["chanfir_launches"]))
        assert s1["overflow_feeds"] == s0["overflow_feeds"]
        frames = n / steps
    return round(statistics.median(times), 3), [round(x, 4) for x in sorted(k1)], frames


def render(iq, fmt):
    import numpy as np
    k = iq.astype(np.float32) * np.float32(GAIN)
    if fmt == 1:
        return np.clip(k, -32768, 32767).astype(np.int16)
    if fmt == 0:
        return np.clip(np.rint(k / np.float32(256.0) + np.float32(127.5)), 0, 255).astype(np.uint8)
    return np.clip(np.rint(k / np.float32(256.0)), -128, 127).astype(np.int8)


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    cfg = workloads.config4(args.duration)
    iq = np.load(CAPTURE + f"_{args.duration:g}.npy")
    res = {"name": args.name}
    for label, fmt in FORMATS:
        host = torch.from_numpy(render(iq, fmt))
        nbytes = host.numel() * host.element_size()
        try:
            rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, fmt, cfg.rx_max_ppm, max_block_bytes=nbytes)
        except vdl2hip.Vdl2HipError as e:
            res[label] = {"error": str(e)}
            continue
        print(f"# {args.name} {label}: receiver ready", file=sys.stderr, flush=True)
        rx.set_profiling(1)
        dev = host.to("cuda:0")
        pin = host.pin_memory()
        del host
        for _ in range(3):                          # (the clocks come up; the first block of an idle receiver is not timed)
            rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed()
        r = {"MB_per_step": round(nbytes / 1e6, 1)}
        r["hbm_ms"], r["k1_ms"], r["frames"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
        r["pinned_ms"], r["k1_pinned_ms"], _ = run(rx, lambda: rx.feed_pinned(pin.data_ptr(), nbytes), args.steps, args.repeats, vdl2hip.MAX_DRAIN_LAG)
        r["fallbacks"] = rx.stats()["front_sync_timeouts"]
        print(f"# {args.name} {label}: {r}", file=sys.stderr, flush=True)
        res[label] = r
        rx.close()
        del dev, pin
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="name=path/to/lib.so; none: the in-tree build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s8_rate.txt"))
    ap.add_argument("--duration", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--name", default="in-tree")
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
    rows = []
    for spec in args.libs or ["in-tree="]:
        name, _, lib = spec.partition("=")
        env = dict(os.environ)
        if lib:
            env["VDL2HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--name", name, "--duration", str(args.duration), "--steps", str(args.steps), "--repeats", str(args.repeats)]
        try:
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout)      # (its progress lines go where ours go)
        except subprocess.TimeoutExpired:
            print(f"{name}: TIMEOUT - nothing more is started", flush=True)
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            print(f"{name}: FAILED rc={p.returncode} - nothing more is started", flush=True)
            break
        rows.append(json.loads(line[-1]))
        print(line[-1], flush=True)
    head = f"{'build':<16} {'format':<6} {'MB/step':>8} {'chanfir ms/launch':>18} {'(min .. max)':>20} {'ms/step HBM':>12} {'ms/step pinned':>15} {'frames/step':>12}"
    lines = [f"config4: 256 channels, {args.duration:g} s per step, profiling level 1; medians of {args.repeats} x {args.steps} steps, six feeds in flight;",
             "chanfir ms/launch: HBM-resident, the median of the repeats and their range", head]
    for r in rows:
        for label, _ in FORMATS:
            v = r.get(label, {})
            if "error" in v or not v:
                lines.append(f"{r['name']:<16} {label:<6} (not accepted by this build)")
            else:
                k = v["k1_ms"]
                span = f"({k[0]} .. {k[-1]})"
                lines.append(f"{r['name']:<16} {label:<6} {v['MB_per_step']:>8} {statistics.median(k):>18.4f} {span:>20} {v['hbm_ms']:>12} {v['pinned_ms']:>15} {v['frames']:>12.1f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
