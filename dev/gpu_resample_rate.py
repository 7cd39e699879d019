"""What the resampler in front of the channeliser costs, on ONE GPU box: config4 (256 channels, 16 s at 2.1 MS/s) is synthesised once,
rendered at 2.5 MS/s (on the GPU, by a windowed-sinc interpolator of this script: 64 taps, 100 dB) as cs16 and as cf32, and a receiver
created with input_rate = 2500000 runs over each rendering, block resident in HBM, six feeds in flight:

  k0       k_resample's own time per feed (resample_ms / feeds, profiling level 2)
  k1       k_chanfir's time for the same feeds (chanfir_ms / chanfir_launches, same run)
  step     ms per step at profiling level 1, and frames per step

Beside them the plain 2.1 MS/s receiver's step over the original capture: the in-tree build's and that of every other library named
(the parent commit's, to show what a receiver that does not resample costs before and after).

  python dev/gpu_resample_rate.py [--out profiles/resample_rate.txt] [name=lib.so ...]

(config4's channels reach +-1.02 MHz, beyond the +-0.84 MHz the resampler passes flat at this ratio: the outermost channels come out
up to 6 dB down - still decodable, and of no consequence for the times.)"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPTURE = "/tmp/vdl2_resample_rate_config4"
RATE_IN, RATE_OUT = 2500000, 2100000


def render_gpu(torch, x, fs_in, fs_out, half=32, beta=10.06):
    """complex64 cuda tensor at fs_in -> at fs_out (fs_out > fs_in): y[m] = sum_k x[k] g(m fs_in / fs_out - k), Kaiser-windowed sinc"""
    g = math.gcd(fs_in, fs_out)
    P, Q = fs_out // g, fs_in // g
    W = half
    nout = x.numel() * P // Q
    m = torch.arange(nout, device=x.device, dtype=torch.int64)
    k0, ph = (m * Q) // P, (m * Q) % P
    del m
    xp = torch.cat([torch.zeros(W, dtype=x.dtype, device=x.device), x, torch.zeros(W + 1, dtype=x.dtype, device=x.device)])
    y = torch.zeros(nout, dtype=torch.complex64, device=x.device)
    frac = torch.arange(P, dtype=torch.float64) / P
    i0b = float(torch.special.i0(torch.tensor(beta, dtype=torch.float64)))
    for i in range(-W + 1, W + 1):
        d = frac - i
        u = d / W
        w = torch.where(u.abs() < 1.0, torch.special.i0(beta * torch.sqrt(torch.clamp(1.0 - u * u, min=0.0))) / i0b, torch.zeros_like(u))
        tap = (0.9 * torch.sinc(0.9 * d) * w).to(torch.float32).to(x.device)
        y += xp[k0 + (i + W)] * tap[ph]
    return y


def run(rx, feed, steps, repeats, lag):
    times, k0, k1, frames = [], [], [], 0
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
        k0.append((s1.get("resample_ms", 0.0) - s0.get("resample_ms", 0.0)) / steps)
        assert s1["overflow_feeds"] == s0["overflow_feeds"]
        frames = n / steps
    return round(statistics.median(times), 3), round(statistics.median(k0), 4), round(statistics.median(k1), 4), frames


def child(args):
    import numpy as np
    import torch
    from dumpvdl2_amd import vdl2hip, workloads
    vdl2hip.load_library()
    cfg = workloads.config4(args.duration)
    iq = np.load(CAPTURE + f"_{args.duration:g}.npy")
    res = {"name": args.name}
    lag = vdl2hip.MAX_DRAIN_LAG

    def measure(rx, dev, nbytes, resampling):
        for _ in range(3):                          # (the clocks come up; the first block of an idle receiver is not timed)
            rx.feed_device(dev.data_ptr(), nbytes); rx.drain_packed()
        r = {"MB_per_step": round(nbytes / 1e6, 1)}
        rx.set_profiling(1)
        r["step_ms"], _, r["k1_ms"], r["frames"] = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, lag)
        if resampling:
            rx.set_profiling(2)
            _, r["k0_ms"], r["k1_level2_ms"], _ = run(rx, lambda: rx.feed_device(dev.data_ptr(), nbytes), args.steps, args.repeats, lag)
        r["fallbacks"] = rx.stats()["front_sync_timeouts"]
        return r

    host = torch.from_numpy(iq)
    nbytes = host.numel() * host.element_size()
    rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, 1, cfg.rx_max_ppm, max_block_bytes=nbytes)
    dev = host.to("cuda:0")
    res["plain"] = measure(rx, dev, nbytes, False)
    rx.close()
    if args.name == "in-tree":
        x = torch.view_as_complex((dev.to(torch.float32) / 32768.0).reshape(-1, 2))
        del dev
        z = render_gpu(torch, x, RATE_OUT, RATE_IN)
        del x
        for label, fmt in (("cs16", 1), ("cf32", 2)):
            zr = torch.view_as_real(z)
            d = torch.clamp(torch.round(zr * 32768.0), -32768, 32767).to(torch.int16).contiguous() if fmt == 1 else zr.contiguous()
            nb = d.numel() * d.element_size()
            rx = vdl2hip.Receiver(cfg.centerfreq, list(cfg.freqs), cfg.oversample, fmt, cfg.rx_max_ppm, max_block_bytes=nb, input_rate=RATE_IN)
            res[label] = measure(rx, d, nb, True)
            rx.close()
            del d
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="name=path/to/lib.so: other builds, for the plain receiver's step (the in-tree build always runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_rate.txt"))
    ap.add_argument("--duration", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
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
    for spec in ["in-tree="] + list(args.libs):
        name, _, lib = spec.partition("=")
        env = dict(os.environ)
        if lib:
            env["VDL2HIP_LIB"] = os.path.abspath(lib)
            env["VDL2HIP_LIB_ANY_ABI"] = "1"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--name", name, "--duration", str(args.duration), "--steps", str(args.steps), "--repeats", str(args.repeats)]
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: TIMEOUT - nothing more is started", flush=True)
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            print(f"{name}: FAILED rc={p.returncode} - nothing more is started\n{p.stderr[-1500:]}", flush=True)
            break
        rows.append(json.loads(line[-1]))
        print(line[-1], flush=True)
    head = f"{'build':<12} {'input':<22} {'MB/step':>8} {'k_resample ms/feed':>19} {'k_chanfir ms/launch':>20} {'k0 / k1':>8} {'ms/step':>9} {'frames/step':>12}"
    lines = [f"config4: 256 channels, {args.duration:g} s per step, block resident in HBM, six feeds in flight; medians of {args.repeats} x {args.steps} steps.",
             "ms/step, frames/step and the plain rows' k_chanfir at profiling level 1; k_resample and the k_chanfir beside it at level 2 (every stage timed).", head]
    for r in rows:
        for label, what in (("plain", "2.1 MS/s cs16"), ("cs16", "2.5 -> 2.1 MS/s cs16"), ("cf32", "2.5 -> 2.1 MS/s cf32")):
            v = r.get(label)
            if not v:
                continue
            if "k0_ms" in v:
                lines.append(f"{r['name']:<12} {what:<22} {v['MB_per_step']:>8} {v['k0_ms']:>19} {v['k1_level2_ms']:>20} {v['k0_ms'] / v['k1_level2_ms']:>8.3f} {v['step_ms']:>9} {v['frames']:>12.1f}")
            else:
                lines.append(f"{r['name']:<12} {what:<22} {v['MB_per_step']:>8} {'-':>19} {v['k1_ms']:>20} {'-':>8} {v['step_ms']:>9} {v['frames']:>12.1f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
