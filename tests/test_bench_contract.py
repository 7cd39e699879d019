"""bench.py's JSON line without a GPU: the parts of it that are plain arithmetic - the roofline object of the dominant kernel
(keys and fractions as the measurement contract names them, SURVEY 8.5's per-unit figures) and the PMC traffic entry it quotes
from profiles/pmc_traffic.json - so that an edit of bench.py cannot silently drop a field the driver's line is checked for."""
import importlib.util
import json
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_roofline_object(bench):
    cs = 33_600_000 * 256                       # channel-samples of one 16 s x 256-channel launch
    t = {"k1_ms": 3.8, "k1_chan_samples": cs}
    case = types.SimpleNamespace(count=256, cfg=types.SimpleNamespace(duration_s=16.0))
    tr = bench.pmc_traffic("config4", case)
    assert tr and tr["traffic_bytes"] > 3.4e9 and "profiles/" in tr["source"]          # at least the 3.44 GB of y it stores
    assert bench.pmc_traffic("config4", types.SimpleNamespace(count=32, cfg=case.cfg)) is None      # quoted only where it was measured
    r = bench.roofline_of(t, tr)
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "hbm_algorithmic", "hbm_physical"):
        assert k in r, k
    assert r["unit"] == "TFLOP/s" and r["peak"] == bench.VALU_PEAK_TFLOPS and r["kernel"] == "k_chanfir"
    assert abs(r["achieved"] - cs * 30.0 / 3.8e-3 / 1e12) < 0.01 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # 4 B per channel-sample in + 8 / oversample out
    a = r["hbm_algorithmic"]
    assert a["bytes_per_chan_sample"] == pytest.approx(4.4) and a["bytes_per_launch"] == pytest.approx(cs * 4.4)
    assert a["achieved"] == pytest.approx(cs * 4.4 / 3.8e-3 / 1e9, rel=1e-3) and a["peak"] == 8000.0
    p = r["hbm_physical"]
    assert p["achieved"] == pytest.approx(tr["traffic_bytes"] / 3.8e-3 / 1e9, rel=1e-3) and p["traffic_over_algorithmic"] < 0.2
    json.dumps(r)
    assert bench.roofline_of(t, None)["hbm_physical"] is None


def test_workload_names_are_baseline_configs(bench):
    from dumpvdl2_amd import workloads
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert bench.WORKLOAD_INDEX == {"config2": 1, "config3": 2, "config4": 3, "config5": 4} and len(base["configs"]) == 5
    for name, idx in bench.WORKLOAD_INDEX.items():
        cfg = getattr(workloads, name)(0.1)
        want = {1: 8, 2: 64, 3: 256, 4: 256}[idx]
        assert len(cfg.freqs) == want and str(want) in base["configs"][idx]
        assert cfg.oversample == 20                    # 2.1 MS/s


def _frame(chan, sync, idx, octets):
    """a frame as vdl2hip.Receiver.unpack() returns it"""
    return {"chan": chan, "freq": 136975000 + chan, "idx": idx, "octets": octets, "synd_weight": 0, "datalen_octets": len(octets),
            "num_fec_corrections": 1, "frame_pwr_dbfs": -20.5, "nf_pwr_dbfs": -50.25, "ppm_error": 0.125, "sync_sample": sync,
            "end_sample": sync + 100, "avlc_status": 0, "dst_addr": 7, "src_addr": 9}


def test_dump_frames_layout_and_order(bench, tmp_path):
    """--dump-outputs: one float64 array per frame field, frames ordered by (channel, sync sample, index), octets one after the other as float32"""
    import numpy as np
    frames = [_frame(3, 500, 1, b"\x01\x02"), _frame(1, 900, 0, b"\xff"), _frame(3, 500, 0, b"\x10\x20\x30"), _frame(1, 100, 0, b"")]
    assert bench.dump_frames(frames, str(tmp_path)) == 4
    assert {p.name for p in tmp_path.iterdir()} == {f"frame_{k}.npy" for k in bench.DUMP_FIELDS + ("octets",)}
    chan, sync, idx = (np.load(tmp_path / f"frame_{k}.npy") for k in ("chan", "sync_sample", "idx"))
    assert chan.dtype == np.float64 and list(chan) == [1, 1, 3, 3] and list(sync) == [100, 900, 500, 500] and list(idx) == [0, 0, 0, 1]
    oct_ = np.load(tmp_path / "frame_octets.npy")
    assert oct_.dtype == np.float32 and list(oct_) == [0xff, 0x10, 0x20, 0x30, 1, 2]
    assert list(np.load(tmp_path / "frame_ppm_error.npy")) == [0.125] * 4


def test_dump_frames_sample_is_bounded_and_fixed(bench, tmp_path, monkeypatch):
    """above the size limit a seeded sample of the frames is written: within the limit, the same frames every time, still in order"""
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20000)
    frames = [_frame(c, 1000 * s, 0, bytes(range(50))) for c in range(16) for s in range(10)]
    n1 = bench.dump_frames(frames, str(tmp_path / "a"))
    n2 = bench.dump_frames(list(reversed(frames)), str(tmp_path / "b"))
    assert 0 < n1 == n2 < len(frames)
    size = sum(np.load(p).nbytes for p in (tmp_path / "a").iterdir())
    assert size <= 20000
    for k in ("chan", "sync_sample"):
        a, b = np.load(tmp_path / "a" / f"frame_{k}.npy"), np.load(tmp_path / "b" / f"frame_{k}.npy")
        assert (a == b).all()
    key = list(zip(np.load(tmp_path / "a" / "frame_chan.npy"), np.load(tmp_path / "a" / "frame_sync_sample.npy")))
    assert key == sorted(key)
