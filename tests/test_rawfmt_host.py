"""The raw-sample conversions of dumpvdl2_amd/csrc/rawfmt.h on the CPU, exhaustively.

tests/rawfmt/rawfmt_host.cpp - a stand-alone program, the header compiled by a plain host compiler - prints every conversion over its
whole domain as the bits of the floats; here they are held against numpy's float32 arithmetic, bit for bit:
  U8    all 256 bytes in both byte positions: the division-free level() and the reference's division ref_level() equal each other and
        float32 (i - 127.5) / 127.5;
  S8    all 256 bytes in both positions: int8 / 128;
  S16   all 65 536 values in both halves: int16 / 32768;
  CF32  -0.0 reads as +0.0; +0.0, +-inf, +-FLT_MAX, +-FLT_MIN and random normals come out with their bits unchanged;
  raw_bytes: 2, 4, 8, 2."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rawfmt", "rawfmt_host.cpp")


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


CF32_SAME = np.concatenate([
    f32_bits([0.0, np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny]),
    f32_bits(np.random.default_rng(3).standard_normal(12) * np.float32(10.0) ** np.random.default_rng(4).integers(-30, 30, 12))])


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rawfmt") / "rawfmt_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", os.path.join(ROOT, "dumpvdl2_amd", "csrc"), "-o", exe, SRC])
    args = ["80000000"] + [f"{int(u):08x}" for u in CF32_SAME]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-500:]
    out = {}
    for ln in p.stdout.splitlines():
        tag, *rest = ln.split()
        out.setdefault(tag, []).append(rest)
    return out


def table(rows, tag):
    """-> (values, [n, 4] uint32: level lo, level hi, ref_level lo, ref_level hi)"""
    r = rows[tag]
    return np.array([int(x[0]) for x in r]), np.array([[int(h, 16) for h in x[1:]] for x in r], dtype=np.uint32)


def test_u8(rows):
    v, got = table(rows, "U8")
    assert v.tolist() == list(range(256))
    want = f32_bits((v.astype(np.float32) - np.float32(127.5)) / np.float32(127.5))
    for k, name in enumerate(["level, low byte", "level, high byte", "ref_level, low byte", "ref_level, high byte"]):
        assert np.array_equal(got[:, k], want), name
    assert np.array_equal(got[:, 0], got[:, 2]) and np.array_equal(got[:, 1], got[:, 3])     # the two conversions, one value


def test_s8(rows):
    v, got = table(rows, "S8")
    assert v.tolist() == list(range(256))
    want = f32_bits(v.astype(np.uint8).view(np.int8).astype(np.float32) / np.float32(128.0))
    for k in range(4):
        assert np.array_equal(got[:, k], want), k
    assert not np.any(got == 0x80000000)             # never a negative zero


def test_s16(rows):
    v, got = table(rows, "S16")
    assert v.tolist() == list(range(65536))
    want = f32_bits(v.astype(np.uint16).view(np.int16).astype(np.float32) / np.float32(32768.0))
    for k in range(4):
        assert np.array_equal(got[:, k], want), k


def test_cf32(rows):
    r = [[int(h, 16) for h in x] for x in rows["CF32"]]
    assert r[0] == [0x80000000, 0, 0]                # -0.0 reads as +0.0
    assert len(r) == 1 + len(CF32_SAME) >= 20
    for (u, a, b), want in zip(r[1:], CF32_SAME):
        assert u == int(want) and a == u and b == u, f"{u:08x} -> {a:08x}, {b:08x}"


def test_sizes_and_dispatch(rows):
    assert rows["BYTES"] == [["2", "4", "8", "2"]]
    assert rows["WITH"] == [["0", "0"], ["1", "1"], ["2", "2"], ["3", "3"]]
