"""The spectrogram's plan of a feed (dumpvdl2_amd/csrc/specgram_plan.h) on the CPU, and the tap's place in the ABI.

tests/specgram/specgram_plan_host.cpp - a stand-alone program, the header compiled by a plain host compiler under the address and
undefined-behaviour sanitizers - runs the plan over a few thousand random streams of feeds (stream position, feed lengths 0 .. 3e5,
N in {64, 1024, 4096}, stride 1 .. 5, R in {1, 2, 3, 16, 1000}, a0, workgroup limit) and the edges (R = 1, no segment, a feed that
completes no line, a feed that completes more than 1024 lines) and checks against brute force: every analysed segment is taken exactly
once, in order; no workgroup leaves more than two pieces; the pieces of a line come in ascending segment order; every line a feed
completes is written to exactly one ring slot, l mod ring_lines; a sequence of feeds yields the lines of the stream in one feed."""
import ctypes as C
import os
import subprocess

import pytest

from dumpvdl2_amd import vdl2hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "specgram", "specgram_plan_host.cpp")
SYMBOLS = ["vdl2hip_specgram_enable", "vdl2hip_specgram_disable", "vdl2hip_specgram_read", "vdl2hip_specgram_lines", "vdl2hip_specgram_channels"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("specgram") / "specgram_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "dumpvdl2_amd", "csrc"), "-o", out, SRC])
    return out


def test_plan_against_brute_force(exe):
    p = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    tag, tuples, feeds = p.stdout.split()
    assert tag == "ok" and int(tuples) == 3000 and int(feeds) > 3 * 3000


def test_the_plan_header_is_plain_cpp():
    """no HIP include: a host compiler takes it as it is, with every warning on"""
    text = open(os.path.join(ROOT, "dumpvdl2_amd", "csrc", "specgram_plan.h")).read()
    assert "#include <hip" not in text
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "dumpvdl2_amd", "csrc"), "-x", "c++", "-"],
                   input='#include "specgram_plan.h"\n', text=True, check=True)


def test_structure_sizes():
    assert C.sizeof(vdl2hip.SpecgramCfg) == 16 and C.sizeof(vdl2hip.SpecgramInfo) == 72
    assert [k for k, _ in vdl2hip.SpecgramInfo._fields_][:8] == ["struct_size", "nfft", "window", "stride", "line_segments", "ring_lines", "sample_rate", "centerfreq"]
    assert vdl2hip.SpecgramInfo.first_segment.offset == 32 and vdl2hip.SpecgramInfo.hold_lines.offset == 64


def test_symbols_are_exported():
    L = vdl2hip.load_library()
    for name in SYMBOLS:
        assert name in vdl2hip.EXPORTS and hasattr(L, name), name
    assert L.vdl2hip_abi_version() == vdl2hip.ABI_VERSION == 6


def test_calls_without_a_receiver_are_refused():
    L = vdl2hip.load_library()
    cfg = vdl2hip.SpecgramCfg(C.sizeof(vdl2hip.SpecgramCfg), 16, 0, 0)
    assert L.vdl2hip_specgram_enable(None, C.byref(cfg)) == -1
    assert L.vdl2hip_specgram_disable(None) == -1
    assert L.vdl2hip_specgram_read(None, None, None, None, 0, 0) == -1
    assert L.vdl2hip_specgram_lines(None, 0, None, None, 0) == -1
    assert L.vdl2hip_specgram_channels(None, None, None, 0) == -1
