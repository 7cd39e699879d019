"""The DEVICE build of the back end piece by piece - the wave primitives (`__ballot`, `__shfl_*`), header_to_geometry, rs_decode_row, decode_burst
with its reserve of frame records (the atomics on the feed-wide counters), and k_frame_finish itself - through the test hooks
vdl2hip_debug_burst_probe, vdl2hip_debug_frame_finish and vdl2hip_debug_core_probe's header kind (kernels.h: k_burst_probe*, k_core_probe),
against the plain references of tests/burst_reference.py: numpy, the oracle's RS decoder, the oracle's own decode_vdl2_burst() on the channel bits
(pyoracle.decode_bits), its AVLC screen, float64 for the power figures.  The same cases, with the same expectations, run through the host build
in tests/test_burst_reference.py; the host build is no reference here.  A few workgroups only, so that a wavefront takes many elements in a row,
each on the LDS state the one before has left.  Every figure is printed before it is asserted; profiles/burst_probe_device.txt keeps the measured ones.

Wall time of the module on an MI355X: see profiles/burst_probe_device.txt."""
import numpy as np
import pytest

import burst_reference as br
import test_unstuff_adversarial as adv
from util import TOL_DB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dumpvdl2_amd import vdl2hip
    return vdl2hip.load_library()


@pytest.fixture(scope="module")
def cases(oracle_mod):
    return br.burst_cases(adversarial=adv.adversarial_bitstrings(np.random.default_rng(2024), 150))


@pytest.fixture(scope="module")
def rs_set(oracle_mod):
    rows, nerr = br.rs_rows()
    ret, out = br.rs_expected(rows)
    for a in (rows, nerr, ret, out):
        a.setflags(write=False)
    return rows, nerr, ret, out


@pytest.mark.parametrize("grid", [1, 3])
def test_wave_primitives(L, grid):
    v = br.wave_vectors()
    out = br.device_wave(L, v, grid)
    exp = br.wave_expected(v)
    names = ["wave_first_flag", "wave_count_flags"] + ["wave_excl_scan64"] * 65 + ["wave_min64"]
    bad = np.argwhere(out != exp)
    print(f"wave primitives: {len(v)} vectors, {grid} workgroups, {len(bad)} values differ")
    assert len(bad) == 0, f"vector {bad[0][0]}: {names[bad[0][1]]} (word {bad[0][1]}) {out[tuple(bad[0])]} != {exp[tuple(bad[0])]}"


def test_header_to_geometry(L):
    w, where = br.header_words()
    out = br.device_header(L, w)
    exp = br.header_expected(w)
    bad = np.flatnonzero((out != exp).any(axis=1))
    print(f"header: {len(w)} words, {bad.size} differ; statuses in the set: {np.bincount(exp[:, 0], minlength=4).tolist()}")
    assert bad.size == 0, f"{bad.size} header words, first {w[bad[0]]:#x}: (status, syndrome, tl, want) {out[bad[0]]} != {exp[bad[0]]}"


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_rs_decode_row(L, rs_set, order):
    rows, nerr, ret_ref, out_ref = rs_set
    cl = br.rs_classes(rows, nerr, ret_ref)
    print(f"rs: {len(rows)} rows, classes {cl}")
    for k, floor in br.RS_FLOORS.items():
        assert cl[k] >= floor, (k, cl)
    idx = np.arange(len(rows)) if order == "forward" else np.arange(len(rows))[::-1]
    ret, out = br.device_rs(L, rows[idx], grid=2)                   # 4 wavefronts, some 1 200 rows each, every row on its predecessor's LDS
    back = np.empty_like(idx); back[idx] = np.arange(len(idx))
    br.rs_compare(rows, ret_ref, out_ref, ret[back], out[back], f"device, {order}")


@pytest.mark.parametrize("grid", [1, 3])
def test_decode_burst(L, cases, grid):
    for group in br.split_by_ring(cases):
        packed = br.pack_bursts(group)
        cap_f, cap_p = 8192, 1 << 18
        out = br.device_bursts(L, packed, grid, cap_f, cap_p)
        fig = br.check_bursts(group, out, grid * br.K_BURST_WAVES, f"device, {grid} workgroups, rings of {packed[2].shape[1]}", cap_f, cap_p, 64, 4096, TOL_DB)
        print(f"bursts: {len(group)} on rings of {packed[2].shape[1]}, {grid} workgroups: {fig}")


@pytest.mark.parametrize("name,cap_f,cap_p", br.CAPACITY)
def test_decode_burst_at_capacity(L, cases, name, cap_f, cap_p):
    group = br.capacity_group(cases, name)
    out = br.device_bursts(L, br.pack_bursts(group), 1, cap_f, cap_p)
    fig = br.check_bursts(group, out, br.K_BURST_WAVES, f"device, capacity {cap_f} / {cap_p}", cap_f, cap_p, 64, 4096, TOL_DB, expect_overflow=True)
    print(f"capacity {cap_f} records / {cap_p} octets ({name}): {fig}")
    assert fig["missing"] > 0


def test_frame_finish(L, oracle_mod):
    worst = 0.0
    lists = br.finish_lists()
    for fl in lists:
        for grid in ((1, 2, 3) if fl.name == "all3000" else (1, 2)):
            worst = max(worst, br.check_finish(fl, br.device_finish(L, fl, grid), f"device, {grid} workgroups", TOL_DB))
    print(f"frame finish: {len(lists)} lists, {sum(len(f.expected) for f in lists)} frames, worst |nf_pwr_dbfs - float64| {worst:.2e} dB")
