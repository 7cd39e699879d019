"""The burst capture's quality figures in numpy (include/vdl2hip.h, "Burst capture"): the float32 steps of the decoder's slicer,
sums in float64.  Shared by tests/test_capture_host.py (the kernels' steps on the CPU) and tests/test_gpu_capture.py.

The bounds.  Two correctly working double-precision atan2 implementations, narrowed to float32, differ by at most one float32 ulp
at pi (2^-22) per phase; a symbol's e uses two phases, scaled by 4 / pi: per symbol |e - e_model| <= E = 2^-20 in units of pi / 4.
So phase_err_rms, _mean and _max are held to E pi / 4 + 2^-23 |value| (the final float32 rounding on either side);
weak_symbols lies between #{|e| > 0.25 + E} and #{|e| > 0.25 - E}; mean_power - float32 terms summed in float64 in another order -
to (nsym + 4) 2^-53 relative plus one float32 rounding; min_power and max_power are exact.
The model asserts that no u lies within E of a half-integer: the rounding is then the same on either side.  That is a condition on
the inputs (another seed), never a reason to leave symbols out."""
import numpy as np

E = 2.0 ** -20
F32, F64 = np.float32, np.float64
BURST_DTYPE = np.dtype([("nsym", "<i4"), ("tl_bits", "<u4"), ("t_first", "<i8"), ("sync_sample", "<i8"), ("end_sample", "<i8"), ("ord", "<i8"),
                        ("prev_n", "<i8"), ("prev_phi0", "<f4"), ("vdphi", "<f4"), ("ppm", "<f4"), ("pad", "<u4")])     # the hooks' burst, 64 bytes


def slice_args(phi, prev_phase, dphi):
    """u_m of vdl2_core.h's slice_symbol(): phi float32 [n] -> float32 [n]"""
    phi = np.asarray(phi, dtype=F32)
    prev = np.concatenate((np.array([prev_phase], dtype=F32), phi[:-1]))
    d = ((phi - prev).astype(F32) - F32(dphi)).astype(F32)
    two_pi = F64(F32(2.0)) * np.pi
    d64 = d.astype(F64)
    d = np.where(d < 0, (d64 + two_pi).astype(F32), np.where(d64 > two_pi, (d64 - two_pi).astype(F32), d)).astype(F32)
    return (d.astype(F64) / (np.pi / 4)).astype(F32)


def quality(sym, prev_phase, dphi):
    """sym: float32 [nsym, 2], the samples y[t_m] -> the figures of the record (float64 where the record rounds to float32 last)"""
    sym = np.asarray(sym, dtype=F32).reshape(-1, 2)
    n = sym.shape[0]
    assert n > 0
    phi = np.arctan2(sym[:, 1].astype(F64), sym[:, 0].astype(F64)).astype(F32)
    u = slice_args(phi, prev_phase, dphi).astype(F64)
    r = np.floor(u + 0.5)
    assert np.all(np.abs(u - np.floor(u) - 0.5) > E), "a u within E of a half-integer: choose another input"
    e = u - r                                                   # (exact in float32 too)
    p = ((sym[:, 0] * sym[:, 0]).astype(F32) + (sym[:, 1] * sym[:, 1]).astype(F32)).astype(F32)
    ae = np.abs(e)
    return dict(nsym=n, e=e, phase_err_rms=np.sqrt(np.sum(e * e) / n) * np.pi / 4, phase_err_mean=np.sum(e) / n * np.pi / 4,
                phase_err_max=ae.max() * np.pi / 4, weak_lo=int(np.sum(ae > 0.25 + E)), weak_hi=int(np.sum(ae > 0.25 - E)),
                mean_power=float(np.sum(p.astype(F64)) / n), min_power=p.min(), max_power=p.max())


def check_quality(rec, q, label=""):
    """rec: the record's fields (dict or numpy record); q: quality() of the same symbols.  Prints each figure before it asserts."""
    worst = 0.0
    for k in ("phase_err_rms", "phase_err_mean", "phase_err_max"):
        bound = E * np.pi / 4 + 2.0 ** -23 * abs(q[k])
        err = abs(float(rec[k]) - q[k])
        worst = max(worst, err / bound)
        print(f"{label} {k}: {float(rec[k]):.9g} model {q[k]:.9g} |diff| / bound = {err / bound:.3f}")
        assert err <= bound, (label, k, float(rec[k]), q[k])
    assert q["weak_lo"] <= int(rec["weak_symbols"]) <= q["weak_hi"], (label, int(rec["weak_symbols"]), q["weak_lo"], q["weak_hi"])
    bound = ((q["nsym"] + 4) * 2.0 ** -53 + 2.0 ** -24) * q["mean_power"]
    err = abs(float(rec["mean_power"]) - q["mean_power"])
    print(f"{label} mean_power: {float(rec['mean_power']):.9g} model {q['mean_power']:.9g} |diff| / bound = {err / bound if bound else 0.0:.3f}")
    assert err <= bound, (label, "mean_power", float(rec["mean_power"]), q["mean_power"])
    assert F32(rec["min_power"]) == q["min_power"] and F32(rec["max_power"]) == q["max_power"], (label, "min/max power")
    return worst


def window(sync_sample, end_sample, pre, post, k_end):
    first = max(0, sync_sample - pre)
    last = min(end_sample + post, k_end - 1)
    return first, last - first + 1
