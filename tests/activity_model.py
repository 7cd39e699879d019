"""A numpy model of the activity monitor's definition (include/vdl2hip.h, "Activity monitor"), shared by the CPU and the GPU tests:
bins in float64, busy flags, the sequential transmission rule, bucket() and the accumulators.  Nothing here looks at the kernels."""
import numpy as np

NBUCKETS = 64


def edges():
    """E[i] = float32(10^((-120 + 2 i) / 10)), i = 0 .. 62: computed in double, rounded once"""
    return np.array([np.float32(10.0 ** ((-120 + 2 * i) / 10)) for i in range(63)], dtype=np.float32)


def threshold(dbfs):
    return np.float32(10.0 ** (float(dbfs) / 10.0))


def bound(B):
    """|p - p_ref| <= (B + 4) 2^-24 p_ref: B - 1 float32 additions of non-negative terms, the square, the add and the scaling"""
    return (B + 4) * 2.0 ** -24


def bin_powers(y, B):
    """y: (n, 2) float32 samples from k_on on -> p_ref[m] of every complete bin, float64"""
    v = np.asarray(y, dtype=np.float64)
    e = v[:, 0] ** 2 + v[:, 1] ** 2
    nb = e.size // B
    return e[:nb * B].reshape(nb, B).sum(axis=1) / B


def bucket(p):
    """#{ i : E[i] <= p }"""
    return np.searchsorted(edges(), np.asarray(p, dtype=np.float32), side="right")


def new_state():
    return dict(open=False, idle=0, first=0, m=0)


def scan(p, thr, H, state=None):
    """The accumulators of the float32 series p (bins state['m'] ...), bin after bin as the header states the rule; `state` carries
    an open transmission (and the bin position) over from an earlier call - a reset between the two zeroes only what is returned."""
    st = new_state() if state is None else state
    p = np.asarray(p, dtype=np.float32)
    busy = p > np.float32(thr)
    tx = longest = 0
    for b in busy:
        m = st["m"]
        if b:
            if not st["open"]:
                tx += 1
                st["open"], st["first"] = True, m
            st["idle"] = 0
            longest = max(longest, m - st["first"] + 1)
        elif st["open"]:
            st["idle"] += 1
            if st["idle"] > H:
                st["open"] = False
        st["m"] = m + 1
    n = p.size
    return dict(bins=n, busy_bins=int(busy.sum()), transmissions=tx, longest_bins=longest,
                sum_power=float(np.sum(p.astype(np.float64))), max_power=np.float32(p.max()) if n else np.float32(0),
                min_power=np.float32(p.min()) if n else np.float32(0), hist=np.bincount(bucket(p), minlength=NBUCKETS).astype(np.uint64),
                open=int(st["open"]), flags=busy)


def assert_clear_of_threshold(p_ref, dbfs, margin_db=1.0, label=""):
    """no bin of the float64 reference within margin_db of the threshold: only then may flags be compared exactly"""
    d = 10 * np.log10(np.maximum(np.asarray(p_ref, dtype=np.float64), 1e-300)) - dbfs
    worst = float(np.min(np.abs(d))) if d.size else np.inf
    assert worst > margin_db, f"{label}: a bin lies {worst:.3f} dB from the threshold - change the seed or the keying"
