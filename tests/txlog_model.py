"""A sequential numpy model of the transmission log's definition (include/vdl2hip.h, "Transmission log"), shared by the CPU and the GPU
tests: the activity model's bin-by-bin state machine (activity_model.scan) extended by what a record holds, and the host's join of
records and frames.  Nothing here looks at the kernels."""
import numpy as np

import activity_model as am

TX_PARTIAL = 1
EXACT = ("first_bin", "last_bin", "peak_bin", "first_sample", "last_sample", "busy_bins", "flags", "peak_power")
MEAN_RTOL = 2.0 ** -23          # S within busy_bins 2^-53 of any order of additions, one rounding to float32


def new_state(m=0, open_=False, idle=0, first=0):
    """an idle start at bin m, or a transmission under way taken over from the activity monitor (open, idle bins behind it, first bin)"""
    st = am.new_state()
    st.update(m=m, open=bool(open_), idle=int(idle), first=int(first), last=m - 1 - int(idle), busy=0, sum=0.0, peak=None, peak_bin=0,
              partial=bool(open_))
    return st


def log(p, thr, H, state, B=105, k_on=0):
    """the records of the transmissions that close within the float32 series p (bins state['m'] ...), in order; `state` carries on"""
    p = np.asarray(p, dtype=np.float32)
    thr = np.float32(thr)
    st, out = state, []
    for v in p:
        m = st["m"]
        if v > thr:
            if not st["open"]:
                st.update(open=True, first=m, busy=0, sum=0.0, peak=None, partial=False)
            st["idle"], st["last"] = 0, m
            st["busy"] += 1
            st["sum"] += float(v)
            if st["peak"] is None or v > st["peak"]:
                st["peak"], st["peak_bin"] = v, m
        elif st["open"]:
            st["idle"] += 1
            if st["idle"] > H:                                   # bin last + H + 1 is complete: closed
                st["open"] = False
                n = st["busy"]
                out.append(dict(first_bin=st["first"], last_bin=st["last"], peak_bin=st["peak_bin"] if n else st["first"],
                                first_sample=k_on + st["first"] * B, last_sample=k_on + (st["last"] + 1) * B - 1,
                                busy_bins=n, flags=TX_PARTIAL if st["partial"] else 0,
                                peak_power=np.float32(st["peak"]) if n else np.float32(0),
                                mean_power=np.float32(st["sum"] / n) if n else np.float32(0)))
        st["m"] = m + 1
    return out


MAIL_RECS = 32                  # hostmem.h, kMailRecs: the records of a feed that come to the host with its header
MAIL_CHANS, MAIL_BINS = 11, 30


def mail_keys(nrec):
    """Per channel [(first busy bin, last busy bin)] for the mailbox boundary: MAIL_CHANS channels of three short transmissions with 3
    idle bins between them, all closed within MAIL_BINS bins at H = 0 - 33 records, one more than the mail holds; nrec 32: the last
    channel has two.  The last channel's third comes when every other channel is idle, so the two streams are the same up to it and
    whatever the one transmission leaks into its neighbours reaches no record.  (test_txlog_host.py holds this to log() on a clean series.)"""
    assert nrec in (MAIL_RECS, MAIL_RECS + 1)
    keys = [[(3, 6), (10, 13), (17, 20)] for _ in range(MAIL_CHANS - 1)] + [[(3, 6), (10, 13), (24, 27)]]
    if nrec == MAIL_RECS:
        keys[-1] = keys[-1][:2]
    return keys


def assert_records(got, want, label=""):
    """got: an array of TX_DTYPE (or a list of dicts); want: log()'s records.  Integer fields and peak_power exactly, mean_power to MEAN_RTOL"""
    assert len(got) == len(want), (label, len(got), len(want))
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        for k in EXACT:
            assert g[k] == w[k], (label, i, k, g[k], w[k])
        a, b = float(g["mean_power"]), float(w["mean_power"])
        assert abs(a - b) <= MEAN_RTOL * abs(b), (label, i, a, b)
        worst = max(worst, abs(a - b) / abs(b) if b else 0.0)
    return worst


def join(records, frames, H, B=105, k_on=0, waiting=None):
    """the host's join, one feed: `frames` = this feed's (sync_sample, burst_ord, ok) of one channel, joined first; `records` = the
    feed's records of that channel (dicts, completed in place) -> (frames matched, frames unmatched); `waiting` carries on"""
    waiting = [] if waiting is None else waiting
    waiting += list(frames)
    matched = unmatched = 0
    for r in records:
        lo, hi = r["first_sample"], k_on + (r["last_bin"] + H + 2) * B
        mine = [f for f in waiting if lo <= f[0] < hi]
        unmatched += sum(1 for f in waiting if f[0] < lo)
        waiting[:] = [f for f in waiting if f[0] >= hi]
        r["frames"], r["frames_ok"] = len(mine), sum(1 for f in mine if f[2])
        r["first_burst_ord"] = min(mine)[1] if mine else -1
        matched += len(mine)
    return matched, unmatched
