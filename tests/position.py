"""Shared by the position tests (test_oracle_position, test_hostsim_position, test_gpu_position): the oracle started at a chosen
stream position.  A position n is a stream that BEGINS at input sample n, at rest - not one that was silent before n."""
import copy
import functools

import numpy as np

import cases

ALIGNED = 52 * 5 * 2**24      # a multiple of 5 * 2^24: every 24-bit NCO phase is 0 again, and it divides by both oversamplings; > 2^32


def round_down(n, os_):
    return n - n % os_


@functools.lru_cache(maxsize=None)
def oracle_at(name, n, trace=True):
    """The oracle's answer for golden case `name` started at input sample n, computed once and shared; leave it unchanged.
    -> dict(frames, counters [per channel, list], avlc, trace [C, D, 2] indexed from K = n / oversample, D, K)"""
    from oracle import pyoracle as po
    cfg, iq, _, _ = cases.load(name)
    return oracle_run(po, cfg, iq, n, trace)


def oracle_run(po, cfg, raw, n, trace=True, sample_fmt=None):
    C = len(cfg.freqs)
    fmt = po.FMT_S16LE if sample_fmt is None else sample_fmt
    o = po.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, sample_fmt=fmt, max_ppm=cfg.rx_max_ppm)
    if n:
        o.set_position(n)
    b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    tr = o.trace_all(b.size // (4 if fmt == po.FMT_S16LE else 2) // cfg.oversample + 4) if trace else None
    o.process(b, block_bytes=1 << 24, nthreads=4)
    D = o.decimated_count(0)
    fr = o.frames()
    out = dict(frames=fr, counters=[list(o.counters(c).values()) for c in range(C)], avlc=po.avlc_counters(fr, C),
               trace=None if tr is None else tr[:, :D, :], D=D, K=n // cfg.oversample)
    o.close()
    return out


def shifted_golden(gold, K):
    """the committed golden answers with every burst timing moved by K decimated samples"""
    g = copy.deepcopy(gold)
    for f in g["frames"]:
        f["sync_sample"] += K
        f["end_sample"] += K
    return g
