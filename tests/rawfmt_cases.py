"""The capture config2_1s in each raw sample format, with the oracle's answer to it - what the format-parametrised tests share
(tests/test_gpu_referee.py's scan tests, the referee tests of tests/test_gpu_s8.py).  Per format: how the int16 capture is quantised to
it, what the oracle is fed (it reads s16 and u8 only; a CF32 or S8 sample is exactly an s16 one), bytes per complex sample.
One oracle run per format and session; nothing here is changed by its users."""
import numpy as np

import cases

FORMATS = ("s16", "u8", "cf32", "s8")
SAMPLE_BYTES = {"s16": 4, "u8": 2, "cf32": 8, "s8": 2}
_cache = {}


def receiver_fmt(vh, name):
    return {"s16": 1, "u8": 0, "cf32": vh.FMT_CF32, "s8": vh.FMT_S8}[name]


def s8_of_s16(raw):
    """int16 I, Q -> int8 I, Q: the nearest byte, saturated"""
    k = np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view("<i2")
    return np.clip(np.rint(k / 256), -128, 127).astype(np.int8)


def s16_of_s8(b):
    """the oracle's input: b << 8 as little-endian int16, as bytes"""
    return (np.ascontiguousarray(b).view(np.int8).reshape(-1).astype("<i2") * 256).view(np.uint8)


def cf32_of_s16(raw):
    """int16 I, Q -> float32 I, Q: k / 32768, exact (process_buf_short(), src/demod.c:362-363)"""
    k = np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view("<i2")
    return k.astype(np.float32) / np.float32(32768.0)


def config2(oracle_mod, name):
    """-> dict: cfg; raw - the bytes a receiver of the format is fed; sb; D - decimated samples per channel; tr - the oracle's decimated
    stream [channel, D, 2]; frames, counters18 - the oracle's frames and the reference's 18 counters per channel"""
    if name in _cache:
        return _cache[name]
    cfg, iq, _, _ = cases.load("config2_1s")
    if name == "s16":
        raw, fed, ofmt = iq.view(np.uint8), iq.view(np.uint8), 1
    elif name == "u8":
        raw = np.clip(np.rint(iq.astype(np.float64) / 256.0 + 127.5), 0, 255).astype(np.uint8)
        fed, ofmt = raw, 0
    elif name == "cf32":
        fed, ofmt = iq.view(np.uint8), 1
        raw = cf32_of_s16(fed).view(np.uint8)
    else:
        b = s8_of_s16(iq)
        assert int(b.min()) == -37 and int(b.max()) == 37                         # (the low-amplitude case too: a quarter of the range)
        raw, fed, ofmt = b.view(np.uint8), s16_of_s8(b), 1
    sb = SAMPLE_BYTES[name]
    D = raw.size // sb // cfg.oversample
    o = oracle_mod.Oracle(cfg.centerfreq, list(cfg.freqs), oversample=cfg.oversample, sample_fmt=ofmt, max_ppm=cfg.rx_max_ppm)
    tr = o.trace_all(D + 4)
    o.process(fed, block_bytes=1 << 24, nthreads=8)
    tr = tr[:, :D, :].copy()
    fo = o.frames()
    co = [list(o.counters(c).values())[:18] for c in range(len(cfg.freqs))]
    o.close()
    if name == "s8":
        assert len(fo) == 41
    tr.setflags(write=False)
    _cache[name] = dict(cfg=cfg, raw=raw, sb=sb, D=D, tr=tr, frames=fo, counters18=co)
    return _cache[name]
