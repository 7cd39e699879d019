"""ctypes binding of libvdl2hip.so - the host-side mirror of the reference's
process_buf_*() -> avlc_decoder_queue_push() boundary (include/vdl2hip.h).

The library is the product; this module only passes pointers and sizes.
It raises if the shared library is missing or no HIP device exists: there is
no CPU implementation to fall back to.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvdl2hip.so")

FMT_U8, FMT_S16LE, FMT_CF32 = 0, 1, 2     # include/vdl2hip.h: VDL2HIP_FMT_* (CF32: np.complex64 / interleaved float32, full scale 1.0)
FMT_S8 = 4                                # signed bytes, interleaved I, Q (np.int8; b / 128: what FMT_S16LE makes of b << 8); 3 is unassigned
COUNTER_NAMES = [
    "demod.sync.good", "decoder.crc.good", "decoder.crc.bad", "decoder.errors.no_header",
    "decoder.errors.too_long", "decoder.errors.no_fec", "decoder.errors.data_truncated",
    "decoder.errors.fec_truncated", "decoder.errors.deinterleave_data",
    "decoder.errors.deinterleave_fec", "decoder.errors.fec_bad", "decoder.errors.bitstream",
    "decoder.errors.truncated_octets", "decoder.errors.unstuff", "decoder.blocks.processed",
    "decoder.blocks.fec_ok", "decoder.msg.good", "decoder.msg.good_loud",
    "demod.ppm_reject", "demod.slicer_neg_idx",
]
NUM_COUNTERS = len(COUNTER_NAMES)
AVLC_COUNTER_NAMES = [
    "avlc.frames.processed", "avlc.errors.too_short", "avlc.frames.good", "avlc.errors.bad_fcs",
    "avlc.msg.air2gnd", "avlc.msg.air2air", "avlc.msg.air2all", "avlc.msg.gnd2air", "avlc.msg.gnd2gnd", "avlc.msg.gnd2all",
]
NUM_AVLC_COUNTERS = len(AVLC_COUNTER_NAMES)
AVLC_OK, AVLC_TOO_SHORT, AVLC_BAD_FCS = 0, 1, 2
ABI_VERSION = 6
MAX_DRAIN_LAG = int(os.environ.get("VDL2HIP_PY_MAX_DRAIN_LAG", "5"))   # include/vdl2hip.h: VDL2HIP_MAX_DRAIN_LAG (the variable: development builds with another depth)
EXPORTS = [
    "vdl2hip_abi_version", "vdl2hip_strerror", "vdl2hip_create", "vdl2hip_destroy", "vdl2hip_feed",
    "vdl2hip_feed_device", "vdl2hip_sync", "vdl2hip_drain", "vdl2hip_counters", "vdl2hip_set_profiling",
    "vdl2hip_drain_packed", "vdl2hip_pack_raw_frame", "vdl2hip_get_stats", "vdl2hip_get_stats_sized", "vdl2hip_stream", "vdl2hip_set_drain_lag", "vdl2hip_get_lpf", "vdl2hip_get_nco_step", "vdl2hip_read_decimated",
    "vdl2hip_avlc_counters", "vdl2hip_set_avlc_filter", "vdl2hip_statsd_lines", "vdl2hip_feed_pinned",
    "vdl2hip_group_create", "vdl2hip_group_destroy", "vdl2hip_group_feed", "vdl2hip_group_feed_pinned", "vdl2hip_group_sync", "vdl2hip_group_drain",
    "vdl2hip_group_set_drain_lag", "vdl2hip_group_counters", "vdl2hip_group_avlc_counters", "vdl2hip_group_size", "vdl2hip_group_ctx",
    "vdl2hip_group_uses_rccl", "vdl2hip_group_set_exchange", "vdl2hip_group_exchange",
    "vdl2hip_read_resampled", "vdl2hip_resampler_design",
    "vdl2hip_spectrum_window", "vdl2hip_spectrum_enable", "vdl2hip_spectrum_read", "vdl2hip_spectrum_channels",
    "vdl2hip_activity_edges", "vdl2hip_activity_enable", "vdl2hip_activity_disable", "vdl2hip_activity_read", "vdl2hip_activity_series",
    "vdl2hip_capture_enable", "vdl2hip_capture_disable", "vdl2hip_capture_info_get", "vdl2hip_capture_read",
    "vdl2hip_txlog_enable", "vdl2hip_txlog_disable", "vdl2hip_txlog_info_get", "vdl2hip_txlog_read",
    "vdl2hip_txsearch_enable", "vdl2hip_txsearch_disable", "vdl2hip_txsearch_info_get", "vdl2hip_txsearch_read",
    "vdl2hip_specgram_enable", "vdl2hip_specgram_disable", "vdl2hip_specgram_read", "vdl2hip_specgram_lines", "vdl2hip_specgram_channels",
    "vdl2hip_txcap_enable", "vdl2hip_txcap_disable", "vdl2hip_txcap_info_get", "vdl2hip_txcap_read", "vdl2hip_txcap_measure",
    "vdl2hip_toa_template", "vdl2hip_toa_enable", "vdl2hip_toa_disable", "vdl2hip_toa_info_get", "vdl2hip_toa_read",
    "vdl2hip_relook_enable", "vdl2hip_relook_disable", "vdl2hip_relook_info_get", "vdl2hip_relook_read",
]
# include/vdl2hip.h: VDL2HIP_RELOOK_NEW_ONLY (cfg.flags), VDL2HIP_RELOOK_* (vdl2hip_relook.flags, beside TX_PARTIAL)
RELOOK_NEW_ONLY = 1
RELOOK_PPM_REJECT, RELOOK_TRUNCATED, RELOOK_NO_ROOM = 2, 4, 8
# include/vdl2hip.h: VDL2HIP_TOA_FAILED_ONLY (cfg.flags), VDL2HIP_TOA_* (vdl2hip_burst_toa.flags)
TOA_FAILED_ONLY = 1
TOA_EARLY, TOA_EDGE, TOA_FLAT, TOA_NO_CURVE = 1, 2, 4, 8
TOA_TAPS = 151
# include/vdl2hip.h: VDL2HIP_TXCAP_* (cfg.flags), VDL2HIP_TXC_* (vdl2hip_tx_capture.flags, beside TX_PARTIAL)
TXCAP_IQ, TXCAP_SPECTRUM, TXCAP_UNDECODED_ONLY = 1, 2, 4
TXC_CLIPPED, TXC_TRUNCATED, TXC_NO_ROOM, TXC_SHORT, TXC_NO_SPECTRUM = 2, 4, 8, 16, 32
# include/vdl2hip.h: VDL2HIP_TXSEARCH_UNDECODED_ONLY (cfg.flags), VDL2HIP_TXS_CLIPPED (vdl2hip_tx_search.flags, beside TX_PARTIAL), VDL2HIP_TXS_* (why)
TXSEARCH_UNDECODED_ONLY, TXS_CLIPPED = 1, 2
TXS_DECODED, TXS_FRAMES_BAD, TXS_LOCK_NO_FRAME, TXS_NO_PREAMBLE = 0, 1, 2, 3
TXLOG_UNDECODED_ONLY, TX_PARTIAL = 1, 1     # include/vdl2hip.h: VDL2HIP_TXLOG_UNDECODED_ONLY (cfg.flags), VDL2HIP_TX_PARTIAL (vdl2hip_tx.flags)
CAPTURE_FAILED_ONLY, BURST_NO_ROOM = 1, 1   # include/vdl2hip.h: VDL2HIP_CAPTURE_FAILED_ONLY (cfg.flags), VDL2HIP_BURST_NO_ROOM (vdl2hip_burst.flags)
WIN_RECT, WIN_HANN, WIN_BH4 = 0, 1, 2     # include/vdl2hip.h: VDL2HIP_WIN_* (the input monitor's analysis windows)


class Cfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("centerfreq", C.c_uint32), ("oversample", C.c_uint32),
                ("sample_fmt", C.c_uint32), ("nchan", C.c_uint32), ("freqs", C.POINTER(C.c_uint32)),
                ("max_ppm", C.c_float), ("device", C.c_int32), ("max_block_bytes", C.c_uint32),
                ("chan_first", C.c_uint32), ("chan_count", C.c_uint32),
                ("reserved0", C.c_uint32), ("input_rate", C.c_uint32), ("reserved1", C.c_uint32)]     # (56 -> 64 bytes: vdl2hip.h)


class CFrame(C.Structure):
    _fields_ = [("chan", C.c_uint32), ("freq", C.c_uint32), ("idx", C.c_int32), ("len", C.c_uint32),
                ("octets", C.POINTER(C.c_uint8)), ("synd_weight", C.c_uint32), ("datalen_octets", C.c_uint32),
                ("num_fec_corrections", C.c_int32), ("frame_pwr_dbfs", C.c_float), ("nf_pwr_dbfs", C.c_float),
                ("ppm_error", C.c_float), ("burst_ord", C.c_int64), ("sync_sample", C.c_int64),
                ("end_sample", C.c_int64), ("avlc_status", C.c_uint32), ("dst_addr", C.c_uint32), ("src_addr", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("feeds", C.c_uint64), ("input_samples", C.c_uint64), ("chan_samples", C.c_uint64),
                ("chanfir_launches", C.c_uint64), ("chanfir_ms", C.c_double), ("phase_ms", C.c_double),
                ("sync_ms", C.c_double), ("walk_ms", C.c_double), ("burst_ms", C.c_double), ("nf_ms", C.c_double),
                ("bursts", C.c_uint64), ("frames", C.c_uint64),
                ("seg_adopted", C.c_uint64), ("seg_walked", C.c_uint64), ("front_sync_timeouts", C.c_uint64),
                ("overflow_feeds", C.c_uint64), ("cold_start_feeds", C.c_uint64),
                ("referee_scans", C.c_uint64), ("referee_cached", C.c_uint64), ("referee_refused", C.c_uint64), ("referee_short", C.c_uint64), ("referee_rewalks", C.c_uint64),
                ("referee_candidate_scans", C.c_uint64), ("referee_header_scans", C.c_uint64), ("referee_symbol_scans", C.c_uint64),
                ("referee_redone_next", C.c_uint64), ("referee_unmet", C.c_uint64), ("referee_retried", C.c_uint64),
                ("resampled_samples", C.c_uint64), ("resample_ms", C.c_double),
                ("referee_symbol_pieces_ahead", C.c_uint64), ("referee_symbol_pieces_late", C.c_uint64)]


class SpectrumCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nfft", C.c_uint32), ("window", C.c_uint32), ("stride", C.c_uint32)]


class SpectrumInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nfft", C.c_uint32), ("window", C.c_uint32), ("stride", C.c_uint32),
                ("sample_rate", C.c_uint32), ("centerfreq", C.c_uint32),
                ("segments", C.c_uint64), ("samples", C.c_uint64), ("clipped", C.c_uint64),
                ("enbw_bins", C.c_double), ("mean_power", C.c_double), ("dc_i", C.c_double), ("dc_q", C.c_double),
                ("peak", C.c_float), ("kernel_ms", C.c_float)]


class SpecgramCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("line_segments", C.c_uint32), ("ring_lines", C.c_uint32), ("reserved", C.c_uint32)]


class SpecgramInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nfft", C.c_uint32), ("window", C.c_uint32), ("stride", C.c_uint32),
                ("line_segments", C.c_uint32), ("ring_lines", C.c_uint32), ("sample_rate", C.c_uint32), ("centerfreq", C.c_uint32),
                ("first_segment", C.c_uint64), ("first_sample", C.c_uint64), ("lines", C.c_uint64),
                ("hold_segments", C.c_uint64), ("hold_lines", C.c_uint64)]


class ActivityCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bin_samples", C.c_uint32), ("hang_bins", C.c_uint32), ("series_bins", C.c_uint32),
                ("threshold_dbfs", C.c_float), ("reserved", C.c_uint32)]


class ActivityInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bin_samples", C.c_uint32), ("hang_bins", C.c_uint32), ("series_bins", C.c_uint32),
                ("threshold_dbfs", C.c_float), ("threshold_power", C.c_float), ("first_sample", C.c_int64), ("bins", C.c_uint64),
                ("kernel_ms", C.c_float), ("reserved", C.c_uint32)]


class ActivityChan(C.Structure):
    _fields_ = [("bins", C.c_uint64), ("busy_bins", C.c_uint64), ("transmissions", C.c_uint64), ("longest_bins", C.c_uint64),
                ("sum_power", C.c_double), ("max_power", C.c_float), ("min_power", C.c_float), ("open", C.c_uint32), ("reserved", C.c_uint32),
                ("hist", C.c_uint64 * 64)]


ACTIVITY_CHAN_DTYPE = np.dtype([("bins", "<u8"), ("busy_bins", "<u8"), ("transmissions", "<u8"), ("longest_bins", "<u8"),
                                ("sum_power", "<f8"), ("max_power", "<f4"), ("min_power", "<f4"), ("open", "<u4"), ("reserved", "<u4"),
                                ("hist", "<u8", (64,))])     # vdl2hip_activity_chan, 568 bytes


class CaptureCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pre_samples", C.c_uint32), ("post_samples", C.c_uint32), ("flags", C.c_uint32),
                ("pool_samples", C.c_uint32), ("reserved", C.c_uint32)]


class CaptureInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pre_samples", C.c_uint32), ("post_samples", C.c_uint32), ("flags", C.c_uint32),
                ("pool_samples", C.c_uint32), ("reserved", C.c_uint32), ("bursts", C.c_uint64), ("iq_samples", C.c_uint64),
                ("iq_dropped", C.c_uint64), ("kernel_ms", C.c_float), ("reserved2", C.c_uint32)]


BURST_DTYPE = np.dtype([("chan", "<u4"), ("freq", "<u4"), ("burst_ord", "<i8"), ("sync_sample", "<i8"), ("end_sample", "<i8"), ("first_symbol", "<i8"),
                        ("nsym", "<u4"), ("tl_bits", "<u4"), ("ppm_error", "<f4"), ("dphi", "<f4"), ("prev_phase", "<f4"), ("flags", "<u4"),
                        ("iq_first", "<i8"), ("iq_count", "<u4"), ("reserved", "<u4"), ("iq_off", "<u8"),
                        ("frames", "<u4"), ("frames_ok", "<u4"), ("fec_corrections", "<i4"), ("weak_symbols", "<u4"),
                        ("mean_power", "<f4"), ("min_power", "<f4"), ("max_power", "<f4"),
                        ("phase_err_rms", "<f4"), ("phase_err_mean", "<f4"), ("phase_err_max", "<f4")])     # vdl2hip_burst, 128 bytes


class TxlogCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pool_records", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class TxlogInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pool_records", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("transmissions", C.c_uint64), ("decoded", C.c_uint64), ("dropped", C.c_uint64),
                ("frames_matched", C.c_uint64), ("frames_unmatched", C.c_uint64), ("kernel_ms", C.c_float), ("reserved2", C.c_uint32)]


TX_DTYPE = np.dtype([("chan", "<u4"), ("freq", "<u4"), ("first_bin", "<u8"), ("last_bin", "<u8"), ("peak_bin", "<u8"),
                     ("first_sample", "<i8"), ("last_sample", "<i8"), ("busy_bins", "<u4"), ("flags", "<u4"),
                     ("peak_power", "<f4"), ("mean_power", "<f4"), ("frames", "<u4"), ("frames_ok", "<u4"),
                     ("first_burst_ord", "<i8")])     # vdl2hip_tx, 80 bytes


class TxsearchCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TxsearchInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("records", C.c_uint64), ("samples_searched", C.c_uint64),
                ("clipped", C.c_uint64), ("kernel_ms", C.c_float), ("reserved", C.c_uint32)]


TXS_DTYPE = np.dtype([("chan", "<u4"), ("freq", "<u4"), ("first_bin", "<u8"), ("search_first", "<i8"), ("search_last", "<i8"),
                      ("best_sample", "<i8"), ("first_lock", "<i8"), ("best_pherr", "<f4"), ("best_slope", "<f4"), ("best_ppm", "<f4"),
                      ("lock_points", "<u4"), ("below_thr", "<u4"), ("lock_phases", "<u4"), ("flags", "<u4"),
                      ("frames", "<u4"), ("frames_ok", "<u4"), ("why", "<u4"), ("reserved", "<u4"), ("reserved2", "<u4")])     # vdl2hip_tx_search, 96 bytes


class RelookCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("threshold", C.c_float), ("max_ppm", C.c_float),
                ("max_anchors", C.c_uint32), ("pool_frames", C.c_uint32), ("pool_octets", C.c_uint32), ("reserved", C.c_uint32)]


class RelookInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("threshold", C.c_float), ("max_ppm", C.c_float),
                ("max_anchors", C.c_uint32), ("pool_frames", C.c_uint32), ("pool_octets", C.c_uint32), ("reserved", C.c_uint32),
                ("records", C.c_uint64), ("anchors_found", C.c_uint64), ("attempts", C.c_uint64), ("frames", C.c_uint64),
                ("frames_ok", C.c_uint64), ("frames_new", C.c_uint64), ("dropped", C.c_uint64), ("kernel_ms", C.c_float), ("reserved2", C.c_uint32)]


RELOOK_DTYPE = np.dtype([("chan", "<u4"), ("freq", "<u4"), ("first_bin", "<u8"), ("anchor", "<i8"), ("end_sample", "<i8"),
                         ("pherr", "<f4"), ("slope", "<f4"), ("ppm_error", "<f4"), ("prev_phase", "<f4"),
                         ("tl_bits", "<u4"), ("nsym", "<u4"), ("synd_weight", "<u4"), ("stop", "<i4"),
                         ("frames", "<u4"), ("frames_ok", "<u4"), ("frames_new", "<u4"), ("fec_corrections", "<i4"),
                         ("frame_first", "<u4"), ("flags", "<u4"), ("new_mask", "<u4"), ("reserved", "<u4"), ("counters", "<u8", (20,))])     # vdl2hip_relook, 256 bytes


class TxcapCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("pre_samples", C.c_uint32), ("post_samples", C.c_uint32),
                ("max_iq_samples", C.c_uint32), ("nfft", C.c_uint32), ("window", C.c_uint32), ("pool_samples", C.c_uint32),
                ("pool_spectra", C.c_uint32), ("reserved", C.c_uint32)]


class TxcapInfo(C.Structure):
    _fields_ = TxcapCfg._fields_ + [("records", C.c_uint64), ("iq_samples", C.c_uint64), ("iq_dropped", C.c_uint64), ("spectra", C.c_uint64),
                                    ("spectra_dropped", C.c_uint64), ("kernel_ms", C.c_float), ("reserved2", C.c_uint32)]


class TxShape(C.Structure):
    _fields_ = [("total", C.c_double), ("peak_hz", C.c_double), ("centroid_hz", C.c_double), ("obw_hz", C.c_double),
                ("peak_bin", C.c_uint32), ("obw_lo", C.c_uint32), ("obw_hi", C.c_uint32), ("reserved", C.c_uint32)]


TXC_DTYPE = np.dtype([("chan", "<u4"), ("freq", "<u4"), ("first_bin", "<u8"), ("win_first", "<i8"), ("win_last", "<i8"),
                      ("iq_off", "<u8"), ("spec_off", "<u8"), ("iq_count", "<u4"), ("flags", "<u4"), ("segments", "<u4"), ("nfft", "<u4"),
                      ("frames", "<u4"), ("frames_ok", "<u4"), ("reserved", "<u4", (2,))])     # vdl2hip_tx_capture, 80 bytes


class ToaCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_lag", C.c_uint32), ("flags", C.c_uint32), ("pool_curves", C.c_uint32)]


class ToaInfo(C.Structure):
    _fields_ = ToaCfg._fields_ + [("bursts", C.c_uint64), ("curves", C.c_uint64), ("curves_dropped", C.c_uint64), ("early", C.c_uint64),
                                  ("edge", C.c_uint64), ("kernel_ms", C.c_float), ("reserved", C.c_uint32)]


BURST_TOA_DTYPE = np.dtype([("chan", "<u4"), ("freq", "<u4"), ("burst_ord", "<i8"), ("sync_sample", "<i8"), ("first_symbol", "<i8"), ("peak_sample", "<i8"),
                            ("peak_lag", "<i4"), ("nlags", "<u4"), ("toa_frac", "<f4"), ("peak_power", "<f4"), ("energy", "<f4"), ("rho", "<f4"),
                            ("carrier_phase", "<f4"), ("cfo_hz", "<f4"), ("dphi", "<f4"), ("resid", "<f4"),
                            ("flags", "<u4"), ("frames", "<u4"), ("frames_ok", "<u4"), ("curve_off", "<u4")])     # vdl2hip_burst_toa, 96 bytes


class PackedFrame(C.Structure):
    _fields_ = [("frame", CFrame), ("octets_off", C.c_uint64)]


FRAME_CB = C.CFUNCTYPE(None, C.POINTER(CFrame), C.c_void_p)
_lib = None


def load_library(path: str = None):
    """path: default = the in-tree build; VDL2HIP_LIB in the environment points development runs at a variant build"""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("VDL2HIP_LIB") or LIB_PATH
    # A ROCm build of PyTorch carries its own libamdhip64.so.7 / libhsa-runtime64.so.1, the same sonames the system ROCm has: whichever
    # is loaded first serves the whole process.  Loaded after this library (which is linked against /opt/rocm), torch ends up on a
    # runtime it was not built with and the next vdl2hip_create() fails with a device error - so where torch is installed it goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing - build it with dumpvdl2_amd.build.build(); there is no CPU fallback")
    L = C.CDLL(path)
    L.vdl2hip_abi_version.restype = C.c_int
    # (development: VDL2HIP_LIB_ANY_ABI=1 lets dev/gpu_variants.py time an OLDER build beside this one - older structures are prefixes of these)
    if L.vdl2hip_abi_version() != ABI_VERSION and not (os.environ.get("VDL2HIP_LIB_ANY_ABI") and L.vdl2hip_abi_version() < ABI_VERSION):      # (the structures below are this version's: a library of another would be read or written out of bounds)
        raise RuntimeError(f"{path} has ABI version {L.vdl2hip_abi_version()}, this binding is for {ABI_VERSION}")
    L.vdl2hip_strerror.restype = C.c_char_p
    L.vdl2hip_strerror.argtypes = [C.c_int]
    L.vdl2hip_create.argtypes = [C.POINTER(Cfg), C.POINTER(C.c_void_p)]
    L.vdl2hip_destroy.argtypes = [C.c_void_p]
    L.vdl2hip_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2hip_feed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2hip_feed_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2hip_sync.argtypes = [C.c_void_p]
    L.vdl2hip_drain.argtypes = [C.c_void_p, FRAME_CB, C.c_void_p]
    L.vdl2hip_drain_packed.argtypes = [C.c_void_p, C.POINTER(PackedFrame), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.vdl2hip_pack_raw_frame.argtypes = [C.POINTER(CFrame), C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]
    L.vdl2hip_counters.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.vdl2hip_avlc_counters.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.vdl2hip_set_avlc_filter.argtypes = [C.c_void_p, C.c_int]
    L.vdl2hip_statsd_lines.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.vdl2hip_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.vdl2hip_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.vdl2hip_set_drain_lag.argtypes = [C.c_void_p, C.c_int]
    L.vdl2hip_stream.restype = C.c_void_p
    L.vdl2hip_stream.argtypes = [C.c_void_p]
    L.vdl2hip_get_lpf.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.vdl2hip_get_nco_step.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.vdl2hip_read_decimated.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_size_t]
    if hasattr(L, "vdl2hip_read_resampled"):                # (absent from older builds loaded through VDL2HIP_LIB for comparisons)
        L.vdl2hip_read_resampled.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t]
        L.vdl2hip_resampler_design.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
    if hasattr(L, "vdl2hip_spectrum_enable"):               # (absent from older builds loaded through VDL2HIP_LIB for comparisons)
        L.vdl2hip_spectrum_window.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
        L.vdl2hip_spectrum_enable.argtypes = [C.c_void_p, C.POINTER(SpectrumCfg)]
        L.vdl2hip_spectrum_read.argtypes = [C.c_void_p, C.POINTER(SpectrumInfo), C.c_void_p, C.c_size_t, C.c_int]
        L.vdl2hip_spectrum_channels.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    if hasattr(L, "vdl2hip_specgram_enable"):               # (absent from older builds loaded through VDL2HIP_LIB for comparisons)
        L.vdl2hip_specgram_enable.argtypes = [C.c_void_p, C.POINTER(SpecgramCfg)]
        L.vdl2hip_specgram_disable.argtypes = [C.c_void_p]
        L.vdl2hip_specgram_read.argtypes = [C.c_void_p, C.POINTER(SpecgramInfo), C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.vdl2hip_specgram_lines.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]
        L.vdl2hip_specgram_channels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    if hasattr(L, "vdl2hip_activity_enable"):               # (absent from older builds loaded through VDL2HIP_LIB for comparisons)
        L.vdl2hip_activity_edges.argtypes = [C.c_void_p, C.c_size_t]
        L.vdl2hip_activity_enable.argtypes = [C.c_void_p, C.POINTER(ActivityCfg)]
        L.vdl2hip_activity_disable.argtypes = [C.c_void_p]
        L.vdl2hip_activity_read.argtypes = [C.c_void_p, C.POINTER(ActivityInfo), C.c_void_p, C.c_size_t, C.c_int]
        L.vdl2hip_activity_series.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_size_t]
    if hasattr(L, "vdl2hip_capture_enable"):                # (absent from older builds loaded through VDL2HIP_LIB for comparisons)
        L.vdl2hip_capture_enable.argtypes = [C.c_void_p, C.POINTER(CaptureCfg)]
        L.vdl2hip_capture_disable.argtypes = [C.c_void_p]
        L.vdl2hip_capture_info_get.argtypes = [C.c_void_p, C.POINTER(CaptureInfo)]
        L.vdl2hip_capture_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "vdl2hip_txlog_enable"):                  # (absent from older builds loaded through VDL2HIP_LIB for comparisons)
        L.vdl2hip_txlog_enable.argtypes = [C.c_void_p, C.POINTER(TxlogCfg)]
        L.vdl2hip_txlog_disable.argtypes = [C.c_void_p]
        L.vdl2hip_txlog_info_get.argtypes = [C.c_void_p, C.POINTER(TxlogInfo)]
        L.vdl2hip_txlog_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    if hasattr(L, "vdl2hip_txsearch_enable"):
        L.vdl2hip_txsearch_enable.argtypes = [C.c_void_p, C.POINTER(TxsearchCfg)]
        L.vdl2hip_txsearch_disable.argtypes = [C.c_void_p]
        L.vdl2hip_txsearch_info_get.argtypes = [C.c_void_p, C.POINTER(TxsearchInfo)]
        L.vdl2hip_txsearch_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    if hasattr(L, "vdl2hip_txcap_enable"):
        L.vdl2hip_txcap_enable.argtypes = [C.c_void_p, C.POINTER(TxcapCfg)]
        L.vdl2hip_txcap_disable.argtypes = [C.c_void_p]
        L.vdl2hip_txcap_info_get.argtypes = [C.c_void_p, C.POINTER(TxcapInfo)]
        L.vdl2hip_txcap_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.vdl2hip_txcap_measure.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(TxShape)]
    if hasattr(L, "vdl2hip_toa_enable"):
        L.vdl2hip_toa_template.argtypes = [C.c_void_p, C.c_size_t]
        L.vdl2hip_toa_enable.argtypes = [C.c_void_p, C.POINTER(ToaCfg)]
        L.vdl2hip_toa_disable.argtypes = [C.c_void_p]
        L.vdl2hip_toa_info_get.argtypes = [C.c_void_p, C.POINTER(ToaInfo)]
        L.vdl2hip_toa_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "vdl2hip_relook_enable"):
        L.vdl2hip_relook_enable.argtypes = [C.c_void_p, C.POINTER(RelookCfg)]
        L.vdl2hip_relook_disable.argtypes = [C.c_void_p]
        L.vdl2hip_relook_info_get.argtypes = [C.c_void_p, C.POINTER(RelookInfo)]
        L.vdl2hip_relook_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(PackedFrame), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.vdl2hip_group_create.argtypes = [C.POINTER(Cfg), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_void_p)]
    L.vdl2hip_group_destroy.argtypes = [C.c_void_p]
    L.vdl2hip_group_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2hip_group_feed_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.vdl2hip_group_sync.argtypes = [C.c_void_p]
    L.vdl2hip_group_drain.argtypes = [C.c_void_p, FRAME_CB, C.c_void_p]
    L.vdl2hip_group_set_drain_lag.argtypes = [C.c_void_p, C.c_int]
    L.vdl2hip_group_counters.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.vdl2hip_group_avlc_counters.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.vdl2hip_group_size.restype = C.c_uint32
    L.vdl2hip_group_size.argtypes = [C.c_void_p]
    L.vdl2hip_group_ctx.restype = C.c_void_p
    L.vdl2hip_group_ctx.argtypes = [C.c_void_p, C.c_uint32]
    L.vdl2hip_group_uses_rccl.argtypes = [C.c_void_p]
    if hasattr(L, "vdl2hip_group_set_exchange"):            # (absent from older builds loaded through VDL2HIP_LIB for comparisons)
        L.vdl2hip_group_set_exchange.argtypes = [C.c_void_p, C.c_int]
        L.vdl2hip_group_exchange.argtypes = [C.c_void_p]
    L.vdl2hip_group_ctx.restype = C.c_void_p
    L.vdl2hip_group_ctx.argtypes = [C.c_void_p, C.c_uint32]
    _lib = L
    return L


class Vdl2HipError(RuntimeError):
    pass


def pack_raw_frame(frame: dict, station_id: Optional[str] = None, tv_sec: int = 0, tv_usec: int = 0) -> bytes:
    """One record of the reference's raw-frame archive (`--output raw:binary:file` / `--raw-frames-file`)."""
    L = load_library()
    octs = frame["octets"]
    buf = (C.c_uint8 * max(1, len(octs)))(*octs)
    f = CFrame(frame["chan"], frame["freq"], frame["idx"], len(octs), C.cast(buf, C.POINTER(C.c_uint8)),
               frame["synd_weight"], frame["datalen_octets"], frame["num_fec_corrections"], frame["frame_pwr_dbfs"],
               frame["nf_pwr_dbfs"], frame["ppm_error"], frame.get("burst_ord", 0), frame.get("sync_sample", 0),
               frame.get("end_sample", 0), 0, 0, 0)
    out = (C.c_uint8 * (len(octs) + 600))()
    n = L.vdl2hip_pack_raw_frame(C.byref(f), station_id.encode() if station_id else None, tv_sec, tv_usec, out, len(out))
    if n < 0:
        raise Vdl2HipError(L.vdl2hip_strerror(n).decode())
    return bytes(out[:n])


def resampler_design(input_rate: int, output_rate: int):
    """The resampler a receiver created with input_rate uses in front of its channeliser (output_rate = 105000 * oversample):
    (L, M, T, taps) with taps float32 [T, L] in prototype order, taps[j, p] = h[j L + p].  Needs no GPU.  Raises Vdl2HipError for a
    ratio the library refuses (vdl2hip.h)."""
    Lib = load_library()
    L, M, T = C.c_uint32(), C.c_uint32(), C.c_uint32()
    r = Lib.vdl2hip_resampler_design(input_rate, output_rate, C.byref(L), C.byref(M), C.byref(T), None, 0)
    if r != -4:                                               # VDL2HIP_E_TOOBIG: the sizes are known now
        raise Vdl2HipError(f"vdl2hip_resampler_design: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    taps = np.zeros(L.value * T.value, dtype=np.float32)
    r = Lib.vdl2hip_resampler_design(input_rate, output_rate, C.byref(L), C.byref(M), C.byref(T), taps.ctypes.data, taps.size)
    if r != taps.size:
        raise Vdl2HipError(f"vdl2hip_resampler_design: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    return L.value, M.value, T.value, taps.reshape(T.value, L.value)


def spectrum_window(nfft: int, window: int = WIN_HANN) -> np.ndarray:
    """The input monitor's analysis window w[0 .. nfft) as float32 (vdl2hip.h, "Input monitor").  Needs no GPU.  Raises Vdl2HipError
    for an nfft (a power of two in 64 .. 4096) or a window the library refuses."""
    Lib = load_library()
    w = np.zeros(max(1, nfft), dtype=np.float32)
    r = Lib.vdl2hip_spectrum_window(nfft, window, w.ctypes.data, w.size)
    if r != nfft or r <= 0:
        raise Vdl2HipError(f"vdl2hip_spectrum_window: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    return w


def _spectrum_read(Lib, ctx, reset: bool, power: bool) -> dict:
    """vdl2hip_spectrum_read() on a context handle -> dict of every info field, plus freq_hz and power where asked for"""
    info = SpectrumInfo(C.sizeof(SpectrumInfo))
    p = np.zeros(4096 if power else 0, dtype=np.float64)      # (the largest nfft: one call, whatever the monitor was enabled with)
    r = Lib.vdl2hip_spectrum_read(ctx, C.byref(info), p.ctypes.data if power else None, p.size, int(reset))
    if r < 0:
        raise Vdl2HipError(f"vdl2hip_spectrum_read: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    p = p[:r].copy()
    out = {k: getattr(info, k) for k, _ in SpectrumInfo._fields_ if k != "struct_size"}
    if power:
        n = info.nfft
        out["freq_hz"] = info.centerfreq + (np.arange(n, dtype=np.float64) - n // 2) * (info.sample_rate / n)
        out["power"] = p
    return out


def _specgram_read(Lib, ctx, reset: bool) -> dict:
    """vdl2hip_specgram_read() on a context handle -> dict of every info field, plus max_hold, floor_hold (float32 [nfft]) and freq_hz"""
    info = SpecgramInfo(C.sizeof(SpecgramInfo))
    mx, fl = np.zeros(4096, dtype=np.float32), np.zeros(4096, dtype=np.float32)      # (the largest nfft: one call)
    r = Lib.vdl2hip_specgram_read(ctx, C.byref(info), mx.ctypes.data, fl.ctypes.data, mx.size, int(reset))
    if r < 0:
        raise Vdl2HipError(f"vdl2hip_specgram_read: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    out = {k: getattr(info, k) for k, _ in SpecgramInfo._fields_ if k != "struct_size"}
    n = info.nfft
    out["freq_hz"] = info.centerfreq + (np.arange(n, dtype=np.float64) - n // 2) * (info.sample_rate / n)
    out["max_hold"], out["floor_hold"] = mx[:n].copy(), fl[:n].copy()
    return out


def _specgram_lines(Lib, ctx, first: int, count: int):
    """vdl2hip_specgram_lines() on a context handle -> (mean, max), float32 [lines, nfft]"""
    info = SpecgramInfo(C.sizeof(SpecgramInfo))
    r = Lib.vdl2hip_specgram_read(ctx, C.byref(info), None, None, 0, 0)
    if r < 0:
        raise Vdl2HipError(f"vdl2hip_specgram_read: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    mean, mx = np.zeros((max(0, count), r), dtype=np.float32), np.zeros((max(0, count), r), dtype=np.float32)
    r = Lib.vdl2hip_specgram_lines(ctx, first, mean.ctypes.data, mx.ctypes.data, mean.shape[0])
    if r < 0:
        raise Vdl2HipError(f"vdl2hip_specgram_lines: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    return mean[:r], mx[:r]


def activity_edges() -> np.ndarray:
    """The 63 edges E[i] = float32(10^((-120 + 2 i) / 10)) of the activity monitor's 64 level buckets (vdl2hip.h, "Activity monitor").
    Needs no GPU."""
    Lib = load_library()
    e = np.zeros(63, dtype=np.float32)
    r = Lib.vdl2hip_activity_edges(e.ctypes.data, e.size)
    if r != 63:
        raise Vdl2HipError(f"vdl2hip_activity_edges: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    return e


def _err(Lib, r, what):
    if r < 0:
        raise Vdl2HipError(f"{what}: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    return r


def _activity_enable(Lib, ctx, bin_samples, threshold_dbfs, hang_bins, series_bins) -> None:
    cfg = ActivityCfg(C.sizeof(ActivityCfg), bin_samples, hang_bins, series_bins, threshold_dbfs, 0)
    _err(Lib, Lib.vdl2hip_activity_enable(ctx, C.byref(cfg)), "vdl2hip_activity_enable")


def _activity_read(Lib, ctx, nchan: int, reset: bool) -> dict:
    """vdl2hip_activity_read() on a context handle -> dict of every info field plus one numpy array per field of vdl2hip_activity_chan
    ([C], hist [C, 64]; its `bins` under the name chan_bins) for the context's own channels, first to last"""
    info = ActivityInfo(C.sizeof(ActivityInfo))
    ch = np.zeros(nchan, dtype=ACTIVITY_CHAN_DTYPE)
    n = _err(Lib, Lib.vdl2hip_activity_read(ctx, C.byref(info), ch.ctypes.data, ch.size, int(reset)), "vdl2hip_activity_read")
    out = {k: getattr(info, k) for k, _ in ActivityInfo._fields_ if k not in ("struct_size", "reserved")}
    for k in ACTIVITY_CHAN_DTYPE.names:
        if k != "reserved":
            out["chan_bins" if k == "bins" else k] = ch[k][:n].copy()     # (info.bins: complete so far; chan_bins: since the last reset)
    return out


def _activity_series(Lib, ctx, chan: int, first_bin: int, count: int) -> np.ndarray:
    buf = np.zeros(max(1, count), dtype=np.float32)
    n = _err(Lib, Lib.vdl2hip_activity_series(ctx, chan, first_bin, buf.ctypes.data, count), "vdl2hip_activity_series")
    return buf[:n]


def _capture_enable(Lib, ctx, pre, post, failed_only, pool_samples) -> None:
    cfg = CaptureCfg(C.sizeof(CaptureCfg), pre, post, CAPTURE_FAILED_ONLY if failed_only else 0, pool_samples, 0)
    _err(Lib, Lib.vdl2hip_capture_enable(ctx, C.byref(cfg)), "vdl2hip_capture_enable")


def _capture_info(Lib, ctx) -> dict:
    info = CaptureInfo(C.sizeof(CaptureInfo))
    _err(Lib, Lib.vdl2hip_capture_info_get(ctx, C.byref(info)), "vdl2hip_capture_info_get")
    return {k: getattr(info, k) for k, _ in CaptureInfo._fields_ if k not in ("struct_size", "reserved", "reserved2")}


def _capture_read(Lib, ctx, cap_recs: int = 4096, cap_pairs: int = 1 << 20):
    """vdl2hip_capture_read() until nothing more comes -> (records as dicts with every field of vdl2hip_burst but `reserved`,
    their windows as complex64 arrays).  cap_recs / cap_pairs: the buffers of one call (a window longer than cap_pairs would
    never be delivered: 2^16 pairs hold any)."""
    recs = np.zeros(max(1, cap_recs), dtype=BURST_DTYPE)
    iq = np.zeros((max(1, cap_pairs), 2), dtype=np.float32)
    out, wins = [], []
    while True:
        used = C.c_size_t(0)
        n = _err(Lib, Lib.vdl2hip_capture_read(ctx, recs.ctypes.data, cap_recs, iq.ctypes.data, cap_pairs, C.byref(used)), "vdl2hip_capture_read")
        if n == 0:
            break
        for r in recs[:n]:
            d = {k: r[k].item() for k in BURST_DTYPE.names if k != "reserved"}
            off, cnt = d["iq_off"], d["iq_count"]
            wins.append(iq[off:off + cnt].copy().view(np.complex64).reshape(-1))
            out.append(d)
    return out, wins


def _txlog_enable(Lib, ctx, undecoded_only, pool_records) -> None:
    cfg = TxlogCfg(C.sizeof(TxlogCfg), pool_records, TXLOG_UNDECODED_ONLY if undecoded_only else 0, 0)
    _err(Lib, Lib.vdl2hip_txlog_enable(ctx, C.byref(cfg)), "vdl2hip_txlog_enable")


def _txlog_info(Lib, ctx) -> dict:
    info = TxlogInfo(C.sizeof(TxlogInfo))
    _err(Lib, Lib.vdl2hip_txlog_info_get(ctx, C.byref(info)), "vdl2hip_txlog_info_get")
    return {k: getattr(info, k) for k, _ in TxlogInfo._fields_ if k not in ("struct_size", "reserved", "reserved2")}


def _read_records(Lib, ctx, name: str, dtype, cap_recs: int) -> np.ndarray:
    """A record tap's read (`name`: vdl2hip_txlog_read, vdl2hip_txsearch_read) until nothing more comes -> the records as one array
    of `dtype` (cap_recs: the buffer of one call)"""
    fn = getattr(Lib, name)
    buf = np.zeros(max(1, cap_recs), dtype=dtype)
    out = []
    while True:
        n = _err(Lib, fn(ctx, buf.ctypes.data, cap_recs), name)
        if n == 0:
            break
        out.append(buf[:n].copy())
    return np.concatenate(out) if out else np.zeros(0, dtype=dtype)


def _txlog_read(Lib, ctx, cap_recs: int = 4096) -> np.ndarray:
    return _read_records(Lib, ctx, "vdl2hip_txlog_read", TX_DTYPE, cap_recs)


def _txsearch_enable(Lib, ctx, undecoded_only) -> None:
    cfg = TxsearchCfg(C.sizeof(TxsearchCfg), TXSEARCH_UNDECODED_ONLY if undecoded_only else 0)
    _err(Lib, Lib.vdl2hip_txsearch_enable(ctx, C.byref(cfg)), "vdl2hip_txsearch_enable")


def _txsearch_info(Lib, ctx) -> dict:
    info = TxsearchInfo(C.sizeof(TxsearchInfo))
    _err(Lib, Lib.vdl2hip_txsearch_info_get(ctx, C.byref(info)), "vdl2hip_txsearch_info_get")
    return {k: getattr(info, k) for k, _ in TxsearchInfo._fields_ if k not in ("struct_size", "reserved")}


def _txsearch_read(Lib, ctx, cap_recs: int = 4096) -> np.ndarray:
    return _read_records(Lib, ctx, "vdl2hip_txsearch_read", TXS_DTYPE, cap_recs)


def _relook_enable(Lib, ctx, threshold, max_anchors, max_ppm, pool_frames, pool_octets, new_only) -> None:
    cfg = RelookCfg(C.sizeof(RelookCfg), RELOOK_NEW_ONLY if new_only else 0, threshold, max_ppm, max_anchors, pool_frames, pool_octets, 0)
    _err(Lib, Lib.vdl2hip_relook_enable(ctx, C.byref(cfg)), "vdl2hip_relook_enable")


def _relook_info(Lib, ctx) -> dict:
    info = RelookInfo(C.sizeof(RelookInfo))
    _err(Lib, Lib.vdl2hip_relook_info_get(ctx, C.byref(info)), "vdl2hip_relook_info_get")
    return {k: getattr(info, k) for k, _ in RelookInfo._fields_ if k not in ("struct_size", "reserved", "reserved2")}


def unpack_frames(n, recs, octets) -> List[dict]:
    """n vdl2hip_packed_frame records and their octets -> one dict per frame"""
    out = []
    for i in range(n):
        f = recs[i].frame; off = recs[i].octets_off
        out.append(dict(chan=f.chan, freq=f.freq, idx=f.idx, octets=bytes(octets[off:off + f.len]),
                        synd_weight=f.synd_weight, datalen_octets=f.datalen_octets,
                        num_fec_corrections=f.num_fec_corrections, frame_pwr_dbfs=f.frame_pwr_dbfs,
                        nf_pwr_dbfs=f.nf_pwr_dbfs, ppm_error=f.ppm_error, burst_ord=f.burst_ord,
                        sync_sample=f.sync_sample, end_sample=f.end_sample,
                        avlc_status=f.avlc_status, dst_addr=f.dst_addr, src_addr=f.src_addr))
    return out


def _relook_read(Lib, ctx, cap_recs: int = 1024, cap_frames: int = 4096, cap_octets: int = 1 << 20):
    """vdl2hip_relook_read until nothing more comes -> (records as an array of RELOOK_DTYPE, frames as a list of dicts): record i's
    frames are frames[rec["frame_first"] : rec["frame_first"] + rec["frames"]]"""
    buf = np.zeros(max(1, cap_recs), dtype=RELOOK_DTYPE)
    pk = (PackedFrame * max(1, cap_frames))()
    po = (C.c_uint8 * max(1, cap_octets))()
    recs, frames = [], []
    while True:
        used = C.c_size_t(0)
        n = _err(Lib, Lib.vdl2hip_relook_read(ctx, buf.ctypes.data, cap_recs, pk, cap_frames, po, cap_octets, C.byref(used)), "vdl2hip_relook_read")
        if n == 0:
            break
        r = buf[:n].copy()
        nfr = int(r["frames"].sum())
        r["frame_first"] = np.where(r["frames"] > 0, r["frame_first"] + len(frames), 0)
        frames += unpack_frames(nfr, pk, memoryview(po)[:used.value])
        recs.append(r)
    return (np.concatenate(recs) if recs else np.zeros(0, dtype=RELOOK_DTYPE)), frames


def _txcap_enable(Lib, ctx, iq, spectrum, pre, post, max_iq_samples, nfft, window, pool_samples, pool_spectra, undecoded_only) -> None:
    flags = (TXCAP_IQ if iq else 0) | (TXCAP_SPECTRUM if spectrum else 0) | (TXCAP_UNDECODED_ONLY if undecoded_only else 0)
    cfg = TxcapCfg(C.sizeof(TxcapCfg), flags, pre, post, max_iq_samples, nfft, window, pool_samples, pool_spectra, 0)
    _err(Lib, Lib.vdl2hip_txcap_enable(ctx, C.byref(cfg)), "vdl2hip_txcap_enable")


def _txcap_info(Lib, ctx) -> dict:
    info = TxcapInfo(C.sizeof(TxcapInfo))
    _err(Lib, Lib.vdl2hip_txcap_info_get(ctx, C.byref(info)), "vdl2hip_txcap_info_get")
    return {k: getattr(info, k) for k, _ in TxcapInfo._fields_ if k not in ("struct_size", "reserved", "reserved2")}


def _txcap_read(Lib, ctx, cap_recs: int = 4096, cap_pairs: int = 1 << 20, cap_floats: int = 1 << 20):
    """vdl2hip_txcap_read() until nothing more comes -> (records as one array of TXC_DTYPE, with iq_off and spec_off as the calls
    gave them; their windows as complex64 arrays; their spectra as float32 arrays, empty where the record has none).  cap_*: the
    buffers of one call (a window longer than cap_pairs or a spectrum longer than cap_floats would never be delivered: 2^16 pairs
    and 1024 floats hold any)."""
    recs = np.zeros(max(1, cap_recs), dtype=TXC_DTYPE)
    iq = np.zeros((max(1, cap_pairs), 2), dtype=np.float32)
    sp = np.zeros(max(1, cap_floats), dtype=np.float32)
    out, wins, spectra = [], [], []
    while True:
        used, fused = C.c_size_t(0), C.c_size_t(0)
        n = _err(Lib, Lib.vdl2hip_txcap_read(ctx, recs.ctypes.data, cap_recs, iq.ctypes.data, cap_pairs, C.byref(used), sp.ctypes.data, cap_floats, C.byref(fused)), "vdl2hip_txcap_read")
        if n == 0:
            break
        out.append(recs[:n].copy())
        for r in recs[:n]:
            off, cnt, so = int(r["iq_off"]), int(r["iq_count"]), int(r["spec_off"])
            nfl = int(r["nfft"]) if not int(r["flags"]) & TXC_NO_SPECTRUM else 0
            wins.append(iq[off:off + cnt].copy().view(np.complex64).reshape(-1))
            spectra.append(sp[so:so + nfl].copy())
    return (np.concatenate(out) if out else np.zeros(0, dtype=TXC_DTYPE)), wins, spectra


def txcap_measure(power, nfft: int = None) -> dict:
    """vdl2hip_txcap_measure(): total, peak_bin / peak_hz, centroid_hz and the 99 % occupied bandwidth obw_hz (obw_lo .. obw_hi) of one
    power[] of a transmission capture's record.  Needs no GPU."""
    Lib = load_library()
    p = np.ascontiguousarray(power, dtype=np.float32)
    out = TxShape()
    r = Lib.vdl2hip_txcap_measure(p.ctypes.data, p.size if nfft is None else nfft, C.byref(out))
    if r != 0:
        raise Vdl2HipError(f"vdl2hip_txcap_measure: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    return {k: getattr(out, k) for k, _ in TxShape._fields_ if k != "reserved"}


def toa_template() -> np.ndarray:
    """vdl2hip_toa_template(): the unique word's waveform the burst timing tap correlates with, 151 complex64 values at the decimated
    rate - index 0 the centre of symbol 0, index 150 that of symbol 15.  Needs no GPU."""
    Lib = load_library()
    s = np.zeros((TOA_TAPS, 2), dtype=np.float32)
    _err(Lib, Lib.vdl2hip_toa_template(s.ctypes.data, TOA_TAPS), "vdl2hip_toa_template")
    return s.view(np.complex64).reshape(-1)


def _toa_enable(Lib, ctx, max_lag, failed_only, pool_curves) -> None:
    cfg = ToaCfg(C.sizeof(ToaCfg), max_lag, TOA_FAILED_ONLY if failed_only else 0, pool_curves)
    _err(Lib, Lib.vdl2hip_toa_enable(ctx, C.byref(cfg)), "vdl2hip_toa_enable")


def _toa_info(Lib, ctx) -> dict:
    info = ToaInfo(C.sizeof(ToaInfo))
    _err(Lib, Lib.vdl2hip_toa_info_get(ctx, C.byref(info)), "vdl2hip_toa_info_get")
    return {k: getattr(info, k) for k, _ in ToaInfo._fields_ if k not in ("struct_size", "reserved")}


def _toa_read(Lib, ctx, cap_recs: int = 4096, cap_floats: int = 1 << 20):
    """vdl2hip_toa_read() until nothing more comes -> (records as one array of BURST_TOA_DTYPE, with curve_off as the calls gave it;
    their curves P(-W .. W) as float32 arrays, empty where the record has none).  cap_*: the buffers of one call (65 floats hold any
    curve)."""
    recs = np.zeros(max(1, cap_recs), dtype=BURST_TOA_DTYPE)
    cv = np.zeros(max(1, cap_floats), dtype=np.float32)
    out, curves = [], []
    while True:
        used = C.c_size_t(0)
        n = _err(Lib, Lib.vdl2hip_toa_read(ctx, recs.ctypes.data, cap_recs, cv.ctypes.data, cap_floats, C.byref(used)), "vdl2hip_toa_read")
        if n == 0:
            break
        out.append(recs[:n].copy())
        for r in recs[:n]:
            nfl = int(r["nlags"]) if not int(r["flags"]) & TOA_NO_CURVE else 0
            curves.append(cv[int(r["curve_off"]):int(r["curve_off"]) + nfl].copy())
    return (np.concatenate(out) if out else np.zeros(0, dtype=BURST_TOA_DTYPE)), curves


def live_resources() -> dict:
    """Test hook: what the process holds through the library's owning types right now - device buffers, page-locked buffers, events.
    Needs no receiver and no GPU."""
    Lib = load_library()
    out = (C.c_longlong * 3)()
    r = Lib.vdl2hip_debug_live_resources(out)
    if r != 0:
        raise Vdl2HipError(f"vdl2hip_debug_live_resources: {Lib.vdl2hip_strerror(r).decode()} ({r})")
    return {"device": out[0], "pinned": out[1], "events": out[2]}


class Receiver:
    """One multi-channel VDL2 receiver on one GPU (= the reference's set of demod threads)."""

    def __init__(self, centerfreq: int, freqs: Sequence[int], oversample: int = 20, sample_fmt: int = FMT_S16LE,
                 max_ppm: float = 0.0, device: int = 0, max_block_bytes: int = 320000,
                 chan_first: int = 0, chan_count: int = 0, input_rate: int = 0):
        """sample_fmt: FMT_U8, FMT_S16LE, FMT_CF32 or FMT_S8 (signed bytes: a HackRF's format; the receiver is an FMT_S16LE one fed b << 8).
        input_rate: the rate of the IQ that will be fed, Hz; 0 = 105000 * oversample.  Any other supported rate is resampled on
        the device ahead of the channeliser (vdl2hip.h, "Resampling")."""
        self.L = load_library()
        self.freqs = list(freqs)
        self._freq_arr = (C.c_uint32 * len(self.freqs))(*self.freqs)
        cfg = Cfg(C.sizeof(Cfg), centerfreq, oversample, sample_fmt, len(self.freqs), self._freq_arr,
                  max_ppm, device, max_block_bytes, chan_first, chan_count, 0, input_rate, 0)
        h = C.c_void_p()
        self._chk(self.L.vdl2hip_create(C.byref(cfg), C.byref(h)), "vdl2hip_create")
        self.h = h
        self.chan_first = chan_first
        self.chan_count = chan_count or (len(self.freqs) - chan_first)

    def _chk(self, r, what):
        if r < 0:
            raise Vdl2HipError(f"{what}: {self.L.vdl2hip_strerror(r).decode()} ({r})")
        return r

    def close(self):
        if getattr(self, "h", None):
            self.L.vdl2hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, raw) -> None:
        """process_buf_uchar()/process_buf_short(): one block of raw IQ from host memory - any array, taken as its bytes (FMT_CF32: np.complex64
        or interleaved np.float32; FMT_S8: np.int8, interleaved)."""
        a = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self._chk(self.L.vdl2hip_feed(self.h, a.ctypes.data, a.size), "vdl2hip_feed")

    def feed_pinned(self, host_ptr: int, nbytes: int) -> None:
        """one block from page-locked host memory, queued without waiting for the copy (see vdl2hip.h for the lifetime rule)"""
        self._chk(self.L.vdl2hip_feed_pinned(self.h, C.c_void_p(host_ptr), nbytes), "vdl2hip_feed_pinned")

    def feed_device(self, dev_ptr: int, nbytes: int) -> None:
        self._chk(self.L.vdl2hip_feed_device(self.h, C.c_void_p(dev_ptr), nbytes), "vdl2hip_feed_device")

    def feed_tensor(self, t) -> None:
        """a block resident on this receiver's device (torch tensor of raw bytes / int8 / int16 values / float32 or complex64 values)"""
        self.feed_device(t.data_ptr(), t.numel() * t.element_size())

    def feed_pinned_tensor(self, t) -> None:
        """a block in page-locked host memory (torch tensor made with pin_memory())"""
        self.feed_pinned(t.data_ptr(), t.numel() * t.element_size())

    def set_drain_lag(self, lag: int) -> None:
        self._chk(self.L.vdl2hip_set_drain_lag(self.h, lag), "vdl2hip_set_drain_lag")

    def sync(self) -> None:
        self._chk(self.L.vdl2hip_sync(self.h), "vdl2hip_sync")

    def drain(self) -> List[dict]:
        out: List[dict] = []

        def cb(fp, _user):
            f = fp.contents
            out.append(dict(chan=f.chan, freq=f.freq, idx=f.idx,
                            octets=bytes(C.string_at(f.octets, f.len)) if f.len else b"",
                            synd_weight=f.synd_weight, datalen_octets=f.datalen_octets,
                            num_fec_corrections=f.num_fec_corrections, frame_pwr_dbfs=f.frame_pwr_dbfs,
                            nf_pwr_dbfs=f.nf_pwr_dbfs, ppm_error=f.ppm_error, burst_ord=f.burst_ord,
                            sync_sample=f.sync_sample, end_sample=f.end_sample,
                            avlc_status=f.avlc_status, dst_addr=f.dst_addr, src_addr=f.src_addr))

        self._cb = FRAME_CB(cb)
        self._chk(self.L.vdl2hip_drain(self.h, self._cb, None), "vdl2hip_drain")
        return out

    def drain_packed(self, cap_frames: int = 1 << 16, cap_octets: int = 1 << 24):
        """One call for all queued frames: returns (records ctypes array view, octets bytes).  Used where a Python
        callback per frame would dominate (bench.py)."""
        if getattr(self, "_pk", None) is None or len(self._pk) < cap_frames or len(self._po) < cap_octets:
            self._pk = (PackedFrame * cap_frames)()
            self._po = (C.c_uint8 * cap_octets)()
        used = C.c_size_t(0)
        n = self._chk(self.L.vdl2hip_drain_packed(self.h, self._pk, cap_frames, self._po, cap_octets, C.byref(used)), "vdl2hip_drain_packed")
        return n, self._pk, memoryview(self._po)[:used.value]

    @staticmethod
    def unpack(n, recs, octets) -> List[dict]:
        out = []
        for i in range(n):
            f = recs[i].frame; off = recs[i].octets_off
            out.append(dict(chan=f.chan, freq=f.freq, idx=f.idx, octets=bytes(octets[off:off + f.len]),
                            synd_weight=f.synd_weight, datalen_octets=f.datalen_octets,
                            num_fec_corrections=f.num_fec_corrections, frame_pwr_dbfs=f.frame_pwr_dbfs,
                            nf_pwr_dbfs=f.nf_pwr_dbfs, ppm_error=f.ppm_error, burst_ord=f.burst_ord,
                            sync_sample=f.sync_sample, end_sample=f.end_sample,
                            avlc_status=f.avlc_status, dst_addr=f.dst_addr, src_addr=f.src_addr))
        return out

    def avlc_counters(self, chan: int) -> dict:
        a = (C.c_uint64 * NUM_AVLC_COUNTERS)()
        self._chk(self.L.vdl2hip_avlc_counters(self.h, chan, a), "vdl2hip_avlc_counters")
        return dict(zip(AVLC_COUNTER_NAMES, list(a)))

    def set_avlc_filter(self, on: bool) -> None:
        self._chk(self.L.vdl2hip_set_avlc_filter(self.h, int(on)), "vdl2hip_set_avlc_filter")

    def statsd_lines(self, ns: str = "dumpvdl2", cap: int = 1 << 20) -> List[str]:
        """the reference's statsd counter traffic since the previous call, one "<ns>.<freq>.<counter>:<delta>|c" per line"""
        buf = C.create_string_buffer(cap)
        n = self._chk(self.L.vdl2hip_statsd_lines(self.h, ns.encode(), buf, cap), "vdl2hip_statsd_lines")
        return buf.raw[:n].decode().splitlines()

    def counters(self, chan: int) -> dict:
        a = (C.c_uint64 * NUM_COUNTERS)()
        self._chk(self.L.vdl2hip_counters(self.h, chan, a), "vdl2hip_counters")
        return dict(zip(COUNTER_NAMES, list(a)))

    def debug_option(self, name: str, value: int) -> None:
        """test hook of the library (not part of include/vdl2hip.h): "no_fuse", "force_timeout" """
        f = self.L.vdl2hip_debug_option
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        self._chk(f(self.h, name.encode(), value), "vdl2hip_debug_option")

    def debug_set_position(self, n: int) -> None:
        """test hook of the library (not part of include/vdl2hip.h): before the first feed, make this a receiver whose stream begins at
        input sample n (a multiple of the oversampling), at rest - every absolute index it keeps (input and decimated sample numbers,
        NCO phase, burst timing, the referee's pieces, the taps' k_on) starts there.  Refused for a fed or a resampling receiver."""
        f = self.L.vdl2hip_debug_set_position
        f.argtypes = [C.c_void_p, C.c_uint64]
        self._chk(f(self.h, n), "vdl2hip_debug_set_position")

    def exact_window(self, chan: int, n_lo: int, n_hi: int) -> bool:
        """test hook: the referee's scan over decimated samples n_lo..n_hi of one channel (True: done; read them with read_decimated)"""
        f = self.L.vdl2hip_debug_exact_window
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64]
        return bool(self._chk(f(self.h, chan, n_lo, n_hi), "vdl2hip_debug_exact_window"))

    def exact_window_many(self, chan: int, n_lo: int, n_hi: int, count: int, stride: int):
        """test hook: `count` wavefronts scan at once (channel chan + b, the stretch moved on by stride * b) -> (stretches done, kernel ms)"""
        f = self.L.vdl2hip_debug_exact_window_many
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_uint32, C.c_int64, C.POINTER(C.c_float)]
        ms = C.c_float(0)
        return self._chk(f(self.h, chan, n_lo, n_hi, count, stride, C.byref(ms)), "vdl2hip_debug_exact_window_many"), ms.value

    def scan_multi(self, chans, los, his, retry=False):
        """test hook: the stretches (chans[i], los[i] .. his[i]) made exact side by side (k_ref_scan_multi) -> (scans run, kernel ms).
        retry: as the product's launches - a scan that has not met its witness is listed and run again from further back"""
        f = self.L.vdl2hip_debug_scan_multi2
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_float)]
        ch = np.ascontiguousarray(chans, dtype=np.int32); lo = np.ascontiguousarray(los, dtype=np.int64); hi = np.ascontiguousarray(his, dtype=np.int64)
        ms = C.c_float(0)
        return self._chk(f(self.h, ch.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(ch), 1 if retry else 0, C.byref(ms)), "vdl2hip_debug_scan_multi2"), ms.value

    def read_sync(self, chan: int, first: int, count: int):
        """test hook: (pf [count, 2] = tabulated {pherr with the referee's mark as its sign, slope}, cand [count] candidate bits) of one channel"""
        f = self.L.vdl2hip_debug_read_sync
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_size_t, C.c_void_p, C.c_void_p]
        pf = np.zeros((count, 2), dtype=np.float32); cand = np.zeros(count, dtype=np.uint8)
        n = self._chk(f(self.h, chan, first, count, pf.ctypes.data, cand.ctypes.data), "vdl2hip_debug_read_sync")
        return pf[:n], cand[:n]

    def read_flags(self, chan: int, first: int, count: int) -> np.ndarray:
        """test hook: the screening tier's verdicts of one channel, one byte per sample ("the exact metric may be under the threshold");
        may reach past the last sample fed, to the end of its 64-sample word"""
        f = self.L.vdl2hip_debug_read_flags
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_size_t, C.c_void_p]
        flag = np.zeros(count, dtype=np.uint8)
        n = self._chk(f(self.h, chan, first, count, flag.ctypes.data), "vdl2hip_debug_read_flags")
        return flag[:n]

    def read_noise_floor(self, chan: int, first_update: int = 0, count: int = 1 << 20):
        """test hook: (nf [n] = mag_nf after first_update + i updates of one channel, from the history ring - entry 0 is the initial 2.0 -,
        evals = the got_sync() evaluations the noise-floor replay has accounted for)"""
        f = self.L.vdl2hip_debug_read_noise_floor
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_size_t, C.c_void_p, C.POINTER(C.c_int64)]
        nf = np.zeros(count, dtype=np.float32); ev = C.c_int64(0)
        n = self._chk(f(self.h, chan, first_update, count, nf.ctypes.data, C.byref(ev)), "vdl2hip_debug_read_noise_floor")
        return nf[:n], int(ev.value)

    def set_profiling(self, level) -> None:
        """0/False off, 1/True: time the channeliser kernel only, 2: every stage (a few percent slower)"""
        self._chk(self.L.vdl2hip_set_profiling(self.h, int(level)), "vdl2hip_set_profiling")

    def stats(self) -> dict:
        s = Stats()
        self._chk(self.L.vdl2hip_get_stats(self.h, C.byref(s)), "vdl2hip_get_stats")
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def stream(self) -> int:
        return self.L.vdl2hip_stream(self.h) or 0

    def lpf(self):
        A = (C.c_float * 3)(); B = (C.c_float * 3)()
        self._chk(self.L.vdl2hip_get_lpf(self.h, A, B), "vdl2hip_get_lpf")
        return np.array(A, dtype=np.float32), np.array(B, dtype=np.float32)

    def nco_step(self, chan: int) -> int:
        d = C.c_uint32()
        self._chk(self.L.vdl2hip_get_nco_step(self.h, chan, C.byref(d)), "vdl2hip_get_nco_step")
        return d.value

    def read_decimated(self, chan: int, first: int, count: int) -> np.ndarray:
        buf = np.zeros((count, 2), dtype=np.float32)
        n = self._chk(self.L.vdl2hip_read_decimated(self.h, chan, first, buf.ctypes.data, count), "vdl2hip_read_decimated")
        return buf[:n]

    def spectrum_enable(self, nfft: int = 1024, window: int = WIN_HANN, stride: int = 1) -> None:
        """switch the input monitor on from the next feed (vdl2hip.h, "Input monitor"): a Welch-averaged power spectrum of nfft bins
        and level statistics of the stream as fed; every stride-th segment of nfft samples is analysed.  Zeroes what was accumulated."""
        cfg = SpectrumCfg(C.sizeof(SpectrumCfg), nfft, window, stride)
        self._chk(self.L.vdl2hip_spectrum_enable(self.h, C.byref(cfg)), "vdl2hip_spectrum_enable")

    def spectrum_disable(self) -> None:
        cfg = SpectrumCfg(C.sizeof(SpectrumCfg), 0, 0, 0)
        self._chk(self.L.vdl2hip_spectrum_enable(self.h, C.byref(cfg)), "vdl2hip_spectrum_enable")

    def spectrum(self, reset: bool = False, power: bool = True) -> dict:
        """what the monitor has accumulated: every field of vdl2hip_spectrum_info and, unless power=False, `power` (float64 [nfft],
        ascending frequency, 1.0 = a full-scale tone on a bin) with `freq_hz`.  reset: zero the accumulators afterwards."""
        return _spectrum_read(self.L, self.h, reset, power)

    def channel_levels(self) -> np.ndarray:
        """dBFS in +-12.5 kHz around every channel of the receiver's frequency list, from the monitor's spectrum (float32 [nchan])"""
        out = np.zeros(len(self.freqs), dtype=np.float32)
        self._chk(self.L.vdl2hip_spectrum_channels(self.h, out.ctypes.data, out.size), "vdl2hip_spectrum_channels")
        return out

    def specgram_enable(self, line_segments: int = 16, ring_lines: int = 0) -> None:
        """switch the spectrogram on from the next feed, on top of the input monitor (vdl2hip.h, "Spectrogram"): per bin the maximum
        since enable, the quietest line, and the last ring_lines lines of line_segments analysed segments each (mean and maximum;
        ring_lines a power of two, 0: what one feed can complete, plus one)."""
        cfg = SpecgramCfg(C.sizeof(SpecgramCfg), line_segments, ring_lines, 0)
        self._chk(self.L.vdl2hip_specgram_enable(self.h, C.byref(cfg)), "vdl2hip_specgram_enable")

    def specgram_disable(self) -> None:
        self._chk(self.L.vdl2hip_specgram_disable(self.h), "vdl2hip_specgram_disable")

    def specgram(self, reset: bool = False) -> dict:
        """every field of vdl2hip_specgram_info, `max_hold` and `floor_hold` (float32 [nfft], ascending frequency, 1.0 = a full-scale
        tone on a bin) and `freq_hz`.  reset: zero the holds and their counts afterwards (lines and the ring stay)."""
        return _specgram_read(self.L, self.h, reset)

    def specgram_lines(self, first: int, count: int):
        """up to `count` lines from line `first` on -> (mean, max), float32 [lines, nfft]"""
        return _specgram_lines(self.L, self.h, first, count)

    def specgram_channels(self):
        """(peak_dbfs, floor_dbfs), float32 [nchan]: per channel of the frequency list the strongest max_hold bin and the floor_hold
        power in +-12.5 kHz (vdl2hip_specgram_channels)"""
        peak, floor = np.zeros(len(self.freqs), dtype=np.float32), np.zeros(len(self.freqs), dtype=np.float32)
        self._chk(self.L.vdl2hip_specgram_channels(self.h, peak.ctypes.data, floor.ctypes.data, peak.size), "vdl2hip_specgram_channels")
        return peak, floor

    def activity_enable(self, bin_samples: int = 105, threshold_dbfs: float = -40.0, hang_bins: int = 0, series_bins: int = 0) -> None:
        """switch the activity monitor on from the next feed (vdl2hip.h, "Activity monitor"): the power of every channel's decimated
        stream in bins of bin_samples (105 = 1 ms); a bin is busy above threshold_dbfs, a transmission bridges up to hang_bins idle bins;
        the device keeps the last series_bins values per channel (a power of two; 0: what one feed can complete)."""
        _activity_enable(self.L, self.h, bin_samples, threshold_dbfs, hang_bins, series_bins)

    def activity_disable(self) -> None:
        self._chk(self.L.vdl2hip_activity_disable(self.h), "vdl2hip_activity_disable")

    def activity(self, reset: bool = False) -> dict:
        """what the monitor has accumulated: the fields of vdl2hip_activity_info, and per field of vdl2hip_activity_chan a numpy array
        over this receiver's channels (hist: [C, 64]; bins since the last reset: chan_bins).  reset: zero the accumulators afterwards (the bin position runs on)."""
        return _activity_read(self.L, self.h, self.chan_count, reset)

    def activity_series(self, chan: int, first_bin: int, count: int) -> np.ndarray:
        """up to `count` bin powers p[first_bin ...] of channel `chan` (its index in the frequency list), float32"""
        return _activity_series(self.L, self.h, chan, first_bin, count)

    def txlog_enable(self, undecoded_only: bool = False, pool_records: int = 0) -> None:
        """switch the transmission log on from the next feed (vdl2hip.h, "Transmission log"; needs the activity monitor): one record
        per transmission the monitor sees, with the frames it yielded.  undecoded_only: deliver only transmissions without a good
        frame; pool_records: records a feed may log (0: 65 536)."""
        _txlog_enable(self.L, self.h, undecoded_only, pool_records)

    def txlog_disable(self) -> None:
        self._chk(self.L.vdl2hip_txlog_disable(self.h), "vdl2hip_txlog_disable")

    def txlog_info(self) -> dict:
        """the fields of vdl2hip_txlog_info: the configuration in force and the totals of the feeds collected so far"""
        return _txlog_info(self.L, self.h)

    def txlog_read(self, cap_recs: int = 4096) -> np.ndarray:
        """the records of the feeds collected so far (sync() or a drain first), oldest first, as an array of TX_DTYPE"""
        return _txlog_read(self.L, self.h, cap_recs)

    def txsearch_enable(self, undecoded_only: bool = False) -> None:
        """Switch the preamble search on (include/vdl2hip.h, "Preamble search"): it needs the transmission log, takes effect with the
        next feed, and searches every transmission the log closes for the reference's preamble metric"""
        _txsearch_enable(self.L, self.h, undecoded_only)

    def txsearch_disable(self) -> None:
        self._chk(self.L.vdl2hip_txsearch_disable(self.h), "vdl2hip_txsearch_disable")

    def txsearch_info(self) -> dict:
        """the fields of vdl2hip_txsearch_info: the flags in force and the totals of the feeds collected so far"""
        return _txsearch_info(self.L, self.h)

    def txsearch_read(self, cap_recs: int = 4096) -> np.ndarray:
        """the records of the feeds collected so far (sync() or a drain first), oldest first, as an array of TXS_DTYPE"""
        return _txsearch_read(self.L, self.h, cap_recs)

    def relook_enable(self, threshold: float = 0.0, max_anchors: int = 0, max_ppm: float = 0.0, pool_frames: int = 0, pool_octets: int = 0,
                      new_only: bool = False) -> None:
        """Switch the second look on (include/vdl2hip.h, "Second look"): for every transmission the log closes, a decode attempt anchored
        on every preamble in it.  Needs the preamble search enabled.  0: the defaults (threshold 4, 4 anchors, no ppm gate)."""
        _relook_enable(self.L, self.h, threshold, max_anchors, max_ppm, pool_frames, pool_octets, new_only)

    def relook_disable(self) -> None:
        self._chk(self.L.vdl2hip_relook_disable(self.h), "vdl2hip_relook_disable")

    def relook_info(self) -> dict:
        """the fields of vdl2hip_relook_info: the configuration in force and the totals of the feeds collected so far"""
        return _relook_info(self.L, self.h)

    def relook_read(self, cap_recs: int = 1024, cap_frames: int = 4096, cap_octets: int = 1 << 20):
        """the attempt records of the feeds collected so far (sync() or a drain first), oldest first, as an array of RELOOK_DTYPE, and
        their frames as a list of dicts (record i's: frames[frame_first : frame_first + frames])"""
        return _relook_read(self.L, self.h, cap_recs, cap_frames, cap_octets)

    def txcap_enable(self, iq: bool = True, spectrum: bool = True, pre: int = 0, post: int = 0, max_iq_samples: int = 0, nfft: int = 0,
                     window: int = WIN_HANN, pool_samples: int = 0, pool_spectra: int = 0, undecoded_only: bool = False) -> None:
        """Switch the transmission capture on (include/vdl2hip.h, "Transmission capture"): it needs the transmission log, takes effect
        with the next feed, and delivers of every transmission the log closes the decimated IQ (iq) and a power spectrum of nfft bins
        (spectrum).  0 for nfft, pool_samples and pool_spectra means 256, 2^20 and 1024."""
        _txcap_enable(self.L, self.h, iq, spectrum, pre, post, max_iq_samples, nfft, window, pool_samples, pool_spectra, undecoded_only)

    def txcap_disable(self) -> None:
        self._chk(self.L.vdl2hip_txcap_disable(self.h), "vdl2hip_txcap_disable")

    def txcap_info(self) -> dict:
        """the fields of vdl2hip_txcap_info: the configuration in force and the totals of the feeds collected so far"""
        return _txcap_info(self.L, self.h)

    def txcap_read(self, cap_recs: int = 4096, cap_pairs: int = 1 << 20, cap_floats: int = 1 << 20):
        """the records of the feeds collected so far (sync() or a drain first), oldest first: (array of TXC_DTYPE, list of complex64
        arrays - their IQ windows -, list of float32 arrays - their spectra, empty where a record has none)"""
        return _txcap_read(self.L, self.h, cap_recs, cap_pairs, cap_floats)

    def toa_enable(self, max_lag: int = 0, failed_only: bool = False, pool_curves: int = 0) -> None:
        """switch burst timing on from the next feed (vdl2hip.h, "Burst timing"): of every burst handed to the burst decoder the
        correlation with the unique word's waveform at 2 max_lag + 1 lags (0: 8) round the decoder's symbol clock - arrival time to a
        fraction of a sample, fit, carrier phase and offset.  failed_only: deliver only bursts without a good frame; pool_curves: the
        records of a feed that also deliver their curve (0: 4096)."""
        _toa_enable(self.L, self.h, max_lag, failed_only, pool_curves)

    def toa_disable(self) -> None:
        self._chk(self.L.vdl2hip_toa_disable(self.h), "vdl2hip_toa_disable")

    def toa_info(self) -> dict:
        """the configuration in force and the totals of the feeds collected so far (vdl2hip_toa_info)"""
        return _toa_info(self.L, self.h)

    def toa_read(self, cap_recs: int = 4096, cap_floats: int = 1 << 20):
        """the records of the feeds collected so far (sync() or a drain collects) -> (array of BURST_TOA_DTYPE, their curves)"""
        return _toa_read(self.L, self.h, cap_recs, cap_floats)

    def capture_enable(self, pre: int = 256, post: int = 32, failed_only: bool = False, pool_samples: int = 0) -> None:
        """switch the burst capture on from the next feed (vdl2hip.h, "Burst capture"): of every burst handed to the burst decoder the
        decimated IQ from `pre` samples before its sync to `post` after its last symbol, its timing and a phase-error quality figure.
        failed_only: deliver only bursts without a good frame; pool_samples: IQ pairs a feed may capture (0: 2^20)."""
        _capture_enable(self.L, self.h, pre, post, failed_only, pool_samples)

    def capture_disable(self) -> None:
        self._chk(self.L.vdl2hip_capture_disable(self.h), "vdl2hip_capture_disable")

    def capture_info(self) -> dict:
        """the configuration in force and bursts / iq_samples / iq_dropped / kernel_ms of the feeds collected so far"""
        return _capture_info(self.L, self.h)

    def capture_read(self, cap_recs: int = 4096, cap_pairs: int = 1 << 20):
        """the bursts of the feeds collected so far (sync() or drain()), oldest first: (list of dicts - the fields of vdl2hip_burst -,
        list of complex64 arrays - their IQ windows, empty where iq_count is 0)"""
        return _capture_read(self.L, self.h, cap_recs, cap_pairs)

    def read_resampled(self, first: int, count: int) -> np.ndarray:
        """up to `count` (re, im) pairs of the resampled stream r[first ...] (receivers created with input_rate; the last six feeds' are kept)"""
        buf = np.zeros((count, 2), dtype=np.float32)
        n = self._chk(self.L.vdl2hip_read_resampled(self.h, first, buf.ctypes.data, count), "vdl2hip_read_resampled")
        return buf[:n]


def _frame_dict(f):
    return dict(chan=f.chan, freq=f.freq, idx=f.idx, octets=bytes(C.string_at(f.octets, f.len)) if f.len else b"",
                synd_weight=f.synd_weight, datalen_octets=f.datalen_octets, num_fec_corrections=f.num_fec_corrections,
                frame_pwr_dbfs=f.frame_pwr_dbfs, nf_pwr_dbfs=f.nf_pwr_dbfs, ppm_error=f.ppm_error, burst_ord=f.burst_ord,
                sync_sample=f.sync_sample, end_sample=f.end_sample, avlc_status=f.avlc_status, dst_addr=f.dst_addr, src_addr=f.src_addr)


class ReceiverGroup:
    """vdl2hip_group: one receiver spread over several GPUs of this process (the C-level multi-GPU path; the per-process form
    used by bench.py is Receiver + dist.ShardedFeeder).  `devices` may name a device more than once (virtual shards)."""

    def __init__(self, centerfreq: int, freqs: Sequence[int], devices: Sequence[int], oversample: int = 20,
                 sample_fmt: int = FMT_S16LE, max_ppm: float = 0.0, max_block_bytes: int = 320000, input_rate: int = 0):
        self.L = load_library()
        self.freqs = list(freqs)
        self._freq_arr = (C.c_uint32 * len(self.freqs))(*self.freqs)
        cfg = Cfg(C.sizeof(Cfg), centerfreq, oversample, sample_fmt, len(self.freqs), self._freq_arr, max_ppm, 0, max_block_bytes, 0, 0, 0, input_rate, 0)
        dev = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        r = self.L.vdl2hip_group_create(C.byref(cfg), dev, len(devices), C.byref(h))
        if r < 0:
            raise Vdl2HipError(f"vdl2hip_group_create: {self.L.vdl2hip_strerror(r).decode()} ({r})")
        self.h = h

    def _chk(self, r, what):
        if r < 0:
            raise Vdl2HipError(f"{what}: {self.L.vdl2hip_strerror(r).decode()} ({r})")
        return r

    def feed(self, raw) -> None:
        """one block of raw IQ from host memory - any array, taken as its bytes (FMT_S8: np.int8), as Receiver.feed() takes it"""
        a = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self._chk(self.L.vdl2hip_group_feed(self.h, a.ctypes.data, a.size), "vdl2hip_group_feed")

    def feed_pinned(self, host_ptr: int, nbytes: int) -> None:
        """one block from page-locked host memory, queued without waiting for the copy"""
        self._chk(self.L.vdl2hip_group_feed_pinned(self.h, C.c_void_p(host_ptr), nbytes), "vdl2hip_group_feed_pinned")

    def sync(self) -> None:
        self._chk(self.L.vdl2hip_group_sync(self.h), "vdl2hip_group_sync")

    def set_drain_lag(self, lag: int) -> None:
        self._chk(self.L.vdl2hip_group_set_drain_lag(self.h, lag), "vdl2hip_group_set_drain_lag")

    def drain(self) -> List[dict]:
        out: List[dict] = []
        self._cb = FRAME_CB(lambda fp, _u: out.append(_frame_dict(fp.contents)))
        self._chk(self.L.vdl2hip_group_drain(self.h, self._cb, None), "vdl2hip_group_drain")
        return out

    def drain_count(self) -> int:
        """deliver (and drop) every finished frame without a callback: the number of frames (throughput loops)"""
        return self._chk(self.L.vdl2hip_group_drain(self.h, C.cast(None, FRAME_CB), None), "vdl2hip_group_drain")

    def counters(self, chan: int) -> dict:
        a = (C.c_uint64 * NUM_COUNTERS)()
        self._chk(self.L.vdl2hip_group_counters(self.h, chan, a), "vdl2hip_group_counters")
        return dict(zip(COUNTER_NAMES, list(a)))

    def size(self) -> int:
        return self.L.vdl2hip_group_size(self.h)

    def uses_rccl(self) -> bool:
        return bool(self.L.vdl2hip_group_uses_rccl(self.h))

    EXCHANGE_FORMS = {"allgather": 0, "broadcast": 1}

    def set_exchange(self, form: str) -> None:
        """how the next blocks reach the members: 'allgather' (striped ingest over every member's own PCIe link, default) or 'broadcast'"""
        self._chk(self.L.vdl2hip_group_set_exchange(self.h, self.EXCHANGE_FORMS[form]), "vdl2hip_group_set_exchange")

    def exchange(self) -> str:
        """what the last feed did"""
        return {0: "broadcast/peer-copy", 1: "broadcast/rccl", 2: "allgather/peer-copy", 3: "allgather/rccl"}.get(self.L.vdl2hip_group_exchange(self.h), "none yet")

    def stats(self) -> dict:
        """the members' statistics, summed"""
        tot = {}
        for i in range(self.size()):
            st = Stats()
            self._chk(self.L.vdl2hip_get_stats(C.c_void_p(self.L.vdl2hip_group_ctx(self.h, i)), C.byref(st)), "vdl2hip_get_stats")
            for k, _ in Stats._fields_:
                tot[k] = tot.get(k, 0) + getattr(st, k)
        return tot

    def read_decimated(self, chan: int, first: int, count: int):
        """`count` decimated (re, im) pairs of channel `chan` from the member that owns it (parity tests)"""
        for i in range(self.size()):
            ctx = self.L.vdl2hip_group_ctx(self.h, i)
            buf = np.empty(2 * count, dtype=np.float32)
            n = self.L.vdl2hip_read_decimated(C.c_void_p(ctx), chan, first, buf.ctypes.data, count)
            if n >= 0:
                return buf[:2 * n].reshape(-1, 2)
        raise Vdl2HipError("no member owns that channel")

    def debug_set_position(self, n: int) -> None:
        """Receiver.debug_set_position() for every member (test hook): the group's stream begins at input sample n"""
        f = self.L.vdl2hip_debug_set_position
        f.argtypes = [C.c_void_p, C.c_uint64]
        for i in range(self.size()):
            self._chk(f(self.member(i), n), "vdl2hip_debug_set_position")

    def member(self, i: int):
        """the context handle of member i (vdl2hip_group_ctx): what the per-context calls take - vdl2hip_spectrum_*, vdl2hip_activity_*, vdl2hip_capture_*, vdl2hip_txlog_*"""
        return C.c_void_p(self.L.vdl2hip_group_ctx(self.h, i))

    def activity_enable(self, bin_samples: int = 105, threshold_dbfs: float = -40.0, hang_bins: int = 0, series_bins: int = 0) -> None:
        """the activity monitor of every member (there is no group call: each member monitors its own channels)"""
        for i in range(self.size()):
            _activity_enable(self.L, self.member(i), bin_samples, threshold_dbfs, hang_bins, series_bins)

    def activity_disable(self) -> None:
        for i in range(self.size()):
            self._chk(self.L.vdl2hip_activity_disable(self.member(i)), "vdl2hip_activity_disable")

    def activity(self, member: int, reset: bool = False) -> dict:
        """Receiver.activity() of one member: its own channels, first to last"""
        return _activity_read(self.L, self.member(member), len(self.freqs), reset)

    def activity_series(self, chan: int, first_bin: int, count: int) -> np.ndarray:
        """Receiver.activity_series() from the member that owns channel `chan`"""
        buf = np.zeros(max(1, count), dtype=np.float32)
        for i in range(self.size()):
            n = self.L.vdl2hip_activity_series(self.member(i), chan, first_bin, buf.ctypes.data, count)
            if n >= 0:
                return buf[:n]
        raise Vdl2HipError("no member holds that channel and bin")

    def txlog_enable(self, undecoded_only: bool = False, pool_records: int = 0) -> None:
        """the transmission log of every member (there is no group call: each member logs its own channels)"""
        for i in range(self.size()):
            _txlog_enable(self.L, self.member(i), undecoded_only, pool_records)

    def txlog_disable(self) -> None:
        for i in range(self.size()):
            self._chk(self.L.vdl2hip_txlog_disable(self.member(i)), "vdl2hip_txlog_disable")

    def txlog_info(self, member: int) -> dict:
        return _txlog_info(self.L, self.member(member))

    def txlog_read(self, member: int, cap_recs: int = 4096) -> np.ndarray:
        """Receiver.txlog_read() of one member: its own channels' transmissions (chan: the index in the group's frequency list)"""
        return _txlog_read(self.L, self.member(member), cap_recs)

    def txsearch_enable(self, undecoded_only: bool = False) -> None:
        """Receiver.txsearch_enable() on every member"""
        for i in range(self.size()):
            _txsearch_enable(self.L, self.member(i), undecoded_only)

    def txsearch_disable(self) -> None:
        for i in range(self.size()):
            self._chk(self.L.vdl2hip_txsearch_disable(self.member(i)), "vdl2hip_txsearch_disable")

    def txsearch_info(self, member: int) -> dict:
        return _txsearch_info(self.L, self.member(member))

    def txsearch_read(self, member: int, cap_recs: int = 4096) -> np.ndarray:
        """Receiver.txsearch_read() of one member: its own channels' transmissions"""
        return _txsearch_read(self.L, self.member(member), cap_recs)

    def txcap_enable(self, iq: bool = True, spectrum: bool = True, pre: int = 0, post: int = 0, max_iq_samples: int = 0, nfft: int = 0,
                     window: int = WIN_HANN, pool_samples: int = 0, pool_spectra: int = 0, undecoded_only: bool = False) -> None:
        """Receiver.txcap_enable() on every member"""
        for i in range(self.size()):
            _txcap_enable(self.L, self.member(i), iq, spectrum, pre, post, max_iq_samples, nfft, window, pool_samples, pool_spectra, undecoded_only)

    def txcap_disable(self) -> None:
        for i in range(self.size()):
            self._chk(self.L.vdl2hip_txcap_disable(self.member(i)), "vdl2hip_txcap_disable")

    def txcap_info(self, member: int) -> dict:
        return _txcap_info(self.L, self.member(member))

    def txcap_read(self, member: int, cap_recs: int = 4096, cap_pairs: int = 1 << 20, cap_floats: int = 1 << 20):
        """Receiver.txcap_read() of one member: its own channels' transmissions"""
        return _txcap_read(self.L, self.member(member), cap_recs, cap_pairs, cap_floats)

    def toa_enable(self, max_lag: int = 0, failed_only: bool = False, pool_curves: int = 0) -> None:
        """burst timing of every member (there is no group call: each member times its own channels' bursts)"""
        for i in range(self.size()):
            _toa_enable(self.L, self.member(i), max_lag, failed_only, pool_curves)

    def toa_disable(self) -> None:
        for i in range(self.size()):
            self._chk(self.L.vdl2hip_toa_disable(self.member(i)), "vdl2hip_toa_disable")

    def toa_info(self, member: int) -> dict:
        return _toa_info(self.L, self.member(member))

    def toa_read(self, member: int, cap_recs: int = 4096, cap_floats: int = 1 << 20):
        """Receiver.toa_read() of one member: its own channels' bursts (chan: the index in the group's frequency list)"""
        return _toa_read(self.L, self.member(member), cap_recs, cap_floats)

    def capture_enable(self, pre: int = 256, post: int = 32, failed_only: bool = False, pool_samples: int = 0) -> None:
        """the burst capture of every member (there is no group call: each member captures its own channels' bursts)"""
        for i in range(self.size()):
            _capture_enable(self.L, self.member(i), pre, post, failed_only, pool_samples)

    def capture_disable(self) -> None:
        for i in range(self.size()):
            self._chk(self.L.vdl2hip_capture_disable(self.member(i)), "vdl2hip_capture_disable")

    def capture_info(self, member: int) -> dict:
        return _capture_info(self.L, self.member(member))

    def capture_read(self, member: int, cap_recs: int = 4096, cap_pairs: int = 1 << 20):
        """Receiver.capture_read() of one member: its own channels' bursts (chan: the index in the group's frequency list)"""
        return _capture_read(self.L, self.member(member), cap_recs, cap_pairs)

    def close(self):
        if getattr(self, "h", None):
            self.L.vdl2hip_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
