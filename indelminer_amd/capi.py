"""ctypes mirror of include/indelminer_amd.h.

Thin plumbing for the tests and bench.py: the product is the HIP library
(indelminer_amd/libindelminer_amd.so) and the C host driver above it.  There is
no CPU fallback here: if the library is missing or no gfx950 device is present,
everything raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MAX_OPS = 64
MAX_EV = 4
MAX_READ = 1020
SHORT_READ = 255        # reads beyond it take the second realign launch (Context.expect_read_length)

IM_OK = 0
E_ARG, E_NOGPU, E_HIP, E_UNSUPPORTED, E_ABORT, E_OVERFLOW = -1, -2, -3, -4, -5, -6
ST_NONE, ST_EVIDENCE, ST_ABORT, ST_OVERFLOW, ST_UNSUPPORTED = 0, 1, -1, -2, -3


class Params(C.Structure):
    _fields_ = [("klength", C.c_uint32), ("numgaps", C.c_uint32),
                ("maxdelsize", C.c_uint32), ("ethreshold", C.c_uint32)]


class Evidence(C.Structure):
    _fields_ = [("cls", C.c_int32), ("b1", C.c_int32), ("b2", C.c_int32), ("seg", C.c_int32),
                ("read_off", C.c_int32), ("lflank", C.c_int32), ("rflank", C.c_int32),
                ("nd_print", C.c_int32), ("nd_filter", C.c_int32)]


class BandAln(C.Structure):
    _fields_ = [("r1", C.c_int32), ("r2", C.c_int32), ("q1", C.c_int32), ("q2", C.c_int32),
                ("low", C.c_int32), ("votes", C.c_int32), ("win_bytes", C.c_int32), ("piece_bytes", C.c_int32)]


class ReadResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("ref_start", C.c_int32), ("n_ops", C.c_int32), ("n_ev", C.c_int32),
                ("n_band", C.c_int32), ("reserved", C.c_int32 * 7),
                ("band", BandAln * 2), ("ev", Evidence * MAX_EV), ("ops", C.c_uint32 * MAX_OPS)]


assert C.sizeof(ReadResult) == 512

# numpy view of the same record
RESULT_DTYPE = np.dtype([
    ("status", "<i4"), ("ref_start", "<i4"), ("n_ops", "<i4"), ("n_ev", "<i4"), ("n_band", "<i4"),
    ("reserved", "<i4", (7,)),
    ("band", [("r1", "<i4"), ("r2", "<i4"), ("q1", "<i4"), ("q2", "<i4"), ("low", "<i4"),
              ("votes", "<i4"), ("win_bytes", "<i4"), ("piece_bytes", "<i4")], (2,)),
    ("ev", [("cls", "<i4"), ("b1", "<i4"), ("b2", "<i4"), ("seg", "<i4"), ("read_off", "<i4"),
            ("lflank", "<i4"), ("rflank", "<i4"), ("nd_print", "<i4"), ("nd_filter", "<i4")], (MAX_EV,)),
    ("ops", "<u4", (MAX_OPS,)),
])
assert RESULT_DTYPE.itemsize == 512


class ReadBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("bases", C.c_void_p), ("base_off", C.c_void_p),
                ("tid", C.c_void_p), ("anchor", C.c_void_p), ("range_max", C.c_void_p)]


class DevBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("bases", C.c_void_p), ("base_off", C.c_void_p), ("read_len", C.c_void_p),
                ("tid", C.c_void_p), ("anchor", C.c_void_p), ("range_max", C.c_void_p), ("out", C.c_void_p),
                ("ev_cls", C.c_void_p), ("ev_b1", C.c_void_p), ("ev_b2", C.c_void_p)]


class DevRecords(C.Structure):
    _fields_ = [("n", C.c_int32), ("raw", C.c_void_p), ("rec_off", C.c_void_p), ("rec_base", C.c_int32)]


class TriageParams(C.Structure):
    _fields_ = [("qthreshold", C.c_int32), ("ethreshold_vcfcheck", C.c_uint32), ("maxpedelsize", C.c_uint32),
                ("want_depth", C.c_int32), ("defer_ranges", C.c_int32), ("restart", C.c_int32)]


class DevCands(C.Structure):
    _fields_ = [("batch", DevBatch), ("cand_rec", C.c_void_p), ("counters", C.c_void_p), ("rec_class", C.c_void_p),
                ("cap_cand", C.c_int32), ("cap_bases", C.c_int64), ("consumed", C.c_void_p)]


class KnownVariant(C.Structure):
    _fields_ = [("tid", C.c_int32), ("start", C.c_int32), ("stop", C.c_int32), ("type", C.c_int32),
                ("alt_off", C.c_int32), ("alt_len", C.c_int32)]


class CountTask(C.Structure):
    _fields_ = [("variant", C.c_int32), ("rstart", C.c_int32), ("rstop", C.c_int32), ("q_off", C.c_int32), ("q_len", C.c_int32),
                ("own_subs", C.c_int32), ("own_indels", C.c_int32), ("own_aligned", C.c_int32), ("flags", C.c_int32)]


assert C.sizeof(KnownVariant) == 24 and C.sizeof(CountTask) == 36
KNOWN_VARIANT_DTYPE = np.dtype([("tid", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("type", "<i4"), ("alt_off", "<i4"), ("alt_len", "<i4")])
COUNT_TASK_DTYPE = np.dtype([("variant", "<i4"), ("rstart", "<i4"), ("rstop", "<i4"), ("q_off", "<i4"), ("q_len", "<i4"),
                             ("own_subs", "<i4"), ("own_indels", "<i4"), ("own_aligned", "<i4"), ("flags", "<i4")])
assert KNOWN_VARIANT_DTYPE.itemsize == 24 and COUNT_TASK_DTYPE.itemsize == 36
CLS_INSERTION, CLS_DELETION = 0, 1
SC_DIRECT, SC_MAPQ_OK, SC_SPANS = 1, 2, 4

REC_SKIP, REC_COUNTED, REC_CAND_UNMAPPED, REC_CAND_PROPER, REC_PE = 0, 1, 2, 3, 4


class IMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("indelminer_amd error %d: %s" % (code, msg))
        self.code = code


_lib = None


def library_path():
    return _build.LIB


def lib():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        path = os.environ.get("INDELMINER_AMD_LIB", _build.LIB)      # diagnostic builds (profiles/) only
        if not os.path.exists(path):
            raise IMError(E_NOGPU, "libindelminer_amd.so is not built; run __graft_entry__.build()")
        L = C.CDLL(path)
        L.im_last_error.restype = C.c_char_p
        L.im_last_error.argtypes = [C.c_void_p]
        L.im_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.im_ctx_destroy.argtypes = [C.c_void_p]
        L.im_ctx_destroy.restype = None
        L.im_set_reference.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
        L.im_realign_batch.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(ReadBatch), C.c_void_p]
        L.im_cluster_sr.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        L.im_dev_realign.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(DevBatch), C.c_void_p]
        L.im_expect_read_length.argtypes = [C.c_void_p, C.c_int32]
        L.im_dev_compact_results.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_comm_unique_id.argtypes = [C.c_void_p]
        L.im_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.im_comm_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_comm_destroy.argtypes = [C.c_void_p]
        L.im_comm_destroy.restype = None
        L.im_comm_last_error.restype = C.c_char_p
        L.im_depth_build.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.im_depth_query.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_depth_query_max.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_depth_median.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_support_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_support_count.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.im_dev_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.im_dev_free.argtypes = [C.c_void_p, C.c_void_p]
        L.im_dev_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.im_dev_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.im_ctx_stream.restype = C.c_void_p
        L.im_ctx_stream.argtypes = [C.c_void_p]
        L.im_stream_sync.argtypes = [C.c_void_p, C.c_void_p]
        L.im_timer_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.im_timer_destroy.argtypes = [C.c_void_p]
        L.im_timer_destroy.restype = None
        L.im_timer_start.argtypes = [C.c_void_p, C.c_void_p]
        L.im_timer_stop.argtypes = [C.c_void_p, C.c_void_p]
        L.im_timer_elapsed_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.im_stream_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.im_stream_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.im_event_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.im_event_destroy.argtypes = [C.c_void_p]
        L.im_event_destroy.restype = None
        L.im_event_record.argtypes = [C.c_void_p, C.c_void_p]
        L.im_event_sync.argtypes = [C.c_void_p]
        L.im_stream_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_stream_wait_event.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_dev_realign_keep.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(DevBatch), C.c_void_p]
        L.im_set_insert_ranges.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p]
        L.im_dev_triage_scratch_bytes.restype = C.c_size_t
        L.im_dev_triage_scratch_bytes.argtypes = [C.c_int32]
        L.im_dev_triage.argtypes = [C.c_void_p, C.POINTER(TriageParams), C.POINTER(DevRecords), C.POINTER(DevCands),
                                    C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_dev_flush_cut.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.im_dev_groupby_scratch_bytes.restype = C.c_size_t
        L.im_dev_groupby_scratch_bytes.argtypes = [C.c_int32]
        L.im_dev_cluster_groupby.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_dev_realign_n.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(DevBatch), C.c_void_p, C.c_int32, C.c_void_p]
        L.im_dev_flush_cut_rec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.im_dev_flush_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.im_dev_flushgroup_scratch_bytes.restype = C.c_size_t
        L.im_dev_flushgroup_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.im_dev_flushgroup_scratch_init.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_dev_flush_groupby.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_dev_triage_scratch_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_dev_groupby_scratch_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_dev_cluster_groupby_n.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_depth_enable.argtypes = [C.c_void_p]
        L.im_host_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.im_host_free.argtypes = [C.c_void_p, C.c_void_p]
        L.im_dev_upload_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_depth_scan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.im_depth_reset.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.im_depth_query_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_depth_median_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_depth_query_max_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_span_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.im_dev_span_scatter.argtypes = [C.c_void_p, C.POINTER(DevRecords), C.c_void_p]
        L.im_span_scan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.im_span_reset.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.im_span_query_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_span_query_ends.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.im_span_build.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        L.im_span_query.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_pairspan_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.im_dev_pairspan_scatter.argtypes = [C.c_void_p, C.POINTER(DevRecords), C.c_void_p]
        L.im_pairspan_scan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.im_pairspan_reset.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.im_pairspan_query_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_pairspan_build.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        L.im_pairspan_query.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_clip_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.im_dev_clip_scatter.argtypes = [C.c_void_p, C.POINTER(DevRecords), C.c_void_p]
        L.im_clip_reset.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.im_clip_query_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_clip_build.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.im_clip_query.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_cliptail_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.im_dev_cliptail_scatter.argtypes = [C.c_void_p, C.POINTER(DevRecords), C.c_void_p]
        L.im_cliptail_add.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_cliptail_verify.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_cliptail_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.im_cliptail_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.im_clip_facing_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        L.im_clip_facing.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        L.im_cliptail_consensus.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_clip_peaks_tid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        L.im_clip_peaks.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        L.im_clip_crossed_tid.argtypes = [C.c_void_p] + [C.c_int32] * 8 + [C.c_void_p] * 9 + [C.POINTER(C.c_int32)]
        L.im_clip_crossed.argtypes = [C.c_void_p] + [C.c_int32] * 8 + [C.c_void_p] * 9 + [C.POINTER(C.c_int32)]
        L.im_clip_inverted_tid.argtypes = [C.c_void_p] + [C.c_int32] * 8 + [C.c_void_p] * 10 + [C.POINTER(C.c_int32)]
        L.im_clip_inverted.argtypes = [C.c_void_p] + [C.c_int32] * 8 + [C.c_void_p] * 10 + [C.POINTER(C.c_int32)]
        L.im_pairlink_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.im_dev_pairlink_scatter.argtypes = [C.c_void_p, C.POINTER(DevRecords), C.c_void_p]
        L.im_pairlink_add.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_pairlink_count.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.im_pairlink_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.im_pairlink_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.im_matelink_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.im_dev_matelink_scatter.argtypes = [C.c_void_p, C.POINTER(DevRecords), C.c_void_p]
        L.im_matelink_add.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_matelink_partner.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
        L.im_matelink_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.im_matelink_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.im_splitlink_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_char_p)]
        L.im_dev_splitlink_scatter.argtypes = [C.c_void_p, C.POINTER(DevRecords), C.c_void_p]
        L.im_splitlink_add.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        L.im_splitlink_count.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 9
        L.im_splitlink_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.im_splitlink_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.im_splitlink_junctions.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 9 + [C.POINTER(C.c_int32)]
        L.im_splitlink_overlap_enable.argtypes = [C.c_void_p]
        L.im_splitlink_add_overlap.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
        L.im_splitlink_overlap.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 3
        L.im_pairlink_stretched_enable.argtypes = [C.c_void_p]
        L.im_junction_pairs.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p] * 2
        L.im_cliptail_junction.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 5
        L.im_dev_memset.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        L.im_dev_copy_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.im_capture_begin.argtypes = [C.c_void_p, C.c_void_p]
        L.im_capture_end.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.im_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
        L.im_graph_destroy.argtypes = [C.c_void_p]
        L.im_graph_destroy.restype = None
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class DevBuf:
    """A device allocation owned through the C ABI."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        ctx._check(lib().im_dev_alloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._check(lib().im_dev_upload(self.ctx.h, self.ptr, _ptr(arr), arr.nbytes))
        return self

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._check(lib().im_dev_download(self.ctx.h, _ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().im_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class DevView:
    """A window into somebody else's device allocation (same download interface as DevBuf)."""

    def __init__(self, ctx, ptr, nbytes):
        self.ctx, self.ptr, self.nbytes = ctx, ptr, int(nbytes)

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._check(lib().im_dev_download(self.ctx.h, _ptr(out), self.ptr, out.nbytes))
        return out


class Event:
    """Stream-to-stream dependency: record on one stream, wait on another."""

    def __init__(self, ctx):
        self.ctx = ctx
        p = C.c_void_p()
        ctx._check(lib().im_event_create(ctx.h, C.byref(p)))
        self.h = p.value

    def record(self, stream):
        self.ctx._check(lib().im_event_record(self.h, stream))

    def wait(self, stream):
        self.ctx._check(lib().im_stream_wait_event(self.ctx.h, stream, self.h))

    def sync(self):
        self.ctx._check(lib().im_event_sync(self.h))

    def follow(self, src, dst):
        """record on stream src, make stream dst wait"""
        self.ctx._check(lib().im_stream_follow(self.h, src, dst))

    def close(self):
        if self.h:
            lib().im_event_destroy(self.h)
            self.h = None


def new_stream(ctx):
    p = C.c_void_p()
    ctx._check(lib().im_stream_create(ctx.h, C.byref(p)))
    return p.value


class Graph:
    """A captured sequence of im_dev_* launches: `with Graph.capture(ctx) as g: ...launches...`, then g.launch()."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = None

    @classmethod
    def capture(cls, ctx):
        return cls(ctx)

    def __enter__(self):
        self.ctx._check(lib().im_capture_begin(self.ctx.h, self.ctx.stream))
        return self

    def __exit__(self, et, ev, tb):
        p = C.c_void_p()
        rc = lib().im_capture_end(self.ctx.h, self.ctx.stream, C.byref(p))
        if et is None:
            self.ctx._check(rc)
            self.h = p.value
        return False

    def launch(self):
        self.ctx._check(lib().im_graph_launch(self.h, self.ctx.stream))

    def close(self):
        if self.h:
            lib().im_graph_destroy(self.h)
            self.h = None


class Timer:
    def __init__(self, ctx):
        self.ctx = ctx
        p = C.c_void_p()
        ctx._check(lib().im_timer_create(ctx.h, C.byref(p)))
        self.h = p.value

    def start(self, stream):
        self.ctx._check(lib().im_timer_start(self.h, stream))

    def stop(self, stream):
        self.ctx._check(lib().im_timer_stop(self.h, stream))

    def elapsed_ms(self):
        ms = C.c_float()
        self.ctx._check(lib().im_timer_elapsed_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def close(self):
        if self.h:
            lib().im_timer_destroy(self.h)
            self.h = None


class Context:
    """One GPU.  Mirrors im_ctx_* / im_set_reference / im_realign_batch / im_cluster_sr."""

    def __init__(self, device=0):
        L = lib()
        h = C.c_void_p()
        rc = L.im_ctx_create(device, C.byref(h))
        if rc != IM_OK:
            raise IMError(rc, L.im_last_error(None).decode())
        self.h = h.value
        self.stream = L.im_ctx_stream(self.h)
        self._keep = None

    def _check(self, rc, allow=()):
        if rc != IM_OK and rc not in allow:
            raise IMError(rc, lib().im_last_error(self.h).decode())
        return rc

    def close(self):
        if self.h:
            lib().im_ctx_destroy(self.h)
            self.h = None

    def set_reference(self, contigs):
        """contigs: list of bytes (upper-cased ASCII, as read_reference keeps them)."""
        n = len(contigs)
        arr = (C.c_char_p * n)(*contigs)
        lens = (C.c_int64 * n)(*[len(c) for c in contigs])
        self._check(lib().im_set_reference(self.h, n, arr, lens))
        self.contig_len = [len(c) for c in contigs]

    def expect_read_length(self, max_len):
        """reads of 256 .. MAX_READ bases occur: every realign launch is followed by the long-read kernel"""
        self._check(lib().im_expect_read_length(self.h, int(max_len)))

    def realign_batch(self, params, reads, tid, anchor, range_max, allow=()):
        """reads: list of bytes.  Returns (rc, numpy structured array of RESULT_DTYPE)."""
        n = len(reads)
        bases = np.frombuffer(b"".join(reads) + b"\0" * 8, dtype=np.uint8).copy()
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r) for r in reads], out=off[1:])
        tid = np.ascontiguousarray(tid, dtype=np.int32)
        anchor = np.ascontiguousarray(anchor, dtype=np.int32)
        range_max = np.ascontiguousarray(range_max, dtype=np.int32)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        b = ReadBatch(n, _ptr(bases), _ptr(off), _ptr(tid), _ptr(anchor), _ptr(range_max))
        rc = lib().im_realign_batch(self.h, C.byref(params), C.byref(b), _ptr(out))
        self._check(rc, allow=allow)
        return rc, out

    # one body per operation of the counted arrays (depth, span, pair-span); fn is the library function of the member
    def _scan(self, fn, tid, stream):
        self._check(fn(self.h, tid, self.stream if stream is None else stream))

    _reset = _scan

    def _build(self, fn, contig_len, start, length, *flank):
        start = np.ascontiguousarray(start, dtype=np.int32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        self._check(fn(self.h, contig_len, len(start), _ptr(start), _ptr(length), *[int(f) for f in flank]))

    def _query(self, fn, beg, end, *tid):
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        out = np.zeros(max(len(beg), 1), dtype=np.uint32)
        self._check(fn(self.h, *tid, len(beg), _ptr(beg), _ptr(end), _ptr(out)))
        return out[:len(beg)]

    def _query_tid(self, fn, tid, beg, end):
        return self._query(fn, beg, end, tid)

    # one body per operation of the keyed tables (clip tails, pair links, mate links); fn is the library function of the table
    def _keyed_enable(self, fn, *params):
        self._check(fn(self.h, *[int(p) for p in params]))

    def _keyed_scatter(self, fn, recs, stream):
        self._check(fn(self.h, C.byref(recs), self.stream if stream is None else stream))

    def _keyed_reset(self, fn, stream):
        self._check(fn(self.h, self.stream if stream is None else stream))

    def _keyed_stats(self, fn):
        stored, dropped = C.c_uint64(0), C.c_uint64(0)
        self._check(fn(self.h, C.byref(stored), C.byref(dropped)))
        return int(stored.value), int(dropped.value)

    def depth_build(self, contig_len, seg_start, seg_len):
        self._build(lib().im_depth_build, contig_len, seg_start, seg_len)

    def depth_query(self, beg, end):
        return self._query(lib().im_depth_query, beg, end)

    def depth_query_max(self, beg, end):
        """(sum, max) per query on what depth_build left: the sum over [beg, end) as depth_query gives it, and the deepest position
        of [beg - 1, end], both clipped to the contig"""
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        assert len(beg) == len(end)
        n = len(beg)
        total, deepest = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
        self._check(lib().im_depth_query_max(self.h, n, _ptr(beg), _ptr(end), _ptr(total), _ptr(deepest)))
        return total[:n], deepest[:n]

    def depth_median(self, beg, end):
        """per query the lower median of min(depth, 4095) over [beg, end); 0xFFFFFFFF for an interval that is empty after the clip"""
        return self._query(lib().im_depth_median, beg, end)

    def support_batch(self, targets, queries):
        """targets / queries: lists of bytes.  Returns int32 [n,4]: subs, indels, aligned, status."""
        n = len(targets)
        t = np.frombuffer(b"".join(targets) + b"\0" * 8, dtype=np.uint8).copy()
        q = np.frombuffer(b"".join(queries) + b"\0" * 8, dtype=np.uint8).copy()
        to = np.zeros(n + 1, np.int64); np.cumsum([len(x) for x in targets], out=to[1:])
        qo = np.zeros(n + 1, np.int64); np.cumsum([len(x) for x in queries], out=qo[1:])
        out = np.zeros((max(n, 1), 4), dtype=np.int32)
        self._check(lib().im_support_batch(self.h, n, _ptr(t), _ptr(to), _ptr(q), _ptr(qo), _ptr(out)))
        return out[:n]

    def support_count(self, variants, alts, tasks, queries):
        """variants: KNOWN_VARIANT_DTYPE array, alts: bytes, tasks: COUNT_TASK_DTYPE array, queries: bytes.
        Returns int32 [n_variants, 3]: N_all, AS, DC."""
        variants = np.ascontiguousarray(variants, dtype=KNOWN_VARIANT_DTYPE)
        tasks = np.ascontiguousarray(tasks, dtype=COUNT_TASK_DTYPE)
        a = np.frombuffer(bytes(alts) + b"\0" * 8, dtype=np.uint8).copy()
        q = np.frombuffer(bytes(queries) + b"\0" * 8, dtype=np.uint8).copy()
        out = np.zeros((max(len(variants), 1), 3), dtype=np.int32)
        self._check(lib().im_support_count(self.h, len(variants), _ptr(variants), _ptr(a), len(alts),
                                           len(tasks), _ptr(tasks), _ptr(q), len(queries), _ptr(out)))
        return out[:len(variants)]

    def set_insert_ranges(self, names, range_max):
        """names in the order they entered the reference's insert-length table; range_max = range[1] of each."""
        n = len(names)
        arr = (C.c_char_p * max(n, 1))(*[x.encode() if isinstance(x, str) else x for x in names])
        rm = np.ascontiguousarray(range_max, dtype=np.int32)
        self._check(lib().im_set_insert_ranges(self.h, n, arr, _ptr(rm)))

    def depth_enable(self):
        self._check(lib().im_depth_enable(self.h))

    def depth_scan(self, tid, stream=None):
        self._scan(lib().im_depth_scan, tid, stream)

    def depth_query_tid(self, tid, beg, end):
        return self._query_tid(lib().im_depth_query_tid, tid, beg, end)

    def depth_query_max_tid(self, tid, beg, end):
        """(sum, max) per query on contig tid (after depth_scan): the sum over [beg, end) as depth_query_tid gives it, and the deepest
        position of [beg - 1, end], both clipped to the contig"""
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        assert len(beg) == len(end)
        n = len(beg)
        total, deepest = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
        self._check(lib().im_depth_query_max_tid(self.h, int(tid), n, _ptr(beg), _ptr(end), _ptr(total), _ptr(deepest)))
        return total[:n], deepest[:n]

    def depth_median_tid(self, tid, beg, end):
        """depth_median over contig tid's run of the genome-wide array (after depth_scan)"""
        return self._query_tid(lib().im_depth_median_tid, tid, beg, end)

    def span_enable(self, flank, min_mapq):
        """the genome-wide array of reference-spanning read counts (the genotype columns), 4 bytes per reference base"""
        self._check(lib().im_span_enable(self.h, int(flank), int(min_mapq)))

    def span_scatter(self, recs, stream=None):
        """recs: a DevRecords chunk, as im_dev_triage takes it (asynchronous)"""
        self._check(lib().im_dev_span_scatter(self.h, C.byref(recs), self.stream if stream is None else stream))

    def span_scan(self, tid, stream=None):
        self._scan(lib().im_span_scan, tid, stream)

    def span_reset(self, tid, stream=None):
        self._reset(lib().im_span_reset, tid, stream)

    def span_query_tid(self, tid, beg, end):
        """per query the minimum of span[p] over [beg, end] inclusive"""
        return self._query_tid(lib().im_span_query_tid, tid, beg, end)

    def span_query_ends(self, tid, pos, slack=0):
        """per end (tid, pos), each on its own contig, the minimum of span[p] over [pos - slack, pos + slack] clipped to the contig: one
        launch for all of them (-K)"""
        tid = np.ascontiguousarray(tid, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        assert len(tid) == len(pos)
        out = np.zeros(max(len(tid), 1), dtype=np.uint32)
        self._check(lib().im_span_query_ends(self.h, len(tid), _ptr(tid), _ptr(pos), int(slack), _ptr(out)))
        return out[:len(tid)]

    def span_build(self, contig_len, run_start, run_len, flank):
        self._build(lib().im_span_build, contig_len, run_start, run_len, flank)

    def span_query(self, beg, end):
        return self._query(lib().im_span_query, beg, end)

    def pairspan_enable(self, flank, min_mapq):
        """a second genome-wide array: concordant pairs whose fragment spans a position (PAIRED_READ genotypes), 4 bytes per base"""
        self._check(lib().im_pairspan_enable(self.h, int(flank), int(min_mapq)))

    def pairspan_scatter(self, recs, stream=None):
        """recs: a DevRecords chunk, as im_dev_triage takes it (asynchronous); needs set_insert_ranges"""
        self._check(lib().im_dev_pairspan_scatter(self.h, C.byref(recs), self.stream if stream is None else stream))

    def pairspan_scan(self, tid, stream=None):
        self._scan(lib().im_pairspan_scan, tid, stream)

    def pairspan_reset(self, tid, stream=None):
        self._reset(lib().im_pairspan_reset, tid, stream)

    def pairspan_query_tid(self, tid, beg, end):
        """per query the minimum of pspan[p] over [beg, end] inclusive"""
        return self._query_tid(lib().im_pairspan_query_tid, tid, beg, end)

    def pairspan_build(self, contig_len, frag_start, frag_len, flank):
        self._build(lib().im_pairspan_build, contig_len, frag_start, frag_len, flank)

    def pairspan_query(self, beg, end):
        return self._query(lib().im_pairspan_query, beg, end)

    def clip_enable(self, min_clip, min_mapq):
        """the two genome-wide arrays of clipped-read counts (right clips at refend, left clips at pos), 8 bytes per reference base"""
        self._check(lib().im_clip_enable(self.h, int(min_clip), int(min_mapq)))

    def clip_scatter(self, recs, stream=None):
        """DevRecords -> the clipped reads of the chunk counted into both arrays (asynchronous; there is no scan)"""
        self._check(lib().im_dev_clip_scatter(self.h, C.byref(recs), self.stream if stream is None else stream))

    def clip_reset(self, tid, stream=None):
        self._reset(lib().im_clip_reset, tid, stream)

    def _clip_query(self, fn, side, beg, end, *tid):
        side = np.ascontiguousarray(side, dtype=np.uint8)
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        assert len(side) == len(beg) == len(end)
        count = np.zeros(max(len(beg), 1), dtype=np.uint32)
        pos = np.zeros(max(len(beg), 1), dtype=np.int32)
        self._check(fn(self.h, *tid, len(beg), _ptr(side), _ptr(beg), _ptr(end), _ptr(count), _ptr(pos)))
        return count[:len(beg)], pos[:len(beg)]

    def clip_query_tid(self, tid, side, beg, end):
        """per query (side 0: right clips, 1: left clips) the largest count over [beg, end] inclusive on contig tid and the
        smallest position that holds it; (0, -1) for an interval that is empty after the clip to the contig"""
        return self._clip_query(lib().im_clip_query_tid, side, beg, end, tid)

    def clip_build(self, contig_len, pos, side):
        """one contig's clip events as the caller found them: positions and sides (0: right, 1: left)"""
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        side = np.ascontiguousarray(side, dtype=np.uint8)
        assert len(pos) == len(side)
        self._check(lib().im_clip_build(self.h, contig_len, len(pos), _ptr(pos), _ptr(side)))

    def clip_query(self, side, beg, end):
        return self._clip_query(lib().im_clip_query, side, beg, end)

    def cliptail_enable(self, min_clip, min_mapq, log2_slots):
        """the keyed table of clipped bases (-V): 2^log2_slots slots of 16 bytes, half of them usable"""
        self._keyed_enable(lib().im_cliptail_enable, min_clip, min_mapq, log2_slots)

    def cliptail_scatter(self, recs, stream=None):
        """DevRecords -> one entry per clipping end of the chunk's clipped reads (asynchronous)"""
        self._keyed_scatter(lib().im_dev_cliptail_scatter, recs, stream)

    def cliptail_add(self, tid, pos, side, nbases, planes):
        """entries of contig tid as the caller found them: position, side (0: right, 1: left), bases 1 .. 32, planes[i] = (low bits, high bits)"""
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        side = np.ascontiguousarray(side, dtype=np.uint8)
        nbases = np.ascontiguousarray(nbases, dtype=np.uint8)
        planes = np.ascontiguousarray(planes, dtype=np.uint32).reshape(-1)
        assert len(pos) == len(side) == len(nbases) and len(planes) == 2 * len(pos)
        self._check(lib().im_cliptail_add(self.h, int(tid), len(pos), _ptr(pos), _ptr(side), _ptr(nbases), _ptr(planes)))

    def cliptail_verify(self, tid, pr, pl, max_shift=32):
        """per query (pr, pl) on contig tid: (v_right, v_left, shift, stored_right, stored_left); after an overflow every value is
        0xFFFFFFFF and every shift -1"""
        pr = np.ascontiguousarray(pr, dtype=np.int32)
        pl = np.ascontiguousarray(pl, dtype=np.int32)
        assert len(pr) == len(pl)
        n = len(pr)
        out = [np.zeros(max(n, 1), dtype=np.int32 if k == 2 else np.uint32) for k in range(5)]
        self._check(lib().im_cliptail_verify(self.h, int(tid), n, _ptr(pr), _ptr(pl), int(max_shift), *[_ptr(o) for o in out]))
        return tuple(o[:n] for o in out)

    def cliptail_reset(self, stream=None):
        self._keyed_reset(lib().im_cliptail_reset, stream)

    def cliptail_stats(self):
        """(entries stored, entries dropped) since the last reset"""
        return self._keyed_stats(lib().im_cliptail_stats)

    def _clip_facing(self, fn, min_reads, max_overlap, cap, *tid):
        """(pr, pl, cr, cl) of the facing piles, sorted by pr; asks again with a larger cap when there are more than cap"""
        while True:
            out = [np.zeros(max(cap, 1), dtype=np.int32 if k < 2 else np.uint32) for k in range(4)]
            found = C.c_int32(0)
            self._check(fn(self.h, *tid, int(min_reads), int(max_overlap), int(cap), *[_ptr(o) for o in out], C.byref(found)))
            if found.value <= cap:
                return tuple(o[:found.value] for o in out)
            cap = found.value

    def clip_facing_tid(self, tid, min_reads, max_overlap, cap=65536):
        """the facing piles of contig tid in the genome-wide clip arrays (-I): right clips piling up at pr with left clips piling up
        at pl in [pr - max_overlap, pr], at least min_reads on either side"""
        return self._clip_facing(lib().im_clip_facing_tid, min_reads, max_overlap, cap, int(tid))

    def clip_facing(self, min_reads, max_overlap, cap=65536):
        """the same on the arrays of the last clip_build"""
        return self._clip_facing(lib().im_clip_facing, min_reads, max_overlap, cap)

    def cliptail_consensus(self, tid, pos, side, min_cover):
        """per query (pos, side) on contig tid: (entries, len, low-bit plane, high-bit plane, agree) of the pile's per-base consensus;
        after an overflow every value is 0xFFFFFFFF"""
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        side = np.ascontiguousarray(side, dtype=np.uint8)
        assert len(pos) == len(side)
        n = len(pos)
        entries, ln, agree = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        planes = np.zeros(2 * max(n, 1), dtype=np.uint32)
        self._check(lib().im_cliptail_consensus(self.h, int(tid), n, _ptr(pos), _ptr(side), int(min_cover), _ptr(entries), _ptr(ln), _ptr(planes), _ptr(agree)))
        return entries[:n], ln[:n], planes[0:2 * n:2], planes[1:2 * n:2], agree[:n]

    def _clip_search(self, fn, kinds, cap, *args):
        """the arrays of a search that counts what it finds, asked again with a larger cap when there is more than cap; None for the
        no-answer value (n_found -1)"""
        while True:
            out = [np.zeros(max(cap, 1), dtype=k) for k in kinds]
            found = C.c_int32(0)
            self._check(fn(self.h, *[int(a) for a in args], int(cap), *[_ptr(o) for o in out], C.byref(found)))
            if found.value < 0:
                return None
            if found.value <= cap:
                return tuple(o[:found.value] for o in out)
            cap = found.value

    def clip_peaks_tid(self, tid, side, min_reads, reach, cap=65536):
        """(pos, count) of the peaks of contig tid's clipR (side 0) or clipL (side 1) in the genome-wide arrays, sorted by position"""
        return self._clip_search(lib().im_clip_peaks_tid, (np.int32, np.uint32), cap, tid, side, min_reads, reach)

    def clip_peaks(self, side, min_reads, reach, cap=65536):
        """the same on the arrays of the last clip_build"""
        return self._clip_search(lib().im_clip_peaks, (np.int32, np.uint32), cap, side, min_reads, reach)

    def pairlink_enable(self, min_mapq, log2_slots):
        """the keyed table of pair links (-M): 2^log2_slots slots of 16 bytes, half of them usable"""
        self._keyed_enable(lib().im_pairlink_enable, min_mapq, log2_slots)

    def pairlink_scatter(self, recs, stream=None):
        """DevRecords -> one link per leftmost record of a pair in an abnormal orientation (asynchronous)"""
        self._keyed_scatter(lib().im_dev_pairlink_scatter, recs, stream)

    def pairlink_add(self, tid, pos, mpos, kind):
        """links of contig tid as the caller found them: pos, mpos, kind (0: everted, 1: both forward, 2: both reverse)"""
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        mpos = np.ascontiguousarray(mpos, dtype=np.int32)
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        assert len(pos) == len(mpos) == len(kind)
        self._check(lib().im_pairlink_add(self.h, int(tid), len(pos), _ptr(pos), _ptr(mpos), _ptr(kind)))

    def pairlink_count(self, tid, kind, a0, a1, b0, b1, min_sep=0):
        """per query (kind, [a0, a1], [b0, b1]) on contig tid: the links of that kind with pos in the first interval, mpos in the second
        and mpos - pos >= min_sep; after an overflow every count is 0xFFFFFFFF"""
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        a0, a1, b0, b1 = (np.ascontiguousarray(x, dtype=np.int32) for x in (a0, a1, b0, b1))
        n = len(kind)
        assert len(a0) == len(a1) == len(b0) == len(b1) == n
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(lib().im_pairlink_count(self.h, int(tid), n, _ptr(kind), _ptr(a0), _ptr(a1), _ptr(b0), _ptr(b1), int(min_sep), _ptr(out)))
        return out[:n]

    def pairlink_reset(self, stream=None):
        self._keyed_reset(lib().im_pairlink_reset, stream)

    def pairlink_stats(self):
        """(links stored, links dropped) since the last reset"""
        return self._keyed_stats(lib().im_pairlink_stats)

    def matelink_enable(self, min_mapq, log2_slots):
        """the keyed table of mate links (-T): 2^log2_slots slots of 16 bytes, half of them usable"""
        self._keyed_enable(lib().im_matelink_enable, min_mapq, log2_slots)

    def matelink_scatter(self, recs, stream=None):
        """DevRecords -> one link per record of a pair whose mate lies on another contig (asynchronous)"""
        self._keyed_scatter(lib().im_dev_matelink_scatter, recs, stream)

    def matelink_add(self, tid, pos, mtid, mpos, kind):
        """links of contig tid as the caller found them: pos, mtid, mpos, kind (read reverse | mate reverse << 1)"""
        pos, mtid, mpos = (np.ascontiguousarray(x, dtype=np.int32) for x in (pos, mtid, mpos))
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        assert len(pos) == len(mtid) == len(mpos) == len(kind)
        self._check(lib().im_matelink_add(self.h, int(tid), len(pos), _ptr(pos), _ptr(mtid), _ptr(mpos), _ptr(kind)))

    def matelink_partner(self, tid, kind, a0, a1):
        """per query (kind, [a0, a1]) on contig tid: (n_links, mtid, n_partner, lo, hi) -- the links of that kind inside the interval,
        the contig most of their mates lie on within two neighbouring 1 024-base cells, their number and their mates' range; mtid -1: no
        link, -2: more than 256 cells; after an overflow every value is 0xFFFFFFFF (mtid, lo, hi: -1)"""
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        a0, a1 = (np.ascontiguousarray(x, dtype=np.int32) for x in (a0, a1))
        n = len(kind)
        assert len(a0) == len(a1) == n
        out = [np.zeros(max(n, 1), dtype=np.uint32 if k in (0, 2) else np.int32) for k in range(5)]
        self._check(lib().im_matelink_partner(self.h, int(tid), n, _ptr(kind), _ptr(a0), _ptr(a1), *[_ptr(o) for o in out]))
        return tuple(o[:n] for o in out)

    def matelink_reset(self, stream=None):
        self._keyed_reset(lib().im_matelink_reset, stream)

    def matelink_stats(self):
        """(links stored, links dropped) since the last reset"""
        return self._keyed_stats(lib().im_matelink_stats)

    def splitlink_enable(self, min_clip, min_mapq, log2_slots, names):
        """the keyed table of split links (-S): 2^log2_slots slots of 16 bytes, half of them usable; names: the contigs' names as the
        BAM header spells them (str or bytes; None stands for a null pointer), in tid order"""
        names = [n.encode() if isinstance(n, str) else n for n in names]
        arr = (C.c_char_p * max(len(names), 1))(*names)
        self._check(lib().im_splitlink_enable(self.h, int(min_clip), int(min_mapq), int(log2_slots), len(names), arr))

    def splitlink_scatter(self, recs, stream=None):
        """DevRecords -> one link per soft-clipped primary record whose SA:Z tag holds one entry (asynchronous)"""
        self._keyed_scatter(lib().im_dev_splitlink_scatter, recs, stream)

    def splitlink_add(self, tid, pos, side, tid2, pos2, side2):
        """links as the caller found them, six columns: end A (tid, pos, side) and end B (tid2, pos2, side2)"""
        tid, pos, tid2, pos2 = (np.ascontiguousarray(x, dtype=np.int32) for x in (tid, pos, tid2, pos2))
        side, side2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (side, side2))
        assert len(tid) == len(pos) == len(side) == len(tid2) == len(pos2) == len(side2)
        self._check(lib().im_splitlink_add(self.h, len(tid), _ptr(tid), _ptr(pos), _ptr(side), _ptr(tid2), _ptr(pos2), _ptr(side2)))

    def splitlink_count(self, tid1, side1, a0, a1, tid2, side2, b0, b1):
        """per query (tid1, side1, [a0, a1], tid2, side2, [b0, b1]): the links from the first end to the second; after an overflow
        every count is 0xFFFFFFFF"""
        tid1, a0, a1, tid2, b0, b1 = (np.ascontiguousarray(x, dtype=np.int32) for x in (tid1, a0, a1, tid2, b0, b1))
        side1, side2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (side1, side2))
        n = len(tid1)
        assert len(side1) == len(a0) == len(a1) == len(tid2) == len(side2) == len(b0) == len(b1) == n
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(lib().im_splitlink_count(self.h, n, _ptr(tid1), _ptr(side1), _ptr(a0), _ptr(a1), _ptr(tid2), _ptr(side2), _ptr(b0), _ptr(b1), _ptr(out)))
        return out[:n]

    def splitlink_reset(self, stream=None):
        self._keyed_reset(lib().im_splitlink_reset, stream)

    def splitlink_stats(self):
        """(links stored, links dropped) since the last reset"""
        return self._keyed_stats(lib().im_splitlink_stats)

    _JUNCTIONS = (np.int32, np.int32, np.uint8, np.int32, np.int32, np.uint8, np.uint32, np.uint32, np.uint32)

    def splitlink_junctions(self, window, min_links, min_span, cap=65536):
        """(tid1, pos1, side1, tid2, pos2, side2, exact, n1, n2) of the junctions the split links name by themselves (-J), sorted by
        (tid1, pos1, tid2, pos2, side1, side2): the distinct end pairs min_span apart that no pair within window at both ends beats
        on exact support, with min_links links between their windows; None once the table has overflowed"""
        return self._clip_search(lib().im_splitlink_junctions, self._JUNCTIONS, cap, window, min_links, min_span)

    def splitlink_overlap_enable(self):
        """the overlap array beside the split-link table (-H): 2 bytes per slot; behind splitlink_enable, in front of the first link"""
        self._check(lib().im_splitlink_overlap_enable(self.h))

    def splitlink_add_overlap(self, tid, pos, side, tid2, pos2, side2, d):
        """splitlink_add with a seventh column: the overlap d of every link (-32767 .. 32767; -32768: unknown)"""
        tid, pos, tid2, pos2 = (np.ascontiguousarray(x, dtype=np.int32) for x in (tid, pos, tid2, pos2))
        side, side2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (side, side2))
        d = np.ascontiguousarray(d, dtype=np.int16)
        assert len(tid) == len(pos) == len(side) == len(tid2) == len(pos2) == len(side2) == len(d)
        self._check(lib().im_splitlink_add_overlap(self.h, len(tid), _ptr(tid), _ptr(pos), _ptr(side), _ptr(tid2), _ptr(pos2), _ptr(side2), _ptr(d)))

    def splitlink_overlap(self, tid1, pos1, side1, tid2, pos2, side2, window):
        """per junction (tid1, pos1, side1, tid2, pos2, side2), the rows of splitlink_junctions: (known, median, agree) of the overlaps of
        the links between the windows around its two ends, from either; after an overflow every value is all ones (median -1)"""
        tid1, pos1, tid2, pos2 = (np.ascontiguousarray(x, dtype=np.int32) for x in (tid1, pos1, tid2, pos2))
        side1, side2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (side1, side2))
        n = len(tid1)
        assert len(pos1) == len(side1) == len(tid2) == len(pos2) == len(side2) == n
        known, median, agree = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
        self._check(lib().im_splitlink_overlap(self.h, n, _ptr(tid1), _ptr(pos1), _ptr(side1), _ptr(tid2), _ptr(pos2), _ptr(side2), int(window),
                                               _ptr(known), _ptr(median), _ptr(agree)))
        return known[:n], median[:n], agree[:n]

    def pairlink_stretched_enable(self):
        """the fourth kind of the pair links (-E), 3 STRETCHED: the normal orientation without the proper-pair flag; behind
        pairlink_enable, in front of the first link"""
        self._check(lib().im_pairlink_stretched_enable(self.h))

    def junction_pairs(self, tid1, pos1, side1, tid2, pos2, side2, reach, back, min_sep):
        """per junction (tid1, pos1, side1, tid2, pos2, side2), the rows of splitlink_junctions: (pe1, pe2), the read pairs between the
        windows of its two ends -- one contig: the pair links, pe2 = 0; two contigs: the mate links from either end; a junction whose
        table has overflowed answers 0xFFFFFFFF twice"""
        tid1, pos1, tid2, pos2 = (np.ascontiguousarray(x, dtype=np.int32) for x in (tid1, pos1, tid2, pos2))
        side1, side2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (side1, side2))
        n = len(tid1)
        assert len(pos1) == len(side1) == len(tid2) == len(pos2) == len(side2) == n
        pe1, pe2 = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        self._check(lib().im_junction_pairs(self.h, n, _ptr(tid1), _ptr(pos1), _ptr(side1), _ptr(tid2), _ptr(pos2), _ptr(side2), int(reach), int(back),
                                            int(min_sep), _ptr(pe1), _ptr(pe2)))
        return pe1[:n], pe2[:n]

    def cliptail_junction(self, tid1, p1, side1, tid2, p2, side2, max_shift=32):
        """per query of two ends (tid, position, side 0: right clips, 1: left clips): (v1, v2, shift, stored1, stored2) -- the entries of
        either end that continue in the other end's contig at the best shift; after an overflow every value is 0xFFFFFFFF and every
        shift -1"""
        tid1, p1, tid2, p2 = (np.ascontiguousarray(x, dtype=np.int32) for x in (tid1, p1, tid2, p2))
        side1, side2 = (np.ascontiguousarray(x, dtype=np.uint8) for x in (side1, side2))
        n = len(tid1)
        assert len(p1) == len(side1) == len(tid2) == len(p2) == len(side2) == n
        out = [np.zeros(max(n, 1), dtype=np.int32 if k == 2 else np.uint32) for k in range(5)]
        self._check(lib().im_cliptail_junction(self.h, n, _ptr(tid1), _ptr(p1), _ptr(side1), _ptr(tid2), _ptr(p2), _ptr(side2), int(max_shift),
                                               *[_ptr(o) for o in out]))
        return tuple(o[:n] for o in out)

    _CROSSED = (np.int32, np.int32, np.uint32, np.uint32, np.uint32, np.uint32, np.int32, np.uint32, np.uint32)

    def clip_crossed_tid(self, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap=65536):
        """(pr, pl, cr, cl, vR, vL, shift, stored right, stored left) of the crossed piles of contig tid (-U), sorted by (pr, pl): a peak
        of clipR with a peak of clipL min_len .. max_len in front of it whose clipped bases verify on either side; None once the
        clip-tail table has overflowed"""
        return self._clip_search(lib().im_clip_crossed_tid, self._CROSSED, cap, tid, min_reads, reach, min_len, max_len, max_shift, min_verified)

    def clip_crossed(self, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap=65536):
        """the same on the arrays of the last clip_build, which must be contig tid's"""
        return self._clip_search(lib().im_clip_crossed, self._CROSSED, cap, tid, min_reads, reach, min_len, max_len, max_shift, min_verified)

    _INVERTED = (np.uint8, np.int32, np.int32, np.uint32, np.uint32, np.uint32, np.uint32, np.int32, np.uint32, np.uint32)

    def clip_inverted_tid(self, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap=65536):
        """(side, x, y, c1, c2, v1, v2, shift, stored at x, stored at y) of the inverted piles of contig tid (-N), sorted by (x, y, side):
        two peaks of ONE clip array (side 0 clipR, 1 clipL) min_len .. max_len apart whose clipped bases are the complement of the
        reference running backwards from the other peak; None once the clip-tail table has overflowed"""
        return self._clip_search(lib().im_clip_inverted_tid, self._INVERTED, cap, tid, min_reads, reach, min_len, max_len, max_shift, min_verified)

    def clip_inverted(self, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap=65536):
        """the same on the arrays of the last clip_build, which must be contig tid's"""
        return self._clip_search(lib().im_clip_inverted, self._INVERTED, cap, tid, min_reads, reach, min_len, max_len, max_shift, min_verified)

    def cluster_sr(self, cls, b1, b2, marker=2**31 - 1, tie_desc=0):
        n = len(cls)
        cls = np.ascontiguousarray(cls, dtype=np.int32)
        b1 = np.ascontiguousarray(b1, dtype=np.int32)
        b2 = np.ascontiguousarray(b2, dtype=np.int32)
        order = np.zeros(max(n, 1), dtype=np.int32)
        first = np.zeros(max(n, 1), dtype=np.int32)
        count = np.zeros(max(n, 1), dtype=np.int32)
        used = np.zeros(max(n, 1), dtype=np.uint8)
        ncl = C.c_int32(0)
        self._check(lib().im_cluster_sr(self.h, n, _ptr(cls), _ptr(b1), _ptr(b2), marker, tie_desc,
                                        _ptr(order), _ptr(first), _ptr(count), _ptr(used), C.byref(ncl)))
        k = ncl.value
        return order[:n], first[:k], count[:k], used[:n], k


class Pipeline:
    """The device-resident hot path the product driver runs per batch of contigs (indelminer_amd/host):
    records -> triage (a1) -> realign (a2-a11) -> flush cuts -> group-by (a12).  Everything stays in HBM
    between the stages; this class only owns the buffers and issues the im_dev_* calls in order."""

    def __init__(self, ctx, n_records, raw_bytes, cap_cand, read_len_max=256, n_pe=0, n_flushes=64, want_depth=False,
                 qthreshold=10, ethreshold_vcfcheck=10, maxpedelsize=1000000, input_from=None):
        L = lib()
        self.ctx = ctx
        self.n_records = int(n_records)
        self.cap_cand = int(cap_cand)
        self.n_pe = int(n_pe)
        self.cap_bases = self.cap_cand * ((read_len_max + 3) // 4 * 4) + 64
        self.n_slots = self.cap_cand * MAX_EV + self.n_pe        # split-read slots, then the host's paired-read entries
        if input_from is not None:          # several output sets over one resident record buffer (bench.py's pipelined steps)
            self.d_raw, self.d_off = input_from.d_raw, input_from.d_off
        else:
            self.d_raw = DevBuf(ctx, raw_bytes + 64)
            self.d_off = DevBuf(ctx, 4 * (n_records + 1))
        self.d_bases = DevBuf(ctx, self.cap_bases)
        self.d_boff = DevBuf(ctx, 8 * self.cap_cand)
        self.d_len = DevBuf(ctx, 4 * self.cap_cand)
        self.d_tid = DevBuf(ctx, 4 * self.cap_cand)
        self.d_anchor = DevBuf(ctx, 4 * self.cap_cand)
        self.d_range = DevBuf(ctx, 4 * self.cap_cand)
        self.d_res = DevBuf(ctx, 512 * self.cap_cand)
        self.d_cls = DevBuf(ctx, 4 * self.n_slots)
        self.d_b1 = DevBuf(ctx, 4 * self.n_slots)
        self.d_b2 = DevBuf(ctx, 4 * self.n_slots)
        self.d_consumed = DevBuf(ctx, 4 * self.n_slots)
        self.d_cand_rec = DevBuf(ctx, 4 * self.cap_cand)
        self.d_counters = DevBuf(ctx, 64)
        self.d_class = DevBuf(ctx, max(n_records, 1))
        self.ts_bytes = L.im_dev_triage_scratch_bytes(n_records)
        self.d_ts = DevBuf(ctx, self.ts_bytes)
        ctx._check(L.im_dev_triage_scratch_init(ctx.h, n_records, self.d_ts.ptr, self.ts_bytes, ctx.stream))
        self.d_cut = DevBuf(ctx, 8 * max(n_flushes, 1))
        self.n_flushes = n_flushes
        self.d_order = DevBuf(ctx, 4 * self.n_slots)
        # {clusters, nodes, 0, 0} then the 16-byte cluster keys, contiguous: the unit a rank contributes to the all-gather
        self.d_clbuf = DevBuf(ctx, 16 + 16 * self.n_slots)
        self.d_counts = DevView(ctx, self.d_clbuf.ptr, 16)
        self.d_clkey = DevView(ctx, self.d_clbuf.ptr + 16, 16 * self.n_slots)
        self.d_clfirst = DevBuf(ctx, 4 * self.n_slots)
        self.d_clcount = DevBuf(ctx, 4 * self.n_slots)
        self.gs_bytes = L.im_dev_groupby_scratch_bytes(self.n_slots)
        self.d_gs = DevBuf(ctx, self.gs_bytes)
        ctx._check(L.im_dev_groupby_scratch_init(ctx.h, self.n_slots, self.d_gs.ptr, self.gs_bytes, ctx.stream))
        # the chip-wide form (im_dev_flush_groupby): its own table + the range-minimum tree over the flush list
        self.fg_bytes = L.im_dev_flushgroup_scratch_bytes(self.cap_cand * MAX_EV, max(n_flushes, 1))
        self.d_fg = DevBuf(ctx, self.fg_bytes)
        ctx._check(L.im_dev_flushgroup_scratch_init(ctx.h, self.cap_cand * MAX_EV, max(n_flushes, 1), self.d_fg.ptr, self.fg_bytes, ctx.stream))
        ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
        self.batch = DevBatch(0, self.d_bases.ptr, self.d_boff.ptr, self.d_len.ptr, self.d_tid.ptr, self.d_anchor.ptr,
                              self.d_range.ptr, self.d_res.ptr, self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr)
        self.cands = DevCands(self.batch, self.d_cand_rec.ptr, self.d_counters.ptr, self.d_class.ptr, self.cap_cand, self.cap_bases, None)
        # the same with the flush marks of new candidates cleared by the triage itself (bind_async: no fill per pass)
        self.cands_clear = DevCands(self.batch, self.d_cand_rec.ptr, self.d_counters.ptr, self.d_class.ptr, self.cap_cand, self.cap_bases,
                                    self.d_consumed.ptr)
        self.recs = DevRecords(self.n_records, self.d_raw.ptr, self.d_off.ptr, 0)
        self.tp = TriageParams(qthreshold, ethreshold_vcfcheck, maxpedelsize, 1 if want_depth else 0, 0, 0)
        self.P = params()
        self.n_cand = None

    def upload(self, raw, rec_off):
        self.d_raw.upload(raw)
        self.d_off.upload(rec_off)

    def set_pe(self, b1, b2):
        """the host's paired-read evidence: entries behind the split-read slots, class 2"""
        n = len(b1)
        assert n <= self.n_pe
        base = self.cap_cand * MAX_EV
        L = lib()
        for buf, arr in ((self.d_cls, np.full(n, 2, np.int32)), (self.d_b1, np.asarray(b1, np.int32)), (self.d_b2, np.asarray(b2, np.int32))):
            if n:
                self.ctx._check(L.im_dev_upload(self.ctx.h, buf.ptr + 4 * base, _ptr(np.ascontiguousarray(arr)), 4 * n))

    def triage(self, stream=None):
        """resets the running counters and the consumed marks, then classifies + compacts the records (asynchronous)"""
        L = lib()
        st = self.ctx.stream if stream is None else stream
        c = self.ctx._check
        c(L.im_dev_memset(self.ctx.h, self.d_counters.ptr, 0, 64, st))
        c(L.im_dev_memset(self.ctx.h, self.d_consumed.ptr, 0, 4 * self.n_slots, st))
        c(L.im_dev_memset(self.ctx.h, self.d_cut.ptr, 0xFF, 8 * self.n_flushes, st))
        c(L.im_dev_triage(self.ctx.h, C.byref(self.tp), C.byref(self.recs), C.byref(self.cands), self.d_ts.ptr, self.ts_bytes, st))

    def triage_append(self, n, rec_base, restart=False, defer=False, stream=None, clear=False):
        """the triage of the n records now in the record buffer the way the product issues it chunk after chunk: no memset in front,
        the candidates go behind those the running counters hold (restart: the call opens a new batch whatever the counters hold),
        cand_rec counts from rec_base.  clear: the call also clears the flush marks of its new candidates (asynchronous)"""
        st = self.ctx.stream if stream is None else stream
        tp = TriageParams(self.tp.qthreshold, self.tp.ethreshold_vcfcheck, self.tp.maxpedelsize, self.tp.want_depth,
                          1 if defer else 0, 1 if restart else 0)
        recs = DevRecords(int(n), self.d_raw.ptr, self.d_off.ptr, int(rec_base))
        self.ctx._check(lib().im_dev_triage(self.ctx.h, C.byref(tp), C.byref(recs), C.byref(self.cands_clear if clear else self.cands),
                                            self.d_ts.ptr, self.ts_bytes, st))

    def fetch_counts(self):
        """the one host synchronisation of a batch: candidates found (sizes the realign grid)"""
        self.sync()                         # the context's stream does not synchronise with the copy below by itself
        c = self.d_counters.download(np.int32, 8)
        self.n_cand = int(c[0])
        return c

    def realign(self, stream=None):
        st = self.ctx.stream if stream is None else stream
        self.batch.n = self.n_cand
        self.ctx._check(lib().im_dev_realign_keep(self.ctx.h, C.byref(self.P), C.byref(self.batch), st))

    def flush(self, k, cand_hi, pe_hi, marker, cand_lo=0, stream=None):
        """flush number k (0-based; its id is k + 1): pending split-read slots of candidates [cand_lo, cand_hi) and
        paired-read entries [0, pe_hi)"""
        st = self.ctx.stream if stream is None else stream
        base = self.cap_cand * MAX_EV
        self.ctx._check(lib().im_dev_flush_cut(self.ctx.h, self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr, self.d_consumed.ptr,
                                               cand_lo * MAX_EV, cand_hi * MAX_EV, base, base + pe_hi, marker, k + 1,
                                               self.d_cut.ptr + 8 * k, st))

    def groupby(self, tie_desc=0, stream=None):
        st = self.ctx.stream if stream is None else stream
        n = self.n_cand * MAX_EV
        self.ctx._check(lib().im_dev_cluster_groupby(self.ctx.h, n, self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr, self.d_consumed.ptr,
                                                     tie_desc, self.d_order.ptr, self.d_clkey.ptr, self.d_clfirst.ptr, self.d_clcount.ptr,
                                                     self.d_counts.ptr, self.d_gs.ptr, self.gs_bytes, st))

    # ---- the same three stages without a host round trip: the candidate count stays on the device ----
    @staticmethod
    def flush_descs(flushes):
        """im_flush_desc[] for [(rec0, rec1, pe_hi, marker)]: a change of rec0 opens a new contig; `last` = the contig's last flush"""
        n = len(flushes)
        desc = np.zeros((max(n, 1), 8), dtype=np.int32)
        for k, (rec0, rec1, pe_hi, marker) in enumerate(flushes):
            desc[k, :6] = (rec0, rec1, 0, pe_hi, marker, k + 1)
        k = 0
        while k < n:
            e = k
            while e + 1 < n and flushes[e + 1][0] == flushes[k][0]:
                e += 1
            desc[k:e + 1, 6] = e
            k = e + 1
        return desc[:n] if n else desc[:0]

    def flush_groupby(self, flushes, tie_desc=0, stream=None, cand_bound=None):
        """the flush list and the group-by chip-wide (im_dev_flush_groupby): three launches, no history"""
        st = self.ctx.stream if stream is None else stream
        desc = self.flush_descs(flushes)
        self.d_desc = DevBuf(self.ctx, max(desc.nbytes, 32)).upload(desc)
        self.ctx._check(lib().im_dev_flush_groupby(
            self.ctx.h, self.d_desc.ptr, len(flushes), self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr, self.d_consumed.ptr,
            self.d_cand_rec.ptr, self.d_counters.ptr, self.cap_cand if cand_bound is None else cand_bound, self.cap_cand * MAX_EV, self.n_pe, tie_desc,
            self.d_order.ptr, self.d_clkey.ptr, self.d_clfirst.ptr, self.d_clcount.ptr, self.d_counts.ptr, self.d_fg.ptr, self.fg_bytes, st))

    def bind_async(self, flushes, stream, tie_desc=0, grid_bound=None, one_launch_flushes=True, depth_tid=None, wide=False):
        """pre-binds one whole pass (triage -> realign -> flush cuts -> group-by) on `stream`; flushes =
        [(rec0, rec1, pe_hi, marker)] with record bounds.  Returns a list of (fn, args) to call in order.
        wide: the flush list + group-by as im_dev_flush_groupby (three chip-wide launches) instead of the
        one-workgroup flush list + the four group-by launches."""
        L = lib()
        h = self.ctx.h
        base = self.cap_cand * MAX_EV
        self.batch_bound = DevBatch(min(self.cap_cand, grid_bound or self.cap_cand), self.d_bases.ptr, self.d_boff.ptr, self.d_len.ptr,
                                    self.d_tid.ptr, self.d_anchor.ptr, self.d_range.ptr, self.d_res.ptr, self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr)
        # a pass over one resident chunk opens a new batch with its one triage call: tp.restart instead of a counters memset
        self.tp_restart = TriageParams(self.tp.qthreshold, self.tp.ethreshold_vcfcheck, self.tp.maxpedelsize, self.tp.want_depth, 0, 1)
        calls = []
        if depth_tid is not None:           # the contig goes through triage again: its run of the depth array starts from zeros
            calls.append((L.im_depth_reset, (h, depth_tid, stream)))
        if not one_launch_flushes and not wide:
            calls += [(L.im_dev_memset, (h, self.d_consumed.ptr, 0, 4 * self.n_slots, stream)),
                      (L.im_dev_memset, (h, self.d_cut.ptr, 0xFF, 8 * self.n_flushes, stream))]
        calls += [(L.im_dev_triage, (h, C.byref(self.tp_restart), C.byref(self.recs), C.byref(self.cands_clear if (one_launch_flushes and not wide) else self.cands),
                                     self.d_ts.ptr, self.ts_bytes, stream)),
                  (L.im_dev_realign_n, (h, C.byref(self.P), C.byref(self.batch_bound), self.d_counters.ptr, 1, stream))]
        self.realign_call_index = len(calls) - 1
        self.triage_call_index = len(calls) - 2
        if depth_tid is not None:           # the contig's records are all in: difference array -> depths (DP= queries of the replay)
            calls.append((L.im_depth_scan, (h, depth_tid, stream)))
        if wide:
            desc = self.flush_descs(flushes)
            self.d_desc = DevBuf(self.ctx, max(desc.nbytes, 32)).upload(desc)
            calls.append((L.im_dev_flush_groupby, (h, self.d_desc.ptr, len(flushes), self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr, self.d_consumed.ptr,
                                                   self.d_cand_rec.ptr, self.d_counters.ptr, self.batch_bound.n, base, self.n_pe, tie_desc,
                                                   self.d_order.ptr, self.d_clkey.ptr, self.d_clfirst.ptr, self.d_clcount.ptr, self.d_counts.ptr,
                                                   self.d_fg.ptr, self.fg_bytes, stream)))
            return calls
        if one_launch_flushes:
            desc = self.flush_descs(flushes)
            self.d_desc = DevBuf(self.ctx, max(desc.nbytes, 32)).upload(desc)
            calls.append((L.im_dev_flush_cuts, (h, self.d_desc.ptr, len(flushes), self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr, self.d_consumed.ptr,
                                                self.d_cand_rec.ptr, self.d_counters.ptr, self.cap_cand, base, self.n_pe, stream)))
        else:
            for k, (rec0, rec1, pe_hi, marker) in enumerate(flushes):
                calls.append((L.im_dev_flush_cut_rec, (h, self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr, self.d_consumed.ptr, rec0, rec1,
                                                       self.d_cand_rec.ptr, self.d_counters.ptr, self.cap_cand, base, base + pe_hi, marker, k + 1,
                                                       self.d_cut.ptr + 8 * k, stream)))
        calls.append((L.im_dev_cluster_groupby_n, (h, self.batch_bound.n * MAX_EV, self.d_counters.ptr, self.d_cls.ptr, self.d_b1.ptr, self.d_b2.ptr,
                                                   self.d_consumed.ptr, tie_desc, self.d_order.ptr, self.d_clkey.ptr, self.d_clfirst.ptr,
                                                   self.d_clcount.ptr, self.d_counts.ptr, self.d_gs.ptr, self.gs_bytes, stream)))
        return calls

    def sync(self, stream=None):
        self.ctx._check(lib().im_stream_sync(self.ctx.h, self.ctx.stream if stream is None else stream))

    def clusters(self):
        """(key[n,4] = flush id, class, b1, b2; first; count; order) after groupby + sync"""
        k, nodes = (int(x) for x in self.d_counts.download(np.int32, 2))
        key = self.d_clkey.download(np.int32, 4 * max(k, 1)).reshape(-1, 4)[:k]
        return key, self.d_clfirst.download(np.int32, max(k, 1))[:k], self.d_clcount.download(np.int32, max(k, 1))[:k], \
            self.d_order.download(np.int32, max(nodes, 1))[:nodes]


COMM_ID_BYTES = 128


def comm_unique_id():
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().im_comm_unique_id(buf)
    if rc != IM_OK:
        raise IMError(rc, lib().im_comm_last_error().decode())
    return buf.raw


class Comm:
    """RCCL communicator over the C ABI (one all-gather of cluster lists per step)."""

    def __init__(self, ctx, id_bytes, rank, world):
        self.ctx, self.rank, self.world = ctx, rank, world
        h = C.c_void_p()
        rc = lib().im_comm_init(ctx.h, id_bytes, rank, world, C.byref(h))
        if rc != IM_OK:
            raise IMError(rc, lib().im_comm_last_error().decode())
        self.h = h.value

    def allgather(self, send_ptr, recv_ptr, bytes_per_rank, stream):
        rc = lib().im_comm_allgather(self.h, send_ptr, recv_ptr, bytes_per_rank, stream)
        if rc != IM_OK:
            raise IMError(rc, lib().im_comm_last_error().decode())

    def close(self):
        if self.h:
            lib().im_comm_destroy(self.h)
            self.h = None


def params(klength=6, numgaps=0, maxdelsize=1000, ethreshold=10):
    return Params(klength, numgaps, maxdelsize, ethreshold)
