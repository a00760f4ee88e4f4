"""Device-layout records of plain matching reads at chosen places: what a test or a probe needs to put chosen events into a
genome-wide difference array through the product's own scatter kernels (host-side data tooling, no compute path).

A read of `bases` bases at (tid, pos) with the CIGAR <bases>M, flag 0, mapping quality 60 and an MQ tag: the pileup depth gets +1 at
pos and -1 at pos + bases; the span array of flank m gets +1 at pos + m and -1 at pos + bases - m + 1 when bases >= 2 m.
"""
import numpy as np

BASES = 4

_REC = np.dtype([("tid", "<i4"), ("pos", "<i4"), ("l_qname", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                 ("l_seq", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("isize", "<i4"),
                 ("qname", "S4"), ("cigar", "<u4"), ("seq", "u1", ((BASES + 1) // 2,)), ("qual", "u1", (BASES,)), ("mq", "u1", (4,)),
                 ("pad", "u1", (2,))])
assert _REC.itemsize == 52 and _REC.itemsize % 4 == 0


def match_records(tid, pos):
    """tid, pos: equal-length integer arrays, sorted by (tid, pos) as a coordinate-sorted file delivers them.
    Returns (raw uint8 with 64 spare bytes behind the last record, rec_off uint32[n + 1])."""
    tid = np.asarray(tid, np.int32); pos = np.asarray(pos, np.int32)
    n = len(tid)
    r = np.zeros(n, _REC)
    r["tid"] = tid; r["pos"] = pos; r["l_qname"] = 4; r["mapq"] = 60; r["bin"] = 4680; r["n_cigar"] = 1; r["flag"] = 0
    r["l_seq"] = BASES; r["mtid"] = -1; r["mpos"] = -1; r["isize"] = 0
    r["qname"] = b"abc"; r["cigar"] = (BASES << 4) | 0; r["seq"] = 0x11; r["qual"] = 0x28
    r["mq"] = np.frombuffer(b"MQC\x3c", np.uint8)
    raw = np.concatenate([r.view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])
    off = (np.arange(n + 1, dtype=np.int64) * _REC.itemsize).astype(np.uint32)
    return raw, off
