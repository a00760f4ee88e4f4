"""What tests/test_gpu_clip.py and tests/test_clip_host.py share: the plain restatement of the clipped-read counts (-C), written
from the definition in include/indelminer_amd.h (seam 5, "Clipped reads"), not from the code under test.
tests/test_clip_host.py pins it to cases worked by hand (no GPU needed).

A record is (tid, pos, mapq, flag, [(op, length)]) with the BAM operation codes M I D N S H P = X = 0 .. 8.  It is eligible iff
its flag has none of 0x4 | 0x100 | 0x200 | 0x400, 0 <= tid < contigs, mapq >= q and its CIGAR has an M / = / X / D / N.  With
first / last = its first / last operation that is not H and refend = pos + the lengths of its M / = / X / D / N:
  last is S of >= min_clip bases and 0 <= refend <= clen   ->  clipR[refend] += 1
  first is S of >= min_clip bases and 0 <= pos <= clen     ->  clipL[pos] += 1
A query (side, beg, end) answers the largest count over [beg, end] clipped to [0, clen] and the smallest position holding it,
(0, -1) when nothing is left of the interval.
"""
import struct

import numpy as np

EXCLUDED = 0x4 | 0x100 | 0x200 | 0x400
REF_OPS = (0, 2, 3, 7, 8)
OP_S, OP_H = 4, 5
RIGHT, LEFT = 0, 1
MIN_LEN, SLACK, MIN_CLIP = 50, 10, 20      # what the host driver uses: END - POS of the shortest record, the windows' slack, -C's min_clip


def events_of(rec, clens, min_clip, q):
    """[(tid, side, position)] of one record"""
    tid, pos, mapq, flag, cigar = rec[:5]
    if flag & EXCLUDED or not 0 <= tid < len(clens) or mapq < q:
        return []
    if not any(op in REF_OPS for op, _ in cigar):
        return []
    seen = [(op, ln) for op, ln in cigar if op != OP_H]
    refend = pos + sum(ln for op, ln in cigar if op in REF_OPS)
    clen = clens[tid]
    ev = []
    if seen[-1][0] == OP_S and seen[-1][1] >= min_clip and 0 <= refend <= clen:
        ev.append((tid, RIGHT, refend))
    if seen[0][0] == OP_S and seen[0][1] >= min_clip and 0 <= pos <= clen:
        ev.append((tid, LEFT, pos))
    return ev


def arrays_of(records, clens, min_clip, q):
    """(clipR, clipL): per contig an int64 array of clen + 1 counts"""
    out = ([np.zeros(l + 1, np.int64) for l in clens], [np.zeros(l + 1, np.int64) for l in clens])
    for rec in records:
        for tid, side, p in events_of(rec, clens, min_clip, q):
            out[side][tid][p] += 1
    return out


def argmax(arr, beg, end):
    """(count, position) of one query on one contig's array (clen + 1 entries)"""
    a, b = max(int(beg), 0), min(int(end), len(arr) - 1)
    if a > b:
        return 0, -1
    best, at = -1, -1
    for p in range(a, b + 1):
        if arr[p] > best:              # strictly: the smallest position among equal counts stays
            best, at = int(arr[p]), p
    return best, at


def argmax_many(right, left, side, beg, end):
    """the same through numpy, for many queries on one contig; the tests check it against argmax first"""
    clen = len(right) - 1
    cnt, pos = [], []
    for s, a, b in zip(side, beg, end):
        a, b = max(int(a), 0), min(int(b), clen)
        if a > b:
            cnt.append(0); pos.append(-1)
            continue
        seg = (left if s else right)[a:b + 1]
        k = int(np.argmax(seg))        # numpy returns the first of equal maxima
        cnt.append(int(seg[k])); pos.append(a + k)
    return np.array(cnt, np.int64), np.array(pos, np.int64)


def windows_of(kind, pos, end, bp_end):
    """((clipR beg, end), (clipL beg, end)) in array coordinates of a DELETION record found by `kind`, printed at POS, END, BP_END"""
    w, amb, hi = SLACK, max(0, bp_end - end), max(end, bp_end)
    if kind == "PAIRED_READ":
        return (pos - w, hi + w), (pos - w, hi + w)
    return (pos - w, pos + amb + w), (end - 1 - w, end - 1 + amb + w)


def evidence_of(right, left, kind, pos, end, bp_end):
    """(CB text, CS text, (count left of the deletion, count right of it)) of a qualifying record: a right clip at array position
    p is the coordinate p, a left clip at p is p + 1; a side without clipped reads prints . and 0"""
    (rb, re_), (lb, le) = windows_of(kind, pos, end, bp_end)
    cr, pr = argmax(right, rb, re_)
    cl, pl = argmax(left, lb, le)
    cb = "%s,%s" % (str(pr) if cr > 0 else ".", str(pl + 1) if cl > 0 else ".")
    return cb, "%d,%d" % (cr, cl), (cr, cl)


def parse_record(b, o, _end):
    """one BAM record at b[o:] -> (tid, pos, mapq, flag, cigar); the CIGAR lies in front of the bases, with qualities or without"""
    tid, pos, l_qname, mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", b, o)
    cw = struct.unpack_from("<%dI" % n_cig, b, o + 32 + l_qname)
    return tid, pos, mapq, flag, [(c & 15, c >> 4) for c in cw]


def arrays_of_bam(bam, min_clip, q):
    from tests.support import spanarrays
    refs, recs = spanarrays.read_bam_records(bam, parse_record=parse_record)
    right, left = arrays_of(recs, [l for _, l in refs], min_clip, q)
    return [n for n, _ in refs], right, left
