"""What tests/test_gpu_cliptail.py and tests/test_cliptail_host.py share: the plain restatement of the clip tails (-V), written from the
definition in include/indelminer_amd.h (seam 5, "Clip tails"), not from the code under test.  tests/test_cliptail_host.py pins it to
cases worked by hand (no GPU needed).  The record rule is -C's and comes from tests/support/clipcounts.py.

A record is (tid, pos, mapq, flag, [(op, length)], l_seq, codes): codes are the l_seq 4-bit base codes of the record as BAM packs them
(= A C M G R S V T W Y H K D B N = 0 .. 15), or None when the packed bases do not lie inside the record.  An ENTRY is
(tid, side, position, bases): bases are 2-bit codes A C G T = 0 1 2 3, bases[0] the clipped base nearest the junction.
  right clip of L >= c bases at refend: n = min(L, 32), bases[i] = read base l_seq - L + i
  left clip of L >= c bases at pos:     n = min(L, 32), bases[i] = read base L - 1 - i
Nothing is stored when one of the n codes is not 1, 2, 4 or 8, when l_seq <= 0, when L > l_seq, or when codes is None.
A query (tid, pr, pl) with S: a right entry at pr matches at shift s iff at most n >> 4 of its bases differ from ref[pl + s + i], a left
entry at pl iff at most n >> 4 differ from ref[pr - 1 - s - i]; outside [0, clen) and bytes other than ACGT are mismatches.  The answer
is (vR, vL, s, stored at (pr, right), stored at (pl, left)) for the s of the largest vR + vL, the smallest among equals; (0, 0, -1) when
pl <= pr or when nothing matches.
"""
import struct

import numpy as np

from tests.support import clipcounts as cc
from tests.support.clipcounts import LEFT, OP_H, RIGHT

BASES, MAX_SHIFT = 32, 32
TWO_BIT = {1: 0, 2: 1, 4: 2, 8: 3}
HASH_MUL = 0x9E3779B97F4A7C15


def entries_of(rec, clens, min_clip, q):
    """[(tid, side, position, bases)] of one record"""
    tid, pos, mapq, flag, cigar, l_seq, codes = rec
    out = []
    for t, side, p in cc.events_of((tid, pos, mapq, flag, cigar), clens, min_clip, q):
        seen = [(op, ln) for op, ln in cigar if op != OP_H]
        L = seen[-1][1] if side == RIGHT else seen[0][1]
        n = min(L, BASES)
        if codes is None or l_seq <= 0 or L > l_seq:
            continue
        idx = [l_seq - L + i for i in range(n)] if side == RIGHT else [L - 1 - i for i in range(n)]
        got = [codes[j] for j in idx]
        if any(c not in TWO_BIT for c in got):
            continue
        out.append((t, side, p, tuple(TWO_BIT[c] for c in got)))
    return out


def table_of(records, clens, min_clip, q):
    """{(tid, side, position): [bases]} of many records"""
    table = {}
    for rec in records:
        for t, side, p, bases in entries_of(rec, clens, min_clip, q):
            table.setdefault((t, side, p), []).append(bases)
    return table


def matches(bases, ref, start, step):
    """whether an entry matches: base i is expected to be ref[start + step * i] (ref: the contig's bytes)"""
    bad = 0
    for i, b in enumerate(bases):
        p = start + step * i
        if not 0 <= p < len(ref) or ref[p:p + 1] not in (b"A", b"C", b"G", b"T") or b"ACGT".index(ref[p:p + 1]) != b:
            bad += 1
    return bad <= len(bases) >> 4


def answer(table, ref, tid, pr, pl, S=MAX_SHIFT):
    """(vR, vL, shift, stored right, stored left) of one query"""
    R, Lf = table.get((tid, RIGHT, pr), []), table.get((tid, LEFT, pl), [])
    best = (0, 0, -1)
    if pl > pr:
        for s in range(S + 1):
            vr = sum(matches(b, ref, pl + s, 1) for b in R)
            vl = sum(matches(b, ref, pr - 1 - s, -1) for b in Lf)
            if vr + vl > best[0] + best[1]:             # strictly: the smallest shift among equal sums stays
                best = (vr, vl, s)
    return best + (len(R), len(Lf))


def ref_codes(ref):
    """the contig as 2-bit codes, 255 where the byte is not A, C, G or T"""
    lut = np.full(256, 255, np.uint8)
    for k, c in enumerate(b"ACGT"):
        lut[c] = k
    return lut[np.frombuffer(ref, np.uint8)]


def answer_many(table, ref, tid, pr, pl, S=MAX_SHIFT):
    """the same through numpy, for many queries on one contig; the tests check it against answer first"""
    code = ref_codes(ref)
    clen = len(code)

    def side_counts(entries, start, step):
        v = np.zeros(S + 1, np.int64)
        for b in entries:
            b = np.array(b, np.uint8)
            idx = start + step * (np.arange(S + 1)[:, None] + np.arange(len(b))[None, :])
            inside = (idx >= 0) & (idx < clen)
            want = np.where(inside, code[np.clip(idx, 0, clen - 1)], 255)
            v += ((want != b[None, :]).sum(1) <= len(b) >> 4)
        return v

    out = []
    for a, b in zip(pr, pl):
        a, b = int(a), int(b)
        R, Lf = table.get((tid, RIGHT, a), []), table.get((tid, LEFT, b), [])
        if b <= a:
            out.append((0, 0, -1, len(R), len(Lf)))
            continue
        vr, vl = side_counts(R, b, 1), side_counts(Lf, a - 1, -1)
        s = int(np.argmax(vr + vl))                     # numpy returns the first of equal maxima
        out.append((int(vr[s]), int(vl[s]), s, len(R), len(Lf)) if vr[s] + vl[s] > 0 else (0, 0, -1, len(R), len(Lf)))
    return out


def planes_of(bases):
    """(low-bit plane, high-bit plane) of an entry, bit i = base i: what im_cliptail_add takes"""
    return sum((b & 1) << i for i, b in enumerate(bases)), sum((b >> 1) << i for i, b in enumerate(bases))


def home_slot(tid, side, position, log2_slots):
    """the first slot an entry of this key probes (the header states the hash): tests place keys on the table's last slots with it"""
    key = (1 << 63) | (tid << 39) | (position << 7) | (side << 6)
    return (((key >> 6) * HASH_MUL) & (2**64 - 1)) >> (64 - log2_slots)


def parse_record(b, o, end):
    """one BAM record at b[o:end] -> (tid, pos, mapq, flag, cigar, l_seq, codes); the packed bases lie behind the CIGAR, with qualities
    behind them or without"""
    tid, pos, l_qname, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, o)
    o_cig = o + 32 + l_qname
    cw = struct.unpack_from("<%dI" % n_cig, b, o_cig)
    o_seq = o_cig + 4 * n_cig
    codes = None
    if l_seq > 0 and o_seq + (l_seq + 1) // 2 <= end:
        packed = b[o_seq:o_seq + (l_seq + 1) // 2]
        codes = [(packed[j >> 1] >> (0 if j & 1 else 4)) & 15 for j in range(l_seq)]
    return tid, pos, mapq, flag, [(c & 15, c >> 4) for c in cw], l_seq, codes


def table_of_bam(bam, min_clip, q):
    """(contig names, the table) of a BAM file"""
    from tests.support import spanarrays
    refs, recs = spanarrays.read_bam_records(bam, parse_record=parse_record)
    return [n for n, _ in refs], table_of(recs, [l for _, l in refs], min_clip, q)


def read_fasta(path):
    """{name: upper-cased bytes}"""
    out, name = {}, None
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            name = ln[1:].split()[0].decode()
            out[name] = []
        elif name is not None:
            out[name].append(ln.strip().upper())
    return {k: b"".join(v) for k, v in out.items()}


def verification_of(table, ref, tid, right, left, kind, pos, end, bp_end):
    """(CV text, CH text) of a printed record that carries CB:CS: the positions come from clipcounts.evidence_of (right, left: the
    contig's clip arrays); a record without both sides, or with the left-clip pile not behind the right-clip pile, prints .,. and ."""
    cb, _cs, (cr, cl) = cc.evidence_of(right, left, kind, pos, end, bp_end)
    if cr == 0 or cl == 0:
        return ".,.", "."
    pr, pl = int(cb.split(",")[0]), int(cb.split(",")[1]) - 1      # a left clip at array position p is printed as p + 1
    if pl <= pr:
        return ".,.", "."
    vr, vl, s, _, _ = answer(table, ref, tid, pr, pl)
    return "%d,%d" % (vr, vl), (str(s) if s >= 0 else ".")


def pack_records(records, qual=True):
    """[(tid, pos, mapq, flag, cigar, l_seq, codes)] -> the device layout (raw uint8, rec_off uint32[n + 1]): core, qname, CIGAR,
    the packed bases of `codes` (two per byte, the earlier one in the high nibble), qualities (qual=False: without them and with
    bin = 0xFFFF, as the product's walkers deliver records), one aux tag.  l_seq goes into the core as it is given: a record may
    claim more bases than it carries."""
    blob, off = bytearray(), [0]
    for i, (tid, pos, mapq, flag, cigar, l_seq, codes) in enumerate(records):
        qname = b"t%d\0" % i
        codes = list(codes) + [0] * (len(codes) & 1)
        packed = bytes((codes[j] << 4) | codes[j + 1] for j in range(0, len(codes), 2))
        core = struct.pack("<iiBBHHHiiii", tid, pos, len(qname), mapq, 4680 if qual else 0xFFFF, len(cigar), flag, l_seq, -1, -1, 0)
        body = (core + qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + packed +
                (b"\x28" * max(min(l_seq, len(codes)), 0) if qual else b"") + b"NMC\x01")
        blob += body + b"\0" * (-len(body) % 4)
        off.append(len(blob))
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint32)


def parse_raw(raw, off):
    b = raw.tobytes()
    return [parse_record(b, int(off[i]), int(off[i + 1])) for i in range(len(off) - 1)]
