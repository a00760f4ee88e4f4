"""Waves (64 records) for the classify kernel of im_triage.hip in its straight-line form: the rule cascade is computed by every
lane and chosen with selects, the three CIGAR walks are one loop of the wave's, the tag walk is a loop of the wave's, and what few
records need sits behind tests on the whole wave.  What can go wrong in that form is one lane's state leaking into its neighbours',
so every generator here MIXES: every class and every exit of the cascade in one wave, CIGAR lengths from 0 to 40 ops in one wave,
pileup lanes beside lanes that do not pile up, aux areas from 0 to 100 bytes in one wave.

tests/test_classify_mixed_waves_host.py proves on the CPU (oracle) that the cases hold what they claim;
tests/test_gpu_classify_mixed_waves.py runs them through the kernels.  A `*_records` generator returns named cases (name, expected
class or size, record bytes); a `*_wave(s)` function returns whole waves of record bytes."""
import struct

import numpy as np

from tests.support import triagecases as tc

WAVE = 64
P = tc.P
NAMES, RANGES = tc.AUX_NAMES, tc.AUX_RANGES            # lib1 500, lib10 600, generic 700, li 800, x * 40 900, lib1b 1000
NAMES_NO_GENERIC = [n for n in NAMES if n != "generic"]
RANGES_NO_GENERIC = [r for n, r in zip(NAMES, RANGES) if n != "generic"]
CONTIGS = [5000, 9000]
DEPTH_WIN = 1024                                       # kDepthWin of im_triage.hip
UNMAPPED = 0x1 | 0x4 | 0x40                            # an unmapped first mate whose mate is mapped
GOOD_PAD = b"\x11\x11\x11"                             # alignment padding that reads as good base codes


# ---- 1. every class and every exit of the rule cascade ------------------------------------------------------------------------------

def cascade_records():
    """one record per exit of the cascade; the expected class with the table NAMES (which holds "generic") and defer off"""
    r, C = tc.rec, tc.CLIP
    clip_tail = ((70, 0), (30, 4))
    bad = bytearray([0x12] * 50); bad[10] = 0x13       # a refused base code at read offset 21
    out = [
        ("secondary", 0, r(P | 0x100, cigar=C)), ("qc_fail", 0, r(P | 0x200, cigar=C)), ("duplicate", 0, r(P | 0x400, cigar=C)),
        ("supplementary", 0, r(P | 0x800, cigar=C)), ("unpaired", 0, r(0x2, cigar=C)), ("tid_ne_mtid", 0, r(P, mtid=1, cigar=C)),
        ("truncated", 21, r(P, cigar=C)[:60]),
        ("rg_type", 16, r(P, cigar=C, tags=b"RGAx")), ("rg_type_int", 16, r(P, cigar=C, tags=b"RGi\1\0\0\0")),
        ("rg_not_in_table", 16, r(P, cigar=C, tags=b"RGZnobody\0")), ("rg_longer_than_stored", 16, r(P, cigar=C, tags=b"RGZlib1bb\0")),
        ("rg_known", 3, r(P, cigar=C, tags=b"RGZlib10\0")), ("rg_known_H", 3, r(P, cigar=C, tags=b"RGHlib1\0")),
        ("no_rg", 3, r(P, cigar=C, mapq=30)),                  # "generic"; ERR_RG with a table that has no such name
        ("mq_type_Z", 17, r(UNMAPPED, cigar=(), tags=b"MQZ12\0")), ("mq_type_f", 17, r(UNMAPPED, cigar=(), tags=b"MQf\0\0\x80\x3f")),
        ("mq_type_A", 17, r(UNMAPPED, cigar=(), tags=b"MQAx")), ("mq_type_B", 17, r(UNMAPPED, cigar=(), tags=b"MQBc\1\0\0\0\x1e")),
        ("mate_unmapped", 1, r(0x1 | 0x8, cigar=C)),
        ("unmapped_mapq_above", 2, r(UNMAPPED, cigar=(), mapq=60)), ("unmapped_mapq_below", 1, r(UNMAPPED, cigar=(), mapq=9)),
        ("unmapped_mapq_at", 2, r(UNMAPPED | 0x20, cigar=(), mapq=10)),
        ("unmapped_mq_above", 2, r(UNMAPPED, cigar=(), mapq=0, tags=b"MQC\x1e")), ("unmapped_mq_below", 1, r(UNMAPPED, cigar=(), mapq=60, tags=b"MQC\x05")),
        ("unmapped_mq_i", 2, r(UNMAPPED | 0x20, cigar=(), mapq=0, tags=b"MQi\x0a\0\0\0")), ("unmapped_mq_s_neg", 1, r(UNMAPPED, cigar=(), mapq=60, tags=b"MQs\xff\xff")),
        ("both_unmapped", 1, r(0x1 | 0x4 | 0x8, cigar=())),
        ("proper_plain", 1, r(P)), ("proper_plain_rc", 1, r(P | 0x10)),
        ("proper_clip_5p_fwd", 3, r(P, cigar=C)), ("proper_clip_3p_fwd", 1, r(P, cigar=clip_tail)),             # the `three` case, forward
        ("proper_clip_3p_rev", 1, r(P | 0x10, cigar=C)), ("proper_clip_5p_rev", 3, r(P | 0x10 | 0x20, cigar=clip_tail)),   # ... and reverse
        ("proper_two_clips", 3, r(P, cigar=((10, 4), (80, 0), (10, 4)))), ("proper_three_and_ins", 3, r(P, cigar=((50, 0), (2, 1), (28, 0), (20, 4)))),
        ("proper_ins", 3, r(P | 0x20, cigar=((50, 0), (3, 1), (47, 0)))), ("proper_del", 3, r(P, cigar=((50, 0), (3, 2), (50, 0)))),
        ("proper_clip_mapq_below", 1, r(P, cigar=C, mapq=9)), ("proper_clip_mq_below", 1, r(P, cigar=C, mapq=60, tags=b"MQC\x09")),
        ("proper_clip_mq_above", 3, r(P, cigar=C, mapq=0, tags=b"MQC\x0a")), ("proper_clip_mq_type_Z", 1, r(P, cigar=C, mapq=60, tags=b"MQZ12\0")),
        ("proper_bad_op", 18, r(P, cigar=((50, 0), (10, 3), (50, 0)))), ("proper_bad_base", 20, r(P, seq=bytes(bad))),
        ("proper_inner_clip", 19, r(P, cigar=((40, 0), (5, 4), (55, 0)))),
        ("pe_inside_range", 1, r(0x1 | 0x20, isize=700)), ("pe_outside_range", 4, r(0x1 | 0x20, isize=701)),
        ("pe_negative", 4, r(0x1 | 0x10, isize=-701)), ("pe_same_strand", 1, r(0x1 | 0x10 | 0x20, isize=5000)), ("pe_same_strand_fwd", 1, r(0x1, isize=5000)),
        ("pe_below_max", 4, r(0x1 | 0x20, isize=999999)), ("pe_at_max", 1, r(0x1 | 0x20, isize=1000000)), ("pe_int_min", 1, r(0x1 | 0x20, isize=-(2 ** 31))),
        ("pe_rg_range", 4, r(0x1 | 0x20, isize=550, tags=b"RGZlib1\0")), ("pe_rg_range_in", 1, r(0x1 | 0x20, isize=550, tags=b"RGZlib10\0")),
    ]
    assert len(out) <= WAVE
    return out


CASCADE_CLASSES = {0, 1, 2, 3, 4, 16, 17, 18, 19, 20, 21}
ODD_LANES = (0, 31, 32, 63)


def cascade_wave(seed):
    """all of cascade_records in one wave (the rest of the 64 lanes repeat them), in a seeded lane order"""
    recs = [x[2] for x in cascade_records()]
    rng = np.random.default_rng(seed)
    fill = [recs[int(k)] for k in rng.integers(0, len(recs), WAVE - len(recs))]
    wave = recs + fill
    return [wave[int(k)] for k in rng.permutation(WAVE)]


def odd_lane_waves(lane):
    """per record of cascade_records two waves of ONE class -- plain proper pairs (class 1, every loop runs for everybody), then
    secondary alignments (class 0, nothing walks but the odd lane) -- with that record alone at `lane`"""
    plain, skip = tc.rec(P), tc.rec(P | 0x100)
    out = []
    for _, _, rec in cascade_records():
        for other in (plain, skip):
            w = [other] * WAVE
            w[lane] = rec
            out += w
    return out


# ---- 2. CIGAR lengths mixed in one wave ---------------------------------------------------------------------------------------------

CIGAR_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 9, 40)
REFUSED_OPS = (3, 5, 6, 9, 15)                          # N H P and two of "op > 8"


def _cigar(n, L=100):
    """n ops over L read bases: M runs with single-base I and D between them (n = 2: a clip and a run)"""
    if n == 0:
        return ()
    if n == 2:
        return ((5, 4), (L - 5, 0))
    ops = [(1, 1) if k % 4 == 1 else (1, 2) if k % 4 == 3 else (0, 0) for k in range(n)]
    n_m, n_i = sum(1 for _, o in ops if o == 0), sum(1 for _, o in ops if o == 1)
    each, rest = divmod(L - n_i, n_m)
    out, first = [], True
    for l, o in ops:
        if o == 0:
            out.append((each + (rest if first else 0), 0)); first = False
        else:
            out.append((l, o))
    assert sum(l for l, o in out if o in (0, 1, 4)) == L and len(out) == n
    return tuple(out)


def _read_offset(cigar, k):
    return sum(l for l, o in cigar[:k] if o in (0, 1, 4, 7, 8))


def cigar_records(seed=11):
    """(name, class, record): every length plain; a refused op first, in the middle, last and beyond the fourth word; a refused base
    just in front of and at that op's read offset; CIGARs reaching past l_seq; an inner soft clip; read offsets at 2^32"""
    rng = np.random.default_rng(seed)
    L = 100
    out = []
    for n in CIGAR_LENGTHS:
        c = _cigar(n)
        out.append(("len%d" % n, 1 if n in (0, 1) else 3, tc.rec(P, cigar=c, seq=tc.pack(tc.good_codes(rng, L)))))
        if n == 0:
            continue
        where = {"first": 0, "mid": n // 2, "last": n - 1}
        if n > 4:
            where["beyond4"] = 4 + (n - 5) // 2
        for tag, k in where.items():
            op = REFUSED_OPS[(n + k) % len(REFUSED_OPS)]
            cc = list(c); cc[k] = (cc[k][0], op)
            q = _read_offset(cc, k)
            out.append(("len%d_%s_op%d" % (n, tag, op), 18, tc.rec(P, cigar=tuple(cc), seq=tc.pack(tc.good_codes(rng, L)))))
            for d in (-1, 0):
                if 0 <= q + d < L:
                    codes = tc.good_codes(rng, L); codes[q + d] = tc.REFUSED[(n + k) % 11]
                    out.append(("len%d_%s_base%+d" % (n, tag, d), 20 if d < 0 else 18, tc.rec(P, cigar=tuple(cc), seq=tc.pack(codes))))
    # the CIGAR reaches past l_seq: the bytes behind the packed bases are read as bases -- the qualities (0x28: C, T), then padding
    for k, inside in ((1, 1), (1, 0), (6, 1), (20, 0)):
        j = L + k - 1 if inside else L + k
        body = bytearray(tc.pack(tc.good_codes(rng, L)) + b"\x28" * L)
        body[j >> 1] = (body[j >> 1] & (0x0F if not j & 1 else 0xF0)) | (3 << (0 if j & 1 else 4))
        out.append(("past_lseq_%d_%s" % (k, "in" if inside else "out"), 20 if inside else 1,
                    tc.rec(P, cigar=((L + k, 0),), seq=bytes(body[:50]), qual=bytes(body[50:]))))
    out.append(("past_record", 1, tc.rec_exact(P, cigar=((5000, 0),), seq=tc.pack(tc.good_codes(rng, L, with_n=False)))))
    out.append(("past_record_9ops", 3, tc.rec_exact(P, cigar=((10, 0), (1, 1)) * 4 + ((5000, 0),), seq=tc.pack(tc.good_codes(rng, L, with_n=False)))))
    out.append(("inner_clip", 19, tc.rec(P, cigar=((40, 0), (5, 4), (55, 0)))))
    out.append(("inner_clip_6ops", 19, tc.rec(P, cigar=((10, 0), (1, 1), (10, 0), (5, 4), (1, 2), (74, 0)))))
    out += [(n, c, r) for n, c, r, _ in wide_offset_records()]
    return out


def wide_offset_records():
    """(name, class, record, class a 32-bit read offset that wraps would give): 2^32 read bases in front of a refused op"""
    big = 2 ** 28 - 1
    front = ((big, 4),) * 16 + ((16, 1),)               # 16 * (2^28 - 1) + 16 = 2^32
    cig = front + ((1, 3), (10, 0))
    bad = bytearray([0x12] * 50); bad[1] = 0x32         # a refused code at read offset 2
    kw = dict(cigar=cig, pad=GOOD_PAD)
    return [("offset_2^32_bad_base_in_front", 20, tc.rec(P, seq=bytes(bad), **kw), 18),      # 2 < 2^32, but not 2 < 0
            ("offset_2^32_clean", 18, tc.rec(P, **kw), 18)]


def cigar_wave(seed):
    """cigar_records in seeded order between plain pairs, whole waves"""
    recs = [x[2] for x in cigar_records()]
    rng = np.random.default_rng(seed)
    recs = [recs[int(k)] for k in rng.permutation(len(recs))]
    return recs + [tc.rec(P)] * ((-len(recs)) % WAVE)


# ---- 3. the pileup ------------------------------------------------------------------------------------------------------------------

def _d(tid, pos, cigar, flag=0):
    return tc._drec(tid, pos, cigar, flag)


M = lambda n: ((n, 0),)                                 # noqa: E731
BIG = 2 ** 28 - 1


def width_edge_records():
    """(name, record, positions the record covers on contig 0 in 64-bit arithmetic, ... when positions wrap at 32 bits)"""
    c0 = CONTIGS[0]
    return [
        # the position passes 2^31: nothing is covered; wrapped, the D ops bring it back to 82 and the M run counts
        ("wraps_past_int_max", _d(0, 2 ** 31 - 10, ((100, 2),) + ((BIG, 2),) * 8 + ((50, 0),)), (0, 0), (82, 132)),
        ("wraps_at_int_max_exactly", _d(0, 2 ** 31 - 5000, ((5000, 2),) + ((BIG, 3),) * 8 + ((8, 2), (30, 0))), (0, 0), (0, 30)),
        ("int_max_M1", _d(0, 2 ** 31 - 1, M(1)), (0, 0), (0, 0)),
        ("int_max_long_M", _d(0, 2 ** 31 - 1, M(BIG)), (0, 0), (0, 0)),
        ("int_min_to_zero", _d(0, -(2 ** 31), ((BIG, 3),) * 8 + ((8, 2), (30, 0))), (0, 30), (0, 30)),
        ("int_min_short", _d(0, -(2 ** 31), M(BIG)), (0, 0), (0, 0)),
        ("negative_over_contig", _d(0, -5, M(BIG)), (0, c0), (0, c0)),
        ("sum_past_2^32", _d(0, 100, ((BIG, 2),) * 17 + ((50, 0),)), (0, 0), (0, 0)),
    ]


def depth_model(rec, tid, clen, bits):
    """imo_depth_add restated with the running position kept in `bits` bits (two's complement)"""
    t, pos = struct.unpack_from("<ii", rec, 0)
    l_qname, n_cig, flag = rec[8], struct.unpack_from("<H", rec, 12)[0], tc.flag_of(rec)
    d = np.zeros(clen, np.int32)
    if t != tid or t < 0 or flag & (0x4 | 0x100 | 0x200 | 0x400):
        return d
    wrap = lambda v: (v + 2 ** (bits - 1)) % 2 ** bits - 2 ** (bits - 1)      # noqa: E731
    x = pos
    for k in range(n_cig):
        cw = struct.unpack_from("<I", rec, 32 + l_qname + 4 * k)[0]
        op, ln = cw & 15, cw >> 4
        if op in (0, 7, 8):
            a, b = max(x, 0), min(wrap(x + ln), clen)
            if a < b:
                d[a:b] += 1
        if op in (0, 2, 3, 7, 8):
            x = wrap(x + ln)
    return d


def pileup_waves():
    """dict name -> 64 records.  `one`: a single eligible lane; `none`: no eligible lane; `window`: events on both sides of the
    1024-position window, in front of it, on a second contig, negative positions, runs ending at and past the contig's end;
    `edges`: width_edge_records between ordinary lanes"""
    c0 = CONTIGS[0]
    un = lambda: _d(0, 50, M(30), 0x4)                   # noqa: E731
    one = [un() for _ in range(WAVE)]; one[37] = _d(1, 4000, ((20, 0), (5, 2), (20, 7), (3, 1), (20, 8)))
    none = [un() for _ in range(20)] + [_d(-1, 10, M(10)) for _ in range(10)] + [_d(2, 10, M(10)) for _ in range(10)]
    none += [_d(0, 10, M(10), f) for f in (0x100, 0x200, 0x400) for _ in range(8)]
    base = 300
    win = [un(), _d(0, base, M(40))]                     # the first eligible lane is lane 1: window base 300 on contig 0
    win += [_d(0, base + DEPTH_WIN - 1, M(10)), _d(0, base + DEPTH_WIN, M(10)), _d(0, base + 2000, M(10)), _d(0, base + DEPTH_WIN - 50, M(50)),
            _d(0, base + DEPTH_WIN - 51, M(50)), _d(0, base + 900, M(300)), _d(0, 100, M(2600)), _d(0, base - 1, M(1)), _d(0, base - 1, M(2))]
    win += [_d(1, 10, M(25)), _d(1, 8970, M(30)), _d(1, 8971, M(30)), _d(1, 8999, M(1)), _d(1, 9000, M(5)), _d(1, 0, M(9000))]
    win += [_d(0, -1, M(20)), _d(0, -20, M(50)), _d(0, -50, M(50)), _d(0, -5, ((10, 2), (10, 0))), _d(0, c0 - 30, M(30)), _d(0, c0 - 29, M(30)),
            _d(0, c0 - 10, M(500)), _d(0, c0, M(5)), _d(0, 0, M(c0))]
    win += [_d(0, base + 10, ((5, 4), (10, 0), (3, 1), (10, 7), (4, 2), (10, 8), (7, 3), (10, 0), (2, 6), (5, 5)))]
    # records that pile up AND are classified: proper pairs with an indel, a refused op in front of an M run
    win += [tc.rec(P, tid=0, pos=base + 20, cigar=((50, 0), (3, 2), (50, 0))), tc.rec(P, tid=0, pos=base + 30, cigar=((50, 0), (10, 3), (50, 0)))]
    win += [_d(0, base + 5 * k, M(33)) for k in range(WAVE - len(win))]
    edges = [_d(0, 200 + 3 * k, M(40)) for k in range(WAVE)]
    for k, (_, rec, _, _) in enumerate(width_edge_records()):
        edges[(9 * k + 5) % WAVE] = rec
    assert len(one) == len(none) == len(win) == len(edges) == WAVE
    return dict(one=one, none=none, window=win, edges=edges)


# ---- 4. aux areas -------------------------------------------------------------------------------------------------------------------

AUX_SIZES = (0, 3, 4, 5, 23, 24, 25, 47, 48, 49, 100)
RG1, MQ30 = tc.RG1, tc.MQ30


def _aux(flag, tags, mapq, **kw):
    r = tc.rec_exact(flag, want_pad=0, tags=tags, mapq=mapq, **kw)
    return r


def aux_records(seed=21):
    """(name, aux bytes, record): per size of the aux area, RG / MQ first, last, absent, of a refused type; a name that runs out
    of the 24-byte window; a B array in front.  Proper pairs with a leading clip and mapq 0 (a candidate only where MQ is found)
    and unmapped reads (where a refused MQ type is an error)."""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, tags, T):
        assert len(tags) == T, (name, len(tags), T)
        has_mq = b"MQ" in tags
        out.append((name, T, _aux(P, tags, 0 if has_mq else 60, cigar=tc.CLIP)))
        out.append((name + "_unmapped", T, _aux(UNMAPPED, tags, 0 if has_mq else 60, cigar=())))

    def fill(n):
        assert n == 0 or n >= 4, n
        return tc.compose(n, rng)[0]
    for T in AUX_SIZES:
        if T == 0:
            add("aux0", b"", 0)
            continue
        if T == 3:
            add("aux3_no_field", b"Xi\1", 3)            # bytes that are no field: fewer than four are padding
            continue
        add("aux%d_absent" % T, fill(T), T)
        for tag, key in ((MQ30, "mq"), (RG1, "rg"), (b"MQZ1\0", "mq_refused"), (b"RGAx", "rg_refused"), (b"RGZx\0", "rg_unknown")):
            n = T - len(tag)
            if n == 0 or n >= 4:
                add("aux%d_%s_first" % (T, key), tag + fill(n), T)
                if n:
                    add("aux%d_%s_last" % (T, key), fill(n) + tag, T)
        n = T - len(RG1) - len(MQ30)
        if n == 0 or n >= 4:
            add("aux%d_rg_mq_last" % T, fill(n) + RG1 + MQ30, T)
            add("aux%d_mq_first_rg_last" % T, MQ30 + fill(n) + RG1, T)
    # a B array in front (its count decides where the walk goes on), and one whose count runs past the record
    arr = tc.field("XB", "B", rng, n=5, etype="s")      # 18 bytes
    add("aux47_B_front", arr + fill(47 - len(arr) - 8) + RG1, 47)
    over = b"XBBi" + struct.pack("<I", 1000) + bytes(8)
    add("aux24_B_over", over + RG1, 24)
    # a read-group name of 40 bytes: wherever it starts it runs out of the window
    long_rg = b"RGZ" + b"x" * 40 + b"\0"
    add("aux48_long_name", long_rg + MQ30, 48)
    add("aux100_long_name_behind", fill(52) + long_rg + MQ30, 100)
    return out


def aux_wave(seed):
    """aux_records in seeded order, whole waves, and the record with the longest aux area last in the chunk"""
    recs = aux_records()
    rng = np.random.default_rng(seed)
    order = [recs[int(k)] for k in rng.permutation(len(recs))]
    longest = max(range(len(order)), key=lambda k: order[k][1])
    order.append(order.pop(longest))
    fillers = [tc.rec(P, tags=MQ30, cigar=tc.CLIP, mapq=0)] * ((-len(order)) % WAVE)
    return fillers + [r for _, _, r in order]


def aux_bytes(rec):
    """bytes of the record's aux area (records with qualities)"""
    l_qname, n_cig, l_seq = rec[8], struct.unpack_from("<H", rec, 12)[0], tc.l_seq_of(rec)
    return len(rec) - (32 + l_qname + 4 * n_cig + (l_seq + 1) // 2 + l_seq)
