"""Inputs that take the triage kernels (classify, emit, decode) to the edges of their index arithmetic: read lengths around the
lanes-per-record switch and the tail loop, refused base codes at every piece boundary, aux areas that make the 24-byte window
slide, read-group tables on both sides of the LDS limit, record counts around the workgroup and group sizes, and pileup
segments around the 4096-position depth window.  Plain numpy + struct: records are built the way `_rec` of
tests/test_gpu_triage.py builds them.  tests/test_triage_cases_host.py proves on the CPU that every generator reaches what it
names; tests/test_gpu_triage_shapes.py runs them through the kernels.

A generator returns a list of (record bytes, meta dict); `batch` turns records into (raw, rec_off)."""
import struct

import numpy as np

GOOD = (1, 2, 4, 8, 15)                                # A C G T N
REFUSED = (0, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14)       # what bit2char exits on
P = 0x1 | 0x2                                          # paired, proper
CLIP = ((30, 4), (70, 0))                              # a leading clip on a forward read: a class 3 candidate

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 131, 255, 256, 257, 287, 288, 289, 511, 512, 513,
           1019, 1020, 1021, 2600]
BASE_LENGTHS = [33, 100, 129, 257, 300, 600]
BASE_POSITIONS = [0, 1, 7, 8, 15, 16, 30, 31, 32, 33, 63, 64, 127, 128, 129, 255, 256, 257, 287, 288]
TILE_COUNTS = [1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 16389]
TILE_PATTERNS = ["all", "none", "first", "last", "lane255", "err_counted", "mix"]
DEPTH_CONTIGS = [5000, 9000]
DEPTH_WIN = 4096                                       # kDepthWin of im_triage.hip
RG_LDS = 2048                                          # kRgLds of im_rg.hpp


def rec(flag, tid=0, pos=100, mtid=0, mpos=300, isize=300, mapq=60, cigar=((100, 0),), seq=None, tags=b"", qname=b"q\0", l_seq=100,
        pad=b"\0\0\0", qual=None, bin_=0):
    seq = seq if seq is not None else bytes([0x12] * ((l_seq + 1) // 2))
    qual = qual if qual is not None else b"\x28" * l_seq
    cig = b"".join(struct.pack("<I", (l << 4) | o) for l, o in cigar)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qname), mapq, bin_, len(cigar), flag, l_seq, mtid, mpos, isize) + qname + cig + seq + qual + tags
    return body + pad[:(-len(body)) % 4]


def rec_exact(flag, want_pad=0, **kw):
    """rec with the qname sized so that the record takes exactly want_pad bytes of alignment padding"""
    for k in range(1, 5):
        r = rec(flag, qname=b"q" * k + b"\0", pad=b"", **kw)
        if (-len(r)) % 4 == want_pad:
            return r
    raise AssertionError("unreachable")


def pack(codes):
    c = np.asarray(codes, np.uint8)
    if len(c) & 1:
        c = np.append(c, np.uint8(0))
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()


def good_codes(rng, n, with_n=True):
    return np.array(GOOD if with_n else GOOD[:4], np.uint8)[rng.integers(0, 5 if with_n else 4, n)]


def batch(recs):
    raw = np.frombuffer(b"".join(recs), dtype=np.uint8).copy()
    off = np.zeros(len(recs) + 1, dtype=np.uint32)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return raw, off


def l_seq_of(r):
    return struct.unpack_from("<i", r, 16)[0]


def flag_of(r):
    return struct.unpack_from("<H", r, 14)[0]


def sweeps(r):
    """the classify kernel's base sweep covers this record (reaches_new_readaln): it decides the wave's lanes per record"""
    f = flag_of(r)
    tid, mtid = struct.unpack_from("<i", r, 0)[0], struct.unpack_from("<i", r, 20)[0]
    return not (f & 0xF00) and (f & 0x3) == 0x3 and not (f & 0xC) and tid == mtid


def filler(l_seq=100):
    return rec(P, l_seq=l_seq, cigar=((l_seq, 0),), seq=bytes([0x12] * ((l_seq + 1) // 2)))


# ---- 1. read lengths -------------------------------------------------------------------------------------------------------------

def length_cases(seed=101):
    """per L: an unmapped read with a mapped mate (class 2), mate strand both ways; for L >= 12 a proper pair with a leading and
    a trailing clip in the four strand combinations (class 3 where the clip is not the one the reference lets pass)"""
    rng = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        for mate_rc in (0, 1):
            seq = pack(good_codes(rng, L))
            out.append((rec(0x1 | 0x4 | 0x40 | (0x20 if mate_rc else 0), cigar=(), l_seq=L, seq=seq),
                        dict(kind="unmapped", L=L, revcomp=not mate_rc)))
        if L < 12:
            continue
        for rc in (0, 1):
            for mate_rc in (0, 1):
                for lead in (0, 1):
                    cigar = ((5, 4), (L - 5, 0)) if lead else ((L - 5, 0), (5, 4))
                    seq = pack(good_codes(rng, L))
                    out.append((rec(P | (0x10 if rc else 0) | (0x20 if mate_rc else 0), cigar=cigar, l_seq=L, seq=seq),
                                dict(kind="clip", L=L, revcomp=rc == mate_rc, cand=bool(lead) != bool(rc))))
    return out


def length_layout(cases):
    """the batch of section 1: waves (64 records each) that differ in what the lanes-per-record ballots see, then every case once.
    Returns (records, waves): waves[k] = (kind, lane of the odd record or None)."""
    recs_all = [r for r, _ in cases]
    short = [r for r in recs_all if l_seq_of(r) <= 128]
    r129 = [r for r in recs_all if l_seq_of(r) == 129 and sweeps(r)]
    r257 = [r for r in recs_all if l_seq_of(r) > 256 and sweeps(r)]
    long_ = [r for r in recs_all if l_seq_of(r) > 128 and sweeps(r)]
    out, waves, at = [], [], [0]

    def shorts(n):
        w = [short[(at[0] + k) % len(short)] for k in range(n)]
        at[0] += n
        return w
    out += shorts(64); waves.append(("short", None))
    for k, lane in enumerate((0, 7, 8, 15, 16, 63)):
        w = shorts(64); w[lane] = r129[k % len(r129)]
        out += w; waves.append(("one129", lane))
    for k, lane in enumerate((0, 37, 63)):
        w = shorts(64); w[lane] = r257[(k * 7) % len(r257)]
        out += w; waves.append(("one257", lane))
    out += [long_[k % len(long_)] for k in range(64)]; waves.append(("long", None))
    return out + recs_all, waves


# ---- 2. refused base codes against refused ops -------------------------------------------------------------------------------------

def _proper(L, codes, cigar=None, **kw):
    return rec(P, l_seq=L, cigar=cigar if cigar is not None else ((L, 0),), seq=pack(codes), **kw)


def base_cases(seed=202):
    rng = np.random.default_rng(seed)
    out = []
    for L in BASE_LENGTHS:
        for p in sorted({q for q in BASE_POSITIONS if q < L} | {L - 1}):
            for code in REFUSED:
                c = good_codes(rng, L); c[p] = code
                out.append((_proper(L, c), dict(kind="one", L=L, p=p, code=code, expect=20)))
        if L & 1:                                       # the padding nibble is no base
            for code in REFUSED[1:]:
                seq = bytearray(pack(good_codes(rng, L))); seq[-1] |= code
                out.append((rec(P, l_seq=L, cigar=((5, 4), (L - 5, 0)), seq=bytes(seq)), dict(kind="padding", L=L, code=code, expect=3)))
        for p1, p2 in ((3, L - 1), (L // 2, L // 2 + 1), (31, 32)):
            c = good_codes(rng, L); c[p1] = 3; c[p2] = 0
            out.append((_proper(L, c), dict(kind="two", L=L, expect=20)))
        # a refused op at read offset q: a refused base in front of it wins, one at or behind it loses
        for q in sorted(x for x in {1, 32, L // 2, L - 2} if x <= L - 2):
            for op in (3, 5, 6, 9):
                for d in (-1, 0, 1):
                    c = good_codes(rng, L); c[q + d] = REFUSED[(q + op + d) % 11]
                    out.append((_proper(L, c, ((q, 0), (4, op), (L - q, 0))), dict(kind="op", L=L, q=q, d=d, op=op, expect=20 if d < 0 else 18)))
        c = good_codes(rng, L); c[3] = 6
        out.append((_proper(L, c, ((10, 4), (L - 10, 0))), dict(kind="in_clip", L=L, expect=20)))
        c = good_codes(rng, L); c[22] = 9
        out.append((_proper(L, c, ((20, 0), (5, 1), (L - 25, 0))), dict(kind="in_ins", L=L, expect=20)))
        # the CIGAR reaches k bases past l_seq: the bytes behind the packed bases are read as bases (for odd L the padding nibble first)
        for k in (1, 6, 20):
            for inside in (1, 0):
                j = L + k - 1 if inside else L + k      # nibble index: the last one inside the reach, the first one outside
                body = bytearray(pack(good_codes(rng, L)) + b"\x28" * L)
                if L & 1:
                    body[L // 2] |= 1                   # a good padding nibble
                body[j >> 1] = (body[j >> 1] & (0x0F if not j & 1 else 0xF0)) | (3 << (0 if j & 1 else 4))
                nb = (L + 1) // 2
                out.append((rec(P, l_seq=L, cigar=((L + k, 0),), seq=bytes(body[:nb]), qual=bytes(body[nb:])),
                            dict(kind="past_lseq", L=L, k=k, expect=20 if inside else 1)))
        # ... and past the end of the record: every byte behind the packed bases counts, and nothing behind the record
        for tags, expect in ((b"", 1), (b"\x11\x12\x14\x18", 1), (b"\x11\x12\x14\x10", 20)):
            seq = bytearray(pack(good_codes(rng, L)))
            if L & 1:
                seq[-1] |= 1
            out.append((rec_exact(P, l_seq=L, cigar=((5000, 0),), seq=bytes(seq), tags=tags), dict(kind="past_record", L=L, expect=expect)))
    return out


def base_layout(cases):
    """every case once; then waves with one case at lane 0 and another at lane 63 between plain reads; then a workgroup that
    ends in a partly filled wave holding a few cases"""
    recs = [r for r, _ in cases]
    pick = recs[::23]
    out = list(recs)
    out += [filler()] * ((-len(out)) % 64)
    for k in range(0, len(pick) - 1, 2):
        out += [pick[k]] + [filler(33 if k & 2 else 100)] * 62 + [pick[k + 1]]
    out += [filler()] * ((-len(out)) % 256)
    out += [filler()] * 128 + recs[5::211][:6]
    return out


# ---- 3. the aux walk ---------------------------------------------------------------------------------------------------------------

AUX_NAMES = ["lib1", "lib10", "generic", "li", "x" * 40, "lib1b"]
AUX_RANGES = [500, 600, 700, 800, 900, 1000]
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}


def field(tag, type_, rng, n=0, etype="c"):
    """one whole aux field; n = string length or array count"""
    t = tag.encode()
    if type_ in FIXED:
        return t + type_.encode() + bytes(rng.integers(1, 256, FIXED[type_], dtype=np.uint8))
    if type_ in "ZH":
        return t + type_.encode() + bytes(rng.integers(0x30, 0x5B, n, dtype=np.uint8)) + b"\0"
    return t + b"B" + etype.encode() + struct.pack("<I", n) + bytes(rng.integers(0, 256, FIXED[etype] * n, dtype=np.uint8))


def compose(T, rng):
    """whole fields of T bytes together (T = 0 or T >= 4); returns (bytes, [(type, offset, size)])"""
    out, parts = b"", []
    while len(out) < T:
        r = T - len(out)
        sizes = [("A", 4), ("c", 4), ("C", 4), ("s", 5), ("S", 5), ("i", 7), ("I", 7), ("f", 7), ("d", 11)]
        sizes += [("Z", 4 + k) for k in range(31)] + [("H", 4 + k) for k in range(31)]
        sizes += [("B" + e, 8 + FIXED[e] * n) for e in "cCsSiIfdA" for n in (0, 1, 5)]
        ok = [(t, s) for t, s in sizes if r - s == 0 or r - s >= 4]
        t, s = ok[int(rng.integers(0, len(ok)))]
        tag = "X" + "abcdefghijklmnop"[len(parts) % 16]
        f = field(tag, t[0], rng, n=s - 4 if t[0] in "ZH" else (s - 8) // FIXED[t[1]] if t[0] == "B" else 0, etype=t[1] if t[0] == "B" else "c")
        assert len(f) == s
        parts.append((t, len(out), s))
        out += f
    return out, parts


def _aux_rec(tags, mapq=0, **kw):
    return rec(P, cigar=CLIP, mapq=mapq, tags=tags, **kw)


RG1, MQ30 = b"RGZlib1\0", b"MQC\x1e"


def aux_cases(seed=303):
    """class 3 candidates (forward read, leading clip); mapq 0, so a record is a candidate only when its MQ field is found,
    and its range names the read group that was found (lib1 = 500, generic = 700)"""
    rng = np.random.default_rng(seed)
    out = []

    def tails(prefix, meta):
        for name, t in (("rg", RG1), ("mq", MQ30), ("rg_mq", RG1 + MQ30), ("mq_rg", MQ30 + RG1)):
            out.append((_aux_rec(prefix + t, mapq=60 if name == "rg" else 0), dict(meta, tail=name)))
    for T in range(61):
        if 0 < T < 4:
            # no whole field is shorter than four bytes: bytes that are no field, which the walk reads as a tag and a type
            tails(b"Xi\1"[:T], dict(kind="prefix", T=T, parts=[]))
            continue
        for _ in range(3 if T else 1):
            pre, parts = compose(T, rng)
            tails(pre, dict(kind="prefix", T=T, parts=parts))
    for t in "ZH":
        for k in range(31):
            tails(field("XS", t, rng, n=k), dict(kind="prefix", T=4 + k, parts=[(t, 0, 4 + k)]))
            tails(field("XA", "i", rng) + field("XS", t, rng, n=k) + field("XB", "s", rng), dict(kind="prefix", T=16 + k, parts=[("i", 0, 7), (t, 7, 4 + k), ("s", 11 + k, 5)]))
    for e in "cCsSiIfdA":
        for n in (0, 1, 5, 40):
            pre = field("XB", "B", rng, n=n, etype=e)
            tails(pre, dict(kind="prefix", T=len(pre), parts=[("B" + e, 0, len(pre))]))
        # a count that runs past the record: the walk stops, RG and MQ behind it do not exist
        over = b"XBB" + e.encode() + struct.pack("<I", 1000) + bytes(16)
        tails(over, dict(kind="b_over", T=len(over), parts=[]))
    for bad in (b"XYq\1", b"XY\0\0", b"XYb\1\2\3\4"):
        tails(bad, dict(kind="unknown_type", T=len(bad), parts=[]))
    return out


def rg_name_table():
    """a name of every length 1..40 (rotated alphabets: the short ones are prefixes of the long ones 26 letters on)"""
    abc = "abcdefghijklmnopqrstuvwxyz" * 3
    names = [abc[k % 26:k % 26 + k] for k in range(1, 41)] + ["generic"]
    return names, [1000 + 7 * k for k in range(len(names))]


def rg_name_cases(seed=404):
    names, _ = rg_name_table()
    rng = np.random.default_rng(seed)
    out = []
    for k in range(1, 41):
        stored = names[k - 1]
        for pre in (b"", field("XA", "Z", rng, n=12)):
            out.append((_aux_rec(pre + b"RGZ" + stored.encode() + b"\0", mapq=60), dict(kind="rg_present", k=k)))
            out.append((_aux_rec(pre + b"RGZ" + b"Q" * k + b"\0", mapq=60), dict(kind="rg_absent", k=k)))
            if k > 1:
                out.append((_aux_rec(pre + b"RGZ" + stored[:-1].encode() + b"\0", mapq=60), dict(kind="rg_prefix", k=k - 1)))
            out.append((_aux_rec(pre + b"RGH" + stored.encode() + b"\0", mapq=60), dict(kind="rg_present_H", k=k)))
    return out


def mq_cases():
    vals = [("c", b"\xff"), ("c", b"\x7f"), ("c", b"\x09"), ("c", b"\x0a"), ("c", b"\x80"), ("C", b"\xff"), ("C", b"\x09"), ("C", b"\x0a"),
            ("s", b"\xff\xff"), ("s", b"\xff\x7f"), ("s", b"\x00\x80"), ("s", b"\x0a\x00"), ("s", b"\x09\x00"), ("S", b"\xff\xff"), ("S", b"\x09\x00"),
            ("S", b"\x00\x80"), ("i", b"\xff\xff\xff\xff"), ("i", b"\xff\xff\xff\x7f"), ("i", b"\x0a\0\0\0"), ("i", b"\0\0\0\x80"), ("i", b"\x09\0\0\0"),
            ("I", b"\xff\xff\xff\xff"), ("I", b"\x0a\0\0\0"), ("I", b"\xff\xff\xff\x7f"), ("I", b"\0\0\0\x80"),
            ("Z", b"12\0"), ("f", b"\0\0\x80\x3f"), ("A", b"x"), ("H", b"1F\0"), ("d", bytes(8)), ("B", b"c\1\0\0\0\x1e")]
    out = []
    for t, v in vals:
        tag = b"MQ" + t.encode() + v
        for pre in (b"", b"XAZ" + b"k" * 19 + b"\0"):          # the value in the first window, and behind a slide
            out.append((_aux_rec(pre + tag), dict(kind="mq_proper", type=t)))
            out.append((rec(0x1 | 0x4 | 0x40, cigar=(), mapq=0, tags=pre + tag), dict(kind="mq_unmapped", type=t)))
    # the value cut off by the record's end, at each byte (a tail of fewer than four bytes is padding: no field at all)
    for t, size in (("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4)):
        for have in range(size):
            tag = b"MQ" + t.encode() + b"\x1e\x00\x00\x00"[:have]
            for pre in (b"", b"XAZ" + b"k" * 19 + b"\0", b"XAi\1\2\3\4"):
                out.append((rec_exact(P, cigar=CLIP, mapq=0, tags=pre + tag), dict(kind="mq_cut", type=t, have=have)))
                out.append((rec_exact(0x1 | 0x4 | 0x40, cigar=(), mapq=0, tags=pre + tag), dict(kind="mq_cut_unmapped", type=t, have=have)))
    # a second RG / MQ further on: the first one wins
    out.append((_aux_rec(b"RGZlib1\0RGZlib10\0MQC\x1e"), dict(kind="second_rg")))
    out.append((_aux_rec(b"RGZlib10\0XAi\1\2\3\4RGZlib1\0MQC\x1e"), dict(kind="second_rg")))
    out.append((_aux_rec(b"MQC\x1eRGZlib1\0MQC\x05"), dict(kind="second_mq")))
    out.append((_aux_rec(b"MQC\x05XAZ" + b"k" * 25 + b"\0MQC\x1e"), dict(kind="second_mq")))
    out.append((_aux_rec(b"RGAxRGZlib1\0", mapq=60), dict(kind="second_rg")))
    # alignment padding that spells a tag (l_seq = 100: the quality-stripped form keeps the record's length modulo 4)
    for npad in range(4):
        for spell in (b"RGZ", b"MQC", b"MQ\0", b"RGA"):
            for tags, mapq in ((b"", 60), (b"MQC\x1e", 0), (b"RGZlib1\0", 60), (b"XAZ" + b"k" * 18 + b"\0MQC\x1e", 0)):
                r = rec_exact(P, want_pad=npad, cigar=CLIP, mapq=mapq, tags=tags)
                out.append((r + spell[:npad], dict(kind="padding_spells", npad=npad)))
    return out


def aux_layout(cases):
    """every case once, then one whose RG tag is the last thing in the chunk: the window's look-ahead lies in the spare bytes"""
    recs = [r for r, _ in cases] + edge_records()
    return recs + [_aux_rec(b"XAZ" + b"k" * 17 + b"\0RGZlib1\0MQC\x1e")]


def edge_records():
    """the classes no other generator gives: a clip inside the CIGAR (19), a secondary alignment (0), a truncated record and
    more CIGAR-derived evidence than the slots hold (21)"""
    return [rec(P, cigar=((40, 0), (5, 4), (55, 0))), rec(P | 0x100), rec(P, cigar=CLIP)[:60],
            rec(P, cigar=((10, 0),) + ((1, 1), (10, 0)) * 6 + ((24, 0),))]


# ---- 4. read-group tables ----------------------------------------------------------------------------------------------------------

def djb2_bin(name):
    h = 5381
    for ch in reversed(name.encode() if isinstance(name, str) else name):
        h = (h * 33 + (ch if ch < 128 else ch - 256)) & 0xFFFFFFFF
    return h & 15


def table_bytes(names):
    """the blob size of im_set_insert_ranges (im_capi.hip)"""
    n = max(len(names), 1)
    return (4 * (20 + 3 * n) + sum(len(x) + 1 for x in names) + 8 + 3) // 4 * 4


def rg_table(target):
    """names (in insertion order) and ranges of a table whose blob takes exactly `target` bytes, with "generic" and, in one bin, a
    name older than a name it extends (the older one answers for the younger one's name)"""
    base = "pfx"
    ext = next(base + a + b for a in "abcdefghij" for b in "abcdefghijklmnopqrstuvwxyz" if djb2_bin(base + a + b) == djb2_bin(base))
    names = [ext, base, "generic"]
    k = 0
    while True:
        nm = "rg%04d" % k + "q" * (k % 9)
        if table_bytes(names + [nm]) > target - 20:
            break
        names.append(nm)
        k += 1
    # 12 bytes of table words + len + 1 per name, rounded up to 4: the last name grows until the size is met
    names.append("z")
    while table_bytes(names) < target:
        names[-1] += "w"
    assert table_bytes(names) == target and len(set(names)) == len(names), (table_bytes(names), target)
    return names, [300 + 3 * i for i in range(len(names))]


def rg_table_cases(names):
    """queries into every bin of the table, the prefix pair, absent names, no tag (generic), a tag of a wrong type"""
    out, seen = [], set()
    for nm in names:
        b = djb2_bin(nm)
        if b not in seen:
            seen.add(b)
            out.append((_aux_rec(b"RGZ" + nm.encode() + b"\0", mapq=60), dict(kind="rg_bin", bin=b)))
    for nm in ("pfx", names[0], "pf", "rg", names[-1], names[-1][:-1], names[len(names) // 2]):
        out.append((_aux_rec(b"RGZ" + nm.encode() + b"\0", mapq=60), dict(kind="rg_query", name=nm)))
    out.append((_aux_rec(b"RGZnobody\0", mapq=60), dict(kind="rg_absent")))
    out.append((_aux_rec(b"", mapq=60), dict(kind="no_rg")))
    out.append((_aux_rec(b"RGAx", mapq=60), dict(kind="rg_type")))
    out.append((_aux_rec(b"RGix\0\0\0", mapq=60), dict(kind="rg_type")))
    out.append((rec(0x1 | 0x4 | 0x40, cigar=(), tags=b"RGZpfx\0"), dict(kind="rg_unmapped")))
    return out


def defer_cases():
    """what defer_ranges = 1 changes: pairs that are not proper, with and without an insert size, strands opposite and equal"""
    out = []
    for isize in (0, 1, -1, 650, -650, 999999, 1000000, -1000000, 2000000, -(2 ** 31)):
        for flag in (0x1 | 0x20, 0x1 | 0x10, 0x1, 0x1 | 0x10 | 0x20):
            for tags in (b"", b"RGZnobody\0", b"RGAx"):
                out.append((rec(flag, isize=isize, tags=tags), dict(kind="pe", isize=isize, opposite=bool(flag & 0x10) != bool(flag & 0x20))))
    return out


# ---- 5. tiles and groups -----------------------------------------------------------------------------------------------------------

def _small(flag, L, cigar, seq_codes, tags=b"", **kw):
    # delivered without base qualities (bin = 0xFFFF), as the product's walkers deliver records
    return rec(flag, l_seq=L, cigar=cigar, seq=pack(seq_codes), qual=b"", tags=tags, bin_=0xFFFF, **kw)


def tile_templates(seed=505):
    """small records by role: candidates (both classes, both strands, with CIGAR-derived evidence), counted non-candidates,
    skipped records, error records"""
    rng = np.random.default_rng(seed)
    cand = []
    for L in (8, 9, 10, 11, 12):
        cand.append(_small(0x1 | 0x4 | 0x40, L, (), good_codes(rng, L)))
        cand.append(_small(0x1 | 0x4 | 0x40 | 0x20, L, (), good_codes(rng, L)))
        cand.append(_small(P, L, ((4, 0), (1, 1), (L - 5, 0)), good_codes(rng, L), pos=1000 + L))
        cand.append(_small(P | 0x10 | 0x20, L, ((3, 0), (2, 2), (L - 3, 0)), good_codes(rng, L), pos=2000 + L))
        cand.append(_small(P | 0x10, L, ((L - 3, 0), (3, 4)), good_codes(rng, L)))
    counted = [_small(P, L, ((L, 0),), good_codes(rng, L)) for L in (8, 10, 12)] + [_small(0x1 | 0x8, 9, ((9, 0),), good_codes(rng, 9))]
    skip = [_small(P | 0x100, 8, ((8, 0),), good_codes(rng, 8)), _small(0x2, 11, ((11, 0),), good_codes(rng, 11))]
    c = good_codes(rng, 10); c[4] = 3
    err = [_small(P, 10, ((10, 0),), c), _small(P, 9, ((4, 0), (2, 3), (5, 0)), good_codes(rng, 9)),
           _small(P, 8, ((8, 0),), good_codes(rng, 8), tags=b"RGAx"), _small(0x1 | 0x4 | 0x40, 8, (), good_codes(rng, 8), tags=b"MQZ1\0")]
    return dict(cand=cand, counted=counted, skip=skip, err=err)


def tile_pattern(name, n, tpl, seed=0):
    """role of each of n records: 0 cand, 1 counted, 2 skip, 3 err; and the template index inside the role"""
    rng = np.random.default_rng(1000 + seed + n)
    i = np.arange(n)
    if name == "all":
        role = np.zeros(n, np.int64)
    elif name == "none":
        role = np.where(i % 3 == 0, 2, 1)
    elif name == "first":
        role = np.where(i == 0, 0, 1)
    elif name == "last":
        role = np.where(i == n - 1, 0, 2)
    elif name == "lane255":
        role = np.where(i % 256 == 255, 0, 1)
    elif name == "err_counted":
        role = np.where((i // 256) % 2 == 0, 3, 1)
    else:
        role = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 4, n))
    keys = ["cand", "counted", "skip", "err"]
    sub = np.select([role == k for k in range(4)], [rng.integers(0, len(tpl[keys[k]]), n) for k in range(4)])
    return role, sub


# ---- 7. the depth feed -------------------------------------------------------------------------------------------------------------

def _drec(tid, pos, cigar, flag=0):
    # unpaired records (class 0): only the pileup sees them; eight bases, whatever the CIGAR says
    return rec(flag, tid=tid, pos=pos, cigar=cigar, l_seq=8, seq=b"\x12" * 4, mtid=-1, mpos=-1, isize=0)


def depth_cases():
    """four workgroups and a tail; returns the records in order (position in the list = record index)"""
    M = lambda n: ((n, 0),)
    un = lambda: _drec(0, 50, M(30), 0x4)                  # unmapped, with a position and a CIGAR: not piled up
    wg0 = [un() for _ in range(128)] + [_drec(-1, 10, M(10)) for _ in range(5)]
    wg0 += [_drec(0, 100, M(50))]                          # the first eligible record, in wave 2: window base 100 on contig 0
    wg0 += [_drec(0, 100 + 3 * k, M(40)) for k in range(60)]
    wg0 += [_drec(0, 4970, M(30)), _drec(0, 4971, M(30)), _drec(0, 4990, M(500))]      # ends at clen, at clen + 1, far past it
    wg0 += [_drec(1, 10 + k, M(25)) for k in range(256 - len(wg0))]                     # the second contig, in the first workgroup
    base = 200
    wg1 = [un() for _ in range(64)] + [_drec(2, 10, M(10)) for _ in range(64)] + [_drec(0, 10, M(10), 0x100) for _ in range(64)]
    wg1 += [_drec(0, 10, M(10), 0x200), _drec(0, 10, M(10), 0x400), _drec(1, 10, M(10), 0x4)]
    wg1 += [_drec(1, base, M(20))]                         # the first eligible record, in wave 3: window base 200 on contig 1
    wg1 += [_drec(1, base + 4095, M(10)), _drec(1, base + 4096, M(10)), _drec(1, base + 5000, M(10))]
    wg1 += [_drec(1, base + 4096 - 50, M(50)), _drec(1, base + 4095 - 50, M(50)), _drec(1, base + 4000, M(200))]    # a run ending at window offset 4096
    wg1 += [_drec(1, base + 10, ((5, 4), (10, 0), (3, 1), (10, 7), (4, 2), (10, 8), (7, 3), (10, 0), (2, 6), (5, 5)))]
    wg1 += [_drec(1, 100, M(2600))]                        # in front of the window base, and long
    wg1 += [_drec(1, base + 30 + k, M(15)) for k in range(256 - len(wg1))]
    wg2 = [_drec(1, 3000, M(10)) for _ in range(256)]      # 256 records at one position
    wg3 = [_drec(1, -1, M(20)), _drec(1, -20, M(50)), _drec(1, -50, M(50)), _drec(1, -5, ((10, 2), (10, 0)))]       # window base 0
    wg3 += [_drec(1, 4000, M(30)), _drec(1, 1000, M(30)), _drec(0, 4000, M(30)), _drec(1, 8970, M(30)), _drec(1, 8971, M(30)), _drec(1, 8999, M(1))]
    wg3 += [_drec(1, 9000, M(5)), _drec(1, 8000, ((10, 0), (2000, 2), (10, 0)))]
    wg3 += [_drec(1, 4090 + k, M(12)) for k in range(256 - len(wg3))]
    tail = [_drec(0, 2500, M(100), 0x10), _drec(1, 2500, M(100)), _drec(0, 0, M(5000)), _drec(1, 0, M(9000))] + [_drec(0, 7 * k, M(33)) for k in range(40)]
    return wg0 + wg1 + wg2 + wg3 + tail


def depth_facts(recs):
    """what the classify kernel's window logic meets on these records, restated: per workgroup the window base (the first
    pile-eligible record of the first wave that has one) and the conditions of tests/test_triage_cases_host.py"""
    facts = set()
    n_ctg = len(DEPTH_CONTIGS)
    for w0 in range(0, len(recs), 256):
        wg = recs[w0:w0 + 256]
        info = []
        for r in wg:
            tid, pos = struct.unpack_from("<ii", r, 0)
            l_qname, n_cig, flag = r[8], struct.unpack_from("<H", r, 12)[0], flag_of(r)
            cig = [struct.unpack_from("<I", r, 32 + l_qname + 4 * k)[0] for k in range(n_cig)]
            elig = 0 <= tid < n_ctg and not flag & (0x4 | 0x100 | 0x200 | 0x400)
            info.append((tid, pos, flag, cig, elig))
            if not elig and n_cig and pos >= 0:
                for bit in (0x4, 0x100, 0x200, 0x400):
                    if flag & bit:
                        facts.add("flag_%x" % bit)
                if tid == -1:
                    facts.add("tid_-1")
                if tid == n_ctg:
                    facts.add("tid_n")
        first = next((k for k, x in enumerate(info) if x[4]), None)
        if first is None:
            continue
        facts.add("first_in_wave_%d" % (first // 64))
        wtid, wpos = info[first][0], max(info[first][1], 0)
        if info[first][1] < 0:
            facts.add("first_pos_negative")
        if len({x[0] for x in info if x[4]}) > 1:
            facts.add("two_contigs_wg%d" % (w0 // 256))
        same = {}
        for tid, pos, flag, cig, elig in info:
            if not elig:
                continue
            same[(tid, pos)] = same.get((tid, pos), 0) + 1
            clen = DEPTH_CONTIGS[tid]
            if pos == -1:
                facts.add("pos_-1")
            if pos < -1:
                facts.add("pos_negative")
            x = pos
            for cw in cig:
                op, ln = cw & 15, cw >> 4
                facts.add("op_%d" % op)
                if op in (0, 7, 8):
                    if ln == 2600:
                        facts.add("2600M")
                    if x + ln == clen:
                        facts.add("ends_at_clen")
                    if x + ln == clen + 1:
                        facts.add("ends_at_clen+1")
                    if tid == wtid:
                        if x - wpos in (4095, 4096, 5000):
                            facts.add("starts_at_%d" % (x - wpos))
                        if x + ln - wpos == 4096:
                            facts.add("ends_at_4096")
                        if x + ln - wpos == 4095:
                            facts.add("ends_at_4095")
                        if x - wpos < 0 and x >= 0:
                            facts.add("in_front_of_window")
                    x += ln
                elif op in (2, 3):
                    x += ln
        if max(same.values()) == 256:
            facts.add("256_at_one_position")
    return facts


DEPTH_FACTS = {"flag_4", "flag_100", "flag_200", "flag_400", "tid_-1", "tid_n", "first_in_wave_2", "first_in_wave_3", "first_pos_negative",
               "two_contigs_wg0", "pos_-1", "pos_negative", "2600M", "ends_at_clen", "ends_at_clen+1", "starts_at_4095", "starts_at_4096",
               "starts_at_5000", "ends_at_4096", "ends_at_4095", "in_front_of_window", "256_at_one_position"} | {"op_%d" % k for k in range(9)}


# ---- 6. one mixed batch for the chunked run ----------------------------------------------------------------------------------------

APPEND_CHUNKS = [1, 255, 256, 257, 700, 1]             # then the rest


def append_batch():
    """about 3000 records of sections 1 to 3, interleaved; the one-record chunk behind the first five holds no candidate"""
    a = [r for r, _ in length_cases()]
    b = [r for r, _ in base_cases()][::2]
    c = [r for r, _ in aux_cases()] + [r for r, _ in mq_cases()]
    out = []
    for k in range(max(len(a), len(b), len(c))):
        for src in (a, b, c):
            if k < len(src):
                out.append(src[k])
    out = out[:3000]
    at = sum(APPEND_CHUNKS[:5])
    out[at] = filler(129)
    return out
