"""What tests/test_gpu_splitlink.py and tests/test_splitlink_host.py share: the plain restatement of the split links (-S), written from
the definition in include/indelminer_amd.h (seam 5, "Split links"), not from the code under test.  tests/test_splitlink_host.py pins it
to cases worked by hand (no GPU needed).

A record is the BYTES of one delivered record (the 32-byte core and what follows it, either delivered form).  link_of restates the rule:
the front, the CIGAR (first / last operation that is not H, refend, L1 / T1), samtools' walk to the first SA tag, the one entry of its
value (a regular expression here, a byte-by-byte automaton on the device), the contig of its name, the side, and the two ends.
A LINK is (tidA, pA, sideA, tidB, pB, sideB); a QUERY is (tid1, side1, a0, a1, tid2, side2, b0, b1).
"""
import re
import struct

import numpy as np

NONE = 0xFFFFFFFF
HASH_MUL = 0x9E3779B97F4A7C15
EXCLUDED = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
REF_OPS = (0, 2, 3, 7, 8)                       # M D N = X
OPS = "MIDNSHP=X"
WINDOW = 32                                     # SPLIT_EV_WINDOW = CLIPTAIL_MAX_SHIFT
AUX_SIZE = {ord(c): n for cs, n in (("AcC", 1), ("sS", 2), ("iIf", 4), ("d", 8)) for c in cs}
ENTRY = re.compile(rb"([^,;\x00]+),([0-9]{1,10}),([+-]),((?:[0-9]{1,9}[MIDNSHP=X])+),([0-9]{1,3}),([0-9]+);?")
CIGAR_OP = re.compile(rb"([0-9]{1,9})([MIDNSHP=X])")


def find_tag(b, o_aux, tag):
    """the offset of the TYPE byte of the first occurrence of `tag` (2 bytes) by samtools' walk, or 0"""
    s, end = o_aux, len(b)
    while s + 4 <= end:
        if b[s:s + 2] == tag:
            return s + 2
        typ = b[s + 2]
        s += 3
        if typ in AUX_SIZE:
            s += AUX_SIZE[typ]
        elif typ in b"ZH":
            while s < end and b[s]:
                s += 1
            s += 1
        elif typ == ord("B"):
            if s + 5 > end:
                return 0
            ns = s + 5 + AUX_SIZE.get(b[s], 0) * struct.unpack_from("<I", b, s + 1)[0]
            if ns > end:
                return 0
            s = ns
        else:
            return 0
    return 0


def link_of(rec, names, clens, c, q):
    """the link of one record, or None"""
    b = bytes(rec)
    if len(b) < 32:
        return None
    tid, pos, l_qname, mapq, bin_, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 0)
    if l_seq < 0:
        return None
    o_cigar = 32 + l_qname
    o_aux = o_cigar + 4 * n_cigar + (l_seq + 1) // 2 + (0 if bin_ == 0xFFFF else l_seq)
    if o_aux > len(b):
        return None
    if flag & EXCLUDED or not 0 <= tid < len(clens) or mapq < q:
        return None
    ops = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_cigar, b, o_cigar)]
    if not any(op in REF_OPS for _, op in ops):
        return None
    body = [x for x in ops if x[1] != 5]
    first, last = body[0], body[-1]
    if len(body) < 2:
        first = last = (0, 0)                   # one operation alone consumes reference: it is no clip
    refend = pos + sum(n for n, op in ops if op in REF_OPS)
    lead = 0
    while ops[lead][1] in (4, 5):
        lead += 1
    trail = len(ops)
    while ops[trail - 1][1] in (4, 5):
        trail -= 1
    L1, T1 = sum(n for n, _ in ops[:lead]), sum(n for n, _ in ops[trail:])
    # the tag
    o = find_tag(b, o_aux, b"SA")
    if not o or b[o] != ord("Z"):
        return None
    z = b.find(b"\0", o + 1)
    if z < 0:
        return None
    m = ENTRY.fullmatch(b[o + 1:z])
    if not m:
        return None
    rname, p, strand, cigar, sa_mapq = m.group(1), int(m.group(2)), m.group(3), m.group(4), int(m.group(5))
    if not 1 <= p <= 2**31 - 1:
        return None
    sa_ops = [(int(n), OPS.index(chr(op[0]))) for n, op in CIGAR_OP.findall(cigar)]
    wanted = [i for i, n in enumerate(names) if (n.encode() if isinstance(n, str) else n) == rname]
    if not wanted:
        return None
    tid2, p2 = wanted[0], p - 1
    span2 = sum(n for n, op in sa_ops if op in REF_OPS)
    e2 = p2 + span2
    if span2 < 1 or e2 > clens[tid2] or sa_mapq < q:
        return None
    L2 = sa_ops[0][0] if sa_ops[0][1] in (4, 5) else 0
    T2 = sa_ops[-1][0] if sa_ops[-1][1] in (4, 5) else 0
    same = (strand == b"-") == bool(flag & 0x10)
    if not same:
        L2, T2 = T2, L2
    if L2 > L1 and T2 < T1:                     # BEHIND
        if not (last[1] == 4 and last[0] >= c and 0 <= refend <= clens[tid]):
            return None
        return (tid, refend, 0) + ((tid2, p2, 1) if same else (tid2, e2, 0))
    if L2 < L1 and T2 > T1:                     # FRONT
        if not (first[1] == 4 and first[0] >= c and 0 <= pos <= clens[tid]):
            return None
        return (tid, pos, 1) + ((tid2, e2, 0) if same else (tid2, p2, 1))
    return None


def split_raw(raw, off):
    raw = np.asarray(raw, np.uint8).tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def links_of(records, names, clens, c, q):
    return [x for x in (link_of(r, names, clens, c, q) for r in records) if x is not None]


def links_of_bam(bam, c, q):
    """(contig names, contig lengths, links) of a BAM file"""
    from indelminer_amd import rawrec
    raw, off, contigs = rawrec.records_from_bam(bam)
    names, clens = [n for n, _ in contigs], [n for _, n in contigs]
    return names, clens, links_of(split_raw(raw, off), names, clens, c, q)


def count(links, clens, query):
    tid1, side1, a0, a1, tid2, side2, b0, b1 = query
    a0, a1, b0, b1 = max(a0, 0), min(a1, clens[tid1]), max(b0, 0), min(b1, clens[tid2])
    if a0 > a1 or b0 > b1:
        return 0
    return sum(1 for ta, pa, sa, tb, pb, sb in links if ta == tid1 and sa == side1 and sb == side2 and a0 <= pa <= a1 and tb == tid2 and b0 <= pb <= b1)


def home_slot(tid, bucket, kind, log2_slots):
    """the first slot a link of this key probes (the header states the hash)"""
    key = (1 << 63) | (tid << 26) | (bucket << 2) | kind
    return ((key * HASH_MUL) & (2**64 - 1)) >> (64 - log2_slots)


# ---------------------------------------------------------------------- records by hand

def cigar_ops(text):
    """'5H35S60M' -> [(5, 5), (35, 4), (60, 0)]"""
    return [(int(n), OPS.index(op)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def sa(value):
    """an SA:Z field of this value"""
    return b"SAZ" + (value if isinstance(value, bytes) else value.encode()) + b"\0"


def make_record(tid=1, pos=1_000, mapq=60, flag=0, cigar="60M40S", aux=b"", l_seq=100, qual=True, cut=None, pad=True):
    """one record's bytes in the device layout (qual=False: without base qualities, bin 0xFFFF); cut: only its first bytes; pad: zeros up
    to a multiple of four, as delivered records have them"""
    ops = cigar_ops(cigar)
    qname = b"r7\0"
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(qname), mapq, 4680 if qual else 0xFFFF, len(ops), flag, l_seq, -1, -1, 0)
    body = core + qname + b"".join(struct.pack("<I", n << 4 | op) for n, op in ops) + b"\x11" * ((l_seq + 1) // 2) + (b"\x28" * l_seq if qual else b"") + aux
    if cut is not None:
        body = body[:cut]
    return body + (b"\0" * (-len(body) % 4) if pad else b"")


# ---------------------------------------------------------------------- the cases worked by hand

NAMES = ["c", "ctg1", "ctg10", "L" * 250]
CLENS = [5_000, 3_000, 2_000, 1_000]
MIN_CLIP, MIN_MAPQ = 20, 10
MD120 = b"MDZ" + b"7A" * 60 + b"\0"
BARR = b"ZBBs" + struct.pack("<I", 9) + b"\1\0" * 9                   # a B array of nine int16
GOOD = "ctg10,501,+,60S40M,60,0;"                                     # behind 60M40S at 1 000 on ctg1: (1, 1060, 0) -> (2, 500, 1)
LINK = (1, 1_060, 0, 2, 500, 1)


def _cases():
    """[(name, keyword arguments of make_record, the link worked by hand or None)]"""
    out = []

    def add(name, want, **kw):
        kw.setdefault("aux", sa(GOOD))
        out.append((name, kw, want))

    # the four strand x side cases (the header's worked examples, x = 1 000, p = 501)
    add("behind, same strand", (1, 1_060, 0, 2, 500, 1), cigar="60M40S", aux=sa("ctg10,501,+,60S40M,60,0;"))
    add("behind, other strand", (1, 1_060, 0, 2, 540, 0), cigar="60M40S", aux=sa("ctg10,501,-,40M60S,60,0;"))
    add("front, same strand", (1, 1_000, 1, 2, 540, 0), cigar="40S60M", aux=sa("ctg10,501,+,40M60S,60,0;"))
    add("front, other strand", (1, 1_000, 1, 2, 500, 1), cigar="40S60M", aux=sa("ctg10,501,-,60S40M,60,0;"))
    # a reverse primary: the strands are compared, not read
    add("reverse primary, '-' is the same strand", (1, 1_060, 0, 2, 500, 1), flag=0x10, aux=sa("ctg10,501,-,60S40M,60,0;"))
    add("reverse primary, '+' is the other strand", (1, 1_060, 0, 2, 540, 0), flag=0x10, aux=sa("ctg10,501,+,40M60S,60,0;"))
    # every clause of the front
    for bit in (0x4, 0x100, 0x200, 0x400, 0x800):
        add("flag 0x%x" % bit, None, flag=bit)
    add("paired, first, mate reverse", LINK, flag=0x1 | 0x40 | 0x20)
    add("mate unmapped does not matter", LINK, flag=0x1 | 0x8)
    add("tid -1", None, tid=-1)
    add("tid n_contigs", None, tid=4)
    add("mapq q - 1", None, mapq=9)
    add("mapq q", LINK, mapq=10)
    add("28 bytes", None, cut=28)
    add("the record ends inside its CIGAR", None, cut=40)
    add("negative l_seq", None, l_seq=-1)
    # the CIGAR
    add("no operation consumes reference", None, cigar="60I40S")
    add("one operation alone", None, cigar="100M")
    add("ties: L2 > L1 but T2 == T1", None, aux=sa("ctg10,501,+,40S20M40S,60,0;"))
    add("ties: clipped on both sides, L2 == L1", None, cigar="40S20M40S", aux=sa("ctg10,501,+,40S60M,60,0;"))
    add("clipped on both sides, the other part behind", (1, 1_020, 0, 2, 500, 1), cigar="40S20M40S", aux=sa("ctg10,501,+,60S40M,60,0;"))
    add("clipped on both sides, the other part in front", (1, 1_000, 1, 2, 540, 0), cigar="40S20M40S", aux=sa("ctg10,501,+,40M60S,60,0;"))
    add("clip of c - 1", None, cigar="81M19S", aux=sa("ctg10,501,+,81S19M,60,0;"))
    add("clip of c", (1, 1_080, 0, 2, 500, 1), cigar="80M20S", aux=sa("ctg10,501,+,80S20M,60,0;"))
    add("H outside S at the end", LINK, cigar="60M35S5H")
    add("H outside S at the start", (1, 1_000, 1, 2, 540, 0), cigar="5H35S60M", aux=sa("ctg10,501,+,40M60H,60,0;"))
    add("H alone is no soft clip", None, cigar="60M40H")
    add("S of c - 1 beside H: T1 counts both, the clip does not", None, cigar="60M19S21H")
    add("D and N and = and X count for refend", (1, 1_075, 0, 2, 500, 1), cigar="20M5D10=10X10N20M5I35S", aux=sa("ctg10,501,+,65S35M,60,0;"))
    add("refend at the contig's length", (1, 3_000, 0, 2, 500, 1), pos=2_940)
    add("refend behind the contig", None, pos=2_941)
    add("front at position 0", (1, 0, 1, 2, 540, 0), pos=0, cigar="40S60M", aux=sa("ctg10,501,+,40M60S,60,0;"))
    add("front at a negative position", None, pos=-1, cigar="40S60M", aux=sa("ctg10,501,+,40M60S,60,0;"))
    # the SA alignment
    add("pos 1", (1, 1_060, 0, 2, 0, 1), aux=sa("ctg10,1,+,60S40M,60,0;"))
    add("pos at the contig's last base", (1, 1_060, 0, 2, 1_999, 1), aux=sa("ctg10,2000,+,60S1M,60,0;"))
    add("pos 0", None, aux=sa("ctg10,0,+,60S40M,60,0;"))
    add("ten digits with leading zeros", LINK, aux=sa("ctg10,0000000501,+,60S40M,60,0;"))
    add("eleven digits", None, aux=sa("ctg10,00000000501,+,60S40M,60,0;"))
    add("pos 2^31", None, aux=sa("ctg10,2147483648,+,60S40M,60,0;"))
    add("pos 2^31 - 1 lies behind the contig", None, aux=sa("ctg10,2147483647,+,60S40M,60,0;"))
    add("pos 9999999999", None, aux=sa("ctg10,9999999999,+,60S40M,60,0;"))
    add("e2 == length", (1, 1_060, 0, 2, 2_000, 0), aux=sa("ctg10,1961,-,40M60S,60,0;"))
    add("e2 == length + 1", None, aux=sa("ctg10,1962,-,40M60S,60,0;"))
    add("e2 == length + 1, the end that is not used", None, aux=sa("ctg10,1962,+,60S40M,60,0;"))
    add("span2 0", None, aux=sa("ctg10,501,+,60S40I,60,0;"))
    add("span2 of D N = X", (1, 1_060, 0, 2, 544, 0), aux=sa("ctg10,501,-,10=10X4D10N10M60S,60,0;"))
    add("SA mapQ q - 1", None, aux=sa("ctg10,501,+,60S40M,9,0;"))
    add("SA mapQ q", LINK, aux=sa("ctg10,501,+,60S40M,10,0;"))
    add("SA mapQ 255", LINK, aux=sa("ctg10,501,+,60S40M,255,12;"))
    add("the same contig", (1, 1_060, 0, 1, 500, 1), aux=sa("ctg1,501,+,60S40M,60,0;"))
    # the names
    add("a name of one byte", (1, 1_060, 0, 0, 500, 1), aux=sa("c,501,+,60S40M,60,0;"))
    add("a name of 250 bytes", (1, 1_060, 0, 3, 500, 1), aux=sa("L" * 250 + ",501,+,60S40M,60,0;"))
    add("a name of 249 of them", None, aux=sa("L" * 249 + ",501,+,60S40M,60,0;"))
    add("a proper prefix of a name", None, aux=sa("ctg,501,+,60S40M,60,0;"))
    add("a name and one byte more", None, aux=sa("ctg100,501,+,60S40M,60,0;"))
    add("an unknown name", None, aux=sa("chrX,501,+,60S40M,60,0;"))
    # each malformed field
    for name, value in (("empty rname", ",501,+,60S40M,60,0;"), ("empty pos", "ctg10,,+,60S40M,60,0;"), ("a letter in pos", "ctg10,5a1,+,60S40M,60,0;"),
                        ("a sign in pos", "ctg10,+501,+,60S40M,60,0;"), ("strand *", "ctg10,501,*,60S40M,60,0;"), ("empty strand", "ctg10,501,,60S40M,60,0;"),
                        ("two strand bytes", "ctg10,501,+-,60S40M,60,0;"), ("empty cigar", "ctg10,501,+,,60,0;"), ("cigar ends in digits", "ctg10,501,+,60S40,60,0;"),
                        ("cigar starts with an operation", "ctg10,501,+,S40M,60,0;"), ("cigar *", "ctg10,501,+,*,60,0;"), ("operation B", "ctg10,501,+,60S40B,60,0;"),
                        ("a lower-case operation", "ctg10,501,+,60s40m,60,0;"), ("ten digits in the cigar", "ctg10,501,+,60S0000000040M,60,0;"),
                        ("empty mapQ", "ctg10,501,+,60S40M,,0;"), ("four digits of mapQ", "ctg10,501,+,60S40M,0060,0;"), ("a letter in mapQ", "ctg10,501,+,60S40M,6o,0;"),
                        ("empty NM", "ctg10,501,+,60S40M,60,;"), ("a letter in NM", "ctg10,501,+,60S40M,60,x;"), ("five fields", "ctg10,501,+,60S40M,60;"),
                        ("seven fields", "ctg10,501,+,60S40M,60,0,7;"), ("two entries", GOOD + "ctg1,7,+,60S40M,60,0;"), ("two semicolons", GOOD + ";"),
                        ("an empty value", ""), ("a semicolon alone", ";"), ("a space behind the entry", GOOD + " ")):
        add(name, None, aux=sa(value))
    add("nine digits in the cigar", LINK, aux=sa("ctg10,501,+,000000060S000000040M,60,0;"))
    add("a long NM", LINK, aux=sa("ctg10,501,+,60S40M,60,0123456789012;"))
    add("no final semicolon", LINK, aux=sa(GOOD[:-1]))
    add("P and I and H in the cigar", LINK, aux=sa("ctg10,501,+,50H10S5P20M3I20M,60,0;"))
    # the tag's type, place and end
    add("no SA tag", None, aux=b"NMC\1")
    add("no aux area", None, aux=b"")
    add("type H", None, aux=b"SAH" + GOOD.encode() + b"\0")
    add("type A", None, aux=b"SAA+" + sa(GOOD))
    add("the first occurrence is taken: a malformed one in front", None, aux=sa("ctg10,501") + sa(GOOD))
    add("the first occurrence is taken: a good one in front", LINK, aux=sa(GOOD) + sa("junk"))
    add("first of three fields", LINK, aux=sa(GOOD) + b"NMC\1" + b"ASi\x07\0\0\0")
    add("middle of three fields", LINK, aux=b"NMC\1" + sa(GOOD) + b"ASi\x07\0\0\0")
    add("last of three fields", LINK, aux=b"NMC\1" + b"ASi\x07\0\0\0" + sa(GOOD))
    add("behind every fixed-size type", LINK, aux=b"XAAx" + b"XcC\1" + b"Xcc\1" + b"XsS\1\0" + b"Xss\1\0" + b"XiI\1\0\0\0" + b"Xii\1\0\0\0" + b"Xff\0\0\0\0" + b"Xdd" + b"\0" * 8 + sa(GOOD))
    add("behind a B array and a long Z", LINK, aux=BARR + MD120 + sa(GOOD))
    add("behind a long Z and an H", LINK, aux=MD120 + b"XHH1A2B\0" + BARR + sa(GOOD))
    add("behind an unknown type", None, aux=b"XXq\1" + sa(GOOD))
    add("behind a B array that runs out of the record", None, aux=b"ZBBs" + struct.pack("<I", 5_000) + sa(GOOD))
    add("behind a Z without its NUL", None, aux=b"MDZ" + GOOD.encode())
    add("the letters SA inside another value", None, aux=b"MDZSAZ" + GOOD.encode() + b"\0")
    add("the tag ends with the record and has no NUL", None, aux=b"NMC\1" + b"SAZ" + GOOD.encode(), pad=False)
    add("the same bytes with their NUL", LINK, aux=b"NMC\1" + b"SAZ" + GOOD.encode()[:-1] + b"\0", pad=False)
    return out


CASES = _cases()
assert all(len(make_record(**kw)) % 4 == 0 for _, kw, _ in CASES)       # the two unpadded ones are multiples of four as they are


def pack(records):
    """[bytes] -> (raw uint8, rec_off uint32[n + 1])"""
    off = np.zeros(len(records) + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in records])
    return np.frombuffer(b"".join(records), np.uint8).copy(), off


# ---------------------------------------------------------------------- chunks through a BAM file

class _Reads:
    pass


def write_records_bam(path, specs, names=NAMES, clens=CLENS):
    """the records of `specs` (keyword arguments of make_record; cut, pad, l_seq and contigs outside the reference cannot go through a
    file) as a BAM file written by bamwrite.write_bam through its per-record overrides"""
    from indelminer_amd import bamwrite
    rd = _Reads()
    n = len(specs)
    rd.n, rd.read_len, rd.mapq = n, 100, 60
    full = [dict(dict(tid=1, pos=1_000, mapq=60, flag=0, cigar="60M40S", aux=b""), **s) for s in specs]
    rd.tid = np.array([s["tid"] for s in full]); rd.pos = np.array([s["pos"] for s in full]); rd.flag = np.array([s["flag"] for s in full])
    rd.mpos = np.full(n, -1); rd.isize = np.zeros(n, np.int64); rd.pair_id = np.full(n, 7)
    rd.ncig = np.ones(n, np.int64); rd.cig_len = np.full((n, 1), 100); rd.cig_op = np.zeros((n, 1), np.int64)
    rd.seq = np.full((n, 100), ord("A"), np.uint8)
    rd.overrides = {i: {"tags": s["aux"], "mapq": s["mapq"], "ops": cigar_ops(s["cigar"]), "mtid": -1} for i, s in enumerate(full)}
    bamwrite.write_bam(path, list(zip(names, clens)), rd)


def file_specs(cases=CASES):
    """the cases a BAM file can hold, as (name, keyword arguments, link)"""
    return [(name, kw, want) for name, kw, want in cases if not {"cut", "l_seq"} & set(kw) and 0 <= kw.get("tid", 1) < len(CLENS)]


# ---------------------------------------------------------------------- the three FILEs with SR=

SR_INFO = ("##INFO=<ID=SR,Number=2,Type=Integer,Description=\"Split reads whose primary part is clipped within 32 bases of the record's first breakpoint and whose SA tag "
           "places the clipped part within 32 bases of its second breakpoint, and the same from the second to the first\">\n")
SPLIT_LINKS = (
    "##splitLinks=\"SR counts primary records (neither unmapped, secondary, supplementary, duplicate nor failing quality control; paired or not) of mapping "
    "quality >= -q with a soft clip of at least 20 bases on the side of the breakpoint whose SA tag holds exactly one entry, of mapping quality >= -q, "
    "inside the contig it names, that places the clipped part of the read: the primary part ends at one breakpoint of the record, on the side the "
    "record's pile is clipped on, and the other part ends at the other, both within 32 bases; the first number counts the reads whose primary record "
    "lies at the record's first breakpoint, the second those at its second; a tag with several entries is not counted; SR is . once the split-link "
    "table has overflowed (stderr says so)\"\n")


def ends_of(svtype, names, fields):
    """the two ends (tid, position, side) of a printed record of -U ("DUP"), -N ("INV") or -T ("BND")"""
    info = dict(kv.split("=") for kv in fields[7].split(";"))
    tid, pos = names.index(fields[0]), int(fields[1])
    if svtype == "DUP":
        return (tid, pos, 1), (tid, int(info["END"]), 0)
    s1, s2 = (0 if x == "3" else 1 for x in info["CT"].split("to"))
    if svtype == "INV":
        return (tid, pos, s1), (tid, int(info["END"]), s2)
    return (tid, pos, s1), (names.index(info["CHR2"]), int(info["POS2"]), s2)


def sr_of(links, clens, first, second):
    q = lambda a, b: count(links, clens, (a[0], a[2], a[1] - WINDOW, a[1] + WINDOW, b[0], b[2], b[1] - WINDOW, b[1] + WINDOW))
    return q(first, second), q(second, first)


def with_sr(text, svtype, names, clens, links, overflowed=False):
    """(a FILE of -U, -N or -T as it is written with -S, [(first end, second end, n1, n2)]): the SR line behind the other ##INFO lines,
    the ##splitLinks line behind the file's description lines, ;SR=n1,n2 at the very end of every record"""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    last_info = max(i for i, ln in enumerate(lines) if ln.startswith("##INFO"))
    chrom = next(i for i, ln in enumerate(lines) if ln.startswith("#CHROM"))
    out, found = [], []
    for i, ln in enumerate(lines[:-1]):
        if i > chrom:
            first, second = ends_of(svtype, names, ln.split("\t"))
            n1, n2 = sr_of(links, clens, first, second)
            found.append((first, second, n1, n2))
            ln += ";SR=." if overflowed else ";SR=%d,%d" % (n1, n2)
        out.append(ln + "\n")
        if i == last_info:
            out.append(SR_INFO)
        if i == chrom - 1:
            out.append(SPLIT_LINKS)
    return "".join(out).encode(), found


# ---------------------------------------------------------------------- the planted data sets: the tags a split aligner would have written

def sa_value(L, s, k, reverse, name, po, so, h, mapq=60, shift=0, flip=False):
    """the SA value of a read of L bases clipped at an end of side s (0: kM(L - k)S, 1: kS(L - k)M) whose clipped bases continue at the
    other end (name, po, so) at micro-homology h -- forwards from po + h when so is 1, backwards from po - 1 - h when it is 0, on the
    other strand iff the sides are equal -- and the position pB it names; shift moves the placement, flip names the wrong strand"""
    n_clip = L - k if s == 0 else k
    n_rest = L - n_clip
    same = s != so
    start = (po + h if so == 1 else po - h - n_clip) + shift
    clip_first = (s == 0) == same               # on the same strand the other part's CIGAR clips what the primary aligns
    cigar = "%dS%dM" % (n_rest, n_clip) if clip_first else "%dM%dS" % (n_clip, n_rest)
    minus = reverse == same
    if flip:
        minus = not minus
    return "%s,%d,%s,%s,%d,0;" % (name, start + 1, "-" if minus else "+", cigar, mapq), (start if so == 1 else start + n_clip)


DECOYS = ("low mapQ", "33 outside", "32 off", "two entries", "strand flipped", "prefix name", "behind MD", "flag 0x800")
COUNTED = {"32 off", "behind MD"}


def plant_tags(rd, names, ends, decoy_ends, q=10):
    """Every clipped read of rd at an end A of `ends` ([(A, B, h)], A and B = (tid, position, side)) gets, through rd.overrides, the SA:Z
    tag of its other part at B.  The clipped reads at the ends of decoy_ends get, in arrival order and going round both ends, one decoy
    of DECOYS each (the eight once).  Returns {(A, B): [planted, decoys that do not count]}."""
    from indelminer_amd import synth
    L = rd.read_len
    rd.overrides = dict(getattr(rd, "overrides", None) or {})
    tally, todo = {}, list(DECOYS)
    at_end = {}
    for A, B, h in ends:
        t, p, s = A
        two = rd.ncig == 2
        if s == 0:
            hit = two & (rd.cig_op[:, 0] == synth.OP_M) & (rd.cig_op[:, 1] == synth.OP_S) & (rd.pos + rd.cig_len[:, 0] == p)
        else:
            hit = two & (rd.cig_op[:, 0] == synth.OP_S) & (rd.cig_op[:, 1] == synth.OP_M) & (rd.pos == p)
        at_end[(A, B, h)] = [int(i) for i in np.nonzero(hit & (rd.tid == t) & ((rd.flag & 0x4) == 0))[0]]
        tally[(A, B)] = [len(at_end[(A, B, h)]), 0]
    decoy_of = {}
    lists = [list(at_end[e]) for e in decoy_ends]
    turn = 0
    while todo and any(lists):
        if lists[turn % len(lists)]:
            decoy_of[lists[turn % len(lists)].pop(0)] = todo.pop(0)
        turn += 1
    assert not todo, "too few clipped reads at the decoy site"
    for (A, B, h), reads in at_end.items():
        for i in reads:
            s = A[2]
            k = int(rd.cig_len[i, 0])
            flag = int(rd.flag[i])
            d = decoy_of.get(i)
            kw = {}
            if d == "low mapQ":
                kw["mapq"] = q - 1
            elif d == "33 outside":
                kw["shift"] = WINDOW + 1 - h if B[2] == 1 else -(WINDOW + 1) + h
            elif d == "32 off":
                kw["shift"] = WINDOW - h if B[2] == 1 else -WINDOW + h
            elif d == "strand flipped":
                kw["flip"] = True
            value, _ = sa_value(L, s, k, bool(flag & 0x10), names[B[0]][:-1] if d == "prefix name" else names[B[0]], B[1], B[2], h, **kw)
            if d == "two entries":
                value += value
            mq = 0 if flag & 0x8 else int(rd.mapq)
            tags = b"MQC" + bytes([mq]) + (MD120 if d == "behind MD" else b"") + sa(value)
            if d == "flag 0x800":
                rd.flag[i] = flag | 0x800
            rd.overrides[i] = dict(rd.overrides.get(i, {}), tags=tags)
            if d is not None and d not in COUNTED:
                tally[(A, B)][1] += 1
    return tally


def planted(kind):
    """(module, refs, rd, names, tally) of the planted data set of -U ("DUP"), -N ("INV") or -T ("BND") with its tags and decoys"""
    from tests.support import crossedpiles, intercontig, invertedpiles
    mod = {"DUP": crossedpiles, "INV": invertedpiles, "BND": intercontig}[kind]
    refs, rd = mod.planted_reads()
    names = ["ctg%d" % t for t in range(len(refs))]
    ends = []
    if kind == "DUP":
        for pl, n in mod.SITES:
            ends += [((0, pl, 1), (0, pl + n, 0), 0), ((0, pl + n, 0), (0, pl, 1), 0)]
        decoys = ends[12:14]                    # the site of 1 000 bases
    elif kind == "INV":
        for a, n in mod.SITES:
            for x, y in ((a, a + n), (a + n, a)):
                ends += [((0, x, 0), (0, y, 0), 0), ((0, x, 1), (0, y, 1), 0)]
        decoys = ends[24:28]
    else:
        for ta, pa, sa_, tb, pb, sb, h in mod.SITES:
            ends += [((ta, pa, sa_), (tb, pb, sb), h), ((tb, pb, sb), (ta, pa, sa_), h)]
        decoys = ends[2:4] + ends[10:12]        # a 3to5 and a 3to3 site, both with 5 bases of homology
    tally = plant_tags(rd, names, ends, decoys)
    return mod, refs, rd, names, tally
