"""A plain restatement of -A (read counts for and against the known indels of annotate mode) for the tests: the
CIGAR bookkeeping of check_for_indel, the window with the variant applied, the span rule and the genotype rule in Python, the
Smith-Waterman statistics from the CPU checker (imo_sw_indel).  It reads only the BAM, the FASTA and the VCF a test hands it."""
import ctypes as C

import numpy as np

from tests.support import bamlite

INS, DEL = 0, 1
M, I, D, N, S, H, P, EQ, X = range(9)


class Known:
    """one record of the VCF as read_variants reads it"""

    def __init__(self, line):
        c = line.split("\t")
        self.chrom, self.start, self.ref, self.alt = c[0], int(c[1]), c[3], c[4]
        info = c[7].split(";")
        self.type = DEL if info[0].startswith("DELETION") else INS
        self.evd = info[1]
        kv = dict(x.split("=") for x in info if "=" in x)
        self.stop, self.bpstop = int(kv["END"]), int(kv["BP_END"])
        self.tagged = None
        self.column = c[9] if len(c) > 9 else None


def read_known(text, sample=None):
    out = []
    for ln in text.split("\n"):
        if ln and not ln.startswith("#"):
            k = Known(ln)
            if sample is not None:
                k.tagged = ln.split("\t")[7].split(";")[-1] == sample
            out.append(k)
    return out


def sw_stats(target, query):
    from tests.support import oraclebind as ob
    s, i, a = C.c_int32(), C.c_int32(), C.c_int32()
    ob.lib().imo_sw_indel(target, len(target), query, len(query), C.byref(s), C.byref(i), C.byref(a))
    return s.value, i.value, a.value


def window(seq, typ, start, stop, alt, rstart, rstop):
    """the reference stretch [rstart, rstop) with the variant applied (src/variant.c:1259-1272), bytes"""
    a_end = min(start, rstop)
    out = seq[rstart:a_end] if a_end > rstart else b""
    if typ == DEL:
        b_beg = stop - 1
        if rstop > b_beg >= 0:
            out += seq[b_beg:rstop]
    else:
        out += alt[1:]
        if rstop > a_end:
            out += seq[a_end:rstop]
    return out


def ref_end(pos, cigar):
    return pos + sum(ln for ln, op in cigar if op in (M, D, N, EQ, X))


def read_task(k, pos, cigar, bases, seq):
    """check_for_indel's bookkeeping for one read (cigar: [(len, op)], bases: bytes, seq: the contig's bytes) ->
    ("skip",) | ("direct",) | ("fatal",) | ("align", rstart, rstop, query, (subs, indels, aligned))"""
    subs = indels = aligned = 0
    overlaps = False
    qstart = qstop = -1
    readindx, refpos = 0, pos
    for sgi, (ln, op) in enumerate(cigar):
        sstart = refpos
        send = refpos + ln if op in (M, EQ, X, D) else refpos
        if not (send < k.start or sstart > k.stop):
            overlaps = True
        if op == S:
            if sgi == len(cigar) - 1:
                qstop = readindx
            readindx += ln
        elif op == I:
            if qstart == -1:
                qstart = readindx
            if k.type == INS and sstart == k.start:
                return ("direct",)
            readindx += ln; indels += ln; aligned += ln
        elif op == D:
            if k.type == DEL and sstart == k.start and send == k.stop - 1:
                return ("direct",)
            indels += ln
        elif op == M:
            if qstart == -1:
                qstart = readindx
            for i in range(ln):
                r = seq[sstart + i] if 0 <= sstart + i < len(seq) else 0
                if bases[readindx + i] != r:
                    subs += 1
            readindx += ln; aligned += ln
        else:
            return ("fatal",)
        refpos = send
    if qstop == -1:
        qstop = aligned + qstart
    if aligned != qstop - qstart:
        return ("fatal",)
    if not overlaps:
        return ("skip",)
    indelsize = abs(len(k.alt) - len(k.ref))
    rstart, rstop = pos, ref_end(pos, cigar)
    if rstop < k.bpstop:
        return ("skip",)
    if qstart == -1 or qstop == -1:
        return ("fatal",)
    rstart = max(rstart - indelsize, 0)
    rstop = min(rstop + indelsize, len(seq))
    return ("align", rstart, rstop, bases[qstart:qstop], (subs, indels, aligned))


def runs_of(pos, cigar):
    out, x, s = [], pos, None
    for ln, op in cigar:
        if op in (M, EQ, X):
            if s is None:
                s = x
            x += ln
            continue
        if s is not None:
            out.append((s, x)); s = None
        if op in (D, N):
            x += ln
    if s is not None:
        out.append((s, x))
    return out


def interval(k):
    return k.start, k.start + max(k.bpstop - k.stop, 0)


def spans_interval(pos, cigar, clen, b0, b1, m):
    for s, e in runs_of(pos, cigar):
        s, e = max(s, 0), min(e, clen)
        if e - s >= 2 * m and s <= b0 - m and b1 + m <= e:
            return True
    return False


def span_arrays(recs, clens, m, q):
    """-G's array: per contig, span[p] = eligible runs [s, e) with s <= p - m and p + m <= e"""
    d = [np.zeros(n + 2, np.int64) for n in clens]
    for r in recs:
        if r.flag & (0x4 | 0x100 | 0x200 | 0x400) or not 0 <= r.tid < len(clens) or r.mapq < q:
            continue
        for s, e in runs_of(r.pos, r.cigar):
            s, e = max(s, 0), min(e, clens[r.tid])
            if e - s >= 2 * m:
                d[r.tid][s + m] += 1
                d[r.tid][e - m + 1] -= 1
    return [np.cumsum(x)[:n + 1] for x, n in zip(d, clens)]


def fetched(recs_of_tid, beg, end):
    """what bam_fetch(tid, beg, end) delivers, in file order; an empty interval delivers nothing"""
    beg = max(beg, 0)
    if end <= beg:
        return []
    out = []
    for r in recs_of_tid:
        if r.pos >= end:
            break
        rend = ref_end(r.pos, r.cigar) if r.cigar else r.pos + 1
        if rend > beg:
            out.append(r)
    return out


def genotype_of(rs, ns):
    E, Cc, Hh = 20000, 44, 3010
    L = [ns * E + rs * Cc, (ns + rs) * Hh, ns * Cc + rs * E]
    lo = min(L)
    L = [x - lo for x in L]
    best = L.index(0)
    second = sorted(L[:best] + L[best + 1:])[0]
    return ("0/0", "0/1", "1/1")[best], min(99, (second + 500) // 1000)


class Restatement:
    def __init__(self, bam, fasta, m, q):
        _, self.refs, recs = bamlite.read_bam(bam)
        names, seqs = bamlite.read_fasta(fasta)
        self.names = [n for n, _ in self.refs]
        self.seqs = [seqs[names.index(n)].encode() for n in self.names]
        self.clens = [l for _, l in self.refs]
        self.m, self.q = m, q
        self.by_tid = [[r for r in recs if r.tid == t] for t in range(len(self.refs))]
        self.span = span_arrays(recs, self.clens, m, q)
        self.sw_tasks = 0

    def counts(self, k):
        """{N_all, AS, DC, RS, aborts}: aborts = the reference meets a read it dies on before any read supports k"""
        tid = self.names.index(k.chrom)
        seq = self.seqs[tid]
        b0, b1 = interval(k)
        n_all = n_as = n_dc = 0
        aborts = False
        bad_seen = False
        for r in fetched(self.by_tid[tid], k.start, k.stop):
            if r.flag & (0x4 | 0x100 | 0x200 | 0x400 | 0x800):
                continue
            t = read_task(k, r.pos, r.cigar, r.seq.encode(), seq)
            if t[0] == "skip":
                continue
            if t[0] == "fatal":
                if not bad_seen and n_all == 0:
                    aborts = True
                bad_seen = True
                continue
            ok = t[0] == "direct"
            if not ok:
                self.sw_tasks += 1
                s, i, a = sw_stats(window(seq, k.type, k.start, k.stop, k.alt.encode(), t[1], t[2]), t[3])
                ok = s <= t[4][0] and i <= t[4][1] and a >= t[4][2]
            if ok:
                n_all += 1
                if r.mapq >= self.q:
                    n_as += 1
                    if spans_interval(r.pos, r.cigar, self.clens[tid], b0, b1, self.m):
                        n_dc += 1
        lo, hi = max(b0, 0), min(b1, self.clens[tid])
        raw = int(self.span[tid][lo:hi + 1].min()) if lo <= hi else 0
        assert raw >= n_dc, (k.chrom, k.start, raw, n_dc)
        return dict(N_all=n_all, AS=n_as, DC=n_dc, RS=raw - n_dc, aborts=aborts)

    def column(self, k):
        if k.evd == "PAIRED_READ":
            return "./.:.,.:.", None
        c = self.counts(k)
        if c["RS"] + c["AS"] == 0:
            return "./.:0,0:.", c
        gt, gq = genotype_of(c["RS"], c["AS"])
        return "%s:%d,%d:%d" % (gt, c["RS"], c["AS"], gq), c


def strip_columns(out):
    """an -A VCF without what -A adds: the ##FORMAT lines, the last two fields of the header line and of every record"""
    lines = []
    for ln in out.decode().split("\n"):
        if ln.startswith("##FORMAT="):
            continue
        if ln and not ln.startswith("##"):
            cols = ln.split("\t")
            assert len(cols) == 10, ln
            ln = "\t".join(cols[:8])
        lines.append(ln)
    return "\n".join(lines).encode()


def check_output(out, rs, sample):
    """every record of an -A run against the restatement `rs`; returns the list of (Known, counts or None)"""
    text = out.decode().split("\n")
    fmt = [ln for ln in text if ln.startswith("##FORMAT=")]
    assert [ln.split(",")[0] for ln in fmt] == ["##FORMAT=<ID=GT", "##FORMAT=<ID=AD", "##FORMAT=<ID=GQ"]
    assert "Number=2" in fmt[1] and "support the indel" in fmt[1]
    assert text.index(fmt[0]) > max(i for i, ln in enumerate(text) if ln.startswith("##INFO="))
    assert [ln for ln in text if ln.startswith("#CHROM")] == ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    res = []
    for ln in text:
        if not ln or ln.startswith("#"):
            continue
        cols = ln.split("\t")
        assert len(cols) == 10 and cols[8] == "GT:AD:GQ", ln
        k = Known(ln)
        k.tagged = cols[7].split(";")[-1] == sample
        want, c = rs.column(k)
        assert cols[9] == want, (ln, want, c)
        res.append((k, c))
    return res
