"""What tests/test_gpu_span.py and tests/test_gpu_pairspan.py share: the genotype rule restated, the interval queries and their
minima, a device context with one genome-wide array of the family enabled, the BAM header walk, the product binary and the golden
VCFs.  The restatements of the two arrays themselves (span_of, pspan_of) and the record parsers stay in their own files."""
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")


def genotype_of(rs, ns):
    """(GT, GQ) in thousandths of a phred, integers only"""
    E, C, H = 20000, 44, 3010
    L = [ns * E + rs * C, (ns + rs) * H, ns * C + rs * E]
    lo = min(L)
    L = [x - lo for x in L]
    best = L.index(0)                       # the lower index wins a tie
    second = sorted(L[:best] + L[best + 1:])[0]
    return ("0/0", "0/1", "1/1")[best], min(99, (second + 500) // 1000)


def read_bam_records(path, parse_record):
    """(contigs [(name, length)], [parse_record(bytes, start, end) of every record]) of a BAM file"""
    from tests.support import bamlite
    raw = bytes(bamlite.bgzf_decompress(path))
    assert raw[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]; p += 4
        name = raw[p:p + l_name - 1].decode(); p += l_name
        refs.append((name, struct.unpack_from("<i", raw, p)[0])); p += 4
    recs = []
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]; p += 4
        recs.append(parse_record(raw, p, p + bs))
        p += bs
    return refs, recs


class Device:
    """one context with the genome-wide array of one family ("span" or "pairspan") enabled for (m, min_mapq) over contigs of the
    given lengths; table: the insert ranges {group: range_max}, set in front of the enable when given"""

    def __init__(self, family, clens, m, min_mapq, table=None, seed=3):
        from indelminer_amd import capi
        self.capi = capi
        rng = np.random.default_rng(seed)
        self.contigs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in clens]
        self.clens = list(clens)
        self.ctx = capi.Context(0)
        self.ctx.set_reference(self.contigs)
        if table is not None:
            self.ctx.set_insert_ranges(list(table), [table[k] for k in table])
        self._scatter, self._scan, self.query_tid = (getattr(self.ctx, family + "_" + op) for op in ("scatter", "scan", "query_tid"))
        getattr(self.ctx, family + "_enable")(m, min_mapq)
        self.keep = []

    def scatter(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        recs = capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)
        self._scatter(recs)
        return recs

    def scan(self):
        for t in range(len(self.clens)):
            self._scan(t)
        self.ctx._check(self.capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def every_position(self, tid):
        p = np.arange(self.clens[tid] + 1, dtype=np.int32)
        return self.query_tid(tid, p, p).astype(np.int64)

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


def interval_queries(rng, clen, n=400):
    """whole intervals: short, longer than a wave's 64 lanes, reaching out of the contig on both sides, the whole contig"""
    beg = rng.integers(-50, clen + 1, n)
    ln = np.concatenate([rng.integers(0, 8, n // 2), rng.integers(60, 700, n - n // 2)])
    end = beg + ln
    beg = np.concatenate([beg, [0, -5, clen, clen - 1]]); end = np.concatenate([end, [clen, clen + 40, clen, clen + 9]])
    return beg.astype(np.int32), end.astype(np.int32)


def interval_minima(span, beg, end, clen):
    out = []
    for a, b in zip(beg, end):
        a, b = max(int(a), 0), min(int(b), clen)
        out.append(int(span[a:b + 1].min()) if a <= b else 0)
    return np.array(out, np.int64)


def check_device(dev, want, rng):
    for tid, clen in enumerate(dev.clens):
        got = dev.every_position(tid)
        bad = np.nonzero(got != want[tid])[0]
        assert len(bad) == 0, (tid, bad[:10], got[bad[:10]], want[tid][bad[:10]])
        beg, end = interval_queries(rng, clen)
        assert np.array_equal(dev.query_tid(tid, beg, end).astype(np.int64), interval_minima(want[tid], beg, end, clen)), tid


def _product():
    from indelminer_amd import build
    build.build()
    return build.build_host()


def _golden(name):
    return open(os.path.join(GOLD, "vcf", name + ".vcf"), "rb").read()
