"""Junction genotypes (-K): span_ends_kernel of im_span.hip behind im_span_query_ends, and what the host driver makes of it (the sample
column of -J's FILE).

The yardsticks are the plain restatements in tests/support/junctiongt.py, written from the rule in include/indelminer_amd.h (seam 5,
"Junction genotypes"), and the span restatement of tests/test_gpu_span.py; tests/test_junction_gt_host.py pins the first to cases worked
by hand.  Every answer is compared exactly.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.support import junctiongt as jg
from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl
from tests.support import spanarrays
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu

IM_OK, IM_E_ARG = 0, -1                          # include/indelminer_amd.h
M, Q = 3, 10


def _span_tests():
    from tests import test_gpu_span
    return test_gpu_span


def reads_on(rng, clens, per_contig):
    """[(tid, pos, mapq, flag, cigar)]: single-M reads of 6 .. 50 bases at random places, some reaching beyond their contig, one in
    twelve below the mapping quality"""
    recs = []
    for tid, (clen, n) in enumerate(zip(clens, per_contig)):
        for pos, ln, low in zip(rng.integers(0, clen, n), rng.choice([6, 7, 20, 50], n), rng.integers(0, 12, n)):
            recs.append((tid, int(pos), Q - 1 if low == 0 else 60, 0x63, [(0, int(ln))]))
    return recs


class Ends:
    """one context with the genome-wide span array over contigs of these lengths, filled through the scatter and the scan"""

    def __init__(self, clens, per_contig, seed, enable=True):
        tgs = _span_tests()
        rng = np.random.default_rng(seed)
        self.clens = list(clens)
        recs = reads_on(rng, clens, per_contig)
        self.want = tgs.span_of(recs, self.clens, M, Q)
        if enable:
            self.dev = spanarrays.Device("span", self.clens, M, Q)
            raw, off = tgs.raw_records(recs)
            self.dev.scatter(raw, off)
            self.dev.scan()
            self.ctx, self.capi = self.dev.ctx, self.dev.capi
        else:
            from indelminer_amd import capi
            self.dev, self.capi = None, capi
            self.ctx = capi.Context(0)
            self.ctx.set_reference([b"A" * n for n in clens])

    def every_end(self):
        tid = np.concatenate([np.full(n + 1, t, np.int32) for t, n in enumerate(self.clens)])
        pos = np.concatenate([np.arange(n + 1, dtype=np.int32) for n in self.clens])
        return tid, pos

    def raw(self, n, tid, pos, slack, null=None):
        """the entry itself: (return code, the answers as given back) over columns of sentinels; null: a column left out"""
        tid, pos = np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(pos, np.int32)
        out = np.full(max(len(tid), 1), 77, np.uint32)
        ptrs = [None if k == null else a.ctypes.data_as(C.c_void_p) for k, a in enumerate((tid, pos, out))]
        rc = self.capi.lib().im_span_query_ends(self.ctx.h, n, ptrs[0], ptrs[1], slack, ptrs[2])
        return rc, out

    def err(self):
        return self.capi.lib().im_last_error(self.ctx.h).decode()

    def close(self):
        if self.dev:
            self.dev.close()
        else:
            self.ctx.close()


@pytest.fixture(scope="module")
def three():
    e = Ends([1, 300, 5_000], [4, 400, 6_000], seed=41)
    yield e
    e.close()


def test_every_position_of_every_contig_in_one_call(three):
    """5 304 ends -- above 1 024, no multiple of 64 -- against the restatement and against im_span_query_tid, contig by contig; then the
    same ends shuffled, so that neighbouring lanes hold different contigs"""
    e = three
    tid, pos = e.every_end()
    assert len(tid) == 5_304 and len(tid) % 64 and e.want[1].max() >= 5 and e.want[2].max() >= 5 and not e.want[0].any()
    want = np.concatenate(e.want)
    got = e.ctx.span_query_ends(tid, pos).astype(np.int64)
    assert np.array_equal(got, want)
    by_tid = np.concatenate([e.dev.every_position(t) for t in range(3)])
    assert np.array_equal(got, by_tid)
    order = np.random.default_rng(8).permutation(len(tid))
    assert (tid[order][:-1] != tid[order][1:]).sum() > 100
    assert np.array_equal(e.ctx.span_query_ends(tid[order], pos[order]).astype(np.int64), want[order])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_counts_around_a_wave(three, n):
    e = three
    tid, pos = e.every_end()
    pick = np.random.default_rng(n).permutation(len(tid))[:n]
    want = np.concatenate(e.want)[pick]
    assert np.array_equal(e.ctx.span_query_ends(tid[pick], pos[pick]).astype(np.int64), want)
    rc, out = e.raw(n, tid[pick], pos[pick], 0)
    assert rc == IM_OK and np.array_equal(out[:n].astype(np.int64), want) and (out[n:] == 77).all()      # nothing behind the n-th answer is written
    if n == 0:
        assert e.raw(0, [], [], 0, null=0)[0] == IM_OK and e.raw(0, [], [], 255, null=2)[0] == IM_OK      # no launch, no column looked at


@pytest.mark.parametrize("slack", [1, 31, 255])
def test_slack_clipped_at_both_edges(three, slack):
    """the interval at the first two and the last two positions of every contig and in its middle: on the contig of one base it is
    wider than the contig, on the one of 300 bases a slack of 255 covers both edges at once"""
    e = three
    ends = sorted({(t, p) for t, n in enumerate(e.clens) for p in (0, 1, n - 1, n, n // 2) if 0 <= p <= n})
    tid, pos = [t for t, _ in ends], [p for _, p in ends]
    assert (0, 1) in ends and (2, 5_000) in ends and len(ends) == 2 + 5 + 5
    want = jg.ends_minima(e.want, tid, pos, slack)
    assert np.array_equal(e.ctx.span_query_ends(tid, pos, slack).astype(np.int64), want)
    # by definition what im_span_query_tid answers for that interval
    for t, p, w in zip(tid, pos, want):
        assert int(e.dev.query_tid(t, [p - slack], [p + slack])[0]) == w
    # and somewhere the slack matters: a random draw of ends, where the minimum is below the value at the end itself
    rng = np.random.default_rng(slack)
    tid = rng.integers(1, 3, 200).astype(np.int32)
    pos = np.array([rng.integers(0, e.clens[t] + 1) for t in tid], np.int32)
    want = jg.ends_minima(e.want, tid, pos, slack)
    assert (want < jg.ends_minima(e.want, tid, pos, 0)).any()
    assert np.array_equal(e.ctx.span_query_ends(tid, pos, slack).astype(np.int64), want)


def test_the_last_position_of_the_last_contig_and_every_argument_error(three):
    e = three
    assert int(e.ctx.span_query_ends([2], [5_000])[0]) == int(e.want[2][5_000]) == 0
    assert int(e.ctx.span_query_ends([2], [4_990])[0]) == int(e.want[2][4_990])
    assert [int(v) for v in e.ctx.span_query_ends([2, 0, 1], [5_000, 1, 300], 255)] == [int(e.want[2][4_745:].min()), 0, int(e.want[1][45:].min())]
    good_t, good_p = [0, 1, 2], [0, 5, 7]
    for args, what in (((-1, good_t, good_p, 0), "n -1"), ((3, good_t, good_p, -1), "slack -1"), ((3, good_t, good_p, 256), "slack 256"),
                       ((3, [0, 1, 3], good_p, 0), "end 2: tid 3"), ((3, [0, -1, 2], good_p, 0), "end 1: tid -1"),
                       ((3, good_t, [0, 301, 7], 0), "end 1: pos 301"), ((3, good_t, [2, 5, 7], 0), "end 0: pos 2"), ((3, good_t, [0, 5, -1], 0), "end 2: pos -1"),
                       ((3, good_t, [0, 5, 5_001], 255), "end 2: pos 5001")):
        rc, out = e.raw(*args)
        assert rc == IM_E_ARG and (out == 77).all() and "im_span_query_ends" in e.err() and what in e.err(), (args, e.err())
    for k in range(3):
        rc, out = e.raw(3, good_t, good_p, 0, null=k)
        assert rc == IM_E_ARG and (out == 77).all() and "null column" in e.err()
    assert e.capi.lib().im_span_query_ends(None, 0, None, None, 0, None) == IM_E_ARG
    assert e.raw(3, good_t, good_p, 255)[0] == IM_OK


def test_a_call_before_the_array_is_enabled():
    cold = Ends([1, 300, 5_000], [0, 0, 0], seed=1, enable=False)
    try:
        rc, out = cold.raw(2, [1, 2], [5, 7], 0)
        assert rc == IM_E_ARG and (out == 77).all() and "im_span_enable has not been called" in cold.err()
        with pytest.raises(cold.capi.IMError, match="im_span_enable has not been called"):
            cold.ctx.span_query_ends([1], [5])
    finally:
        cold.close()


def test_contigs_of_several_scan_tiles():
    """the scan leaves tile-local sums and a run of tile offsets per contig (8 192 positions a tile): ends on either side of every tile
    edge of two contigs of three and two tiles, and a random draw, each lane with its own contig's offsets"""
    e = Ends([20_000, 9_000], [30_000, 12_000], seed=43)
    try:
        edges = [(t, p + d) for t, n in enumerate(e.clens) for p in range(8_192, n, 8_192) for d in (-1, 0, 1)] + [(0, 20_000), (1, 9_000), (1, 0), (0, 0)]
        rng = np.random.default_rng(9)
        tid = np.concatenate([[t for t, _ in edges], rng.integers(0, 2, 3_000)]).astype(np.int32)
        pos = np.concatenate([[p for _, p in edges], [rng.integers(0, e.clens[t] + 1) for t in tid[len(edges):]]]).astype(np.int32)
        assert e.want[0][8_192:].max() >= 10 and e.want[1][8_192:].max() >= 10
        for slack in (0, 40):
            assert np.array_equal(e.ctx.span_query_ends(tid, pos, slack).astype(np.int64), jg.ends_minima(e.want, tid, pos, slack)), slack
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ the product

def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r


def _err(r):
    """stderr without the whole seconds of its time stamps, which differ between two runs that straddle a second"""
    return re.sub(rb" : \d+ sec\. elapsed\n", b"\n", r.stderr)


BASE = ["-i", "cfg.txt", "-s", "100"]
ENVS = ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})


def _write(kind, tmp_path):
    if kind == "TRUTH":
        refs, rd = jg.planted_truth()
        return jg.write_planted(str(tmp_path), refs, rd)
    mod, refs, rd, _, _ = sl.planted(kind)
    return mod.write_planted(str(tmp_path), refs, rd)


@pytest.mark.parametrize("kind", ["TRUTH", "DUP", "INV", "BND"])
def test_product_file_on_the_planted_data_sets(kind, tmp_path):
    """the data set with planted truth and the planted data sets of -U, -N and -T with the tags a split aligner would have written: FILE
    with -K byte for byte the restatement's, alone and behind the whole chain, on the pipelined path, on the record-at-a-time path and with
    three walkers; without -K the parent's FILE; stdout, stderr and the other FILEs what they are without -K"""
    d = _write(kind, tmp_path)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    want, found, calls = jg.render_of_bam(bam, fa)
    plain = sj.render_of_bam(bam, fa, 10)[0]
    assert len(found) >= 4 and want.count(b"\n") == jg.header().count("\n") + len(found) and want != plain
    tgs = _span_tests()
    refs, recs = tgs.read_bam_records(bam)
    spans = jg.spans_of_bam(bam)[2]
    assert all(np.array_equal(a, b) for a, b in zip(spans, tgs.span_of(recs, [n for _, n in refs], jg.FLANK, jg.MIN_MAPQ)))      # the two restatements of span[]
    if kind == "TRUTH":
        assert [c[0] for c in calls] == ["0/1", "1/1", "0/1", "1/1"]
    else:
        assert {c[0] for c in calls} >= {"0/1"} and any(c[4] != c[5] for c in calls) and max(c[4] for c in calls) >= 5
    prod = _product()
    path = lambda name: str(tmp_path / name)
    read = lambda name: open(path(name), "rb").read()
    chain = lambda k: ["-G", "-C", "-V", "-U", path("u%d" % k), "-N", path("n%d" % k), "-T", path("t%d" % k), "-M", "-S", "-J", path("j%d" % k)]
    r0 = _ok(_run(prod, BASE + chain(0), d))
    r1 = _ok(_run(prod, BASE + chain(1) + ["-K"], d))
    assert read("j0") == plain and read("j1") == want
    assert r1.stdout == r0.stdout and _err(r1) == _err(r0) and (read("u1"), read("n1"), read("t1")) == (read("u0"), read("n0"), read("t0")) and len(r0.stdout) > 500
    g0 = _ok(_run(prod, BASE + ["-G", "-J", path("j2")], d))
    g1 = _ok(_run(prod, BASE + ["-K", "-G", "-J", path("j3")], d))
    assert read("j2") == plain and read("j3") == want and g1.stdout == g0.stdout and _err(g1) == _err(g0)
    for k, env in enumerate(ENVS, 4):
        r = _ok(_run(prod, BASE + ["-G", "-J", path("j%d" % k), "-K"], d, env=env))
        assert read("j%d" % k) == want and r.stdout == g0.stdout, env
    if kind == "TRUTH":
        column = [ln.split(b"\t")[9].decode() for ln in read("j1").split(b"\n") if ln and not ln.startswith(b"#")]
        assert column == ["0/1:10,10:99:10,10", "1/1:0,20:59:0,0", "0/1:10,10:99:20,20", "1/1:0,20:59:20,20"]


def test_product_detailed_output_ignores_the_option_and_it_is_refused_alone(tmp_path):
    d = _write("TRUTH", tmp_path)
    prod = _product()
    fo = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-J", fo, "-K"], d))
    assert d1.stdout == d0.stdout and _err(d1) == _err(d0) and not os.path.exists(fo)
    r = _run(prod, BASE + ["-G", "-K"], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -K needs -J\n"
    r = _run(prod, BASE + ["-K", "-J", fo], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -J needs -G\n" and not os.path.exists(fo)


def test_product_after_an_overflow_of_the_split_link_table(tmp_path):
    """2 100 more split reads than the planted ones against the 2 048 links the table of a small BAM keeps (the means of
    tests/test_gpu_splitjunction.py): FILE holds the header of -K alone, and stderr says what it says without -K"""
    from indelminer_amd import synth
    mod, refs, rd, names, _ = sl.planted("DUP")
    plain = np.nonzero((rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & 0x4) == 0) & (rd.pos > 200) & (rd.pos < 50_000))[0]
    for i in plain[::3][:2_100]:
        i = int(i)
        rd.cig_op[i, :2] = (synth.OP_M, synth.OP_S); rd.cig_len[i, :2] = (70, 30); rd.ncig[i] = 2
        mq = 0 if int(rd.flag[i]) & 0x8 else int(rd.mapq)
        rd.overrides[i] = {"tags": b"MQC" + bytes([mq]) + sl.sa("ctg0,%d,%s,70S30M,60,0;" % (int(rd.pos[i]) + 5_001, "-" if int(rd.flag[i]) & 0x10 else "+"))}
    d = mod.write_planted(str(tmp_path), refs, rd)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    _, clens, links = sl.links_of_bam(bam, sl.MIN_CLIP, 10)
    assert len(links) >= 2_100 and os.path.getsize(bam) < 64 << 16
    prod = _product()
    f0, f1 = str(tmp_path / "j0"), str(tmp_path / "j1")
    r0 = _run(prod, BASE + ["-G", "-J", f0], d)
    r1 = _run(prod, BASE + ["-G", "-J", f1, "-K"], d)
    assert r0.returncode == 0 and r1.returncode == 0
    assert open(f0, "rb").read() == sj.HEADER.encode() and open(f1, "rb").read() == jg.header().encode() == jg.render_of_bam(bam, fa, overflowed=True)[0]
    line = b"indelminer: -J: the split-link table overflowed (2048 links stored, %d dropped): its file has no records\n" % (len(links) - 2_048)
    assert r1.stdout == r0.stdout and _err(r1) == _err(r0) and _err(r1).endswith(line)
