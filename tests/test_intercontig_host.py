"""-T (breakpoints between contigs) where there is no GPU: the restatement the GPU tests measure against (tests/support/intercontig.py)
pinned on cases worked by hand, on the planted tables of the one-contig rules it generalises, and on the planted data set of
tests/test_gpu_intercontig.py; and the host driver linked against tests/shim/im_shim.c, which must say what -T needs."""
import os
import subprocess

import numpy as np
import pytest

from tests.support import intercontig as ic
from tests.support.intercontig import Rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")
ENTRY_POINTS = ["im_matelink_enable", "im_dev_matelink_scatter", "im_matelink_add", "im_matelink_partner", "im_matelink_reset", "im_matelink_stats",
                "im_cliptail_junction"]
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]

# two contigs of 200 bases, written out
A = b"GCTTAAAAGCCATGGAATCTTACGCAGCCCCCTCGTACGAGGGTCTTTCATTCGATTCTATTTGATGATACTTACTGACGACCCGATTGTAGTGGGGGGGGTTCTAGTTTTCATTGGTCATTGGTCTGTGCCGCATTTCATCATCTGTAATTTGTATAAAAACGGCCGGAGTAGCTCGCCGAATTAGGCACAGGCTGCTT"
B = b"ATCGCTTCCAAACACAGTCTAAAGGTCGTCACAGGATTGACAATCATAGAGAGACTGGTCCATTGCATTGGATAATGACAGCCCGCCTACCTCATCATGCATCCTCGTCCGGAGTACATAGACGTGCCCCTATCATAATGCGCAACAACGACTATCTAGTGGTCTCCGTTCCAATAGATATGACCTATCAGTCGATGAAT"


def test_record_rule_on_cases_worked_by_hand():
    clens = [1_000, 500, 70]
    r = lambda **kw: Rec(**dict(dict(tid=0, pos=100, mapq=60, flag=0x1 | 0x40, mtid=1, mpos=400), **kw))
    link = lambda **kw: ic.link_of(r(**kw), clens, 10)
    assert link() == (0, 0, 100, 1, 400)
    # the four kinds: this read reverse is bit 0, its mate reverse bit 1
    assert [link(flag=0x1 | f)[1] for f in (0, 0x10, 0x20, 0x30)] == [0, 1, 2, 3]
    # no leftmost-read rule: both reads of a pair store a link, each at its own contig; first and second in pair alike
    assert link(flag=0x1 | 0x80) == (0, 0, 100, 1, 400) and link(tid=1, pos=400, mtid=0, mpos=100) == (1, 0, 400, 0, 100)
    assert link(flag=0x1 | 0x2 | 0x40) is not None                                      # the proper-pair bit does not matter
    # every clause
    assert link(flag=0x40) is None                                                     # not paired
    assert all(link(flag=0x1 | bit) is None for bit in (0x4, 0x8, 0x100, 0x200, 0x400, 0x800))
    assert link(mtid=0) is None and link(tid=1, mtid=1) is None                        # the mate on the same contig
    assert link(mtid=-1) is None and link(mtid=3) is None and link(tid=-1) is None and link(tid=3) is None
    assert link(mtid=2, mpos=70) == (0, 0, 100, 2, 70)
    assert link(mapq=9) is None and link(mapq=10) is not None
    assert link(pos=0) is not None and link(pos=-1) is None and link(pos=1_000) is not None and link(pos=1_001) is None
    assert link(mpos=0) is not None and link(mpos=-1) is None and link(mpos=500) is not None and link(mpos=501) is None
    assert link(mtid=2, mpos=71) is None and link(tid=2, pos=70, mtid=0, mpos=1_000) == (2, 0, 70, 0, 1_000)
    recs = [r(), r(mapq=3), r(tid=1, pos=400, mtid=0, mpos=100, flag=0x1 | 0x80 | 0x30)]
    assert ic.links_of(recs, clens, 10) == [(0, 0, 100, 1, 400), (1, 3, 400, 0, 100)]


def test_partner_vote_on_cases_worked_by_hand():
    clens = [100_000, 50_000, 300_000]
    q = lambda links, *a: ic.partner(links, clens, 0, *a)
    L = lambda mtid, mpos, pos=500, kind=0: (0, kind, pos, mtid, mpos)
    assert q([], 0, 0, 1_000) == (0, -1, 0, 0, 0)
    # the interval is inclusive, the kind and the contig are the query's, the clip is to [0, length]
    links = [L(1, 3_000, pos=100), L(1, 3_010, pos=200), L(1, 3_020, pos=201), L(1, 3_030, pos=150, kind=1), (2, 0, 150, 1, 3_040)]
    assert q(links, 0, 100, 200) == (2, 1, 2, 3_000, 3_010) and q(links, 0, 101, 201) == (2, 1, 2, 3_010, 3_020)
    assert q(links, 1, 0, 1_000) == (1, 1, 1, 3_030, 3_030) and q(links, 2, 0, 1_000) == (0, -1, 0, 0, 0)
    assert q(links, 0, -50_000, 15_535) == (3, 1, 3, 3_000, 3_020) and q(links, 0, 202, 100_500) == (0, -1, 0, 0, 0)
    assert q([L(1, 7, pos=0), L(1, 9, pos=100_000)], 0, -5, 100_005) == (2, 1, 2, 7, 9)
    # two neighbouring cells count together: 1 023 | 1 024 is a border, 2 047 | 2 048 the next
    assert q([L(1, 1_023), L(1, 1_024)], 0, 0, 1_000) == (2, 1, 2, 1_023, 1_024)
    assert q([L(1, 1_023), L(1, 1_024), L(1, 2_047), L(1, 2_048)], 0, 0, 1_000) == (4, 1, 3, 1_023, 2_047)       # cells 0 + 1 = cells 1 + 2 = 3: the smaller c
    assert q([L(1, 1_023), L(1, 2_048)], 0, 0, 1_000) == (2, 1, 1, 1_023, 1_023)                                  # cells 0 and 2 are no neighbours
    assert q([L(1, 1_023), L(1, 2_048), L(1, 2_049)], 0, 0, 1_000) == (3, 1, 2, 2_048, 2_049)
    assert q([L(1, 0), L(1, 2_047), L(1, 2_048), L(1, 4_000)], 0, 0, 1_000) == (4, 1, 2, 0, 2_047)                # (0, 1) ties with (1, 2) and (2, 3)
    # equal scores on two contigs: the smaller mtid; on two cells: the smaller cell; a larger score beats both
    assert q([L(2, 5_000), L(2, 5_001), L(1, 9_000), L(1, 9_001)], 0, 0, 1_000) == (4, 1, 2, 9_000, 9_001)
    assert q([L(2, 5_000), L(2, 5_001), L(2, 5_002), L(1, 9_000), L(1, 9_001)], 0, 0, 1_000) == (5, 2, 3, 5_000, 5_002)
    assert q([L(1, 20_000), L(1, 20_001), L(1, 9_000), L(1, 9_001)], 0, 0, 1_000) == (4, 1, 2, 9_000, 9_001)
    # 255, 256 and 257 distinct cells: the cap is on the cells, not on the links
    many = [L(2, 1_024 * c) for c in range(257)]
    assert q(many[:255] + [L(2, 5)], 0, 0, 1_000) == (256, 2, 3, 0, 1_024)
    assert q(many[:256] + [L(2, 5)], 0, 0, 1_000) == (257, 2, 3, 0, 1_024)
    assert q(many, 0, 0, 1_000) == (257, -2, 0, 0, 0) and q(many + many, 0, 0, 1_000) == (514, -2, 0, 0, 0)
    assert q(many[::-1], 0, 0, 1_000) == (257, -2, 0, 0, 0) and q(many[:256][::-1] + [L(2, 5)], 0, 0, 1_000) == (257, 2, 3, 0, 1_024)


def _codes(text):
    return tuple(b"ACGT".index(c) for c in text)


def _comp(text):
    return bytes(b"TGCA"[b"ACGT".index(c)] for c in text)


def test_junction_four_cases_at_shifts_0_and_5_worked_by_hand():
    refs = [A, B]
    for s in (0, 5):
        # 3to5: right clips at A:100 go on forwards from B:50 + s; left clips at B:50 go on backwards from A:99 - s
        t = {(0, 0, 100): [_codes(B[50 + s:70 + s])] * 2, (1, 1, 50): [_codes(A[80 - s:100 - s][::-1])] * 3}
        assert ic.junction(t, refs, 0, 100, 0, 1, 50, 1) == (2, 3, s, 2, 3)
        assert ic.junction(t, refs, 1, 50, 1, 0, 100, 0) == (3, 2, s, 3, 2)            # the ends the other way round
        # 5to3: left clips at A:100 go on backwards from B:49 - s; right clips at B:50 go on forwards from A:100 + s
        t = {(0, 1, 100): [_codes(B[30 - s:50 - s][::-1])] * 2, (1, 0, 50): [_codes(A[100 + s:120 + s])] * 3}
        assert ic.junction(t, refs, 0, 100, 1, 1, 50, 0) == (2, 3, s, 2, 3)
        # 3to3: both piles of right clips, each the complement of the other contig running backwards
        t = {(0, 0, 100): [_codes(_comp(B[30 - s:50 - s][::-1]))] * 2, (1, 0, 50): [_codes(_comp(A[80 - s:100 - s][::-1]))] * 3}
        assert ic.junction(t, refs, 0, 100, 0, 1, 50, 0) == (2, 3, s, 2, 3)
        assert ic.junction(t, refs, 0, 100, 0, 1, 50, 1)[:3] == (0, 0, -1)             # the same piles asked as another case
        # 5to5: both piles of left clips, each the complement of the other contig running forwards
        t = {(0, 1, 100): [_codes(_comp(B[50 + s:70 + s]))] * 2, (1, 1, 50): [_codes(_comp(A[100 + s:120 + s]))] * 3}
        assert ic.junction(t, refs, 0, 100, 1, 1, 50, 1) == (2, 3, s, 2, 3)
        assert ic.junction(t, refs, 0, 100, 1, 1, 50, 1, S=4) == ((2, 3, 0, 2, 3) if s == 0 else (0, 0, -1, 2, 3))
    # the tolerance: 16 .. 31 bases allow one difference, 32 allow two; 15 allow none
    good = B[50:82]
    bad = lambda n, k: _codes(bytes(good[:n - k]) + _comp(good[n - k:n]))
    t = {(0, 0, 100): [bad(15, 1), bad(16, 1), bad(16, 2), bad(31, 1), bad(31, 2), bad(32, 2), bad(32, 3)]}
    assert ic.junction(t, refs, 0, 100, 0, 1, 50, 1) == (3, 0, 0, 7, 0)
    # positions outside either contig are mismatches; a pile outside [0, length] has no entry; other bytes are mismatches
    t = {(0, 0, 100): [_codes(B[190:200]) + (0,) * 6], (1, 1, 190): [_codes(A[84:100][::-1])]}
    assert ic.junction(t, refs, 0, 100, 0, 1, 190, 1) == (0, 1, 0, 1, 1)
    t = {(0, 0, 100): [_codes(B[184:200])], (1, 1, 184): [_codes(A[84:100][::-1])], (1, 1, 201): [_codes(A[84:100][::-1])]}
    assert ic.junction(t, refs, 0, 100, 0, 1, 184, 1) == (1, 1, 0, 1, 1) and ic.junction(t, refs, 0, 100, 0, 1, 201, 1) == (0, 0, -1, 1, 0)
    with_n = [A, B[:60] + b"N" + B[61:]]
    t = {(0, 0, 100): [_codes(B[50:66])], (1, 1, 50): [_codes(A[84:100][::-1])]}
    assert ic.junction(t, with_n, 0, 100, 0, 1, 50, 1) == (1, 1, 0, 1, 1)              # one difference in 16 is allowed
    t = {(0, 0, 100): [_codes(B[50:65])]}
    assert ic.junction(t, refs, 0, 100, 0, 1, 50, 1)[:3] == (1, 0, 0) and ic.junction(t, with_n, 0, 100, 0, 1, 50, 1)[:3] == (0, 0, -1)
    # the smallest shift among equal sums
    t = {(0, 0, 100): [_codes(B[50:70]), _codes(B[53:73])]}
    assert ic.junction(t, refs, 0, 100, 0, 1, 50, 1) == (1, 0, 0, 2, 0)


def test_junction_on_one_contig_is_the_verify_the_crossed_and_the_inverted_rules(tmp_path):
    """on THEIR planted tables: every printed record of the three data sets, and every pair of peaks around them"""
    from indelminer_amd import rawrec, synth
    from tests.support import clipcounts as cc, cliptails as ct, crossedpiles as cp, invertedpiles as ip
    # -V: the planted deletions of the composite data set; pl > pr answers verify's, pl <= pr is the crossed rule (verify says 0, 0, -1)
    refs, rd = synth.simulate(seed=3, ref_len=200_000, coverage=30, n_contigs=2, big_every=5)
    recs = ct.parse_raw(*rawrec.records(rd))
    clens = [len(r) for r in refs]
    table = ct.table_of(recs, clens, cc.MIN_CLIP, 10)
    right, left = cc.arrays_of([r[:5] for r in recs], clens, cc.MIN_CLIP, 10)
    R = [r.tobytes() for r in refs]
    n = 0
    for tid in range(2):
        behind = np.nonzero(left[tid] >= 3)[0]
        for a in np.nonzero(right[tid] >= 3)[0][:40]:
            for b in [int(b) for b in behind if 0 < b - a < 900][:2]:
                assert ic.junction(table, R, tid, int(a), 0, tid, b, 1) == ct.answer(table, R[tid], tid, int(a), b)
                n += 1
    assert n >= 30
    # -U and -N: their planted data sets, every candidate of the first peaks
    for mod, kind in ((cp, "crossed"), (ip, "inverted")):
        d = tmp_path / kind
        d.mkdir()
        refs, rd = mod.planted_reads()
        mod.write_planted(str(d), refs, rd)
        names, right, left = cc.arrays_of_bam(str(d / "aln.bam"), cc.MIN_CLIP, 10)
        table = ct.table_of_bam(str(d / "aln.bam"), cc.MIN_CLIP, 10)[1]
        ref = refs[0].tobytes()
        printed = mod.records_of(names, {names[0]: ref}, right, left, table)[0]
        assert len(printed) >= 9
        if kind == "crossed":
            for _, pr, pl, _cr, _cl, vr, vl, s, nr, nl in printed:
                assert ic.junction(table, [ref], 0, pr, 0, 0, pl, 1) == (vr, vl, s, nr, nl)
            pr_list, pl_list = cp.peaks_many(right[0], 3, 30)[:12], cp.peaks_many(left[0], 3, 30)[:12]
            for pr, _ in pr_list:
                for pl, _ in pl_list:
                    vr, vl, s = cp.chosen(table.get((0, 0, pr), []), table.get((0, 1, pl), []), ref, pr, pl, 32)
                    assert ic.junction(table, [ref], 0, pr, 0, 0, pl, 1)[:3] == ((vr, vl, s) if vr + vl else (0, 0, -1))
        else:
            for _, side, x, y, _c1, _c2, v1, v2, s, n1, n2 in printed:
                assert ic.junction(table, [ref], 0, x, side, 0, y, side) == (v1, v2, s, n1, n2)
            for side, arr in ((0, right[0]), (1, left[0])):
                pk = cp.peaks_many(arr, 3, 30)[:10]
                for x, _ in pk:
                    for y, _ in pk:
                        if x < y:
                            v1, v2, s = ip.chosen(table.get((0, side, x), []), table.get((0, side, y), []), ref, side, x, y, 32)
                            assert ic.junction(table, [ref], 0, x, side, 0, y, side)[:3] == ((v1, v2, s) if v1 + v2 else (0, 0, -1))


def test_restatement_on_the_planted_data_set_names_exactly_the_planted_junctions(tmp_path):
    """what keeps the product test of tests/test_gpu_intercontig.py honest: the nine callable sites, every one with PE=3,3, at its
    shift, with every clipped read verified; none of the three sites that must not be called"""
    refs, rd = ic.planted_reads()
    d = ic.write_planted(str(tmp_path), refs, rd)
    text, records = ic.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    want = sorted((ta, pa, sa, tb, pb, sb, h) for ta, pa, sa, tb, pb, sb, h in ic.SITES)
    assert [(r[0], r[1], r[2], r[3], r[4], r[5], r[10]) for r in records] == want
    assert len({ic.CT[(s[2], s[5])] for s in ic.SITES[:8]}) == 4 and sorted(s[6] for s in ic.SITES[:8]) == [0] * 4 + [5] * 4
    for r in records:
        c1, c2, v1, v2, _s, st1, st2, n1, n2 = r[6:]
        assert c1 >= 3 and c2 >= 3 and (v1, v2) == (st1, st2) == (c1, c2) and (n1, n2) == (3, 3)
    lines = text.decode().split("\n")
    assert lines[-1] == "" and sum(1 for ln in lines if ln and not ln.startswith("#")) == 9
    assert "ctg0\t6700\t.\t" in text.decode() and ";CT=3to5;HOMLEN=0;" in lines[-10]
    # why the other three are not called
    from tests.support import clipcounts as cc, cliptails as ct
    names, right, left = cc.arrays_of_bam(d + "/aln.bam", cc.MIN_CLIP, 10)
    table = ct.table_of_bam(d + "/aln.bam", cc.MIN_CLIP, 10)[1]
    R = [np.asarray(r, np.uint8).tobytes() for r in refs]
    _, clens, links = ic.links_of_bam(d + "/aln.bam", 10)
    ask = lambda t, p, s, m: ic.partner(links, clens, t, s | m << 1, *ic.read_window(p, s))
    ta, pa, sa, tb, pb, sb, _ = ic.ONE_PAIR
    assert ask(ta, pa, sa, sb)[1:3] == (tb, 1) and ask(tb, pb, sb, sa)[1:3] == (ta, 1)
    v1, v2, s, _, _ = ic.junction(table, R, ta, pa, sa, tb, pb, sb)
    assert v1 >= 3 and v2 >= 3 and s == 0
    ta, pa, sa, tb, pb, sb, _ = ic.RANDOM_TAILS
    assert ask(ta, pa, sa, sb)[1:3] == (tb, 3) and ask(tb, pb, sb, sa)[1:3] == (ta, 3)
    assert ic.junction(table, R, ta, pa, sa, tb, pb, sb)[:3] == (0, 0, -1)
    ta, pa, sa, tb, pb, sb, _ = ic.OUTVOTED
    assert ask(ta, pa, sa, sb)[:3] == (5, ic.ELSEWHERE[0], 3) and ask(tb, pb, sb, sa)[0] == 0
    v1, v2, s, _, _ = ic.junction(table, R, ta, pa, sa, tb, pb, sb)
    assert v1 >= 3 and v2 >= 3                                                        # it would be called, had the vote named this contig
    # the bundle across the cell border: one mate in cell 0, two in cell 1, all three counted
    ta, pa, sa, tb, pb, sb, _ = ic.SITES[ic.CELL_SITE]
    assert ask(ta, pa, sa, sb) == (3, tb, 3, 1_023, 1_600)


def _shim():
    from tests.support.shimbuild import build_shim
    return build_shim()


def _run(args, cwd, env=None):
    return subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def _refused(r, line):
    assert r.returncode != 0 and r.stdout == b"", r
    assert r.stderr.count(b"\n") == 1 and line in r.stderr, r.stderr


def test_the_option_is_refused_where_it_does_not_apply_and_output_is_unchanged_without_it(tmp_path):
    shim = _shim()
    f = str(tmp_path / "bnd.vcf")
    _refused(_run([shim] + BASE + ["-T", f] + IN, TD), b"indelminer: -T needs -V")
    _refused(_run([shim] + BASE + ["-T", f, "-o", "detailed"] + IN, TD), b"indelminer: -T needs -V")
    _refused(_run([shim] + BASE + ["-G", "-C", "-T", f] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-V", "-T", f] + IN, TD), b"indelminer: -V needs -C")
    _refused(_run([shim] + BASE + ["-M", "-T", f] + IN, TD), b"indelminer: -M needs -U or -N")          # -M's refusals come first
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-T", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -C is not available with -c")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-T", f] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-T", f] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    assert not os.path.exists(f)                                                        # a refused run writes no FILE
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()
    h = _run([shim, "-h"], TD)
    assert h.returncode == 0 and b"\t-T, with -G -C -V: write breakpoints between two contigs to this file" in h.stdout


def test_a_library_with_every_earlier_entry_family_and_without_the_mate_link_entries(tmp_path):
    """the shim beside stubs of -C's, -V's, -I's, -U's, -N's and -M's entries: -T's own refusal, behind theirs"""
    from indelminer_amd import build
    srcs = [os.path.join(build.HOST_DIR, s) for s in build.HOST_SOURCES]
    srcs += [os.path.join(ROOT, "tests", "shim", s) for s in ("im_shim.c", "clip_entries_stub.c", "cliptail_entries_stub.c", "facing_entries_stub.c",
                                                              "crossed_entries_stub.c", "inverted_entries_stub.c", "pairlink_entries_stub.c")]
    srcs += [os.path.join(ROOT, "oracle", "im_oracle.c"), os.path.join(ROOT, "oracle", "im_oracle_triage.c")]
    binary = str(tmp_path / "indelminer_shim_pairlink")
    subprocess.check_call(["gcc", "-O0", "-std=c11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "indelminer_amd", "host"), "-o", binary] + srcs + ["-lz", "-lm"])
    f, u = str(tmp_path / "bnd.vcf"), str(tmp_path / "dup.vcf")
    for flags in (["-G", "-C", "-V", "-T", f], ["-T", f, "-V", "-C", "-G"], ["-G", "-C", "-V", "-U", u, "-M", "-T", f], ["-G", "-C", "-V", "-T", f, "-o", "detailed"]):
        _refused(_run([binary] + BASE + flags + IN, TD), b"indelminer: breakpoints between contigs (-T) needs the device library")
    _refused(_run([binary] + BASE + ["-G", "-C", "-T", f] + IN, TD), b"indelminer: -T needs -V")
    _refused(_run([binary] + BASE + ["-G", "-C", "-V", "-M", "-T", f] + IN, TD), b"indelminer: -M needs -U or -N")
    assert not os.path.exists(f) and not os.path.exists(u)
    r = _run([binary] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    capi = open(os.path.join(ROOT, "indelminer_amd", "capi.py")).read()
    csrc = open(os.path.join(ROOT, "indelminer_amd", "csrc", "im_capi.hip")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header and "L.%s.argtypes" % name in capi and "\nint %s(" % name in csrc, name
    assert "#define IM_ABI_VERSION 3" in header and "#define IM_MATELINK_CELLS 256" in header
    shim = open(os.path.join(ROOT, "tests", "shim", "im_shim.c")).read()
    assert "im_matelink" not in shim and "im_cliptail_junction" not in shim           # additive: the shim stays without the entries
    from indelminer_amd import build
    assert "im_links.hip" in build.SOURCES and "im_matelink.hip" not in build.SOURCES
