"""-H (junction overlap) where there is no GPU: the restatement the GPU tests measure against (tests/support/splitoverlap.py) pinned on
the header's worked examples, on cases worked by hand and on a data set with planted truth, the restatement of FILE pinned on its
literal lines, and the host driver linked against tests/shim/im_shim.c, which must say what -H needs."""
import os
import re
import subprocess

import pytest

from tests.support import junctiongt as jg
from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl
from tests.support import splitoverlap as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]


def _d(cigar, entry, flag=0):
    rec = sl.make_record(cigar=cigar, flag=flag, aux=sl.sa(entry))
    got = so.overlap_of(rec, so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)
    assert got is not None and got[0] == sl.link_of(rec, so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)
    return got[1]


def test_the_worked_examples_of_the_header_read_literally():
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    assert "Junction overlap (-H)" in header and "#define IM_ABI_VERSION 3" in header
    section = header[header.index("Junction overlap (-H)"):header.index("int im_splitlink_overlap_enable(im_ctx* ctx);")]
    rows = re.findall(r"^ \*   (\S+)   ctgB,p,([+-]),(\S+),60,0;   d = (-?\d+)$", section, re.M)
    assert rows == [("60M40S", "+", "60S40M", "0"), ("65M35S", "+", "60S40M", "5"), ("55M45S", "+", "65S35M", "-10"), ("40S60M", "+", "40M60S", "0"),
                    ("60M40S", "-", "40M60S", "0")]
    for cigar, strand, entry, d in rows:
        assert _d(cigar, "ctg10,501,%s,%s,60,0;" % (strand, entry)) == int(d), (cigar, entry)
    # the rule's own lines
    for line in ("BEHIND:    d = (Q1 - T1) - L2", "FRONT:     d = (Q1 - T2) - L1", "Q1 != Q2:  d is unknown", "d outside -32767 .. 32767:  d is unknown",
                 "0 = unknown, otherwise d + 32768"):
        assert line in section, line


@pytest.mark.parametrize("case", so.HAND, ids=[c[0] for c in so.HAND])
def test_rule_on_cases_worked_by_hand(case):
    name, kw, want = case
    for qual in (True, False):
        rec = sl.make_record(qual=qual, **kw)
        link = sl.link_of(rec, so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)
        assert link is not None, name
        assert so.overlap_of(rec, so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ) == (link, want), name


def test_hand_cases_cover_what_they_must():
    links = [sl.link_of(sl.make_record(**kw), so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ) for _, kw, _ in so.HAND]
    signs = {}
    for (name, kw, d), l in zip(so.HAND[:12], links):
        signs.setdefault((l[2], l[2] != l[5]), set()).add((d > 0) - (d < 0))     # (behind or front, same strand or other) -> signs of d
    assert signs == {(s, same): {-1, 0, 1} for s in (0, 1) for same in (False, True)}
    ds = [d for _, _, d in so.HAND]
    assert so.D_MAX in ds and -so.D_MAX in ds and ds.count(None) == 5
    assert all(sl.link_of(sl.make_record(**kw), so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)[2] == 0 for n, kw, _ in so.HAND if n.startswith("d = "))
    text = " ".join(kw["cigar"] + " " + kw["aux"].decode("latin1") for _, kw, _ in so.HAND)
    assert all(op in text for op in "MIDNSHP=X")
    # no record without a link has an overlap
    assert so.overlap_of(sl.make_record(cigar="100M"), so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ) is None
    assert all(so.overlap_of(sl.make_record(**kw), sl.NAMES, sl.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ) is None for _, kw, want in sl.CASES if want is None)
    # and every link of the split links' own hand cases has one, known or not
    assert all(so.overlap_of(sl.make_record(**kw), sl.NAMES, sl.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)[0] == want for _, kw, want in sl.CASES if want is not None)


@pytest.mark.parametrize("ds, want", [
    ([], (0, 0, 0)), ([None, None], (0, 0, 0)), ([4], (1, 4, 1)), ([-3, None], (1, -3, 1)),
    ([9, 2], (2, 2, 1)),                                    # the lower median
    ([5, -1, 5], (3, 5, 2)), ([0, 7, -7], (3, 0, 1)),
    ([3, 3, 8, 8], (4, 3, 2)),                              # an even count with two modes: the lower one
    ([8, 3, 8, 3, None, 12], (5, 8, 2)),
    ([-32767, 32767, 32767, -32767], (4, -32767, 2)),
])
def test_summary_on_small_multisets(ds, want):
    assert so.summary(ds) == want
    assert so.summary(ds[::-1]) == want


def test_junction_summary_pools_both_directions_and_takes_a_link_once():
    clens = [10_000, 5_000]
    a = (0, 1_000, 0, 1, 500, 1)
    pairs = [(a, 4), (a, 4), (sj.rev(a), 6), ((0, 1_032, 0, 1, 532, 1), None), ((0, 1_033, 0, 1, 500, 1), 9), ((0, 1_000, 1, 1, 500, 1), 9), ((0, 1_000, 0, 0, 500, 1), 9)]
    assert so.junction_ds(pairs, clens, a + (3, 3, 1)) == [4, 4, 6, None]
    assert so.junction_summary(pairs, clens, a + (3, 3, 1)) == (3, 4, 2)
    assert so.summaries_fast(pairs, clens, [a + (3, 3, 1)]) == [(3, 4, 2)]
    # both ends on one contig and side, windows that overlap: a link that both count queries count is one link
    b = (0, 2_000, 0, 0, 2_050, 0)
    inside = (0, 2_030, 0, 0, 2_030, 0)
    assert sl.count([inside], clens, (0, 0, 1_968, 2_032, 0, 0, 2_018, 2_082)) == 1 and sl.count([inside], clens, (0, 0, 2_018, 2_082, 0, 0, 1_968, 2_032)) == 1
    pairs = [(b, 1), (sj.rev(b), 2), (inside, 3)]
    assert so.junction_summary(pairs, clens, b + (2, 2, 2)) == (3, 2, 1)
    assert so.summaries_fast(pairs, clens, [b + (2, 2, 2)]) == [(3, 2, 1)]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    refs, rd = so.planted_truth()
    d = so.write_planted(str(tmp_path_factory.mktemp("splitoverlap")), refs, rd)
    return d, rd


def test_planted_truth_is_what_it_says(planted):
    """the reads the data set promises, counted from the BAM file"""
    d, rd = planted
    assert rd.n < 400
    names, clens, pairs = so.overlaps_of_bam(d + "/aln.bam")
    assert names == ["ctg0"] and clens == [so.CONTIG] and len(pairs) == 4 * so.N_SPLIT + 3
    _, found, sums = so.render_of_bam(d + "/aln.bam", d + "/ref.fa")
    assert [j[:6] for j in found] == [(0, a, 0, 0, b, 1) for _, a, b, _ in so.PLANTED]
    assert sums == so.PLANTED_SUMMARY == [(10, 0, 10), (12, 7, 10), (10, 40, 10), (10, -12, 10)]
    for (what, a, b, d_), j in zip(so.PLANTED, found):
        ds = so.junction_ds(pairs, clens, j)
        assert ds.count(d_) == so.N_SPLIT and len(ds) == j[7] + j[8], what
        from_a = [x for (l, x) in pairs if l[:3] == (0, a, 0)]
        from_b = [x for (l, x) in pairs if l[2] == 1 and abs(l[1] - b) <= 2]
        assert from_a.count(d_) == from_b.count(d_) == so.N_SPLIT // 2, what         # reads from both ends
    assert [x for l, x in pairs].count(None) == 1 and [x for l, x in pairs].count(5) == 2
    # 40 bases of homology are more than the 32 a pile search compares
    assert so.PLANTED[2][3] > sl.WINDOW


def test_planted_file_lines_stated_literally(planted):
    d, _ = planted
    text, found, _ = so.render_of_bam(d + "/aln.bam", d + "/ref.fa")
    records = [ln for ln in text.decode().split("\n") if ln and not ln.startswith("#")]
    assert [ln.split("\t")[7].split(";", 6)[6] for ln in records] == so.PLANTED_INFO
    ref = records[2].split("\t")[3]
    assert records[2] == "ctg0\t11000\t.\t%s\t%s[ctg0:12000[\t.\t.\tSVTYPE=BND;CHR2=ctg0;POS2=12000;CT=3to5;JT=DEL;SVLEN=1000;SE=10;SR=5,5;HOMLEN=40;INSLEN=0;OA=10,10" % (ref, ref)
    assert records[3].endswith(";SE=10;SR=5,5;HOMLEN=0;INSLEN=12;OA=10,10")
    both = so.render_of_bam(d + "/aln.bam", d + "/ref.fa", genotype=True)[0].decode()
    rec_k = [ln for ln in both.split("\n") if ln and not ln.startswith("#")]
    assert [ln.split("\t")[:8] for ln in rec_k] == [ln.split("\t") for ln in records]
    assert all(ln.split("\t")[8] == "GT:AD:GQ:RB" and len(ln.split("\t")) == 10 for ln in rec_k)
    assert so.info_of((0, 0, 0)) == ";HOMLEN=.;INSLEN=.;OA=0,0" and so.info_of((3, -4, 2)) == ";HOMLEN=0;INSLEN=4;OA=2,3"


def test_file_with_the_option_is_the_file_without_it_and_what_it_adds(planted):
    d, _ = planted
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    for genotype, without in ((False, sj.render_of_bam(bam, fa, 10)[0].decode()), (True, jg.render_of_bam(bam, fa)[0].decode())):
        with_h = so.render_of_bam(bam, fa, genotype=genotype)[0].decode()
        a, b = without.split("\n"), with_h.split("\n")
        added = [ln for ln in b if ln not in a]
        assert [ln.split(",")[0] for ln in added[:4]] == ["##INFO=<ID=HOMLEN", "##INFO=<ID=INSLEN", "##INFO=<ID=OA", "##junctionOverlap=\"every split read states its own overlap d in its two CIGARs: with L1"]
        assert len(added) == 4 + 4 and with_h.count("##INFO=<ID=") == 8 + 3 and with_h.count("##junctionOverlap=") == 1
        # the three lines stand behind the present ##INFO lines, the description as the last line in front of the column line
        assert b[b.index(added[0]) - 1].startswith("##INFO=<ID=SR,") and b[b.index(added[3]) + 1].startswith("#CHROM\t")
        assert [ln for ln in b if ln not in added[:4] and not (ln and ln[0] != "#")] == [ln for ln in a if not (ln and ln[0] != "#")]
        rec_a, rec_b = [ln.split("\t") for ln in a if ln and ln[0] != "#"], [ln.split("\t") for ln in b if ln and ln[0] != "#"]
        assert len(rec_a) == len(rec_b) == 4
        for x, y, info in zip(rec_a, rec_b, so.PLANTED_INFO):
            assert y[:7] == x[:7] and y[8:] == x[8:] and y[7].startswith(x[7] + ";HOMLEN=") and y[7].endswith(info)
            assert [kv.split("=")[0] for kv in y[7][len(x[7]) + 1:].split(";")] == ["HOMLEN", "INSLEN", "OA"]
        over = so.render_of_bam(bam, fa, genotype=genotype, overflowed=True)[0].decode()
        assert over == with_h[:with_h.index("#CHROM")] + with_h[with_h.index("#CHROM"):].split("\n")[0] + "\n"


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
    f = str(tmp_path / "junc.vcf")
    _refused(_run([shim] + BASE + ["-H"] + IN, TD), b"indelminer: -H needs -J")
    _refused(_run([shim] + BASE + ["-G", "-H"] + IN, TD), b"indelminer: -H needs -J")
    _refused(_run([shim] + BASE + ["-H", "-o", "detailed"] + IN, TD), b"indelminer: -H needs -J")
    _refused(_run([shim] + BASE + ["-H", "-J", f] + IN, TD), b"indelminer: -J needs -G")                            # through -J, through -G
    _refused(_run([shim] + BASE + ["-G", "-H", "-J", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -J is not available with -c")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-H"] + IN, TD), b"indelminer: split-link junctions (-J) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-K", "-H"] + IN, TD), b"indelminer: split-link junctions (-J) needs the device library")
    assert not os.path.exists(f)
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()
    h = _run([shim, "-h"], TD)
    assert h.returncode == 0 and b"\t-H, with -J: add HOMLEN, INSLEN and OA to its records" in h.stdout
    assert h.stdout.index(b"\t-J, with") < h.stdout.index(b"\t-K, with") < h.stdout.index(b"\t-H, with") < h.stdout.index(b"Assumptions:")


def test_entry_points_are_declared_bound_exported_and_weak():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    header, capi, csrc = read("include", "indelminer_amd.h"), read("indelminer_amd", "capi.py"), read("indelminer_amd", "csrc", "im_capi.hip")
    kern, keyed, host = read("indelminer_amd", "csrc", "im_links.hip"), read("indelminer_amd", "csrc", "im_keyed.hpp"), read("indelminer_amd", "host", "imhost.c")
    assert "int im_splitlink_overlap_enable(im_ctx* ctx);" in header
    assert "int im_splitlink_add_overlap(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2, const int32_t* pos2,\n" in header
    assert "int im_splitlink_overlap(im_ctx* ctx, int32_t n, const int32_t* tid1, const int32_t* pos1, const uint8_t* side1, const int32_t* tid2, const int32_t* pos2,\n" in header
    assert "const uint8_t* side2, int32_t window, uint32_t* known, int32_t* median, uint32_t* agree);" in header
    for name in ("im_splitlink_overlap_enable", "im_splitlink_add_overlap", "im_splitlink_overlap"):
        assert "L.%s.argtypes" % name in capi and "def %s(" % name[3:] in capi and "\nint %s(" % name in csrc, name
        assert re.search(r"extern int %s\(im_ctx\*[^;]*\) __attribute__\(\(weak\)\);" % name, host), name
    assert "void splitlink_overlap_kernel(" in kern and "void splitlink_scatter_overlap_kernel(" in kern and "void splitlink_add_overlap_kernel(" in kern
    assert "void splitlink_scatter_kernel(SplitScatterArgs A)" in kern                     # the form without the array keeps its name and arguments
    assert "keyed_place_at(" in keyed and "__device__ __forceinline__ void keyed_place(" in keyed
    assert "#define SPLITOVERLAP_API_PRESENT (SPLITJUNC_API_PRESENT && im_splitlink_overlap_enable && im_splitlink_add_overlap && im_splitlink_overlap)" in host
    shim = read("tests", "shim", "im_shim.c")
    assert "im_splitlink_overlap" not in shim and "im_splitlink_add_overlap" not in shim        # additive: the shim stays without the entries
