"""-J (split junctions) where there is no GPU: the restatement the GPU tests measure against (tests/support/splitjunctions.py) pinned on
cases worked by hand, the restatement of FILE pinned on a planted data set, and the host driver linked against tests/shim/im_shim.c,
which must say what -J needs."""
import os
import subprocess

import pytest

from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]


@pytest.mark.parametrize("case", sj.HAND, ids=[c[0] for c in sj.HAND])
def test_rule_on_cases_worked_by_hand(case):
    name, links, kw, want = case
    assert sj.junctions(links, sj.HAND_CLENS, **kw) == want
    assert sj.junctions(links[::-1], sj.HAND_CLENS, **kw) == want          # no answer depends on the order of arrival
    assert sj.junctions_fast(links, sj.HAND_CLENS, **kw) == want


def test_the_worked_example_of_the_header():
    links = ([(0, 1_000, 0, 0, 5_000, 1)] * 3 + [(0, 5_000, 1, 0, 1_000, 0)] * 2 + [(0, 1_020, 0, 0, 5_010, 1)] * 2 + [(0, 1_040, 0, 0, 5_030, 1)] +
             [(0, 1_010, 0, 0, 1_030, 1)])
    assert sj.junctions(links, [10_000]) == [(0, 1_000, 0, 0, 5_000, 1, 5, 5, 2)]
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    assert "Split junctions" in header and "(0, 1000, 0, 0, 5000, 1), E = 5, n1 = 5, n2 = 2" in header


def test_n1_and_n2_are_the_count_query_of_the_split_links():
    rng_links = [(0, 1_000 + 7 * (i % 9), i & 1, 1, 500 + 5 * (i % 7), (i >> 1) & 1) for i in range(120)]
    rng_links += [sj.rev(l) for l in rng_links[::3]]
    found = sj.junctions(rng_links, sj.HAND_CLENS)
    assert len(found) >= 4
    for t1, p1, s1, t2, p2, s2, e, n1, n2 in found:
        assert n1 == sl.count(rng_links, sj.HAND_CLENS, (t1, s1, p1 - 32, p1 + 32, t2, s2, p2 - 32, p2 + 32))
        assert n2 == sl.count(rng_links, sj.HAND_CLENS, (t2, s2, p2 - 32, p2 + 32, t1, s1, p1 - 32, p1 + 32))
        assert e == rng_links.count((t1, p1, s1, t2, p2, s2)) + rng_links.count((t2, p2, s2, t1, p1, s1)) and n1 + n2 >= e
    assert sj.junctions_fast(rng_links, sj.HAND_CLENS) == found


def test_file_on_cases_worked_by_hand():
    names, refs = ["a", "b"], [b"ACGT" * 30, b"TTGCA" * 30]
    found = [(0, 10, 0, 0, 80, 1, 3, 3, 0), (0, 11, 1, 0, 90, 0, 4, 1, 3), (0, 12, 0, 0, 95, 0, 3, 3, 0), (0, 13, 1, 1, 70, 1, 5, 2, 3), (0, 14, 0, 1, 7, 1, 3, 3, 0),
             (0, 0, 1, 1, 9, 0, 3, 3, 0), (0, 15, 0, 1, 0, 1, 3, 3, 0)]
    text = sj.render(names, refs, found).decode()
    assert text.startswith(sj.HEADER) and text.count("##INFO=<ID=") == 8 and text.count("##splitJunctions=") == 1
    body = text[len(sj.HEADER):].split("\n")
    assert body == [
        "a\t10\t.\tC\tC[a:80[\t.\t.\tSVTYPE=BND;CHR2=a;POS2=80;CT=3to5;JT=DEL;SVLEN=70;SE=3;SR=3,0",
        "a\t11\t.\tG\t]a:90]G\t.\t.\tSVTYPE=BND;CHR2=a;POS2=90;CT=5to3;JT=DUP;SVLEN=79;SE=4;SR=1,3",
        "a\t12\t.\tT\tT]a:95]\t.\t.\tSVTYPE=BND;CHR2=a;POS2=95;CT=3to3;JT=INV;SVLEN=83;SE=3;SR=3,0",
        "a\t13\t.\tA\t[b:70[A\t.\t.\tSVTYPE=BND;CHR2=b;POS2=70;CT=5to5;JT=TRA;SE=5;SR=2,3",
        "a\t14\t.\tC\tC[b:7[\t.\t.\tSVTYPE=BND;CHR2=b;POS2=7;CT=3to5;JT=TRA;SE=3;SR=3,0",
        ""]                                                                 # POS 0 and POS2 0 are skipped
    assert sj.render(names, refs, None) == sj.HEADER.encode()              # after an overflow: the header alone


def test_file_on_the_planted_insertion_names_the_junction_no_pile_search_reports(tmp_path):
    """the reads of the site carry RANDOM clipped bases: -T's restatement has no record there, -J's has one, with every planted read"""
    ic, refs, rd, names, site = sj.planted_insertion()
    d = ic.write_planted(str(tmp_path), refs, rd)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    text, found = sj.render_of_bam(bam, fa, 10)
    bnd = ic.render_of_bam(bam, fa, 10)[0]
    ta, pa, sa, tb, pb, sb = site
    assert len(found) == 1 and found[0][:6] == site and found[0][6] >= 6 and found[0][7] >= 3 and found[0][8] >= 3
    assert text.count(b"\n") == sj.HEADER.count("\n") + 1
    assert b"\n%s\t%d\t" % (names[ta].encode(), pa) in text and b"\n%s\t%d\t" % (names[ta].encode(), pa) not in bnd
    assert b";CT=3to5;JT=TRA;SE=%d;SR=%d,%d\n" % found[0][6:] in text
    assert sj.render_of_bam(bam, fa, 10, overflowed=True)[0] == sj.HEADER.encode()


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
    _refused(_run([shim] + BASE + ["-J", f] + IN, TD), b"indelminer: -J needs -G")
    _refused(_run([shim] + BASE + ["-J", f, "-o", "detailed"] + IN, TD), b"indelminer: -J needs -G")
    _refused(_run([shim] + BASE + ["-C", "-V", "-S", "-J", f] + IN, TD), b"indelminer: -C needs -G")               # every other refusal comes first
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -J is not available with -c")
    _refused(_run([shim] + BASE + ["-G", "-J", f] + IN, TD), b"indelminer: split-link junctions (-J) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-o", "detailed"] + IN, TD), b"indelminer: split-link junctions (-J) needs the device library")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-J", f] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-J", f, IN[0], "indels.vcf", IN[1]], TD), b"-G is not available with a VCF argument")
    assert not os.path.exists(f)
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()
    h = _run([shim, "-h"], TD)
    assert h.returncode == 0 and b"\t-J, with -G: write the junctions the split reads name by themselves to this file" in h.stdout
    assert h.stdout.index(b"\t-S, with") < h.stdout.index(b"\t-J, with")


def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    capi = open(os.path.join(ROOT, "indelminer_amd", "capi.py")).read()
    csrc = open(os.path.join(ROOT, "indelminer_amd", "csrc", "im_capi.hip")).read()
    host = open(os.path.join(ROOT, "indelminer_amd", "host", "imhost.c")).read()
    assert "int im_splitlink_junctions(" in header and "L.im_splitlink_junctions.argtypes" in capi and "\nint im_splitlink_junctions(" in csrc
    assert "def splitlink_junctions(" in capi
    assert "#define IM_ABI_VERSION 3" in header
    shim = open(os.path.join(ROOT, "tests", "shim", "im_shim.c")).read()
    assert "im_splitlink" not in shim                                      # additive: the shim stays without the entry
    assert "SPLITJUNC_API_PRESENT" in host and "#define SPLITTABLE_ON (SPLITLINK_ON || SPLITJUNC_ON)" in host
