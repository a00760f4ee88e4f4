"""-K (junction genotypes) where there is no GPU: the restatement the GPU tests measure against (tests/support/junctiongt.py) pinned on
cases worked by hand and on a data set with planted truth, the restatement of FILE pinned on its literal lines, and the host driver
linked against tests/shim/im_shim.c, which must say what -K needs."""
import os
import subprocess

import pytest

from tests.support import junctiongt as jg
from tests.support import splitjunctions as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]


@pytest.mark.parametrize("case", jg.HAND, ids=[c[0] for c in jg.HAND])
def test_rule_on_cases_worked_by_hand(case):
    name, junction, at, want = case
    assert jg.call(junction, jg.hand_spans(junction, at)) == want


def test_hand_cases_cover_what_they_must():
    kinds = {sj.jt_of(j[0], j[2], j[3], j[5]) for _, j, _, _ in jg.HAND}
    assert kinds == {"DEL", "DUP", "INV", "TRA"}
    assert {w[0] for _, _, _, w in jg.HAND} == {"0/0", "0/1", "1/1"} and any(w[3] == 99 for _, _, _, w in jg.HAND)
    dup = [(min(at), j[7] + j[8]) for _, j, at, _ in jg.HAND if sj.jt_of(j[0], j[2], j[3], j[5]) == "DUP"]
    assert any(a < b for a, b in dup) and any(a == b for a, b in dup) and any(a > b for a, b in dup)


def test_the_worked_example_of_the_header():
    del_, dup = (0, 1_000, 0, 0, 1_500, 1, 10, 5, 5), (0, 3_000, 1, 0, 3_400, 0, 20, 10, 10)
    import numpy as np
    spans = [np.zeros(5_001, np.int64)]
    spans[0][[1_000, 1_500, 3_000, 3_400]] = (10, 12, 20, 20)
    assert jg.call(del_, spans) == ("0/1", 10, 10, 99, 10, 12)
    assert jg.call(dup, spans) == ("1/1", 0, 20, 59, 20, 20)
    assert jg.call(dup, spans, dup_correction=False) == ("0/1", 20, 20, 99, 20, 20)
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    assert "Junction genotypes (-K)" in header and "L = (400000, 60200, 880): GT 1/1, GQ 59" in header and "L = (200440, 60200, 200440): GT 0/1, GQ 99" in header


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    refs, rd = jg.planted_truth()
    d = jg.write_planted(str(tmp_path_factory.mktemp("junction_gt")), refs, rd)
    return d, rd


def test_planted_truth_is_what_it_says(planted):
    """the reads the data set promises, counted from the BAM file: reference reads through each end, split reads from either part"""
    d, rd = planted
    assert 300 <= rd.n <= 400
    names, clens, spans = jg.spans_of_bam(d + "/aln.bam")
    assert names == ["ctg0"] and clens == [jg.CONTIG]
    _, found, _ = jg.render_of_bam(d + "/aln.bam", d + "/ref.fa")
    assert len(found) == len(jg.PLANTED)
    for (what, a, b, n_ref, n_split), j in zip(jg.PLANTED, found):
        assert j[:6] == (0, min(a, b), 0 if a < b else 1, 0, max(a, b), 1 if a < b else 0), what
        assert sj.jt_of(j[0], j[2], j[3], j[5]) == what.split()[1]
        assert (spans[0][a], spans[0][b]) == (n_ref, n_ref) and j[6] == n_split and j[7] == j[8] == n_split // 2, what


def test_planted_genotypes_stated_literally(planted):
    d, _ = planted
    text, found, calls = jg.render_of_bam(d + "/aln.bam", d + "/ref.fa")
    assert [c[0] for c in calls] == jg.PLANTED_GT == ["0/1", "1/1", "0/1", "1/1"]
    records = [ln for ln in text.decode().split("\n") if ln and not ln.startswith("#")]
    assert [ln.split("\t")[8:] for ln in records] == [["GT:AD:GQ:RB", c] for c in jg.PLANTED_COLUMN]
    assert records[3] == "ctg0\t15000\t.\t%s\t]ctg0:16000]%s\t.\t.\tSVTYPE=BND;CHR2=ctg0;POS2=16000;CT=5to3;JT=DUP;SVLEN=1000;SE=20;SR=10,10\tGT:AD:GQ:RB\t1/1:0,20:59:20,20" % (
        (records[3].split("\t")[3],) * 2)


def test_without_the_correction_the_homozygous_duplication_is_called_heterozygous(planted):
    """the tooth of the DUP correction: 20 reads run through either outer boundary of a duplication that is on both copies"""
    d, _ = planted
    spans = jg.spans_of_bam(d + "/aln.bam")[2]
    _, found, _ = jg.render_of_bam(d + "/aln.bam", d + "/ref.fa")
    off = jg.calls(found, spans, dup_correction=False)
    assert [c[0] for c in off] == jg.PLANTED_WITHOUT_THE_CORRECTION == ["0/1", "1/1", "0/1", "0/1"]
    assert off[3] == ("0/1", 20, 20, 99, 20, 20) and off[:2] == jg.calls(found, spans)[:2]


def test_file_with_the_option_is_the_file_without_it_and_what_it_adds(planted):
    d, _ = planted
    with_k = jg.render_of_bam(d + "/aln.bam", d + "/ref.fa")[0].decode()
    without = sj.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)[0].decode()
    assert with_k.startswith(jg.header()) and with_k.count("##FORMAT=<ID=") == 4 and with_k.count("##junctionGenotype=") == 1 and with_k.count("##INFO=<ID=") == 8
    assert "no genotype;" in without and "no genotype;" not in with_k
    assert [ln.split(",")[0] for ln in with_k.split("\n") if ln.startswith("##FORMAT")] == ["##FORMAT=<ID=" + k for k in ("GT", "AD", "GQ", "RB")]
    assert "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n" in with_k
    strip = lambda text: [ln.split("\t")[:8] for ln in text.split("\n") if ln and not ln.startswith("#")]
    assert strip(with_k) == strip(without) and len(strip(without)) == 4
    assert jg.render_of_bam(d + "/aln.bam", d + "/ref.fa", overflowed=True)[0].decode() == jg.header()
    assert jg.render_of_bam(d + "/aln.bam", d + "/ref.fa", sample="tumour")[0].decode().count("\tFORMAT\ttumour\n") == 1


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
    _refused(_run([shim] + BASE + ["-K"] + IN, TD), b"indelminer: -K needs -J")
    _refused(_run([shim] + BASE + ["-G", "-K"] + IN, TD), b"indelminer: -K needs -J")
    _refused(_run([shim] + BASE + ["-K", "-o", "detailed"] + IN, TD), b"indelminer: -K needs -J")
    _refused(_run([shim] + BASE + ["-K", "-J", f] + IN, TD), b"indelminer: -J needs -G")                            # through -J, through -G
    _refused(_run([shim] + BASE + ["-G", "-K", "-J", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -J is not available with -c")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-K"] + IN, TD), b"indelminer: split-link junctions (-J) needs the device library")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-K"] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-K", IN[0], "indels.vcf", IN[1]], TD), b"-G is not available with a VCF argument")
    assert not os.path.exists(f)
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()
    h = _run([shim, "-h"], TD)
    assert h.returncode == 0 and b"\t-K, with -J: genotype its junctions (FORMAT GT:AD:GQ:RB)" in h.stdout
    assert h.stdout.index(b"\t-J, with") < h.stdout.index(b"\t-K, with")


def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    capi = open(os.path.join(ROOT, "indelminer_amd", "capi.py")).read()
    csrc = open(os.path.join(ROOT, "indelminer_amd", "csrc", "im_capi.hip")).read()
    kern = open(os.path.join(ROOT, "indelminer_amd", "csrc", "im_span.hip")).read()
    host = open(os.path.join(ROOT, "indelminer_amd", "host", "imhost.c")).read()
    assert "int im_span_query_ends(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, int32_t slack, uint32_t* min_out);" in header
    assert "L.im_span_query_ends.argtypes" in capi and "def span_query_ends(" in capi and "\nint im_span_query_ends(" in csrc
    assert "void span_ends_kernel(" in kern and "launch_span_query_ends" in kern
    assert "#define IM_ABI_VERSION 3" in header
    shim = open(os.path.join(ROOT, "tests", "shim", "im_shim.c")).read()
    assert "im_span_query_ends" not in shim                                # additive: the shim stays without the entry
    assert "#define SPANENDS_API_PRESENT (SPAN_API_PRESENT && im_span_query_ends)" in host and "__attribute__((weak))" in host
