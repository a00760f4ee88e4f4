"""-E (junction pairs) where there is no GPU: the restatement the GPU tests measure against (tests/support/junctionpairs.py) pinned on the
header's worked examples and on cases worked by hand, the planted data sets counted from their BAM files, the restatement of FILE pinned
on its literal lines, and the host driver linked against tests/shim/im_shim.c -- alone and beside stubs of every earlier entry family --
which must say what -E needs."""
import os
import re
import subprocess

import pytest

from tests.support import intercontig as ic
from tests.support import junctionpairs as jp
from tests.support import pairlinks as pk
from tests.support import splitjunctions as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]
Q = 10


def _answer(recs, junction, clens=jp.HAND_CLENS, **kw):
    return jp.junction_pairs(jp.pair_links_of(recs, clens, Q), ic.links_of(recs, clens, Q), clens, junction, **kw)


@pytest.mark.parametrize("case", jp.HAND, ids=[c[0] for c in jp.HAND])
def test_rule_on_cases_worked_by_hand(case):
    name, recs, junction, want = case
    assert _answer(recs, junction) == want
    assert _answer(recs[::-1], junction) == want                                     # no answer depends on the order of arrival
    pairs, mates = jp.pair_links_of(recs, jp.HAND_CLENS, Q), ic.links_of(recs, jp.HAND_CLENS, Q)
    assert jp.answers_fast(pairs, mates, jp.HAND_CLENS, [junction]) == [want]
    if name in jp.HAND_NO_SEP:
        assert _answer(recs, junction, min_sep=0) == jp.HAND_NO_SEP[name]
    # the links of kinds 0 .. 2 are the pair links' own, with the switch and without
    assert [l for l in pairs if l[1] < 3] == pk.links_of(recs, jp.HAND_CLENS, Q) == jp.pair_links_of(recs, jp.HAND_CLENS, Q, stretched=False)


def test_hand_cases_cover_what_they_must():
    assert len(jp.HAND) >= 30
    one = [(j[2], j[5]) for _, _, j, w in jp.HAND if j[0] == j[3] and w[0] > 0]
    two = [(j[2], j[5]) for _, _, j, w in jp.HAND if j[0] != j[3] and w[0] > 0 and w[1] > 0]
    assert set(one) == set(two) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(j[0] == j[3] and j[1] > j[4] for _, _, j, _ in jp.HAND) and any(j[0] == j[3] and j[1] == j[4] for _, _, j, _ in jp.HAND)
    assert any(w[0] != w[1] and j[0] != j[3] for _, _, j, w in jp.HAND)
    links = [l for _, recs, _, _ in jp.HAND for l in jp.pair_links_of(recs, jp.HAND_CLENS, Q)]
    assert {l[1] for l in links} == {0, 1, 2, 3} and any(l[2] == l[3] for l in links)
    assert {l[2] & 255 for l in links} >= {255, 0} and any(l[2] == 0 for l in links) and any(l[3] == jp.HAND_CLENS[l[0]] for l in links)


def test_the_worked_examples_of_the_header_read_literally():
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    assert "Junction pairs (-E)" in header and "#define IM_ABI_VERSION 3" in header
    section = header[header.index("Junction pairs (-E)"):header.index("int im_pairlink_stretched_enable(im_ctx* ctx);")]
    rows = re.findall(r"^ \*   (DEL|DUP|INV 3to3|INV 5to5|TRA) +\((\d+), (\d+), (\d), (\d+), (\d+), (\d)\)", section, re.M)
    assert [r[0] for r in rows] == ["DEL", "DUP", "INV 3to3", "INV 5to5", "TRA"]
    assert "reach 1000, back 32, min_sep 50, on contigs of 100 000 bases" in section
    clens = [100_000, 100_000]
    windows = {r[0]: [jp.window(int(r[2]), int(r[3]), clens[0]), jp.window(int(r[5]), int(r[6]), clens[1])] for r in rows}
    assert windows["DEL"] == [(4_000, 5_032), (5_368, 6_400)] and windows["DUP"] == [(4_968, 6_000), (4_400, 5_432)]
    assert windows["INV 3to3"] == [(4_000, 5_032), (8_000, 9_032)] and windows["INV 5to5"] == [(4_968, 6_000), (8_968, 10_000)]
    assert windows["TRA"] == [(4_000, 5_032), (6_968, 8_000)]
    for text in ("[4000, 5032] -> reverse in [5368, 6400]", "[4968, 6000] -> forward in [4400, 5432]", "[4000, 5032] -> forward in [8000, 9032]",
                 "[4968, 6000] -> reverse in [8968, 10000]", "kind 0 | 1 << 1 = 2, forward in [4000, 5032], mate on contig 1 in [6968, 8000]",
                 "kind 1 | 0 << 1 = 1, reverse in [6968, 8000], mate on contig 0 in [4000, 5032]"):
        assert text in section, text
    kinds = {r[0]: jp.KIND[(int(r[3]), int(r[6]))] for r in rows[:4]}
    assert kinds == {"DEL": 3, "DUP": 0, "INV 3to3": 1, "INV 5to5": 2}
    for k, name in enumerate(("DUP", "INV 3to3", "INV 5to5", "DEL")):
        assert "kind K(%d,%d) = %d" % ([s for s, v in jp.KIND.items() if v == k][0] + (k,)) in section, name
    for line in ("K(1,0) = 0, K(0,0) = 1, K(1,1) = 2, K(0,1) = 3", "W(p, s) = s ? [p - back, p + reach] : [p - reach, p + back]",
                 "flag & 0x2 (proper pair) is CLEAR", "end 1 on a tie", "pe2 = 0", "kind s1 | s2 << 1", "kind s2 | s1 << 1", "min_sep does not apply"):
        assert line in section, line


@pytest.fixture(scope="module")
def deletion(tmp_path_factory):
    refs, rd = jp.planted_deletion()
    return jp.write_planted(str(tmp_path_factory.mktemp("junctionpairs")), refs, rd), rd


def test_planted_deletion_is_what_it_says(deletion):
    d, rd = deletion
    assert rd.n == 2 * (jp.DEL_N_SPLIT + len(jp.DEL_COUNTED) + len(jp.DEL_DECOYS))
    names, clens, pairs, mates = jp.links_of_bam(d + "/aln.bam", Q)
    assert names == ["ctg0", "ctg1"] and clens == jp.DEL_CLENS
    stretched = sorted((p, m) for _, k, p, m in pairs if k == jp.STRETCHED)
    # the six, and the four decoys that are links outside a window; the proper, the low-quality, the duplicate and the far one store none
    outside = [(p, m) for what, p, m in jp.DEL_DECOYS if what.startswith("one base")]
    assert stretched == sorted(jp.DEL_COUNTED + outside) and len(outside) == 4 and not [l for l in pairs if l[1] != jp.STRETCHED]
    assert sorted(mates) == [(0, 2, 7_450, 1, 1_000), (1, 1, 1_000, 0, 7_450)]
    assert jp.junction_pairs(pairs, mates, clens, jp.DEL_JUNCTION) == (jp.DEL_PE, 0)
    a, b = jp.window(jp.DEL_A, 0, clens[0]), jp.window(jp.DEL_B, 1, clens[0])
    assert {p for p, _ in jp.DEL_COUNTED} >= set(a) and {m for _, m in jp.DEL_COUNTED} >= set(b)          # starts exactly on every edge
    assert jp.pair_links_of([], clens, Q) == [] and not jp.links_of_bam(d + "/aln.bam", Q, stretched=False)[2]
    with_e, plain, kept, pes = jp.render_of_bam(d + "/aln.bam", d + "/ref.fa")
    assert [j[:6] for j in kept] == [jp.DEL_JUNCTION] and pes == [(jp.DEL_PE, 0)] and kept[0][6:] == (10, 5, 5)


def test_file_lines_stated_literally_with_and_without_the_options_in_front(deletion):
    d, _ = deletion
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    for genotype in (False, True):
        for overlap in (False, True):
            with_e, plain, kept, pes = jp.render_of_bam(bam, fa, genotype=genotype, overlap=overlap)
            a, b = plain.decode().split("\n"), with_e.decode().split("\n")
            added = [ln for ln in b if ln not in a]
            assert added[0] + "\n" == jp.PE_INFO and added[1] + "\n" == jp.JUNCTION_PAIRS and len(added) == 3
            assert with_e.count(b"##INFO=<ID=PE,Number=.,") == 1 and with_e.count(b"##junctionPairs=") == 1
            # the ##INFO line behind the present ones, the description as the last line in front of the column line
            last_info = max(i for i, ln in enumerate(a) if ln.startswith("##INFO"))
            assert b[b.index(added[0]) - 1] == a[last_info] and b[b.index(added[1]) + 1].startswith("#CHROM\t")
            assert [ln for ln in b if ln not in added] == [ln for ln in a if ln and ln[0] == "#"] + [""]
            x, y = a[-2].split("\t"), b[-2].split("\t")
            assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + ";PE=6" and len(y) == (10 if genotype else 8)
            if overlap:
                assert x[7].endswith(";HOMLEN=0;INSLEN=0;OA=10,10")
            over = jp.render_of_bam(bam, fa, genotype=genotype, overlap=overlap, pair_over=True)[0].decode().split("\n")
            assert over[-2].split("\t")[7] == x[7] + ";PE=." and over[:-2] == b[:-2]
            assert jp.render_of_bam(bam, fa, genotype=genotype, overlap=overlap, mate_over=True)[0] == with_e      # the other table's overflow
    rec = jp.render_of_bam(bam, fa)[0].decode().split("\n")[-2]
    ref = rec.split("\t")[3]
    assert rec == "ctg0\t8000\t.\t%s\t%s[ctg0:8400[\t.\t.\tSVTYPE=BND;CHR2=ctg0;POS2=8400;CT=3to5;JT=DEL;SVLEN=400;SE=10;SR=5,5;PE=6" % (ref, ref)
    one, two = (0, 5, 0, 0, 9, 1), (0, 5, 0, 1, 9, 1)
    assert [jp.info_of(one, (3, 0)), jp.info_of(one, (jp.NONE, jp.NONE)), jp.info_of(two, (3, 0)), jp.info_of(two, (jp.NONE, jp.NONE))] == [
        ";PE=3", ";PE=.", ";PE=3,0", ";PE=.,."]


def test_file_on_hand_made_junctions():
    names, refs = ["a", "b"], [b"ACGT" * 50, b"TTGCA" * 40]
    found = [(0, 10, 0, 0, 150, 1, 4, 2, 2), (0, 20, 1, 1, 30, 0, 3, 3, 0), (0, 0, 1, 1, 9, 0, 3, 3, 0), (1, 40, 1, 1, 120, 1, 5, 5, 0)]
    plain = sj.render(names, refs, found)
    kept = [j for j in found if j[1] and j[4]]
    text = jp.with_pairs(plain, kept, [(7, 0), (2, 1), (jp.NONE, jp.NONE)]).decode().split("\n")
    assert len(kept) == 3 and [ln.split("\t")[7].rsplit(";", 1)[1] for ln in text[-4:-1]] == ["PE=7", "PE=2,1", "PE=."]
    assert text[-4].startswith("a\t10\t.\t") and ";SE=4;SR=2,2;PE=7" in text[-4] and "JT=TRA" in text[-3] and "JT=INV" in text[-2]
    with pytest.raises(AssertionError):
        jp.with_pairs(plain, kept, [(7, 0)])


def test_planted_sets_hold_pairs_at_their_junctions(tmp_path):
    """the pairs that -M's and -T's tests plant are there beside the tags that -J's tests plant: most junctions have pairs"""
    for kind, least in (("DUP", 3), ("BND", 3)):
        mod, refs, rd = jp.planted(kind)
        os.makedirs(str(tmp_path / kind))
        d = mod.write_planted(str(tmp_path / kind), refs, rd)
        with_e, plain, kept, pes = jp.render_of_bam(d + "/aln.bam", d + "/ref.fa")
        assert len(kept) >= 7 and sum(1 for pe in pes if pe[0] >= least) >= 4, (kind, pes)
        if kind == "BND":
            assert all(j[0] != j[3] for j in kept) and any(pe[1] >= least for pe in pes)
        assert with_e.count(b";PE=") == len(kept)


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
    _refused(_run([shim] + BASE + ["-E"] + IN, TD), b"indelminer: -E needs -J")
    _refused(_run([shim] + BASE + ["-G", "-E"] + IN, TD), b"indelminer: -E needs -J")
    _refused(_run([shim] + BASE + ["-E", "-o", "detailed"] + IN, TD), b"indelminer: -E needs -J")
    _refused(_run([shim] + BASE + ["-E", "-J", f] + IN, TD), b"indelminer: -J needs -G")                            # through -J, through -G
    _refused(_run([shim] + BASE + ["-G", "-E", "-J", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -J is not available with -c")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-E"] + IN, TD), b"indelminer: split-link junctions (-J) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-J", f, "-K", "-H", "-E"] + IN, TD), b"indelminer: split-link junctions (-J) needs the device library")
    assert not os.path.exists(f)
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()
    h = _run([shim, "-h"], TD)
    assert h.returncode == 0 and b"\t-E, with -J: add PE to its records, the read pairs on either side of the junction" in h.stdout
    assert h.stdout.index(b"\t-K, with") < h.stdout.index(b"\t-H, with") < h.stdout.index(b"\t-E, with") < h.stdout.index(b"Assumptions:")


def test_a_library_with_every_earlier_entry_and_without_these_two_is_refused(tmp_path):
    """the shim beside stubs of the pair links', the mate links', the split links', the junctions', -K's and -H's entries: -E's own refusal"""
    from indelminer_amd import build
    srcs = [os.path.join(build.HOST_DIR, s) for s in build.HOST_SOURCES]
    srcs += [os.path.join(ROOT, "tests", "shim", s) for s in ("im_shim.c", "pairlink_entries_stub.c", "matelink_entries_stub.c", "splitjunc_entries_stub.c")]
    srcs += [os.path.join(ROOT, "oracle", "im_oracle.c"), os.path.join(ROOT, "oracle", "im_oracle_triage.c")]
    binary = str(tmp_path / "indelminer_shim_splitjunc")
    subprocess.check_call(["gcc", "-O0", "-std=c11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "indelminer_amd", "host"), "-o", binary] + srcs + ["-lz", "-lm"])
    f = str(tmp_path / "junc.vcf")
    for flags in (["-G", "-J", f, "-E"], ["-E", "-J", f, "-G"], ["-G", "-J", f, "-H", "-E"], ["-G", "-J", f, "-E", "-o", "detailed"]):
        _refused(_run([binary] + BASE + flags + IN, TD), b"indelminer: junction pairs (-E) needs the device library")
    _refused(_run([binary] + BASE + ["-G", "-E"] + IN, TD), b"indelminer: -E needs -J")
    # without -E the same library gets as far as -G's refusal: the stubs stand for every family in front
    _refused(_run([binary] + BASE + ["-G", "-J", f, "-H"] + IN, TD), b"indelminer: genotyping (-G) needs the device library")
    # -K stands on -G's span array, which the shim lacks: its refusal comes in front of -E's
    _refused(_run([binary] + BASE + ["-G", "-J", f, "-K", "-E"] + IN, TD), b"indelminer: junction genotypes (-K) needs the device library")
    assert not os.path.exists(f)
    r = _run([binary] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_entry_points_are_declared_bound_exported_and_weak():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    header, capi, csrc = read("include", "indelminer_amd.h"), read("indelminer_amd", "capi.py"), read("indelminer_amd", "csrc", "im_capi.hip")
    kern, host, setup = read("indelminer_amd", "csrc", "im_links.hip"), read("indelminer_amd", "host", "imhost.c"), read("indelminer_amd", "host", "host_setup.c")
    assert "int im_pairlink_stretched_enable(im_ctx* ctx);" in header
    assert "int im_junction_pairs(im_ctx* ctx, int32_t n, const int32_t* tid1, const int32_t* pos1, const uint8_t* side1, const int32_t* tid2, const int32_t* pos2,\n" in header
    assert "const uint8_t* side2, int32_t reach, int32_t back, int32_t min_sep, uint32_t* pe1, uint32_t* pe2);" in header
    for name in ("im_pairlink_stretched_enable", "im_junction_pairs"):
        assert "L.%s.argtypes" % name in capi and "def %s(" % name[3:] in capi and "\nint %s(" % name in csrc, name
        assert re.search(r"extern int %s\(im_ctx\*[^;]*\) __attribute__\(\(weak\)\);" % name, host), name
    assert "void junction_pairs_kernel(" in kern and "void pairlink_scatter_stretched_kernel(LinkScatterArgs A)" in kern
    assert "void pairlink_scatter_kernel(LinkScatterArgs A)" in kern                        # the form without the fourth kind keeps its name and arguments
    assert "#define PAIRTABLE_ON (PAIRLINK_ON || JUNCPAIR_ON)" in host and "#define MATETABLE_ON (MATELINK_ON || JUNCPAIR_ON)" in host
    assert "JUNCPAIR_API_PRESENT" in host and "LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, LINK_EV_MIN_SEP, pe, pe + m)" in setup
    shim = read("tests", "shim", "im_shim.c")
    assert "im_junction_pairs" not in shim and "im_pairlink_stretched_enable" not in shim   # additive: the shim stays without the entries
