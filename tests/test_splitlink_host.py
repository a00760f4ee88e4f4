"""-S (split links) where there is no GPU: the restatement the GPU tests measure against (tests/support/splitlinks.py) pinned on cases
worked by hand and on the planted data sets of -U, -N and -T with the tags a split aligner would have written; and the host driver
linked against tests/shim/im_shim.c, which must say what -S needs."""
import os
import subprocess

import pytest

from tests.support import splitlinks as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")
ENTRY_POINTS = ["im_splitlink_enable", "im_dev_splitlink_scatter", "im_splitlink_add", "im_splitlink_count", "im_splitlink_reset", "im_splitlink_stats"]
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]


@pytest.mark.parametrize("qual", [True, False])
def test_record_rule_on_cases_worked_by_hand(qual):
    assert len(sl.CASES) >= 100 and sum(1 for _, _, want in sl.CASES if want is not None) >= 35
    for name, kw, want in sl.CASES:
        assert sl.link_of(sl.make_record(qual=qual, **kw), sl.NAMES, sl.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ) == want, name
    kinds = {(x[2], x[5]) for _, _, x in sl.CASES if x is not None}
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # min_clip and min_mapq are the call's
    rec = sl.make_record(cigar="95M5S", mapq=3, aux=sl.sa("ctg10,501,+,95S5M,3,0;"))
    assert sl.link_of(rec, sl.NAMES, sl.CLENS, 5, 3) == (1, 1_095, 0, 2, 500, 1)
    assert sl.link_of(rec, sl.NAMES, sl.CLENS, 6, 3) is None and sl.link_of(rec, sl.NAMES, sl.CLENS, 5, 4) is None


def test_count_on_cases_worked_by_hand():
    clens = [10_000, 5_000]
    links = [(0, 1_000, 0, 1, 500, 1), (0, 1_032, 0, 1, 468, 1), (0, 1_033, 0, 1, 500, 1), (0, 1_000, 0, 1, 533, 1), (0, 1_000, 1, 1, 500, 1),
             (0, 1_000, 0, 1, 500, 0), (0, 1_000, 0, 0, 500, 1), (1, 1_000, 0, 1, 500, 1), (0, 0, 0, 1, 5_000, 1), (0, 10_000, 0, 1, 0, 1)]
    q = lambda *a: sl.count(links, clens, a)
    assert q(0, 0, 968, 1_032, 1, 1, 468, 532) == 2                      # inclusive at all four edges; 1 033 and 533 are outside
    assert q(0, 0, 968, 1_033, 1, 1, 468, 533) == 4
    assert q(0, 0, 1_001, 1_031, 1, 1, 0, 5_000) == 0
    assert q(0, 1, 968, 1_032, 1, 1, 468, 532) == 1 and q(0, 0, 968, 1_032, 1, 0, 468, 532) == 1 and q(0, 1, 968, 1_032, 1, 0, 468, 532) == 0      # the kind
    assert q(0, 0, 968, 1_032, 0, 1, 468, 532) == 1                      # tid1 == tid2: the tidB filter
    assert q(1, 0, 968, 1_032, 1, 1, 468, 532) == 1
    assert q(0, 0, -50, 10, 1, 1, 4_990, 5_100) == 1 and q(0, 0, 9_990, 10_050, 1, 1, -40, 0) == 1                                               # clipped at 0 and at the length
    assert q(0, 0, 10_001, 10_050, 1, 1, 0, 5_000) == 0 and q(0, 0, -50, -1, 1, 1, 0, 5_000) == 0 and q(0, 0, 0, 10_000, 1, 1, 5_001, 5_100) == 0  # empty after the clip
    assert q(0, 0, 5, 4, 1, 1, 0, 5_000) == 0
    assert sl.home_slot(0, 0, 0, 6) == ((1 << 63) * sl.HASH_MUL % 2**64) >> 58 and sl.home_slot(3, 7, 2, 12) == ((((1 << 63) | 3 << 26 | 7 << 2 | 2) * sl.HASH_MUL) % 2**64) >> 52


def test_tags_of_a_planted_read_name_the_other_end():
    """the four junction kinds, with and without homology: what sa_value writes, read back by the rule"""
    names, clens = ["ctg0", "ctg1"], [60_000, 40_000]
    for s, so in ((0, 1), (1, 0), (0, 0), (1, 1)):
        for h in (0, 5):
            for reverse in (False, True):
                k = 37
                value, pb = sl.sa_value(100, s, k, reverse, "ctg1", 6_200, so, h)
                rec = sl.make_record(tid=0, pos=6_700 - (k if s == 0 else 0), flag=0x10 if reverse else 0, cigar="%dM%dS" % (k, 100 - k) if s == 0 else "%dS%dM" % (k, 100 - k), aux=sl.sa(value))
                assert sl.link_of(rec, names, clens, 20, 10) == (0, 6_700, s, 1, pb, so), (s, so, h, reverse, value)
                assert pb == (6_200 + h if so == 1 else 6_200 - h)


@pytest.mark.parametrize("kind", ["DUP", "INV", "BND"])
def test_planted_data_sets_give_every_pile_its_split_reads_minus_the_decoys(kind, tmp_path):
    """what keeps the product test of tests/test_gpu_splitlink.py honest: on every record SR is the clipped reads planted at its two piles
    minus the decoys that must not count, and no record has SR=0,0"""
    from tests.support import pairlinks as pk
    mod, refs, rd, names, tally = sl.planted(kind)
    d = mod.write_planted(str(tmp_path), refs, rd)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    plain = (pk.render_of_bam(kind, bam, fa, 10)[1] if kind != "BND" else mod.render_of_bam(bam, fa, 10)[0])
    _, clens, links = sl.links_of_bam(bam, 20, 10)
    text, found = sl.with_sr(plain, kind, names, clens, links)
    assert len(found) >= 9 and text.count(b";SR=") == len(found) and text.count(b"##INFO=<ID=SR,") == 1 and text.count(b"##splitLinks=") == 1
    assert sum(t[1] for t in tally.values()) == 6                        # the eight decoys, two of which count
    seen = 0
    for first, second, n1, n2 in found:
        for a, b, n in ((first, second, n1), (second, first, n2)):
            if (a, b) in tally:
                planted, decoys = tally[(a, b)]
                assert planted >= 3 and n == planted - decoys, (a, b, n, planted, decoys)
                seen += 1
    assert seen >= 2 * 9
    lines = text.decode().split("\n")
    chrom = next(i for i, ln in enumerate(lines) if ln.startswith("#CHROM"))
    assert lines[chrom - 1].startswith("##splitLinks=") and all(ln.split(";")[-1].startswith("SR=") for ln in lines[chrom + 1:-1])
    assert sl.with_sr(plain, kind, names, clens, links, overflowed=True)[0].count(b";SR=.\n") == len(found)


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
    f = str(tmp_path / "dup.vcf")
    _refused(_run([shim] + BASE + ["-S"] + IN, TD), b"indelminer: -S needs -U, -N or -T")
    _refused(_run([shim] + BASE + ["-S", "-o", "detailed"] + IN, TD), b"indelminer: -S needs -U, -N or -T")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-S"] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    _refused(_run([shim] + BASE + ["-S", "-U", f] + IN, TD), b"indelminer: -U needs -V")                   # every other refusal comes first
    _refused(_run([shim] + BASE + ["-S", "-N", f] + IN, TD), b"indelminer: -N needs -V")
    _refused(_run([shim] + BASE + ["-S", "-T", f] + IN, TD), b"indelminer: -T needs -V")
    _refused(_run([shim] + BASE + ["-S", "-M"] + IN, TD), b"indelminer: -M needs -U or -N")
    _refused(_run([shim] + BASE + ["-G", "-V", "-S", "-U", f] + IN, TD), b"indelminer: -V needs -C")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-S", "-U", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -C is not available with -c")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-S", "-U", f] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-S", "-U", f] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    assert not os.path.exists(f)
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()
    h = _run([shim, "-h"], TD)
    assert h.returncode == 0 and b"\t-S, with -U, -N or -T: add SR= to their records, the split reads" in h.stdout
    assert h.stdout.index(b"\t-T, with") < h.stdout.index(b"\t-S, with")


def test_a_library_with_every_earlier_entry_family_and_without_the_split_link_entries(tmp_path):
    """the shim beside stubs of -C's, -V's, -I's, -U's, -N's, -M's and -T's entries: -S's own refusal, behind theirs"""
    from indelminer_amd import build
    srcs = [os.path.join(build.HOST_DIR, s) for s in build.HOST_SOURCES]
    srcs += [os.path.join(ROOT, "tests", "shim", s) for s in ("im_shim.c", "clip_entries_stub.c", "cliptail_entries_stub.c", "facing_entries_stub.c",
                                                              "crossed_entries_stub.c", "inverted_entries_stub.c", "pairlink_entries_stub.c",
                                                              "matelink_entries_stub.c")]
    srcs += [os.path.join(ROOT, "oracle", "im_oracle.c"), os.path.join(ROOT, "oracle", "im_oracle_triage.c")]
    binary = str(tmp_path / "indelminer_shim_matelink")
    subprocess.check_call(["gcc", "-O0", "-std=c11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "indelminer_amd", "host"), "-o", binary] + srcs + ["-lz", "-lm"])
    u, n, t = (str(tmp_path / x) for x in ("dup.vcf", "inv.vcf", "bnd.vcf"))
    own = b"indelminer: split links (-S) needs the device library"
    for flags in (["-G", "-C", "-V", "-U", u, "-S"], ["-S", "-N", n, "-V", "-C", "-G"], ["-G", "-C", "-V", "-T", t, "-S"],
                  ["-G", "-C", "-V", "-U", u, "-N", n, "-M", "-T", t, "-S"], ["-G", "-C", "-V", "-U", u, "-S", "-o", "detailed"]):
        _refused(_run([binary] + BASE + flags + IN, TD), own)
    _refused(_run([binary] + BASE + ["-G", "-C", "-V", "-S"] + IN, TD), b"indelminer: -S needs -U, -N or -T")
    _refused(_run([binary] + BASE + ["-G", "-C", "-V", "-M", "-T", t, "-S"] + IN, TD), b"indelminer: -M needs -U or -N")
    _refused(_run([binary] + BASE + ["-G", "-C", "-S", "-T", t] + IN, TD), b"indelminer: -T needs -V")
    assert not any(os.path.exists(x) for x in (u, n, t))
    r = _run([binary] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    capi = open(os.path.join(ROOT, "indelminer_amd", "capi.py")).read()
    csrc = open(os.path.join(ROOT, "indelminer_amd", "csrc", "im_capi.hip")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header and "L.%s.argtypes" % name in capi and "\nint %s(" % name in csrc, name
        assert "def %s(" % name.replace("im_dev_", "").replace("im_", "") in capi, name
    assert "#define IM_ABI_VERSION 3" in header and "Split links" in header
    shim = open(os.path.join(ROOT, "tests", "shim", "im_shim.c")).read()
    assert "im_splitlink" not in shim and "im_dev_splitlink" not in shim                 # additive: the shim stays without the entries
    from indelminer_amd import build
    assert build.SOURCES == ["im_realign.hip", "im_realign_long.hip", "im_realign_any.hip", "im_results.hip", "im_depth.hip", "im_span.hip", "im_cliptail.hip",
                             "im_links.hip", "im_support.hip", "im_triage.hip", "im_flush.hip", "im_flushwide.hip", "im_capi.hip", "im_comm.hip"]
