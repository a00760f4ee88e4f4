"""-U (tandem duplications from crossed clip piles) where there is no GPU: the host driver linked against tests/shim/im_shim.c, which
implements the C ABI without the clip, clip-tail, facing and crossed entry points.  The driver must still link, behave as before without
-U, and say what -U needs.  The restatement the GPU tests measure against (tests/support/crossedpiles.py) is pinned here on cases worked
by hand and on the planted data set of tests/test_gpu_crossed.py."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")

CROSSED_ENTRY_POINTS = ["im_clip_peaks_tid", "im_clip_peaks", "im_clip_crossed_tid", "im_clip_crossed"]
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]
KNOWN = ["reference.fa", "known.vcf", "sample=alignments.bam"]


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
    f, g = str(tmp_path / "dup.vcf"), str(tmp_path / "ins.vcf")
    _refused(_run([shim] + BASE + ["-G", "-C", "-U", f] + ["-q", "10"] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-U", f] + IN, TD), b"indelminer: -U needs -V")
    _refused(_run([shim] + BASE + ["-U", f] + IN, TD), b"indelminer: -U needs -V")
    # -I's refusal comes first when both lack -V
    _refused(_run([shim] + BASE + ["-U", f, "-I", g] + IN, TD), b"indelminer: -I needs -V")
    # every other refusal reaches it through -G, -C and -V, and theirs come first
    _refused(_run([shim] + BASE + ["-G", "-V", "-U", f] + IN, TD), b"indelminer: -V needs -C")
    _refused(_run([shim] + BASE + ["-C", "-V", "-U", f] + IN, TD), b"indelminer: -C needs -G")
    _refused(_run([shim] + BASE + ["-C", "-V", "-U", f] + KNOWN, TD), b"indelminer: -C is not available with a VCF argument (annotate mode)")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-U", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -C is not available with -c")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-U", f] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-D", "-C", "-V", "-U", f] + IN, TD), b"indelminer: depth evidence (-D) needs the device library")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-U", f] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-U", f] + KNOWN, TD), b"-G is not available with a VCF argument")
    assert not os.path.exists(f) and not os.path.exists(g)          # a refused run writes no FILE
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_a_library_with_the_clip_clip_tail_and_facing_entries_and_without_the_crossed_entries(tmp_path):
    """the shim beside stubs of -C's six, -V's six and -I's three entries: -U's own refusal, behind theirs"""
    from indelminer_amd import build
    srcs = [os.path.join(build.HOST_DIR, s) for s in build.HOST_SOURCES]
    srcs += [os.path.join(ROOT, "tests", "shim", s) for s in ("im_shim.c", "clip_entries_stub.c", "cliptail_entries_stub.c", "facing_entries_stub.c")]
    srcs += [os.path.join(ROOT, "oracle", "im_oracle.c"), os.path.join(ROOT, "oracle", "im_oracle_triage.c")]
    binary = str(tmp_path / "indelminer_shim_facing")
    subprocess.check_call(["gcc", "-O0", "-std=c11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "indelminer_amd", "host"), "-o", binary] + srcs + ["-lz", "-lm"])
    f, g = str(tmp_path / "dup.vcf"), str(tmp_path / "ins.vcf")
    for flags in (["-G", "-C", "-V", "-U", f], ["-U", f, "-V", "-C", "-G"], ["-G", "-C", "-V", "-I", g, "-U", f]):
        _refused(_run([binary] + BASE + flags + IN, TD), b"indelminer: tandem-duplication evidence (-U) needs the device library")
    _refused(_run([binary] + BASE + ["-G", "-C", "-U", f] + IN, TD), b"indelminer: -U needs -V")
    assert not os.path.exists(f) and not os.path.exists(g)
    r = _run([binary] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_help_names_the_option():
    h = _run([_shim(), "-h"], TD)
    assert h.returncode == 0 and re.search(rb"^\t-U, with -G -C -V", h.stdout, re.M) and re.search(rb"^\t-I, with -G -C -V", h.stdout, re.M)


def test_crossed_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    from indelminer_amd import build, capi
    import ctypes as C
    L = C.CDLL(build.build())
    src = open(capi.__file__).read()
    for s in CROSSED_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % s, text), s
        assert hasattr(L, s), s
        assert "L.%s.argtypes" % s in src, s
    for s in ("clip_peaks_tid", "clip_peaks", "clip_crossed_tid", "clip_crossed"):
        assert callable(getattr(capi.Context, s)), s
    # the definition is stated in seam 5, behind what it reads
    assert text.index("The consensus of a pile (-I)") < text.index("Crossed piles, the breakpoints of tandem duplications (-U)") < text.index("multi-GPU: one collective")
    for words in ("A[p] > A[x] for every x in [p - T, p)", "A[p] >= A[x] for every", "at least T + 1 apart", "dmin <= pr - pl <= dmax",
                  "ref[pl + s + i]", "ref[pr - 1 - s - i]", "without its pl > pr condition", "the smallest s among equals",
                  "vR >= mv and vL >= mv", "sorted by (pr, pl)", "*n_found = -1", "no\n * answer, not a wrong one", "T = reach (0 .. 64)"):
        assert words in text, words
    # additive: the ABI version and the mirrored structs keep their layout; the shim stays without the entries
    assert "#define IM_ABI_VERSION 3" in text
    assert C.sizeof(capi.TriageParams) == 24 and C.sizeof(capi.DevRecords) == 32
    shim = open(os.path.join(ROOT, "tests", "shim", "im_shim.c")).read()
    assert "im_clip_peaks" not in shim and "im_clip_crossed" not in shim


def test_crossed_restatement_on_cases_worked_by_hand():
    """the yardstick of the GPU tests (tests/support/crossedpiles.py), pinned here where no GPU is needed"""
    from tests.support import crossedpiles as cp
    from tests.support.clipcounts import LEFT, RIGHT

    def array(clen, piles):
        A = np.zeros(clen + 1, np.int64)
        for p, v in piles:
            A[p] = v
        return A

    same = lambda A, m, T: cp.peaks(A, m, T) if cp.peaks(A, m, T) == cp.peaks_many(A, m, T) else "the two forms differ"
    # ---- peaks
    assert same(array(100, [(50, 3)]), 3, 30) == [(50, 3)] and same(array(100, [(50, 2)]), 3, 30) == []
    # equal peaks at distance T: the left one; at T + 1: both
    assert same(array(200, [(50, 4), (80, 4)]), 3, 30) == [(50, 4)] and same(array(200, [(50, 4), (81, 4)]), 3, 30) == [(50, 4), (81, 4)]
    # a higher count T to the right or to the left hides the pile, one at T + 1 does not
    assert same(array(200, [(50, 4), (80, 5)]), 3, 30) == [(80, 5)] and same(array(200, [(50, 4), (81, 5)]), 3, 30) == [(50, 4), (81, 5)]
    assert same(array(200, [(50, 5), (80, 4)]), 3, 30) == [(50, 5)] and same(array(200, [(49, 5), (80, 4)]), 3, 30) == [(49, 5), (80, 4)]
    # a count below m still hides nothing, and a count below m that is higher cannot exist; a lower one beside the peak is ignored
    assert same(array(100, [(50, 3), (51, 2), (49, 2)]), 3, 30) == [(50, 3)]
    # T = 0: every position on its own; the contig's ends; a contig shorter than the reach
    assert same(array(100, [(50, 1), (51, 2), (52, 1)]), 1, 0) == [(50, 1), (51, 2), (52, 1)]
    assert same(array(100, [(0, 3), (100, 4)]), 3, 30) == [(0, 3), (100, 4)]
    assert same(array(40, [(0, 3), (40, 3)]), 3, 64) == [(0, 3)] and same(array(40, [(0, 3), (40, 4)]), 3, 64) == [(40, 4)]
    assert same(np.zeros(11, np.int64), 1, 30) == []

    # ---- crossed pairs on a reference written by hand
    rng = np.random.default_rng(5)
    ref = bytearray(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 2_000)))
    code = lambda lo, n, step=1: tuple(b"ACGT".index(ref[lo + step * i]) for i in range(n))

    def both(R, L, table, *par):
        a, b = cp.crossed(R, L, table, bytes(ref), 0, *par, many=False), cp.crossed(R, L, table, bytes(ref), 0, *par, many=True)
        assert a == b, (a, b)
        return a[0]

    def pair(pr, pl, nr=3, nl=3, shift=0):
        """the arrays and the table of one duplication of [pl, pr): nr right entries of ref[pl + shift ..], nl left ones of ref[.. pr - 1 - shift]"""
        return array(2_000, [(pr, nr)]), array(2_000, [(pl, nl)]), {(0, RIGHT, pr): [code(pl + shift, 30)] * nr, (0, LEFT, pl): [code(pr - 1 - shift, 30, -1)] * nl}

    par = (3, 30, 50, 400, 32, 2)
    # the distance window's four edges
    for d, n in ((49, 0), (50, 1), (400, 1), (401, 0)):
        R, L, table = pair(1_000, 1_000 - d)
        got = both(R, L, table, *par)
        assert got == ([(1_000, 1_000 - d, 3, 3, 3, 3, 0, 3, 3)] if n else []), (d, got)
    # homology: the aligner extended the reads from the left by 5 (their tails start 5 behind pl), at shift 5 both sides verify; the
    # reads from the right extended instead move pl, and the left entries verify 5 further in front
    R, L, table = pair(1_000, 800, shift=5)
    assert both(R, L, table, *par) == [(1_000, 800, 3, 3, 3, 3, 5, 3, 3)]
    R, L, table = pair(1_000, 800)
    table[(0, RIGHT, 1_000)] = [code(805, 30)] * 3
    assert both(R, L, table, *par) == []                            # shift 0: vL = 3, vR = 0; shift 5: vR = 3, vL = 0; neither has both
    table[(0, LEFT, 800)] = [code(999, 30, -1)] * 3 + [code(994, 30, -1)] * 2; L[800] = 5
    assert both(R, L, table, *par) == [(1_000, 800, 3, 5, 3, 2, 5, 3, 5)]       # the sum is 3 at shift 0 and 5 at shift 5
    # equal sums: the smaller shift
    table = {(0, RIGHT, 1_000): [code(800, 30)] * 2 + [code(807, 30)] * 2, (0, LEFT, 800): [code(999, 30, -1)] * 2 + [code(992, 30, -1)] * 2}
    assert both(array(2_000, [(1_000, 4)]), array(2_000, [(800, 4)]), table, *par) == [(1_000, 800, 4, 4, 2, 2, 0, 4, 4)]
    # min_verified on one side only; the tolerance of 1 in 16
    R, L, table = pair(1_000, 800, nl=3)
    table[(0, LEFT, 800)] = [code(999, 30, -1)] + [code(300, 30, -1)] * 2
    assert both(R, L, table, *par) == [] and both(R, L, table, 3, 30, 50, 400, 32, 1) == [(1_000, 800, 3, 3, 3, 1, 0, 3, 3)]
    flip = lambda t, where: tuple((b + 1) % 4 if i in where else b for i, b in enumerate(t))
    R, L, table = pair(1_000, 800)
    table[(0, RIGHT, 1_000)] = [flip(code(800, 30), (3,)), flip(code(800, 30), (3, 9)), code(800, 30)]
    assert both(R, L, table, *par) == [(1_000, 800, 3, 3, 2, 3, 0, 3, 3)]
    # a peak with two qualifying partners: the duplicated stretch starts with a repeat, ref[700 ..] = ref[800 ..]
    ref[700:740] = ref[800:840]
    R, L, table = pair(1_000, 800)
    L[700] = 4
    table[(0, LEFT, 700)] = [code(999, 30, -1)] * 4
    assert both(R, L, table, *par) == [(1_000, 700, 3, 4, 3, 4, 0, 3, 4), (1_000, 800, 3, 3, 3, 3, 0, 3, 3)]
    # ... and a left peak with two right partners comes back sorted by (pr, pl)
    R[1_100] = 3
    table[(0, RIGHT, 1_100)] = [code(800, 30)] * 3
    ref[1_060:1_100] = ref[960:1_000]
    got = both(R, L, table, *par)
    assert [g[:2] for g in got] == [(1_000, 700), (1_000, 800), (1_100, 700), (1_100, 800)]
    # windows that reach past either end of the contig are mismatches there, an N is one too
    short = bytes(ref[:1_010])
    R, L, table = array(1_010, [(1_000, 3)]), array(1_010, [(800, 3)]), {(0, RIGHT, 1_000): [code(800, 30)] * 3, (0, LEFT, 800): [code(999, 30, -1)] * 3}
    assert cp.crossed(R, L, table, short, 0, *par)[0] == cp.crossed(R, L, table, short, 0, *par, many=False)[0] == [(1_000, 800, 3, 3, 3, 3, 0, 3, 3)]
    R2, L2 = array(1_010, [(1_000, 3)]), array(1_010, [(10, 3)])
    t2 = {(0, RIGHT, 1_000): [code(10, 30)] * 3, (0, LEFT, 10): [code(999, 30, -1)] * 3}
    assert cp.crossed(R2, L2, t2, short, 0, 3, 30, 50, 2_000, 32, 2)[0] == [(1_000, 10, 3, 3, 3, 3, 0, 3, 3)]
    withn = bytearray(short); withn[805] = ord("N"); withn[806] = ord("N")
    assert cp.crossed(R, L, table, bytes(withn), 0, *par)[0] == cp.crossed(R, L, table, bytes(withn), 0, *par, many=False)[0] == []
    # the rendering: POS, REF, INFO; POS 0 is skipped
    fasta = {"c": short}
    text = cp.render(["c"], fasta, [R], [L], table).decode()
    assert text == cp.header(False) + "c\t800\t.\t%s\t<DUP:TANDEM>\t.\t.\tSVTYPE=DUP;END=1000;SVLEN=200;HOMLEN=0;CR=3,3;CN=3,3;CV=3,3\n" % chr(short[799])
    depth = np.full(1_010, 30, np.int64); depth[800:1_000] = 45
    assert cp.render(["c"], fasta, [R], [L], table, [depth]).decode().endswith("CV=3,3;DM=45,30,30;DFC=1500\n")
    assert cp.header(True).count("##INFO") == cp.header(False).count("##INFO") + 2


def test_crossed_restatement_on_the_planted_data_set(tmp_path):
    """what tests/test_gpu_crossed.py relies on: with the driver's constants, -q 10 and clips of 20 bases the restatement finds 19 + 19
    peaks and 182 candidates on the planted data set, of which 9 qualify -- all 9 at planted sites, at shift 0 and with every clipped
    read verified; no chance pair does.  The driver's CPU stand-in runs on it to exit status 0."""
    from tests.support import crossedpiles as cp
    refs, rd = cp.planted_reads()
    d = cp.write_planted(str(tmp_path), refs, rd)
    text, recs, n_cand, n_peaks = cp.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    assert len(cp.SITES) >= 8 and min(n for _, n in cp.SITES) == 50 and max(n for _, n in cp.SITES) > 4_900
    assert n_peaks == (19, 19) and n_cand == 182
    assert [(r[2], r[1] - r[2]) for r in recs] == cp.SITES                                          # every site, and nothing else
    assert all(r[7] == 0 and r[3] >= 3 and r[4] >= 3 and (r[5], r[6]) == (r[8], r[9]) == (r[3], r[4]) for r in recs), recs
    lines = text.decode().split("\n")
    for pl, n in cp.SITES:
        assert sum(1 for ln in lines if ln.startswith("ctg0\t%d\t" % pl) and "END=%d;SVLEN=%d;HOMLEN=0;" % (pl + n, n) in ln) == 1, (pl, n)
    assert text.startswith(cp.header(False).encode()) and text.count(b"\n") == cp.header(False).count("\n") + len(cp.SITES)
    r = _run([_shim(), "-i", "cfg.txt", "-s", "100", "ref.fa", "sample=aln.bam"], d)
    assert r.returncode == 0 and len(r.stdout) > 1000
