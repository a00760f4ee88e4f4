"""-N (inversion breakpoints from same-side clip piles) where there is no GPU: the host driver linked against tests/shim/im_shim.c, which
implements the C ABI without the clip, clip-tail, facing, crossed and inverted entry points.  The driver must still link, behave as
before without -N, and say what -N needs.  The restatement the GPU tests measure against (tests/support/invertedpiles.py) is pinned here
on cases worked by hand and on the planted data set of tests/test_gpu_inverted.py."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")

INVERTED_ENTRY_POINTS = ["im_clip_inverted_tid", "im_clip_inverted"]
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
    f, g, u = str(tmp_path / "inv.vcf"), str(tmp_path / "ins.vcf"), str(tmp_path / "dup.vcf")
    _refused(_run([shim] + BASE + ["-G", "-C", "-N", f] + ["-q", "10"] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-N", f] + IN, TD), b"indelminer: -N needs -V")
    _refused(_run([shim] + BASE + ["-N", f] + IN, TD), b"indelminer: -N needs -V")
    # -I's and -U's refusals come first when all lack -V
    _refused(_run([shim] + BASE + ["-N", f, "-I", g] + IN, TD), b"indelminer: -I needs -V")
    _refused(_run([shim] + BASE + ["-N", f, "-U", u] + IN, TD), b"indelminer: -U needs -V")
    _refused(_run([shim] + BASE + ["-N", f, "-U", u, "-I", g] + IN, TD), b"indelminer: -I needs -V")
    # every other refusal reaches it through -G, -C and -V, and theirs come first
    _refused(_run([shim] + BASE + ["-G", "-V", "-N", f] + IN, TD), b"indelminer: -V needs -C")
    _refused(_run([shim] + BASE + ["-C", "-V", "-N", f] + IN, TD), b"indelminer: -C needs -G")
    _refused(_run([shim] + BASE + ["-C", "-V", "-N", f] + KNOWN, TD), b"indelminer: -C is not available with a VCF argument (annotate mode)")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-N", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -C is not available with -c")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-N", f] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-D", "-C", "-V", "-N", f] + IN, TD), b"indelminer: depth evidence (-D) needs the device library")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-N", f] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-N", f] + KNOWN, TD), b"-G is not available with a VCF argument")
    assert not os.path.exists(f) and not os.path.exists(g) and not os.path.exists(u)        # a refused run writes no FILE
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_a_library_with_the_clip_clip_tail_facing_and_crossed_entries_and_without_the_inverted_entries(tmp_path):
    """the shim beside stubs of -C's six, -V's six, -I's three and -U's four entries: -N's own refusal, behind theirs"""
    from indelminer_amd import build
    srcs = [os.path.join(build.HOST_DIR, s) for s in build.HOST_SOURCES]
    srcs += [os.path.join(ROOT, "tests", "shim", s) for s in ("im_shim.c", "clip_entries_stub.c", "cliptail_entries_stub.c", "facing_entries_stub.c",
                                                              "crossed_entries_stub.c")]
    srcs += [os.path.join(ROOT, "oracle", "im_oracle.c"), os.path.join(ROOT, "oracle", "im_oracle_triage.c")]
    binary = str(tmp_path / "indelminer_shim_crossed")
    subprocess.check_call(["gcc", "-O0", "-std=c11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "indelminer_amd", "host"), "-o", binary] + srcs + ["-lz", "-lm"])
    f, g, u = str(tmp_path / "inv.vcf"), str(tmp_path / "ins.vcf"), str(tmp_path / "dup.vcf")
    for flags in (["-G", "-C", "-V", "-N", f], ["-N", f, "-V", "-C", "-G"], ["-G", "-C", "-V", "-I", g, "-U", u, "-N", f]):
        _refused(_run([binary] + BASE + flags + IN, TD), b"indelminer: inversion evidence (-N) needs the device library")
    _refused(_run([binary] + BASE + ["-G", "-C", "-N", f] + IN, TD), b"indelminer: -N needs -V")
    assert not os.path.exists(f) and not os.path.exists(g) and not os.path.exists(u)
    r = _run([binary] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_help_names_the_option():
    h = _run([_shim(), "-h"], TD)
    assert h.returncode == 0 and re.search(rb"^\t-N, with -G -C -V", h.stdout, re.M) and re.search(rb"^\t-U, with -G -C -V", h.stdout, re.M)


def test_inverted_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    from indelminer_amd import build, capi
    import ctypes as C
    L = C.CDLL(build.build())
    src = open(capi.__file__).read()
    for s in INVERTED_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % s, text), s
        assert hasattr(L, s), s
        assert "L.%s.argtypes" % s in src, s
    for s in ("clip_inverted_tid", "clip_inverted"):
        assert callable(getattr(capi.Context, s)), s
    capi.lib()
    assert len(capi.lib().im_clip_inverted_tid.argtypes) == len(capi.lib().im_clip_inverted.argtypes) == 20 and len(capi.Context._INVERTED) == 10
    # the definition is stated in seam 5, behind the crossed piles and in front of the multi-GPU part
    assert (text.index("Crossed piles, the breakpoints of tandem duplications (-U)") < text.index("Inverted piles, the breakpoints of inversions (-N)")
            < text.index("multi-GPU: one collective"))
    for words in ("two peaks x < y of the SAME array with dmin <= y - x <= dmax", "comp(ref[y - 1 - s - i])", "comp(ref[x - 1 - s - i])",
                  "comp(ref[y + s + i])", "comp(ref[x + s + i])", "the complement is both planes inverted", "s = h1 + h2", "the smallest s among equals",
                  "v1 >= mv and v2 >= mv", "sorted by (x, y, side)", "PEAK is the definition of \"Crossed piles\", unchanged", "at most n >> 4",
                  "T = reach (0 .. 64)"):
        assert words in text, words
    assert text.count("*n_found = -1") >= 2
    # additive: the ABI version and the mirrored structs keep their layout; the shim stays without the entries
    assert "#define IM_ABI_VERSION 3" in text
    assert C.sizeof(capi.TriageParams) == 24 and C.sizeof(capi.DevRecords) == 32
    shim = open(os.path.join(ROOT, "tests", "shim", "im_shim.c")).read()
    assert "im_clip_inverted" not in shim and "im_clip_crossed" not in shim


def test_inverted_restatement_on_cases_worked_by_hand():
    """the yardstick of the GPU tests (tests/support/invertedpiles.py), pinned here where no GPU is needed"""
    from tests.support import invertedpiles as ip
    from tests.support.clipcounts import LEFT, RIGHT

    def array(clen, piles):
        A = np.zeros(clen + 1, np.int64)
        for p, v in piles:
            A[p] += v
        return A

    rng = np.random.default_rng(6)
    ref = bytearray(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 2_000)))
    code = lambda lo, n, step=1: tuple(b"ACGT".index(ref[lo + step * i]) for i in range(n))
    comp = lambda lo, n, step=1: tuple(3 - c for c in code(lo, n, step))

    def both(R, L, table, *par, r=None):
        r = bytes(ref) if r is None else r
        a, b = ip.inverted(R, L, table, r, 0, *par, many=False), ip.inverted(R, L, table, r, 0, *par, many=True)
        assert a == b, (a, b)
        return a[0]

    def junction(side, a, b, n1=3, n2=3, h1=0, h2=0, n=30):
        """the arrays and the table of one junction of an inversion of [a, b) whose aligner extended the reads by h1 bases at a's pile
        and by h2 at b's: right clips move behind, left clips in front"""
        A = [array(2_000, []), array(2_000, [])]
        if side == RIGHT:
            x, y = a + h1, b + h2
            table = {(0, RIGHT, x): [comp(b - 1 - h1, n, -1)] * n1, (0, RIGHT, y): [comp(a - 1 - h2, n, -1)] * n2}
        else:
            x, y = a - h1, b - h2
            table = {(0, LEFT, x): [comp(b + h1, n)] * n1, (0, LEFT, y): [comp(a + h2, n)] * n2}
        A[side][x] += n1; A[side][y] += n2
        return A[0], A[1], table

    par = (3, 30, 50, 400, 32, 2)
    for side in (RIGHT, LEFT):
        # the definition, read off at shift 0
        assert both(*junction(side, 800, 1_000), *par) == [(side, 800, 1_000, 3, 3, 3, 3, 0, 3, 3)]
        # entries equal to the reference itself, not complemented, do NOT match; nor do complemented entries in the wrong direction
        R, L, table = junction(side, 800, 1_000)
        same = {k: [tuple(3 - c for c in e) for e in v] for k, v in table.items()}
        assert both(R, L, same, *par) == []
        step = 1 if side == RIGHT else -1
        at = lambda p: p - 1 if side == LEFT else p
        wrong = {(0, side, 800): [comp(at(1_000), 30, step)] * 3, (0, side, 1_000): [comp(at(800), 30, step)] * 3}
        assert both(R, L, wrong, *par) == []
        # ... and so do entries that belong to the other side's junction at the same positions
        other = junction(1 - side, 800, 1_000)[2]
        assert both(R, L, {(0, side, p): other[(0, 1 - side, p)] for p in (800, 1_000)}, *par) == []
        # the distance window's four edges
        for d, ok in ((49, False), (50, True), (400, True), (401, False)):
            got = both(*junction(side, 1_000 - d, 1_000), *par)
            assert got == ([(side, 1_000 - d, 1_000, 3, 3, 3, 3, 0, 3, 3)] if ok else []), (side, d, got)
        # homology of 5 on the x pile and 3 on the y pile: both verify at the one shift 8
        sign = 1 if side == RIGHT else -1
        got = both(*junction(side, 800, 1_000, h1=5, h2=3), *par)
        assert got == [(side, 800 + 5 * sign, 1_000 + 3 * sign, 3, 3, 3, 3, 8, 3, 3)], got
        # shifts 32 and 33
        got = both(*junction(side, 800, 1_000, h1=20, h2=12), *par)
        assert got == [(side, 800 + 20 * sign, 1_000 + 12 * sign, 3, 3, 3, 3, 32, 3, 3)], got
        assert both(*junction(side, 800, 1_000, h1=20, h2=13), *par) == []
        assert both(*junction(side, 800, 1_000, h1=5, h2=3), 3, 30, 50, 400, 7, 2) == []

    # x < y is reported once, not twice: the same pair with the roles swapped does not appear
    got = both(*junction(RIGHT, 800, 1_000), 3, 30, 1, 2_000, 32, 2)
    assert got == [(RIGHT, 800, 1_000, 3, 3, 3, 3, 0, 3, 3)]
    # equal sums: the smaller shift
    table = {(0, RIGHT, 800): [comp(999, 30, -1)] * 2 + [comp(992, 30, -1)] * 2, (0, RIGHT, 1_000): [comp(799, 30, -1)] * 2 + [comp(792, 30, -1)] * 2}
    assert both(array(2_000, [(800, 4), (1_000, 4)]), array(2_000, []), table, *par) == [(RIGHT, 800, 1_000, 4, 4, 2, 2, 0, 4, 4)]
    # min_verified failing on one pile only
    R, L, table = junction(LEFT, 800, 1_000)
    table[(0, LEFT, 1_000)] = [comp(800, 30)] + [comp(300, 30)] * 2
    assert both(R, L, table, *par) == [] and both(R, L, table, 3, 30, 50, 400, 32, 1) == [(LEFT, 800, 1_000, 3, 3, 3, 1, 0, 3, 3)]
    R, L, table = junction(RIGHT, 800, 1_000)
    table[(0, RIGHT, 800)] = [comp(999, 30, -1)] + [comp(300, 30, -1)] * 2
    assert both(R, L, table, *par) == [] and both(R, L, table, 3, 30, 50, 400, 32, 1) == [(RIGHT, 800, 1_000, 3, 3, 1, 3, 0, 3, 3)]
    # the tolerance: n >> 4 differences, at n = 15, 16, 31 and 32
    flip = lambda t, where: tuple((b + 1) % 4 if i in where else b for i, b in enumerate(t))
    for n, allowed in ((15, 0), (16, 1), (31, 1), (32, 2)):
        R, L, table = junction(RIGHT, 800, 1_000, n=n)
        e = comp(999, n, -1)
        table[(0, RIGHT, 800)] = [flip(e, range(3, 3 + allowed)), flip(e, range(3, 4 + allowed)), e]
        assert both(R, L, table, 3, 30, 50, 400, 32, 1) == [(RIGHT, 800, 1_000, 3, 3, 2, 3, 0, 3, 3)], n
    # a peak that is the y of one pair and the x of another: [600, 800) and [800, 1 000) inverted, the piles at 800 hold both
    R = array(2_000, [(600, 3), (800, 6), (1_000, 3)])
    table = {(0, RIGHT, 600): [comp(799, 30, -1)] * 3, (0, RIGHT, 800): [comp(599, 30, -1)] * 3 + [comp(999, 30, -1)] * 3, (0, RIGHT, 1_000): [comp(799, 30, -1)] * 3}
    assert both(R, array(2_000, []), table, 3, 30, 50, 300, 32, 2) == [(RIGHT, 600, 800, 3, 6, 3, 3, 0, 3, 6), (RIGHT, 800, 1_000, 6, 3, 3, 3, 0, 6, 3)]
    # a peak with two partners: ref[900 ..] repeats at ref[1 100 ..], so the pile at 800 continues behind either
    ref[1_060:1_100] = ref[960:1_000]
    R = array(2_000, [(800, 3), (1_000, 3), (1_100, 4)])
    table = {(0, RIGHT, 800): [comp(999, 30, -1)] * 3, (0, RIGHT, 1_000): [comp(799, 30, -1)] * 3, (0, RIGHT, 1_100): [comp(799, 30, -1)] * 4}
    got = both(R, array(2_000, []), table, *par)
    assert got == [(RIGHT, 800, 1_000, 3, 3, 3, 3, 0, 3, 3), (RIGHT, 800, 1_100, 3, 4, 3, 4, 0, 3, 4)], got
    # a right pair and a left pair on the same positions: sorted by (x, y, side), with a pair in front and one behind
    tables = [junction(RIGHT, 800, 1_000), junction(LEFT, 800, 1_000), junction(LEFT, 700, 900), junction(RIGHT, 800, 1_200, n1=0, n2=4)]
    R, L, table = sum(t[0] for t in tables), sum(t[1] for t in tables), {}
    for t in tables:
        for k, v in t[2].items():
            table[k] = table.get(k, []) + v
    ref[1_160:1_200] = ref[960:1_000]                               # so that the pile at 800 verifies against 1 200 as well
    got = both(R, L, table, *par)
    assert [g[:3] for g in got] == [(LEFT, 700, 900), (RIGHT, 800, 1_000), (LEFT, 800, 1_000), (RIGHT, 800, 1_200)], got
    # windows that reach past either end of the contig are mismatches there
    short = bytes(ref[:1_010])
    for n, ok in ((10, True), (11, False)):                         # the left entries at 800 are expected to hold comp(ref[1 000 + i]): 10 bases exist
        R, L = array(1_010, []), array(1_010, [(800, 3), (1_000, 3)])
        table = {(0, LEFT, 800): [comp(1_000, 10) + (0,) * (n - 10)] * 3, (0, LEFT, 1_000): [comp(800, 30)] * 3}
        assert (both(R, L, table, *par, r=short) == [(LEFT, 800, 1_000, 3, 3, 3, 3, 0, 3, 3)]) == ok, n
    for n, ok in ((5, True), (6, False)):                           # the right entries at 205 are expected to hold comp(ref[4 - i]): 5 bases exist
        R, L = array(1_010, [(5, 3), (205, 3)]), array(1_010, [])
        table = {(0, RIGHT, 5): [comp(204, 30, -1)] * 3, (0, RIGHT, 205): [comp(4, 5, -1) + (0,) * (n - 5)] * 3}
        assert (both(R, L, table, *par, r=short) == [(RIGHT, 5, 205, 3, 3, 3, 3, 0, 3, 3)]) == ok, n
    # an N is a mismatch: one in 30 bases is within the tolerance, two are not
    R, L, table = junction(RIGHT, 800, 1_000)
    R, L = R[:1_011], L[:1_011]
    withn = bytearray(short); withn[995] = ord("N")
    assert both(R, L, table, *par, r=bytes(withn)) == [(RIGHT, 800, 1_000, 3, 3, 3, 3, 0, 3, 3)]
    withn[990] = ord("N")
    assert both(R, L, table, *par, r=bytes(withn)) == []
    # v1 >= mv at one shift only, and the largest sum lies elsewhere: the chosen shift is the sum's, where v1 is one short
    R = array(2_000, [(800, 3), (1_000, 4)])
    table = {(0, RIGHT, 800): [comp(994, 30, -1)] * 2 + [comp(999, 30, -1)], (0, RIGHT, 1_000): [comp(799, 30, -1)] * 4}
    assert both(R, array(2_000, []), table, *par) == []
    assert both(R, array(2_000, []), table, 3, 30, 50, 400, 32, 1) == [(RIGHT, 800, 1_000, 3, 4, 1, 4, 0, 3, 4)]
    assert both(R, array(2_000, []), table, 3, 30, 50, 400, 4, 2) == []                         # S = 4: shift 5 is not even tried
    # the rendering: POS, REF, INFO, CT; POS 0 is skipped
    fasta = {"c": bytes(ref)}
    tables = [junction(RIGHT, 800, 1_000), junction(LEFT, 800, 1_000, h1=2, h2=1), junction(LEFT, 0, 200)]
    R, L, table = sum(t[0] for t in tables), sum(t[1] for t in tables), {}
    for t in tables:
        table.update(t[2])
    assert [g[:3] for g in both(R, L, table, *par)] == [(LEFT, 0, 200), (LEFT, 798, 999), (RIGHT, 800, 1_000)]
    text = ip.render(["c"], fasta, [R], [L], table).decode()
    assert text == ip.header() + (
        "c\t798\t.\t%s\t<INV>\t.\t.\tSVTYPE=INV;END=999;SVLEN=201;CT=5to5;HOMLEN=3;CR=3,3;CN=3,3;CV=3,3\n"
        "c\t800\t.\t%s\t<INV>\t.\t.\tSVTYPE=INV;END=1000;SVLEN=200;CT=3to3;HOMLEN=0;CR=3,3;CN=3,3;CV=3,3\n" % (chr(ref[797]), chr(ref[799])))
    assert ip.header().count("##INFO") == 8 and "##ALT=<ID=INV," in ip.header() and ip.header().count("##inversion=\"") == 1


def test_inverted_restatement_on_the_planted_data_set(tmp_path):
    """what tests/test_gpu_inverted.py relies on: with the driver's constants, -q 10 and clips of 20 bases the restatement finds 28 + 28
    peaks and 378 candidates per side on the planted data set, of which 9 per side qualify -- exactly the nine sites, at shift 0 and
    with every clipped read verified; no chance pair does.  The crossed search finds nothing on it and the facing search 28 piles: today
    these inversions are printed as insertions.  The driver's CPU stand-in runs on it to exit status 0."""
    from tests.support import clipcounts as cc
    from tests.support import cliptails as ct
    from tests.support import crossedpiles as cp
    from tests.support import facingpiles as fp
    from tests.support import invertedpiles as ip
    refs, rd = ip.planted_reads()
    d = ip.write_planted(str(tmp_path), refs, rd)
    text, recs, n_cand, n_peaks = ip.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    assert len(ip.SITES) == 9 and min(n for _, n in ip.SITES) == 50 and max(n for _, n in ip.SITES) > 4_900
    assert n_peaks == (28, 28) and n_cand == (378, 378)
    for side in (0, 1):
        assert [(r[2], r[3] - r[2]) for r in recs if r[1] == side] == ip.SITES                   # every site, and nothing else
    assert len(recs) == 18 and recs == sorted(recs, key=lambda r: (r[2], r[3], r[1]))
    assert all(r[8] == 0 and r[4] >= 3 and r[5] >= 3 and (r[6], r[7]) == (r[9], r[10]) == (r[4], r[5]) for r in recs), recs
    lines = text.decode().split("\n")
    for a, n in ip.SITES:
        for ct_ in ("3to3", "5to5"):
            assert sum(1 for ln in lines if ln.startswith("ctg0\t%d\t" % a) and "END=%d;SVLEN=%d;CT=%s;HOMLEN=0;" % (a + n, n, ct_) in ln) == 1, (a, n, ct_)
    assert text.startswith(ip.header().encode()) and text.count(b"\n") == ip.header().count("\n") + 2 * len(ip.SITES)
    # what the other two searches make of it
    names, right, left = cc.arrays_of_bam(d + "/aln.bam", cc.MIN_CLIP, 10)
    table = ct.table_of_bam(d + "/aln.bam", cc.MIN_CLIP, 10)[1]
    fasta = ct.read_fasta(d + "/ref.fa")
    assert cp.crossed(right[0], left[0], table, fasta[names[0]], 0, cp.MIN_READS, cp.REACH, cp.MIN_LEN, cp.MAX_LEN, cp.MAX_SHIFT, cp.MIN_VERIFIED)[0] == []
    assert len(fp.facing_many(right[0], left[0], fp.MIN_READS, fp.MAX_OVERLAP)) == 28
    r = _run([_shim(), "-i", "cfg.txt", "-s", "100", "ref.fa", "sample=aln.bam"], d)
    assert r.returncode == 0 and len(r.stdout) > 1000
