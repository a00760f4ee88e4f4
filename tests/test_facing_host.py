"""-I (large insertions from facing clip piles) where there is no GPU: the host driver linked against tests/shim/im_shim.c, which
implements the C ABI without the clip, clip-tail and facing entry points.  The driver must still link, behave as before without -I, and
say what -I needs.  The restatement the GPU tests measure against (tests/support/facingpiles.py) is pinned here on cases worked by hand
and on the planted data set of tests/test_gpu_facing.py."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")

FACING_ENTRY_POINTS = ["im_clip_facing_tid", "im_clip_facing", "im_cliptail_consensus"]
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
    f = str(tmp_path / "ins.vcf")
    _refused(_run([shim] + BASE + ["-G", "-C", "-I", f] + ["-q", "10"] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    _refused(_run([shim] + BASE + ["-G", "-I", f] + IN, TD), b"indelminer: -I needs -V")
    _refused(_run([shim] + BASE + ["-I", f] + IN, TD), b"indelminer: -I needs -V")
    # every other refusal reaches it through -G, -C and -V, and theirs come first
    _refused(_run([shim] + BASE + ["-G", "-V", "-I", f] + IN, TD), b"indelminer: -V needs -C")
    _refused(_run([shim] + BASE + ["-C", "-V", "-I", f] + IN, TD), b"indelminer: -C needs -G")
    _refused(_run([shim] + BASE + ["-C", "-V", "-I", f] + KNOWN, TD), b"indelminer: -C is not available with a VCF argument (annotate mode)")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-I", f, "-c", "reference:1-5000"] + IN, TD), b"indelminer: -C is not available with -c")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-I", f] + IN, TD), b"indelminer: clip evidence (-C) needs the device library")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-I", f] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-C", "-V", "-I", f] + KNOWN, TD), b"-G is not available with a VCF argument")
    assert not os.path.exists(f)                                    # a refused run writes no FILE
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_a_library_with_the_clip_and_clip_tail_entries_and_without_the_facing_entries(tmp_path):
    """the shim beside stubs of -C's six and -V's six entries: -I's own refusal, behind theirs"""
    from indelminer_amd import build
    srcs = [os.path.join(build.HOST_DIR, s) for s in build.HOST_SOURCES]
    srcs += [os.path.join(ROOT, "tests", "shim", s) for s in ("im_shim.c", "clip_entries_stub.c", "cliptail_entries_stub.c")]
    srcs += [os.path.join(ROOT, "oracle", "im_oracle.c"), os.path.join(ROOT, "oracle", "im_oracle_triage.c")]
    binary = str(tmp_path / "indelminer_shim_cliptail")
    subprocess.check_call(["gcc", "-O0", "-std=c11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "indelminer_amd", "host"), "-o", binary] + srcs + ["-lz", "-lm"])
    f = str(tmp_path / "ins.vcf")
    for flags in (["-G", "-C", "-V", "-I", f], ["-I", f, "-V", "-C", "-G"]):
        _refused(_run([binary] + BASE + flags + IN, TD), b"indelminer: large-insertion evidence (-I) needs the device library")
    _refused(_run([binary] + BASE + ["-G", "-C", "-I", f] + IN, TD), b"indelminer: -I needs -V")
    assert not os.path.exists(f)
    r = _run([binary] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_help_names_the_option():
    h = _run([_shim(), "-h"], TD)
    assert h.returncode == 0 and re.search(rb"^\t-I, with -G -C -V", h.stdout, re.M)


def test_facing_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    from indelminer_amd import build, capi
    import ctypes as C
    L = C.CDLL(build.build())
    src = open(capi.__file__).read()
    for s in FACING_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % s, text), s
        assert hasattr(L, s), s
        assert "L.%s.argtypes" % s in src, s
    for s in ("clip_facing_tid", "clip_facing", "cliptail_consensus"):
        assert callable(getattr(capi.Context, s)), s
    # the definitions are stated in seam 5, behind what they read
    assert text.index("Clipped reads, the breakpoint evidence") < text.index("Facing piles, the breakpoints of large insertions") < \
        text.index("Clip tails, what the clipped reads were clipped OF") < text.index("The consensus of a pile (-I)")
    for words in ("R[p] > R[x] for every x in [p - T, p)", "R[p] >= R[x] for every x in (p, p + T]", "the largest x among equals", "0 <= T <= 64",
                  "*n_found is ALWAYS the number of piles", "sorted by pr ascending", "never enters",
                  "cover(i) = #{e : n_e > i}", "len = #{i < 32 : cover(i) >= c}", "the smallest code (A < C < G < T) among equals",
                  "min(n_e, len) >> 4", "independent of the order", "answers all zeros", "tens of reads"):
        assert words in text, words
    # additive: the ABI version and the mirrored structs keep their layout; the shim stays without the entries
    assert "#define IM_ABI_VERSION 3" in text
    assert C.sizeof(capi.TriageParams) == 24 and C.sizeof(capi.DevRecords) == 32
    shim = open(os.path.join(ROOT, "tests", "shim", "im_shim.c")).read()
    assert "im_clip_facing" not in shim and "im_cliptail" not in shim


def test_facing_restatement_on_cases_worked_by_hand():
    """the yardstick of the GPU tests (tests/support/facingpiles.py), pinned here where no GPU is needed"""
    from tests.support import facingpiles as fp

    def arrays(clen, right=(), left=()):
        R, L = np.zeros(clen + 1, np.int64), np.zeros(clen + 1, np.int64)
        for p, v in right:
            R[p] = v
        for p, v in left:
            L[p] = v
        return R, L

    both = lambda R, L, m, T: (fp.facing(R, L, m, T), fp.facing_many(R, L, m, T))
    same = lambda R, L, m, T: both(R, L, m, T)[0] if both(R, L, m, T)[0] == both(R, L, m, T)[1] else "the two forms differ"
    # one pile, its partner 4 in front: pr, pl, cr, cl
    assert same(*arrays(100, [(50, 5)], [(46, 3)]), 3, 30) == [(50, 46, 5, 3)]
    # counts of m and m - 1 on either side
    assert same(*arrays(100, [(50, 3)], [(46, 3)]), 3, 30) == [(50, 46, 3, 3)]
    assert same(*arrays(100, [(50, 2)], [(46, 3)]), 3, 30) == [] and same(*arrays(100, [(50, 3)], [(46, 2)]), 3, 30) == []
    # pl = pr; a left pile BEHIND the right pile is a deletion's, never a facing pile
    assert same(*arrays(100, [(50, 3)], [(50, 4)]), 3, 30) == [(50, 50, 3, 4)]
    assert same(*arrays(100, [(50, 3)], [(51, 9)]), 3, 30) == []
    # the partner at exactly p - T and at p - T - 1
    assert same(*arrays(100, [(50, 3)], [(20, 3)]), 3, 30) == [(50, 20, 3, 3)] and same(*arrays(100, [(50, 3)], [(19, 3)]), 3, 30) == []
    # the largest L, the largest x among equals
    assert same(*arrays(100, [(50, 3)], [(40, 3), (45, 4), (48, 3)]), 3, 30) == [(50, 45, 3, 4)]
    assert same(*arrays(100, [(50, 3)], [(40, 4), (45, 4), (48, 3)]), 3, 30) == [(50, 45, 3, 4)]
    # equal peaks at distance T: the left one wins; at T + 1 both are piles
    assert same(*arrays(200, [(50, 4), (80, 4)], [(50, 3), (80, 3)]), 3, 30) == [(50, 50, 4, 3)]
    assert same(*arrays(200, [(50, 4), (81, 4)], [(50, 3), (81, 3)]), 3, 30) == [(50, 50, 4, 3), (81, 81, 4, 3)]
    # a higher peak T to the right hides the pile (and takes its partner, which stands at exactly its own p - T), one T + 1 to the right
    # does not; a higher peak T to the left hides it too
    assert same(*arrays(200, [(50, 4), (80, 5)], [(50, 3)]), 3, 30) == [(80, 50, 5, 3)] and same(*arrays(200, [(50, 4), (81, 5)], [(50, 3)]), 3, 30) == [(50, 50, 4, 3)]
    assert same(*arrays(200, [(50, 5), (80, 4)], [(80, 3)]), 3, 30) == [] and same(*arrays(200, [(49, 5), (80, 4)], [(80, 3)]), 3, 30) == [(80, 80, 4, 3)]
    # a peak that has no partner still hides its neighbours: being a peak does not depend on L
    assert same(*arrays(200, [(50, 5), (60, 4)], [(60, 3)]), 3, 30) == []
    # piles at 0 and at clen: the windows stop at the contig's entries
    assert same(*arrays(100, [(0, 3), (100, 4)], [(0, 3), (98, 5)]), 3, 30) == [(0, 0, 3, 3), (100, 98, 4, 5)]
    # a contig shorter than one window
    assert same(*arrays(70, [(40, 3)], [(10, 3)]), 3, 30) == [(40, 10, 3, 3)] and same(*arrays(70, [(40, 3)], [(10, 3)]), 3, 64) == [(40, 10, 3, 3)]
    assert same(*arrays(70, [(40, 3), (70, 3)], [(0, 3)]), 3, 64) == [(40, 0, 3, 3)]       # 70 is no peak: 40 is within reach and further left
    # T = 0: every position on its own; m = 1
    assert same(*arrays(100, [(50, 1), (51, 2), (52, 1)], [(50, 1), (52, 1)]), 1, 0) == [(50, 50, 1, 1), (52, 52, 1, 1)]
    assert same(np.zeros(11, np.int64), np.zeros(11, np.int64), 1, 30) == []

    # ---- the consensus
    A, C_, G, T = 0, 1, 2, 3
    assert fp.consensus([], 1) == (0, 0, (), 0)
    assert fp.consensus([(A, C_, G)], 1) == (1, 3, (A, C_, G), 1) and fp.consensus([(A, C_, G)], 2) == (1, 0, (), 0)
    # cover falls inside the bases: len is where min_cover entries still reach
    e = [(A, C_, G, T, A), (A, C_, G), (A, C_, G, T)]
    assert fp.consensus(e, 1) == (3, 5, (A, C_, G, T, A), 3) and fp.consensus(e, 2) == (3, 4, (A, C_, G, T), 3)
    assert fp.consensus(e, 3) == (3, 3, (A, C_, G), 3) and fp.consensus(e, 4) == (3, 0, (), 0)
    # the majority per base; 2 : 2 is the smallest code; the order of arrival does not matter
    e = [(G, G, T), (C_, G, T), (G, C_, T), (C_, C_, A)]
    assert fp.consensus(e, 2) == (4, 3, (C_, C_, T), 0) and fp.consensus(e[::-1], 2) == fp.consensus(e, 2)
    # the tolerance: min(n, len) >> 4 differences in the first min(n, len) bases
    base = tuple(int(x) for x in np.random.default_rng(1).integers(0, 4, 32))
    flip = lambda t, where: tuple((b + 1) % 4 if i in where else b for i, b in enumerate(t))
    e = [base] * 5 + [flip(base, (0, 31)), flip(base, (0, 15, 31)), flip(base[:20], (19,)), flip(base[:20], (0, 19)), flip(base[:15], (3,))]
    n, ln, cons, agree = fp.consensus(e, 2)
    assert (n, ln, cons) == (10, 32, base) and agree == 5 + 1 + 0 + 1 + 0 + 0
    # ... and what counts is what lies inside len: with min_cover 8 only 20 bases are covered, and the flips at 31 are outside
    n, ln, cons, agree = fp.consensus(e, 8)
    assert (n, ln, cons) == (10, 20, base[:20]) and agree == 5 + 1 + 0 + 1 + 0 + 0
    n, ln, cons, agree = fp.consensus(e + [flip(base, (0, 25, 31))], 9)
    assert (ln, agree) == (20, 5 + 1 + 0 + 1 + 0 + 0 + 1)
    # the planes of the answer, and a position outside the contig
    table = {(0, 0, 50): [(A, C_, G, T), (A, C_, G, T)]}
    assert fp.answer(table, 0, 50, 0, 2, 100) == (2, 4, 0b1010, 0b1100, 2)
    assert fp.answer(table, 0, 50, 1, 2, 100) == (0, 0, 0, 0, 0) and fp.answer(table, 0, 101, 0, 2, 100) == (0, 0, 0, 0, 0)
    assert fp.answer(table, 0, -1, 0, 2, 100) == (0, 0, 0, 0, 0)


def test_facing_restatement_on_the_planted_data_set(tmp_path):
    """what tests/test_gpu_facing.py relies on: with m = 3, T = 30, -q 10 and clips of 20 bases the restatement finds 18 piles on the
    planted data set -- 8 at planted sites, with END - POS of 0, 3, 6, 9, 12, 15, 24 and 27, and the 10 short insertions the simulator
    plants itself, with POS = END -- in a table of 276 entries under 41 keys; the driver's CPU stand-in runs on it to exit status 0"""
    from tests.support import facingpiles as fp
    refs, rd, insertions = fp.planted_reads()
    d = fp.write_planted(str(tmp_path), refs, rd)
    text, recs, table = fp.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    sites = dict(fp.SITES)
    assert len(recs) == 18
    assert [r[1] - r[2] for r in recs if r[1] in sites] == [0, 3, 6, 9, 12, 15, 24, 27]
    assert all(r[1] - r[2] == sites[r[1]] for r in recs if r[1] in sites)
    assert [r[1] - r[2] for r in recs if r[1] not in sites] == [0] * 10
    assert (sum(len(v) for v in table.values()), len(table)) == (276, 41)
    # at the site without a duplication both consensus sequences are the planted insertion's
    (site0,) = [r for r in recs if r[1] == fp.SITES[0][0]]
    ins = [b"ACGT".index(bytes([c])) for c in insertions[0]]
    (_, ln_r, cons_r, _), (_, ln_l, cons_l, _) = site0[5], site0[6]
    assert ln_r >= 20 and ln_l >= 20 and list(cons_r) == ins[:ln_r] and list(cons_l[::-1]) == ins[len(ins) - ln_l:]
    assert text.startswith(fp.HEADER.encode()) and text.count(b"\n") == fp.HEADER.count("\n") + 18
    r = _run([_shim(), "-i", "cfg.txt", "-s", "100", "ref.fa", "sample=aln.bam"], d)
    assert r.returncode == 0 and len(r.stdout) > 1000
