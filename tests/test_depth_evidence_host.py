"""-D (depth evidence for large deletions) where there is no GPU: the host driver linked against tests/shim/im_shim.c, which
implements the C ABI without the median entry points.  The driver must still link, behave as before without -D, and say what
-D needs."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")

MEDIAN_ENTRY_POINTS = ["im_depth_median_tid", "im_depth_median"]
BASE = ["-i", "indelminer.config"]
IN = ["reference.fa", "sample=alignments.bam"]


def _shim():
    from tests.support.shimbuild import build_shim
    return build_shim()


def _run(args, cwd, env=None):
    return subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def _refused(r, line):
    assert r.returncode != 0 and r.stdout == b"", r
    assert r.stderr.count(b"\n") == 1 and line in r.stderr, r.stderr


def test_shim_binary_refuses_depth_evidence_and_is_unchanged_without_it():
    shim = _shim()
    for flags in (["-D", "-G"], ["-G", "-D"]):
        _refused(_run([shim] + BASE + flags + IN, TD), b"indelminer: depth evidence (-D) needs the device library")
    r = _run([shim] + BASE + IN, TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_the_option_is_refused_where_it_does_not_apply():
    shim = _shim()
    _refused(_run([shim] + BASE + ["-D"] + IN, TD), b"indelminer: -D needs -G")
    _refused(_run([shim] + BASE + ["-D", "reference.fa", "known.vcf", "sample=alignments.bam"], TD),
             b"indelminer: -D is not available with a VCF argument (annotate mode)")
    _refused(_run([shim] + BASE + ["-G", "-D", "-c", "reference:1-5000"] + IN, TD), b"indelminer: -D is not available with -c")
    # the refusals of -G, -A and -P are unchanged and come first
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    _refused(_run([shim] + BASE + ["-G", "-D"] + IN, TD, env=env), b"-G is not available with more than one rank")
    _refused(_run([shim] + BASE + ["-G", "-D", "reference.fa", "known.vcf", "sample=alignments.bam"], TD), b"-G is not available with a VCF argument")
    _refused(_run([shim] + BASE + ["-A", "-D"] + IN, TD), b"-A needs a VCF argument")
    _refused(_run([shim] + BASE + ["-P", "-D"] + IN, TD), b"indelminer: -P needs -G or -A")
    _refused(_run([shim] + BASE + ["-P", "-G", "-D"] + IN, TD), b"indelminer: genotyping paired-read records (-P) needs the device library")


def test_restatements_on_cases_worked_by_hand():
    """the yardsticks of the GPU tests (tests/support/depthmedian.py), pinned here where no GPU is needed"""
    import numpy as np
    from tests.support.depthmedian import NONE, evidence_of, medians
    d = np.array([5, 1, 9, 3], np.int64)
    assert list(medians(d, [0, 0, 1, 3, 4, 2, -3], [4, 3, 2, 9, 9, 1, 2])) == [3, 5, 1, 3, NONE, NONE, 1]     # even length: the lower of the two
    assert list(medians(np.array([5000, 4095, 4094]), [0, 0], [1, 3])) == [4095, 4095]
    d = np.array([30] * 1000 + [2, 1, 3, 0] + [28] * 1000 + [9] * 10, np.int64)
    assert evidence_of(d, 1000, 1004) == ("1,30,28", "34")          # (2000 * 1 + 29) // 58
    assert evidence_of(d, 0, 1000) == ("30,.,28", "1071")           # no left flank: (30000 + 14) // 28
    assert evidence_of(d[:1004], 1000, 1004) == ("1,30,.", "33")    # no right flank: (1000 + 15) // 30
    assert evidence_of(np.zeros(3000, np.int64), 1000, 1100) == ("0,0,0", ".")


def test_help_names_the_option():
    h = _run([_shim(), "-h"], TD)
    assert h.returncode == 0 and re.search(rb"^\t-D, ", h.stdout, re.M)


def test_median_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    from indelminer_amd import build, capi
    import ctypes as C
    L = C.CDLL(build.build())
    src = open(capi.__file__).read()
    for s in MEDIAN_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % s, text), s
        assert hasattr(L, s), s
        assert "L.%s.argtypes" % s in src, s
    for s in ("depth_median_tid", "depth_median"):
        assert callable(getattr(capi.Context, s)), s
    assert "0xFFFFFFFF" in text and "4095" in text and "(n + 1) / 2" in text       # the definition and the saturation are stated
    # additive: the ABI version and the mirrored structs keep their layout
    assert "#define IM_ABI_VERSION 3" in text
    assert C.sizeof(capi.TriageParams) == 24 and C.sizeof(capi.DevRecords) == 32
