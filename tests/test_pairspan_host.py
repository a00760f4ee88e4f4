"""-P (genotype columns of PAIRED_READ records) where there is no GPU: the host driver linked against tests/shim/im_shim.c, which
implements the C ABI without the pair-span entry points.  The driver must still link, behave as before without -P, and say what
-P needs."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")

PAIRSPAN_ENTRY_POINTS = ["im_pairspan_enable", "im_dev_pairspan_scatter", "im_pairspan_scan", "im_pairspan_reset", "im_pairspan_query_tid",
                         "im_pairspan_build", "im_pairspan_query"]


def _shim():
    from tests.support.shimbuild import build_shim
    return build_shim()


def _run(args, cwd, env=None):
    return subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def test_shim_binary_refuses_paired_read_genotyping_and_is_unchanged_without_it():
    shim = _shim()
    g = _run([shim, "-i", "indelminer.config", "-P", "-G", "reference.fa", "sample=alignments.bam"], TD)
    assert g.returncode != 0 and g.stdout == b""
    assert b"indelminer: genotyping paired-read records (-P) needs the device library" in g.stderr
    r = _run([shim, "-i", "indelminer.config", "reference.fa", "sample=alignments.bam"], TD)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLD, "vcf", "default_config.vcf"), "rb").read()


def test_the_option_alone_is_refused():
    shim = _shim()
    p = _run([shim, "-i", "indelminer.config", "-P", "reference.fa", "sample=alignments.bam"], TD)
    assert p.returncode != 0 and p.stdout == b"" and b"indelminer: -P needs -G or -A" in p.stderr
    # the refusals of -G and -A are unchanged and come first
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    w = _run([shim, "-i", "indelminer.config", "-G", "-P", "reference.fa", "sample=alignments.bam"], TD, env=env)
    assert w.returncode != 0 and w.stdout == b"" and b"-G is not available with more than one rank" in w.stderr
    a = _run([shim, "-i", "indelminer.config", "-A", "-P", "reference.fa", "sample=alignments.bam"], TD)
    assert a.returncode != 0 and a.stdout == b"" and b"-A needs a VCF argument" in a.stderr


def test_help_names_the_option():
    h = _run([_shim(), "-h"], TD)
    assert h.returncode == 0 and re.search(rb"^\t-P, ", h.stdout, re.M)


def test_pairspan_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    from indelminer_amd import build, capi
    import ctypes as C
    L = C.CDLL(build.build())
    src = open(capi.__file__).read()
    for s in PAIRSPAN_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % s, text), s
        assert hasattr(L, s), s
        assert "L.%s.argtypes" % s in src, s
    for s in ("pairspan_enable", "pairspan_scatter", "pairspan_scan", "pairspan_reset", "pairspan_query_tid", "pairspan_build", "pairspan_query"):
        assert callable(getattr(capi.Context, s)), s
    # additive: the ABI version and the mirrored structs keep their layout
    assert "#define IM_ABI_VERSION 3" in text
    assert C.sizeof(capi.TriageParams) == 24 and C.sizeof(capi.DevRecords) == 32
