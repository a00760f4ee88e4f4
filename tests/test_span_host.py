"""-G (genotype columns) where there is no GPU: the host driver linked against tests/shim/im_shim.c, which implements the C ABI
without the span entry points.  The driver must still link, behave as before without -G, and say what -G needs."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")

SPAN_ENTRY_POINTS = ["im_span_enable", "im_dev_span_scatter", "im_span_scan", "im_span_reset", "im_span_query_tid", "im_span_build", "im_span_query"]


def _shim():
    from tests.support.shimbuild import build_shim
    return build_shim()


def _golden(name):
    return open(os.path.join(GOLD, "vcf", name + ".vcf"), "rb").read()


def _run(args, cwd):
    return subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_shim_binary_refuses_genotyping_and_is_unchanged_without_it():
    shim = _shim()
    g = _run([shim, "-i", "indelminer.config", "-G", "reference.fa", "sample=alignments.bam"], TD)
    assert g.returncode != 0 and g.stdout == b""
    assert b"genotyping (-G) needs the device library" in g.stderr
    r = _run([shim, "-i", "indelminer.config", "reference.fa", "sample=alignments.bam"], TD)
    assert r.returncode == 0 and r.stdout == _golden("default_config")


def test_genotyping_is_refused_in_annotate_mode_and_across_ranks():
    shim = _shim()
    a = _run([shim, "-i", "indelminer.config", "-G", "reference.fa", "indelminer.expected.vcf", "sample=alignments.bam"], TD)
    assert a.returncode != 0 and a.stdout == b"" and b"-G is not available with a VCF argument" in a.stderr
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    w = subprocess.run([shim, "-i", "indelminer.config", "-G", "reference.fa", "sample=alignments.bam"], cwd=TD, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert w.returncode != 0 and w.stdout == b"" and b"-G is not available with more than one rank" in w.stderr


def test_help_names_the_option():
    h = _run([_shim(), "-h"], TD)
    assert h.returncode == 0 and re.search(rb"^\t-G, ", h.stdout, re.M)


def with_genotype_columns(vcf):
    """a plain VCF of the driver dressed as -G writes it: ##FORMAT lines behind the ##INFO block, two more columns per line"""
    out = []
    for ln in vcf.decode().split("\n"):
        if ln.startswith("#CHROM"):
            out += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', '##FORMAT=<ID=AD,Number=2,Type=Integer,Description="Read support">',
                    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">']
            ln += "\tFORMAT\tt"
        elif ln and not ln.startswith("#"):
            ln += "\tGT:AD:GQ\t./.:.,3:." if "PAIRED_READ" in ln.split("\t")[7].split(";") else "\tGT:AD:GQ\t0/1:12,9:99"
        out.append(ln)
    return "\n".join(out).encode()


def test_annotate_mode_reads_a_genotyped_vcf(tmp_path):
    """read_variants takes eight columns of a line and leaves what follows alone: a VCF with the genotype columns annotates like
    the plain one (the golden was made by the reference from the plain one)"""
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    d = str(tmp_path)
    mg.write_dataset(d, mg.SYNTH_TN["normal"], "normal_")
    dressed = with_genotype_columns(_golden("synth_tn_tumor"))
    assert dressed.count(b"GT:AD:GQ") > 10
    open(os.path.join(d, "tumor_g.vcf"), "wb").write(dressed)
    a = _run([_shim(), "-i", "cfg.txt", "-q", "0", "-a", "-e", "1", "ref.fa", "tumor_g.vcf", "normal=normal_aln.bam"], d)
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert a.stdout == _golden("synth_tn_annotate")


def test_span_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    from indelminer_amd import build, capi
    import ctypes as C
    L = C.CDLL(build.build())
    src = open(capi.__file__).read()
    for s in SPAN_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % s, text), s
        assert hasattr(L, s), s
        assert "L.%s.argtypes" % s in src, s
    # additive: the ABI version and the mirrored structs keep their layout
    assert "#define IM_ABI_VERSION 3" in text
    assert C.sizeof(capi.TriageParams) == 24 and C.sizeof(capi.DevRecords) == 32
