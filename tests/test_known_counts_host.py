"""-A (genotype the known indels of annotate mode) where there is no GPU: the host driver linked against tests/shim/im_shim.c,
which implements the C ABI without im_support_count and the span entry points.  The driver must still link, annotate as before
without -A, and say what -A needs."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")


def _shim():
    from tests.support.shimbuild import build_shim
    return build_shim()


def _golden(name):
    return open(os.path.join(GOLD, "vcf", name + ".vcf"), "rb").read()


def _run(args, cwd, env=None):
    return subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


# the `annotate` golden was made from the golden default_config.vcf with these options (tests/test_host_driver.py)
ANNOTATE = ["-i", "indelminer.config", "-q", "0", "-a", "-e", "1", "reference.fa", os.path.join(GOLD, "vcf", "default_config.vcf"), "normal=alignments.bam"]


def test_shim_binary_refuses_known_counts_and_annotates_as_before_without_them():
    shim = _shim()
    a = _run([shim, "-A"] + ANNOTATE, TD)
    assert a.returncode != 0 and a.stdout == b""
    assert b"indelminer: genotyping known indels (-A) needs the device library" in a.stderr
    assert len(a.stderr.strip().split(b"\n")) == 1
    r = _run([shim] + ANNOTATE, TD)
    assert r.returncode == 0 and r.stdout == _golden("annotate")


def test_known_counts_need_a_vcf_argument():
    a = _run([_shim(), "-i", "indelminer.config", "-A", "reference.fa", "sample=alignments.bam"], TD)
    assert a.returncode != 0 and a.stdout == b""
    assert a.stderr.strip() == b"indelminer: -A needs a VCF argument (annotate mode)"


def test_known_counts_are_refused_across_ranks():
    for extra in ({"WORLD_SIZE": "2", "RANK": "0"}, {"INDELMINER_FORCE_MGPU": "1"}):
        w = _run([_shim(), "-A"] + ANNOTATE, TD, env=dict(os.environ, **extra))
        assert w.returncode != 0 and w.stdout == b"", extra
        assert len(w.stderr.strip().split(b"\n")) == 1 and b"-A" in w.stderr, w.stderr


def test_help_names_the_option():
    h = _run([_shim(), "-h"], TD)
    assert h.returncode == 0 and re.search(rb"^\t-A, ", h.stdout, re.M)
    assert re.search(rb"^\t-G, ", h.stdout, re.M)


def test_annotate_mode_on_the_tumour_normal_pair_is_unchanged_without_the_option(tmp_path):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    d = str(tmp_path)
    mg.write_dataset(d, mg.SYNTH_TN["normal"], "normal_")
    open(os.path.join(d, "tumor.vcf"), "wb").write(_golden("synth_tn_tumor"))
    a = _run([_shim(), "-i", "cfg.txt", "-q", "0", "-a", "-e", "1", "ref.fa", "tumor.vcf", "normal=normal_aln.bam"], d)
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert a.stdout == _golden("synth_tn_annotate")


def test_count_entry_point_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "indelminer_amd.h")).read()
    from indelminer_amd import build, capi
    L = C.CDLL(build.build())
    src = open(capi.__file__).read()
    assert re.search(r"\bint im_support_count\(", text)
    assert "src/variant.c:1427-1573" in text
    assert hasattr(L, "im_support_count")
    assert "L.im_support_count.argtypes" in src
    # the mirrored task and variant records have the header's layout: 6 and 9 int32
    assert C.sizeof(capi.KnownVariant) == 24 == capi.KNOWN_VARIANT_DTYPE.itemsize
    assert C.sizeof(capi.CountTask) == 36 == capi.COUNT_TASK_DTYPE.itemsize
    for name, n in (("im_known_variant", 6), ("im_count_task", 9)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for f in decl.split(",")]
        mirror = capi.KnownVariant if n == 6 else capi.CountTask
        assert fields == [f[0] for f in mirror._fields_], name
    assert (capi.SC_DIRECT, capi.SC_MAPQ_OK, capi.SC_SPANS) == tuple(int(re.search(r"#define IM_SC_%s\s+(\d+)" % k, text).group(1)) for k in ("DIRECT", "MAPQ_OK", "SPANS"))
    # additive: the ABI version and the existing mirrored structs keep their layout
    assert "#define IM_ABI_VERSION 3" in text and L.im_abi_version() == 3
    assert C.sizeof(capi.TriageParams) == 24 and C.sizeof(capi.DevRecords) == 32
    assert C.sizeof(capi.ReadResult) == 512 and C.sizeof(capi.Params) == 16 and C.sizeof(capi.Evidence) == 36
    assert C.sizeof(capi.DevBatch) == 88 and C.sizeof(capi.DevCands) == 136 and C.sizeof(capi.ReadBatch) == 48
