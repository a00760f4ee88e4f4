"""The product with a stream per walker on small inputs.

On real data every walker has a stream of its own (host_pipeline.c:pipe_init) and up to 16 of them upload, triage and scatter into the
same genome-wide arrays and keyed tables at once.  An input below 64 MB falls back to the context's stream -- and every product test of
the evidence options uses such an input, so -G -P -D -C -V -M -I -U -N only ever ran on one stream.  Here the planted data sets of those
tests run once more with INDELMINER_STREAMS=own on small pieces and four walkers.  The FILEs of -I, -U and -N must be the CPU
restatements' renderings byte for byte, the -G -P -D columns the restatements' values and the committed golden underneath them, and
everything must equal what the default run of the same input prints.  INDELMINER_TIMING's "a pipeline's buffers" line names the kind of
stream each pipeline got: the test asserts that the run really was in the mode it names.

A race between walkers' scatters (a lost update of a counted array, a keyed-table slot claimed twice) or a per-pipeline scratch shared
by mistake shows here as a wrong count, genotype, verification or PE value in some record.  One product process runs at a time.
"""
import importlib.util
import os
import subprocess

import pytest

from tests.support import crossedpiles as cp
from tests.support import facingpiles as fp
from tests.support import invertedpiles as ip
from tests.support import pairlinks as pk
from tests.support.spanarrays import GOLD, _golden, _product, genotype_of

pytestmark = pytest.mark.gpu

OWN = {"INDELMINER_STREAMS": "own", "INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "4"}
BASE = ["-i", "cfg.txt", "-s", "100"]


def _run(flags, cwd, env):
    e = dict(os.environ)
    e.update(env)
    e["INDELMINER_TIMING"] = "1"
    r = subprocess.run([_product()] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r


def both_runs(flags_of, cwd):
    """the default run and the own-streams run of flags_of(suffix), each asserted to have run in its mode; returns their results"""
    default, own = _run(flags_of("default"), cwd, {}), _run(flags_of("own"), cwd, OWN)
    lines = lambda r: [ln for ln in r.stderr.decode().split("\n") if "a pipeline's buffers" in ln]
    assert len(lines(default)) >= 1 and all("shared stream" in ln and "own stream" not in ln for ln in lines(default)), lines(default)
    assert len(lines(own)) >= 2 and all("own stream" in ln and "shared stream" not in ln for ln in lines(own)), lines(own)
    assert own.stdout == default.stdout and len(default.stdout) > 1000
    return default, own


def read(cwd, name):
    return open(os.path.join(cwd, name), "rb").read()


def test_large_insertions_on_own_streams(tmp_path):
    """-G -C -V -I over facingpiles' ten planted insertions"""
    refs, rd, _ = fp.planted_reads()
    d = fp.write_planted(str(tmp_path), refs, rd)
    text, recs, _ = fp.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    both_runs(lambda s: BASE + ["-G", "-C", "-V", "-I", "ins_%s.vcf" % s], d)
    assert len(recs) == 18 and read(d, "ins_own.vcf") == text == read(d, "ins_default.vcf")


def test_tandem_duplications_on_own_streams(tmp_path):
    """-G -D -C -V -U over crossedpiles' nine planted duplications: the FILE with its depth fields"""
    from tests.test_gpu_depth_evidence import depth_of_bam
    refs, rd = cp.planted_reads()
    d = cp.write_planted(str(tmp_path), refs, rd)
    text_d, recs = cp.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10, depth_of_bam(d + "/aln.bam")[1])[:2]
    both_runs(lambda s: BASE + ["-G", "-D", "-C", "-V", "-U", "dup_%s.vcf" % s], d)
    assert [(r[2], r[1] - r[2]) for r in recs] == cp.SITES and text_d.count(b";DFC=") == len(recs)
    assert read(d, "dup_own.vcf") == text_d == read(d, "dup_default.vcf")


def test_inversion_breakpoints_on_own_streams(tmp_path):
    """-G -C -V -N over invertedpiles' nine planted inversions"""
    refs, rd = ip.planted_reads()
    d = ip.write_planted(str(tmp_path), refs, rd)
    text, recs = ip.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)[:2]
    both_runs(lambda s: BASE + ["-G", "-C", "-V", "-N", "inv_%s.vcf" % s], d)
    assert len(recs) == 18 and read(d, "inv_own.vcf") == text == read(d, "inv_default.vcf")


@pytest.mark.parametrize("svtype", ["DUP", "INV"])
def test_pair_links_on_own_streams(svtype, tmp_path):
    """-G -C -V -I -U -N -M over the planted duplications (or inversions) with their planted pairs: PE in both FILEs"""
    refs, rd, _ = pk.planted_dup_reads() if svtype == "DUP" else pk.planted_inv_reads()
    d = pk.write_planted(str(tmp_path), refs, rd)
    _, dup_pe, dup_found = pk.render_of_bam("DUP", d + "/aln.bam", d + "/ref.fa", 10)
    _, inv_pe, inv_found = pk.render_of_bam("INV", d + "/aln.bam", d + "/ref.fa", 10)
    found = dup_found if svtype == "DUP" else inv_found
    assert [f[4] for f in found] == [0] * (len(found) * 5 // 9) + [3] * (len(found) * 4 // 9) and len(found) in (9, 18)
    both_runs(lambda s: BASE + ["-G", "-C", "-V", "-I", "i_%s" % s, "-U", "u_%s" % s, "-N", "n_%s" % s, "-M"], d)
    assert read(d, "u_own") == dup_pe == read(d, "u_default") and read(d, "n_own") == inv_pe == read(d, "n_default")
    assert read(d, "i_own") == read(d, "i_default")


def test_genotypes_pairs_and_depth_on_own_streams(tmp_path):
    """-G -P -D over the two-contig composite sample: without what the three options add the output is the committed golden; the
    reference-spanning counts, the concordant-pair counts and the depth medians are the restatements' values, record by record"""
    from tests import test_gpu_depth_evidence as de
    from tests import test_gpu_pairspan as ps
    from tests import test_gpu_span as sp
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    d = str(tmp_path)
    mg.write_dataset(d, mg.SYNTH_E2E["synth_2ctg_composite"])
    bam = os.path.join(d, "aln.bam")
    names, depth = de.depth_of_bam(bam)
    _, pspan = ps.pspan_of_bam(bam, 10, 10, ps.GENERIC)
    # as the golden was made: split-read and composite records
    _, own = both_runs(lambda s: ["-i", "cfg.txt", "-G", "-P", "-D"], d)
    assert ps.strip_columns(de.strip_evidence(own.stdout)) == _golden("synth_2ctg_composite")
    # with -s 100 the large deletions are PAIRED_READ records: the concordant-pair counts
    _, own_s = both_runs(lambda s: BASE + ["-G", "-P", "-D"], d)
    refs, recs = sp.read_bam_records(bam)
    span = sp.span_of(recs, [n for _, n in refs], 10, 10)
    n_paired = n_others = 0
    for out in (own.stdout, own_s.stdout):
        de.check_header(out, True)
        seen, kinds = de.check_records(out, names, depth)
        assert len(seen) >= 5 and {"short", "insertion"} <= kinds, kinds
        bare = de.strip_evidence(out)                       # the GT:AD:GQ columns alone, as the two restatements below read them
        n_paired += len(ps.check_paired_columns(bare, names, pspan))
        for cols in ps.records_of(bare):
            if ps.is_paired(cols):
                continue
            info = dict(kv.split("=") for kv in cols[7].split(";") if "=" in kv)
            pos, end, bp_end, ns = int(cols[1]), int(info["END"]), int(info["BP_END"]), int(info["NS"])
            rs = int(span[names.index(cols[0])][pos:pos + (bp_end - end) + 1].min())
            gt, gq = genotype_of(rs, ns)
            assert cols[8] == "GT:AD:GQ" and cols[9] == "%s:%d,%d:%d" % (gt, rs, ns, gq), (cols, rs)
            n_others += 1
    assert n_paired >= 5 and n_others > 200
