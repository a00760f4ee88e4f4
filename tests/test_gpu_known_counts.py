"""-A as a whole program: annotate mode with GT:AD:GQ per known indel.  Everything printed without -A is printed unchanged, and
every column equals the restatement (tests/support/knowncounts.py) computed from the sample's BAM."""
import importlib.util
import os
import subprocess
import types

import numpy as np
import pytest

from tests.support import knowncounts as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TD = os.path.join(GOLD, "test_data")


def _product():
    from indelminer_amd import build
    build.build()
    return build.build_host()


def _golden(name):
    return open(os.path.join(GOLD, "vcf", name + ".vcf"), "rb").read()


def _run(flags, cwd, ref, vcf, bam, sample="normal", env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([_product()] + flags + [ref, vcf, sample + "=" + bam], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


@pytest.fixture(scope="module")
def synth_tn(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tn"))
    mg = _make_golden()
    mg.write_dataset(d, mg.SYNTH_TN["normal"], "normal_")
    return d


TN_FLAGS = ["-i", "cfg.txt", "-q", "0", "-a", "-e", "1"]
TN_VCF = os.path.join(GOLD, "vcf", "synth_tn_tumor.vcf")


def test_product_known_counts_tumour_normal(synth_tn):
    """SYNTH_TN.  By the restatement's own count this pair has 14 records with RS > 0 and AS > 0 (the simulator's normal carries
    every germline indel on all its reads): the assertion on 100 such records is made on a pair that has them, in
    test_product_known_counts_heterozygous_normal."""
    r = _run(TN_FLAGS + ["-A"], synth_tn, "ref.fa", TN_VCF, "normal_aln.bam")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert kc.strip_columns(r.stdout) == _golden("synth_tn_annotate")
    rs = kc.Restatement(os.path.join(synth_tn, "normal_aln.bam"), os.path.join(synth_tn, "ref.fa"), 10, 0)
    res = kc.check_output(r.stdout, rs, "normal")
    assert len(res) == 305 and sum(k.tagged for k, _ in res) == 296
    for k, c in res:
        if c is None:
            continue
        assert not (k.evd == "SPLIT_READ" and not k.tagged) or c["AS"] == 0, (k.start, c)
        assert c["AS"] == 0 or k.tagged, (k.start, c)
    # the record-at-a-time path prints the same bytes
    h = _run(TN_FLAGS + ["-A"], synth_tn, "ref.fa", TN_VCF, "normal_aln.bam", env={"INDELMINER_PIPELINE": "host"})
    assert h.returncode == 0 and h.stdout == r.stdout
    # -q 30: the columns follow, the tags stay
    r30 = _run(["-i", "cfg.txt", "-q", "30", "-a", "-e", "1", "-A"], synth_tn, "ref.fa", TN_VCF, "normal_aln.bam")
    assert r30.returncode == 0, r30.stderr.decode()[-2000:]
    p30 = _run(["-i", "cfg.txt", "-q", "30", "-a", "-e", "1"], synth_tn, "ref.fa", TN_VCF, "normal_aln.bam")
    assert kc.strip_columns(r30.stdout) == p30.stdout
    rs30 = kc.Restatement(os.path.join(synth_tn, "normal_aln.bam"), os.path.join(synth_tn, "ref.fa"), 10, 30)
    kc.check_output(r30.stdout, rs30, "normal")
    # without -A: the parent's bytes
    assert _run(TN_FLAGS, synth_tn, "ref.fa", TN_VCF, "normal_aln.bam").stdout == _golden("synth_tn_annotate")


def test_product_known_counts_heterozygous_normal(tmp_path):
    """a normal that carries half of its reads without the tumour's further indels: at least 100 records have reads for the
    reference (RS > 0) and reads for the indel (AS > 0)"""
    from indelminer_amd import bamwrite, synth
    kw = dict(seed=6, ref_len=300_000, coverage=15, n_contigs=2)
    refs, a = synth.simulate(**kw)
    refs_b, b = synth.simulate(read_seed=77, somatic_spacing=2_500, **kw)
    rd = synth.Reads()
    order = np.lexsort((np.concatenate([a.pos, b.pos]), np.concatenate([a.tid, b.tid])))
    for f in ("tid", "pos", "flag", "mpos", "isize", "seq", "cig_op", "cig_len", "ncig", "mate_first"):
        setattr(rd, f, np.concatenate([getattr(a, f), getattr(b, f)])[order])
    rd.pair_id = np.concatenate([a.pair_id, b.pair_id + int(a.pair_id.max()) + 1])[order]
    rd.n, rd.read_len, rd.range_max, rd.mapq = a.n + b.n, a.read_len, a.range_max, a.mapq
    contigs = [("ctg%d" % i, len(x)) for i, x in enumerate(refs)]
    d = str(tmp_path)
    bamwrite.write_fasta(d + "/ref.fa", contigs, refs)
    bamwrite.write_bam(d + "/mixed.bam", contigs, rd)
    bamwrite.write_bam(d + "/tumor.bam", contigs, b)
    open(d + "/cfg.txt", "w").write("IL generic 300 700\n")
    t = subprocess.run([_product(), "-i", "cfg.txt", "ref.fa", "t=tumor.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert t.returncode == 0, t.stderr.decode()[-2000:]
    open(d + "/tumor.vcf", "wb").write(t.stdout)
    plain = _run(TN_FLAGS, d, "ref.fa", "tumor.vcf", "mixed.bam")
    r = _run(TN_FLAGS + ["-A"], d, "ref.fa", "tumor.vcf", "mixed.bam")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert kc.strip_columns(r.stdout) == plain.stdout
    res = kc.check_output(r.stdout, kc.Restatement(d + "/mixed.bam", d + "/ref.fa", 10, 0), "normal")
    both = sum(1 for _, c in res if c is not None and c["RS"] > 0 and c["AS"] > 0)
    assert both >= 100, (both, len(res))


def test_product_known_counts_test_data():
    """the `annotate` golden was made from the golden default_config.vcf (tests/test_host_driver.py); indelminer.expected.vcf holds
    the same records with another order of the BF= flanks, which annotate mode echoes: its run is compared with its own plain run"""
    flags = ["-i", "indelminer.config", "-q", "0", "-a", "-e", "1"]
    rs = kc.Restatement(os.path.join(TD, "alignments.bam"), os.path.join(TD, "reference.fa"), 10, 0)
    r = _run(flags + ["-A"], TD, "reference.fa", os.path.join(GOLD, "vcf", "default_config.vcf"), "alignments.bam")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert kc.strip_columns(r.stdout) == _golden("annotate")
    assert len(kc.check_output(r.stdout, rs, "normal")) > 5
    e = _run(flags + ["-A"], TD, "reference.fa", "indelminer.expected.vcf", "alignments.bam")
    assert e.returncode == 0, e.stderr.decode()[-2000:]
    assert kc.strip_columns(e.stdout) == _run(flags, TD, "reference.fa", "indelminer.expected.vcf", "alignments.bam").stdout
    kc.check_output(e.stdout, rs, "normal")
    assert [ln.split("\t")[9] for ln in e.stdout.decode().split("\n") if ln and ln[0] != "#"] == \
           [ln.split("\t")[9] for ln in r.stdout.decode().split("\n") if ln and ln[0] != "#"]


# ------------------------------------------------------------------------------------------ a hand-made sample

L = 100
POS, DLEN = 5000, 7                      # the known deletion: VCF POS 5000, END 5008


def _hand_made(d, n_first):
    """reads around one known deletion ref[5000, 5007) on a random contig.  n_first: the read with an N operation comes first"""
    from indelminer_amd import bamwrite
    rng = np.random.default_rng(5)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), 12_000)
    ref[POS - 1] = ord("A"); ref[POS:POS + DLEN] = np.frombuffer(b"CGTACGT", np.uint8); ref[POS + DLEN] = ord("A")      # no other placement of the deletion
    alt_allele = np.concatenate([ref[:POS], ref[POS + DLEN:]])
    reads = []                           # (pos, cigar [(len, op)], bases, flag, mapq)

    def from_alt(start, cigar, flag=0, mapq=60):
        """a read of the sample's indel allele, placed by the aligner with `cigar`"""
        reads.append((start, cigar, alt_allele[start:start + L].copy(), flag, mapq))
    if n_first:
        reads.append((POS - 99, [(40, 0), (10, 3), (60, 0)], ref[POS - 99:POS - 59].tolist() + ref[POS - 49:POS + 11].tolist(), 0, 60))
    # the aligner pushed these across the breakpoint with mismatches: 100M over the deletion, the tail shifted by 7
    for off in (84, 86, 88, 90):                                   # each ends behind BP_END and spans POS with 10 bases on both sides
        from_alt(POS - off, [(L, 0)])
    from_alt(POS - 89, [(L, 0)], mapq=3)                           # a low-MAPQ supporter: in N_all, not in AS
    from_alt(POS - 60, [(60, 0), (DLEN, 2), (40, 0)])              # carries the D
    from_alt(POS - 50, [(50, 0), (DLEN, 2), (50, 0)])
    from_alt(POS - 87, [(L, 0)], flag=0x800)                       # supplementary: not considered
    if not n_first:
        reads.append((POS - 40, [(30, 0), (10, 3), (70, 0)], ref[POS - 40:POS - 10].tolist() + ref[POS:POS + 70].tolist(), 0, 60))
    for off in (70, 55, 35, 30):                                   # reads of the reference allele
        reads.append((POS - off, [(L, 0)], ref[POS - off:POS - off + L].copy(), 0, 60))
    reads.sort(key=lambda r: r[0])
    if n_first:
        assert reads[0][1][1][1] == 3
    rd = types.SimpleNamespace()
    rd.n, rd.read_len, rd.mapq, rd.rg_names = len(reads), L, 60, None
    rd.tid = np.zeros(rd.n, np.int32); rd.pos = np.array([r[0] for r in reads], np.int32)
    rd.flag = np.array([r[3] for r in reads], np.int32)
    rd.mpos = rd.pos.copy(); rd.isize = np.zeros(rd.n, np.int32); rd.pair_id = np.arange(rd.n)
    rd.seq = [np.asarray(r[2], np.uint8) for r in reads]
    rd.ncig = np.array([len(r[1]) for r in reads], np.int32)
    rd.cig_len = np.zeros((rd.n, 4), np.int32); rd.cig_op = np.zeros((rd.n, 4), np.int32)
    for i, r in enumerate(reads):
        for j, (ln, op) in enumerate(r[1]):
            rd.cig_len[i, j], rd.cig_op[i, j] = ln, op
    rd.overrides = {i: {"mapq": r[4]} for i, r in enumerate(reads)}
    contigs = [("c", len(ref))]
    bamwrite.write_fasta(d + "/ref.fa", contigs, [ref])
    bamwrite.write_bam(d + "/s.bam", contigs, rd)
    open(d + "/cfg.txt", "w").write("IL generic 300 700\n")
    refstr = bytes(ref[POS - 1:POS + DLEN]).decode()
    open(d + "/known.vcf", "w").write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                                      "c\t%d\t.\t%s\t%s\t.\t.\tDELETION;SPLIT_READ;NS=9;END=%d;BP_END=%d;NFS=5;NRS=4;UTAILS=9;MQ=60;MQ30=9;DF=0;DP=20;BF=50,50\n"
                                      % (POS, refstr, refstr[0], POS + DLEN + 1, POS + DLEN + 1))


def test_product_known_counts_hand_made_sample(tmp_path):
    d = str(tmp_path)
    _hand_made(d, n_first=False)
    flags = ["-i", "cfg.txt", "-q", "10"]
    plain = _run(flags, d, "ref.fa", "known.vcf", "s.bam", sample="s")
    r = _run(flags + ["-A"], d, "ref.fa", "known.vcf", "s.bam", sample="s")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert plain.returncode == 0 and kc.strip_columns(r.stdout) == plain.stdout
    (k, c), = kc.check_output(r.stdout, kc.Restatement(d + "/s.bam", d + "/ref.fa", 10, 10), "s")
    assert k.tagged and not c["aborts"]
    # 4 pushed reads + the low-MAPQ one + 2 with the D; the span array holds the 4 pushed reads, the supplementary one and the 4
    # reads of the reference allele at POS
    assert c["DC"] == 4 and c["N_all"] == 7 and c["AS"] == 6 and c["RS"] == 5, c
    h = _run(flags + ["-A"], d, "ref.fa", "known.vcf", "s.bam", sample="s", env={"INDELMINER_PIPELINE": "host"})
    assert h.returncode == 0 and h.stdout == r.stdout


def test_product_known_counts_dies_where_the_reference_would(tmp_path):
    d = str(tmp_path)
    _hand_made(d, n_first=True)
    flags = ["-i", "cfg.txt", "-q", "10"]
    plain = _run(flags, d, "ref.fa", "known.vcf", "s.bam", sample="s")
    r = _run(flags + ["-A"], d, "ref.fa", "known.vcf", "s.bam", sample="s")
    assert plain.returncode != 0 and r.returncode != 0
    assert b"Implement new_readseg_bam:164" in plain.stderr and b"Implement new_readseg_bam:164" in r.stderr
    k = kc.read_known(open(d + "/known.vcf").read())[0]
    assert kc.Restatement(d + "/s.bam", d + "/ref.fa", 10, 10).counts(k)["aborts"]
