"""Split junctions (-J): the sweep, count and peak kernels of im_links.hip behind im_splitlink_junctions, and what the host driver makes
of them (FILE).

The yardstick is the plain restatement in tests/support/splitjunctions.py, written from the rule in include/indelminer_amd.h (seam 5,
"Split junctions"), not from the code under test; tests/test_splitjunction_host.py pins it to cases worked by hand.  Every answer is
compared exactly.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu

IM_OK, IM_E_ARG = 0, -1                          # include/indelminer_amd.h
W, SPAN, LINKS = sj.WINDOW, sj.MIN_SPAN, sj.MIN_LINKS


def contigs(clens, seed=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in clens]


class Device:
    """one context over contigs of these lengths with the split-link table enabled"""

    def __init__(self, clens, log2_slots=13, enable=True):
        from indelminer_amd import capi
        self.capi, self.clens = capi, clens
        self.ctx = capi.Context(0)
        self.ctx.set_reference(contigs(clens))
        if enable:
            self.ctx.splitlink_enable(sl.MIN_CLIP, sl.MIN_MAPQ, log2_slots, ["c%d" % t for t in range(len(clens))])

    def add(self, links):
        self.ctx.splitlink_add(*[[x[k] for x in links] for k in range(6)])

    def reset(self):
        self.ctx.splitlink_reset(self.ctx.stream)

    def junctions(self, window=W, min_links=LINKS, min_span=SPAN, cap=65536):
        out = self.ctx.splitlink_junctions(window, min_links, min_span, cap)
        return None if out is None else [tuple(int(col[i]) for col in out) for i in range(len(out[0]))]

    def raw(self, window, min_links, min_span, cap, null=None, no_found=False):
        """the entry itself: (return code, found, the nine columns as given back), columns of `cap` sentinels; null: a column left out"""
        kinds = self.capi.Context._JUNCTIONS
        cols = [np.full(max(cap, 1), 77, dtype=k) for k in kinds]
        found = C.c_int32(-99)
        ptrs = [None if k == null else c.ctypes.data_as(C.c_void_p) for k, c in enumerate(cols)]
        rc = self.capi.lib().im_splitlink_junctions(self.ctx.h, window, min_links, min_span, cap, *ptrs, None if no_found else C.byref(found))
        return rc, found.value, cols

    def count(self, queries):
        return [int(v) for v in self.ctx.splitlink_count(*[[q[k] for q in queries] for k in range(8)])]

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def hand_device():
    dev = Device(sj.HAND_CLENS)
    yield dev
    dev.close()


@pytest.mark.parametrize("case", sj.HAND, ids=[c[0] for c in sj.HAND])
def test_cases_worked_by_hand(hand_device, case):
    """every case of tests/test_splitjunction_host.py, on one table that is reset in between; the links in the order given, reversed,
    and in three add calls"""
    name, links, kw, want = case
    dev = hand_device
    for order in (links, links[::-1]):
        dev.reset()
        dev.add(order)
        assert dev.ctx.splitlink_stats() == (len(links), 0)
        assert dev.junctions(**kw) == want
    dev.reset()
    for part in (links[0::3], links[1::3], links[2::3]):
        if part:
            dev.add(part)
    assert dev.junctions(**kw) == want
    dev.reset()
    assert dev.ctx.splitlink_stats() == (0, 0) and dev.junctions(**kw) == []


def test_all_hand_cases_of_the_drivers_parameters_in_one_table(hand_device):
    """the cases that use the driver's parameters stand far enough apart to share a table: the union of their links answers the union of
    their junctions, whatever the order"""
    dev = hand_device
    pick = [c for c in sj.HAND if not c[2]]
    pick = [pick[4]] + pick[6:]                                         # the first six stand on one site: one of them
    links = [l for _, ls, _, _ in pick for l in ls]
    want = sj.junctions(links, sj.HAND_CLENS)
    assert len(want) >= 9
    rng = np.random.default_rng(5)
    for _ in range(2):
        dev.reset()
        dev.add([links[i] for i in rng.permutation(len(links))])
        assert dev.junctions() == want


def test_a_64_slot_table_whose_probe_runs_wrap():
    clens = [200_000, 70_000, 9_000]
    dev = Device(clens, log2_slots=6)
    try:
        # the runs of both kinds of a junction start in the table's last slots: the links one way, their reverses, a neighbour
        found = [(b, b2) for b in range(3, 200) for b2 in range(3, 200) if sl.home_slot(0, b, 2, 6) >= 60 and sl.home_slot(1, b2, 1, 6) >= 60][:1]
        assert found
        b, b2 = found[0]
        a = (0, 256 * b + 40, 0, 1, 256 * b2 + 50, 1)
        near = (0, 256 * b + 45, 0, 1, 256 * b2 + 50, 1)
        links = [a] * 9 + [sj.rev(a)] * 8 + [near] * 6 + [sj.rev(near)] * 5 + [(2, 100, 1, 2, 4_000, 1)] * 3
        assert len(links) == 31
        dev.add(links)
        assert dev.ctx.splitlink_stats() == (31, 0)
        want = sj.junctions(links, clens)
        assert want == [a + (17, 15, 13), (2, 100, 1, 2, 4_000, 1, 3, 3, 0)]
        assert dev.junctions() == want
        # one more than half of the slots: no answer, not a wrong one
        dev.add([(0, 5, 0, 1, 5, 1)] * 2)
        assert dev.ctx.splitlink_stats() == (32, 1)
        assert dev.junctions() is None
        rc, n, cols = dev.raw(W, LINKS, SPAN, 4)
        assert (rc, n) == (IM_OK, -1) and all((c == 77).all() for c in cols)
        dev.reset()
        assert dev.junctions() == []
        dev.add(links[:20])
        assert dev.junctions() == sj.junctions(links[:20], clens)
    finally:
        dev.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_one_tuple_held_by_many_links(n):
    """a probe run that spans several batches of a walk: E and the counts of a tuple held by n links, n // 3 of them the other way
    round, beside a neighbour of one link in the same bucket and a junction of another bucket"""
    clens = [100_000, 50_000]
    dev = Device(clens, log2_slots=10)
    try:
        a = (0, 30_000, 1, 1, 20_000, 0)
        links = [a] * (n - n // 3) + [sj.rev(a)] * (n // 3) + [(0, 30_010, 1, 1, 20_000, 0)] + [(0, 29_950, 1, 1, 19_990, 0)] * 4
        rng = np.random.default_rng(n)
        links = [links[i] for i in rng.permutation(len(links))]
        dev.add(links)
        want = sj.junctions(links, clens, min_links=1)
        assert want == [(0, 29_950, 1, 1, 19_990, 0, 4, 4, 0), a + (n, n - n // 3 + 1, n // 3)]
        assert dev.junctions(min_links=1) == want
        assert dev.junctions() == sj.junctions(links, clens)
    finally:
        dev.close()


def test_cap_one_too_small_then_the_retry_and_the_arguments():
    clens = [100_000, 50_000]
    dev = Device(clens, log2_slots=10)
    try:
        links = [(0, 1_000 * k, 0, 1, 500 * k, 1) for k in range(1, 8) for _ in range(3)]
        dev.add(links)
        want = sj.junctions(links, clens)
        assert len(want) == 7
        rc, n, cols = dev.raw(W, LINKS, SPAN, 6)
        assert (rc, n) == (IM_OK, 7) and all((c == 77).all() for c in cols)        # nothing is written; the caller asks again
        assert dev.junctions(cap=6) == want
        rc, n, cols = dev.raw(W, LINKS, SPAN, 7)
        assert (rc, n) == (IM_OK, 7) and [tuple(int(c[i]) for c in cols) for i in range(7)] == want
        rc, n, cols = dev.raw(W, LINKS, SPAN, 0, null=3)
        assert (rc, n) == (IM_OK, 7)                                               # cap 0 asks for the number alone
        assert dev.raw(W, 50, SPAN, 0)[:2] == (IM_OK, 0)
        # every argument error, with its message
        err = lambda: dev.capi.lib().im_last_error(dev.ctx.h).decode()
        for args, what in (((-1, LINKS, SPAN, 8), "window -1"), ((256, LINKS, SPAN, 8), "window 256"), ((W, 0, SPAN, 8), "min_links 0"),
                           ((W, LINKS, -1, 8), "min_span -1"), ((W, LINKS, SPAN, -1), "cap -1")):
            rc, n, _ = dev.raw(*args)
            assert rc == IM_E_ARG and n == -99 and what in err(), (args, err())
        for k in range(9):
            assert dev.raw(W, LINKS, SPAN, 8, null=k)[0] == IM_E_ARG and "null column" in err()
        assert dev.raw(W, LINKS, SPAN, 8, no_found=True)[0] == IM_E_ARG and "found is null" in err()
        assert dev.raw(255, 1, 0, 8)[0] == IM_OK
        assert dev.capi.lib().im_splitlink_junctions(None, W, LINKS, SPAN, 0, *[None] * 10) == IM_E_ARG
    finally:
        dev.close()
    cold = Device(clens, enable=False)
    try:
        with pytest.raises(cold.capi.IMError, match="im_splitlink_enable has not been called"):
            cold.junctions()
    finally:
        cold.close()


def soak_links(rng, clens, n=20_000, n_hot=300):
    """n links on n_hot hot ends: every hot end has three partners, nine links in ten name the two hot positions to the base and the
    tenth is up to 40 bases off at either end, one link in three is stored from the far end"""
    hot = [(int(t), int(rng.integers(0, clens[t] + 1)), int(rng.integers(0, 2))) for t in rng.integers(0, len(clens), n_hot)]
    hot[:4] = [(0, 0, 1), (0, clens[0], 0), (1, 255, 0), (1, 256, 1)]
    partners = [[int(x) for x in rng.integers(0, n_hot, 3)] for _ in range(n_hot)]
    links = []
    for _ in range(n):
        i = int(rng.integers(0, n_hot))
        (ta, pa, sa), (tb, pb, sb) = hot[i], hot[partners[i][int(rng.integers(0, 3))]]
        if rng.random() < 0.1:
            pa, pb = pa + int(rng.integers(-40, 41)), pb + int(rng.integers(-40, 41))
        pa, pb = min(max(pa, 0), clens[ta]), min(max(pb, 0), clens[tb])
        l = (ta, pa, sa, tb, pb, sb)
        links.append(sj.rev(l) if rng.random() < 0.33 else l)
    return links


@pytest.fixture(scope="module")
def soak():
    rng = np.random.default_rng(2025)
    clens = [150_000, 90_000, 40_000]
    links = soak_links(rng, clens)
    dev = Device(clens, log2_slots=16)
    for k in range(0, len(links), 7_000):
        dev.add(links[k:k + 7_000])
    yield dev, clens, links
    dev.close()


def test_seeded_soak_against_the_restatement(soak):
    """20 000 links on 300 hot ends over 3 contigs, with the driver's parameters and with the widest window, no span and no threshold"""
    dev, clens, links = soak
    assert dev.ctx.splitlink_stats() == (len(links), 0)
    want = sj.junctions_fast(links, clens)
    assert 500 <= len(want) <= 1_200 and {(j[2], j[5]) for j in want} == {(0, 0), (0, 1), (1, 0), (1, 1)} and max(j[6] for j in want) >= 20
    assert any(j[0] == j[3] for j in want) and any(j[7] > 0 and j[8] > 0 for j in want)
    assert dev.junctions() == want
    wide = sj.junctions_fast(links, clens, window=255, min_links=1, min_span=0)
    assert len(wide) < len(want) and dev.junctions(255, 1, 0) == wide
    assert dev.junctions(0, 1, SPAN, cap=16) == sj.junctions_fast(links, clens, window=0, min_links=1)


def test_n1_and_n2_of_every_junction_are_two_count_queries(soak):
    dev, clens, links = soak
    found = dev.junctions()
    q1 = [(t1, s1, p1 - W, p1 + W, t2, s2, p2 - W, p2 + W) for t1, p1, s1, t2, p2, s2, _, _, _ in found]
    q2 = [(t2, s2, p2 - W, p2 + W, t1, s1, p1 - W, p1 + W) for t1, p1, s1, t2, p2, s2, _, _, _ in found]
    assert dev.count(q1) == [j[7] for j in found] and dev.count(q2) == [j[8] for j in found] and len(found) > 100


# ------------------------------------------------------------------------------------------ the product

def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r


def _err(r):
    """stderr without the whole seconds of its time stamps, which differ between two runs that straddle a second"""
    return re.sub(rb" : \d+ sec\. elapsed\n", b"\n", r.stderr)


BASE = ["-i", "cfg.txt", "-s", "100"]
ENVS = ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})


@pytest.mark.parametrize("kind", ["DUP", "INV", "BND"])
def test_product_file_on_the_planted_data_sets(kind, tmp_path):
    """the planted data sets of -U, -N and -T with the tags a split aligner would have written: FILE byte for byte the restatement's,
    alone and behind the whole chain, on the pipelined path, on the record-at-a-time path and with three walkers; stdout and the other
    FILEs what they are without -J"""
    mod, refs, rd, names, tally = sl.planted(kind)
    d = mod.write_planted(str(tmp_path), refs, rd)
    want, found = sj.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    assert len(found) >= 7 and want.count(b"\n") == sj.HEADER.count("\n") + len(found) and all(j[6] >= 3 and j[7] + j[8] >= j[6] for j in found)
    prod = _product()
    path = lambda name: str(tmp_path / name)
    read = lambda name: open(path(name), "rb").read()
    chain = lambda k: ["-G", "-C", "-V", "-U", path("u%d" % k), "-N", path("n%d" % k), "-T", path("t%d" % k), "-M", "-S"]
    r0 = _ok(_run(prod, BASE + chain(0), d))
    r1 = _ok(_run(prod, BASE + chain(1) + ["-J", path("j1")], d))
    assert read("j1") == want
    assert r1.stdout == r0.stdout and _err(r1) == _err(r0) and (read("u1"), read("n1"), read("t1")) == (read("u0"), read("n0"), read("t0")) and len(r0.stdout) > 1000
    g0 = _ok(_run(prod, BASE + ["-G"], d))
    g1 = _ok(_run(prod, BASE + ["-G", "-J", path("j2")], d))
    assert read("j2") == want and g1.stdout == g0.stdout and _err(g1) == _err(g0)
    for k, env in enumerate(ENVS, 3):
        r = _ok(_run(prod, BASE + ["-G", "-J", path("j%d" % k)], d, env=env))
        assert read("j%d" % k) == want and r.stdout == g0.stdout, env


def test_product_an_insertion_at_the_junction_is_in_this_file_and_in_no_other(tmp_path):
    """split reads whose clipped bases are random: -T's FILE has no record at the site, -J's has the one"""
    ic, refs, rd, names, site = sj.planted_insertion()
    d = ic.write_planted(str(tmp_path), refs, rd)
    want, found = sj.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    assert len(found) == 1 and found[0][:6] == site
    prod = _product()
    t, j = str(tmp_path / "t"), str(tmp_path / "j")
    _ok(_run(prod, BASE + ["-G", "-C", "-V", "-T", t, "-J", j], d))
    at = b"\nctg%d\t%d\t" % (site[0], site[1])
    bnd = open(t, "rb").read()
    assert open(j, "rb").read() == want and at in want and at not in bnd and bnd == ic.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)[0]
    assert bnd.count(b"\nctg") == len(ic.SITES)                             # -T's own sites are all there


def test_product_detailed_output_ignores_the_option(tmp_path):
    mod, refs, rd, _, _ = sl.planted("DUP")
    d = mod.write_planted(str(tmp_path), refs, rd)
    prod = _product()
    fo = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-J", fo], d))
    assert d1.stdout == d0.stdout and _err(d1) == _err(d0) and len(d0.stdout) > 0 and not os.path.exists(fo)
    r = _run(prod, BASE + ["-J", fo], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -J needs -G\n" and not os.path.exists(fo)


def test_product_after_an_overflow_of_the_split_link_table(tmp_path):
    """2 100 more split reads than the planted ones against the 2 048 links the table of a small BAM keeps: FILE holds its header alone
    and stderr says so once, at the end"""
    from indelminer_amd import synth
    mod, refs, rd, names, _ = sl.planted("DUP")
    plain = np.nonzero((rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & 0x4) == 0) & (rd.pos > 200) & (rd.pos < 50_000))[0]
    for i in plain[::3][:2_100]:
        i = int(i)
        rd.cig_op[i, :2] = (synth.OP_M, synth.OP_S); rd.cig_len[i, :2] = (70, 30); rd.ncig[i] = 2
        mq = 0 if int(rd.flag[i]) & 0x8 else int(rd.mapq)
        rd.overrides[i] = {"tags": b"MQC" + bytes([mq]) + sl.sa("ctg0,%d,%s,70S30M,60,0;" % (int(rd.pos[i]) + 5_001, "-" if int(rd.flag[i]) & 0x10 else "+"))}
    d = mod.write_planted(str(tmp_path), refs, rd)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    _, clens, links = sl.links_of_bam(bam, sl.MIN_CLIP, 10)
    assert len(links) >= 2_100 and os.path.getsize(bam) < 64 << 16
    prod = _product()
    f = str(tmp_path / "j")
    r0 = _ok(_run(prod, BASE + ["-G"], d))
    r1 = _run(prod, BASE + ["-G", "-J", f], d)
    assert r1.returncode == 0 and open(f, "rb").read() == sj.HEADER.encode() == sj.render_of_bam(bam, fa, 10, overflowed=True)[0]
    line = b"indelminer: -J: the split-link table overflowed (2048 links stored, %d dropped): its file has no records\n" % (len(links) - 2_048)
    assert r1.stdout == r0.stdout and _err(r1) == _err(r0) + line
