"""The batches of tests/support/recordbounds.py are what they claim (CPU only): reads whose oracle result sits at an exact
distance from the result record's bounds (IM_MAX_OPS = 64 segment words, IM_MAX_EV = 4 evidence records), on both sides, per
realign route.  tests/test_gpu_record_bounds.py runs the same batches through the kernels."""
import pytest

from tests.support import gpucmp, recordbounds as rb

ROUTES = sorted(rb.ROUTES)


@pytest.mark.parametrize("name", ROUTES)
def test_every_class_is_present(name):
    B = rb.select(name)
    msg = rb.report(B)
    assert not B.missing, "classes short of their count (found, wanted) %r -- %s" % (B.missing, msg)
    for label, pred, want, need in rb.ROUTES[name]["classes"]:
        got = [i for c, i in zip(B.cases, B.info) if c["label"] == label]
        assert need <= len(got) <= want and all(pred(i) for i in got), (label, len(got), msg)
    assert 100 <= len(B.cases) <= 250 and 60000 <= len(B.contig) <= 80000, msg
    bound = sum(c["label"] is not None for c in B.cases)
    assert bound and len(B.cases) - bound >= bound, msg         # at least as many ordinary reads as bound reads
    assert 1000 <= B.n_candidates <= 4000 or name == "any_g8", msg      # any_g8: nearly every candidate yields (402 of 460)


@pytest.mark.parametrize("name", ROUTES)
def test_no_chosen_read_is_ambiguous(name):
    """a read whose final list fits while a piece's CIGAR is beyond IM_MAX_OPS: the rule gives no answer for it, the selector
    rejects and counts it"""
    B = rb.select(name)
    n = sum(i.ambiguous for i in B.info)
    assert n == 0, "%d ambiguous reads chosen -- %s" % (n, rb.report(B))
    assert all(gpucmp.expected_status(i.st, i.res) is not None for i in B.info), rb.report(B)


@pytest.mark.parametrize("name", ROUTES)
def test_the_bound_each_route_can_reach(name):
    """which bound the candidates of a route get beyond: reads of up to 255 bases stay far below 64 segments (a list grows by
    at most 2 words per ~12 bases), numgaps == 0 leaves one indel per read"""
    B = rb.select(name)
    msg = rb.report(B)
    if "ops" in B.reaches:
        assert B.densest > rb.MAX_OPS, msg
    else:
        assert 11 <= B.densest < 40, "densest list of %d candidates: %d segments -- %s" % (B.n_candidates, B.densest, msg)
    if name in ("short", "band_g2", "band_g8", "band_g60", "any_g61"):      # the routes of reads up to 255 bases
        assert max(len(c["read"]) for c in B.cases) <= 255 and "ops" not in B.reaches and B.densest >= 19, msg
    if "ev" in B.reaches:
        assert B.densest_ev > rb.MAX_EV, msg
    else:
        assert B.densest_ev == (1 if B.kw["numgaps"] == 0 else 2), msg


@pytest.mark.parametrize("name", ["long_k6", "long_k9"])
def test_long_read_route_takes_both_length_families(name):
    B = rb.select(name)
    lens = [len(c["read"]) for c in B.cases if c["label"]]
    assert 1020 in lens and min(lens) <= 600 and max(lens) == 1020, (sorted(lens), rb.report(B))


@pytest.mark.parametrize("name", ROUTES)
def test_overflow_reads_at_both_ends(name):
    """a route with overflow classes opens and closes its batch with an overflow read: ops[] is the record's last field, a write
    behind it lands in the next record -- or, for the last read, behind the results"""
    B = rb.select(name)
    if any(i.overflow for i in B.info):
        assert B.info[0].overflow and B.info[-1].overflow, rb.report(B)
    else:
        assert name == "short"


@pytest.mark.parametrize("name", ROUTES)
def test_shim_rule_and_gpucmp_rule_agree(name):
    """the CPU shim's rule (tests/shim/im_shim.c, im_realign_batch) and gpucmp.expected_status give every chosen read the same
    status; a rule off by one at either bound does not (which is what makes the classes sit AT the bounds)"""
    B = rb.select(name)
    msg = rb.report(B)
    want = [gpucmp.expected_status(i.st, i.res) for i in B.info]
    assert [rb.shim_status(i) for i in B.info] == want, msg
    # the bound a variant of the rule holds instead, and the reads that alone tell it from the rule
    variants = {"n_ops > 63": ((63, 4), lambda i: i.n_ops == 64 and i.n_ev <= 4), "n_ops > 65": ((65, 4), lambda i: i.n_ops == 65 and i.n_ev <= 4),
                "n_ev > 3": ((64, 3), lambda i: i.n_ev == 4 and i.n_ops <= 64), "n_ev > 5": ((64, 5), lambda i: i.n_ev == 5 and i.n_ops <= 64)}
    caught = set()
    for v, ((max_ops, max_ev), tells) in variants.items():
        differs = [rb.shim_status(i, max_ops, max_ev) for i in B.info] != want
        assert differs == any(tells(i) for i in B.info), (v, msg)
        if differs:
            caught.add(v)
    must = {"": set(), "ops": {"n_ops > 65"} if name == "any_g3" else {"n_ops > 63", "n_ops > 65"}, "ev": {"n_ev > 3", "n_ev > 5"}}[B.reaches]
    assert must <= caught, (must - caught, msg)


def test_the_restated_shim_rule_is_the_shims():
    """recordbounds.shim_status restates one line of tests/shim/im_shim.c (the shim is a program, not a library): that line is
    still there; tests/test_host_driver.py runs the shim itself over a read of 65 segments"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "im_shim.c")).read()
    assert "if (r->n_ops > IM_MAX_OPS || r->n_ev > IM_MAX_EV) { o->status = IM_ST_OVERFLOW; worst = IM_E_OVERFLOW;" in src
    assert "o->status = st == IMO_OK ? IM_ST_EVIDENCE : st == IMO_NONE ? IM_ST_NONE : st == IMO_ABORT ? IM_ST_ABORT : IM_ST_OVERFLOW;" in src


def test_gpucmp_rule_is_not_hip_vs_oracles_early_return():
    """hip_vs_oracle returns at a negative status before it looks at the bands; the rule at the bounds does look"""
    import numpy as np
    from indelminer_amd import capi
    B = rb.select("band_g8")
    i = next(i for i in B.info if i.overflow)
    rec = np.zeros(1, capi.RESULT_DTYPE)[0]
    rec["status"] = capi.ST_OVERFLOW
    assert gpucmp.hip_vs_oracle(rec, capi.ST_OVERFLOW, i.res) is None
    assert "n_band" in gpucmp.hip_vs_oracle_at_bounds(rec, i.st, i.res)
    rec["status"] = capi.ST_EVIDENCE
    assert "IM_ST_OVERFLOW expected" in gpucmp.hip_vs_oracle_at_bounds(rec, i.st, i.res)
