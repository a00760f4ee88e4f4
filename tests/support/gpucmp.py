"""Field-by-field comparison of a HIP result record with the CPU oracle's result."""
from . import oraclebind as ob

_ST = {1: 1, 0: 0, -1: -1, -2: -2}


def _bands(rec, res):
    """the record's band bookkeeping against the oracle's"""
    nb = res.n_band
    if int(rec["n_band"]) != nb:
        return "n_band hip %d oracle %d" % (rec["n_band"], nb)
    for b in range(nb):
        h = rec["band"][b]
        o = res.piece[b]
        got = (int(h["r1"]), int(h["r2"]), int(h["q1"]), int(h["q2"]))
        want = (o.r1, o.r2, o.q1, o.q2)
        if got != want:
            return "band %d (r1,r2,q1,q2) hip %r oracle %r (low hip %d oracle %d)" % (b, got, want, h["low"], o.low)
        if int(h["low"]) != o.low and want != (0, 0, 0, 0):
            return "band %d low hip %d oracle %d" % (b, h["low"], o.low)
        if (int(h["win_bytes"]), int(h["piece_bytes"])) != (res.win_bytes[b], res.piece_bytes[b]):
            return "band %d bytes hip %r oracle %r" % (b, (h["win_bytes"], h["piece_bytes"]), (res.win_bytes[b], res.piece_bytes[b]))
    return None


def hip_vs_oracle(rec, st, res, check_bands=True):
    """rec: one element of capi.RESULT_DTYPE; st/res: oracle status and Result."""
    if int(rec["status"]) != _ST.get(st, st):
        return "status hip %d oracle %d" % (rec["status"], st)
    if st < 0:
        return None
    if check_bands:
        msg = _bands(rec, res)
        if msg:
            return msg
    if st != 1:
        return None
    if int(rec["ref_start"]) != res.ref_start:
        return "ref_start hip %d oracle %d" % (rec["ref_start"], res.ref_start)
    hops = [int(x) for x in rec["ops"][:int(rec["n_ops"])]]
    oops = [res.ops[i] for i in range(res.n_ops)]
    if hops != oops:
        return "ops hip %r oracle %r" % ([(w >> 4, w & 15) for w in hops], [(w >> 4, w & 15) for w in oops])
    if int(rec["n_ev"]) != res.n_ev:
        return "n_ev hip %d oracle %d" % (rec["n_ev"], res.n_ev)
    for k in range(res.n_ev):
        h = rec["ev"][k]
        o = res.ev[k]
        for f in ("cls", "b1", "b2", "seg", "read_off", "lflank", "rflank", "nd_print", "nd_filter"):
            if int(h[f]) != getattr(o, f):
                return "ev[%d].%s hip %d oracle %d" % (k, f, h[f], getattr(o, f))
    return None


MAX_OPS, MAX_EV = 64, 4         # IM_MAX_OPS, IM_MAX_EV: the result record's bounds, which the oracle (256, 32) does not have


def expected_status(st, res, max_ops=MAX_OPS, max_ev=MAX_EV):
    """The status the kernels owe for a read the oracle answered with (st, res): the oracle's own for NONE and ABORT;
    IM_ST_EVIDENCE for a result inside the record's bounds, IM_ST_OVERFLOW for one beyond either.  None where the rule gives no
    answer: the oracle ran into its own caps, or the final list fits while a piece's CIGAR is beyond IM_MAX_OPS (either answer
    could be defended; the tests keep such reads out of their batches and count them)."""
    if st in (0, -1):
        return st
    if st != 1:
        return None
    if res.n_ops > max_ops or res.n_ev > max_ev:
        return -2
    if max(res.piece[0].n_ops, res.piece[1].n_ops) > max_ops:
        return None
    return 1


def hip_vs_oracle_at_bounds(rec, st, res):
    """hip_vs_oracle for reads at the bounds of the result record.  A read whose oracle result fits is held to every field
    hip_vs_oracle compares; one beyond IM_MAX_OPS or IM_MAX_EV must come back IM_ST_OVERFLOW with n_ev = n_ops = ref_start = 0
    (what finish() leaves behind every status but IM_ST_EVIDENCE) and -- unlike hip_vs_oracle, which returns at a negative
    status -- with the band bookkeeping of the oracle's result: both band searches were done before the list was found too long."""
    want = expected_status(st, res)
    if want is None:
        return "the rule has no answer for this read (oracle status %d, n_ops %d, pieces %d / %d)" % (
            st, res.n_ops, res.piece[0].n_ops, res.piece[1].n_ops)
    if want != -2:
        return hip_vs_oracle(rec, st, res)
    if int(rec["status"]) != -2:
        return "status hip %d, oracle n_ops %d n_ev %d: IM_ST_OVERFLOW expected" % (rec["status"], res.n_ops, res.n_ev)
    msg = _bands(rec, res)
    if msg:
        return "overflow record: " + msg
    left = (int(rec["n_ev"]), int(rec["n_ops"]), int(rec["ref_start"]))
    if left != (0, 0, 0):
        return "overflow record: (n_ev, n_ops, ref_start) = %r, finish() leaves zeros" % (left,)
    return None
