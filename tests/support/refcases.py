"""Inputs of the oracle-against-reference checks (tests/test_oracle_vs_ref.py), regenerated from their seeds wherever the
tests run.  The reference's answers to them are committed in tests/golden/ref_fuzz.json (tests/golden/make_golden_fuzz.py)."""
import json
import random

# k stops at 11 here: the reference allocates and clears two 4^k-entry tables per band search
# (src/alignment.c:38-39), 128 MB per call at k = 12 and 8 GB at k = 15
FUZZ = [(6, 0, 11), (6, 1, 12), (8, 2, 13), (5, 0, 14),
        (2, 0, 21), (3, 0, 22), (4, 0, 23), (7, 0, 24), (10, 0, 25), (11, 0, 26),
        (6, 3, 31), (6, 5, 32), (6, 8, 33), (6, 12, 34), (11, 4, 35)]
LEFT_EDGE = [(6, 0, 1), (6, 0, 2), (6, 1, 3), (6, 2, 4), (6, 5, 5), (8, 3, 6), (4, 0, 7), (6, 12, 8)]

GOLDEN_NAME = "ref_fuzz.json"


def fuzz(seed):
    """(maxdel, contig, [dict(anchor, range_max, read)]): 150 reads with one deletion or insertion (and sometimes a
    substitution) around random anchors of a random 6 kb contig"""
    rng = random.Random(seed)
    maxdel = rng.choice([1000, 200])
    contig = "".join(rng.choice("ACGT") for _ in range(6000))
    cases = []
    for _ in range(150):
        L = rng.choice([100, 100, 76, 150])
        anchor = rng.randint(0, len(contig) - 1)
        p = max(0, min(len(contig) - L - 60, anchor + rng.randint(-700, 700)))
        d = rng.choice([1, 3, 10, 50, 300])
        cut = rng.randint(5, L - 5)
        if rng.random() < 0.6:
            read = contig[p:p + cut] + contig[p + cut + d:p + cut + d + (L - cut)]
        else:
            ins = "".join(rng.choice("ACGT") for _ in range(min(d, 30)))
            read = (contig[p:p + cut] + ins + contig[p + cut:p + L])[:L]
        if rng.random() < 0.3:
            i = rng.randrange(len(read))
            read = read[:i] + rng.choice("ACGT") + read[i + 1:]
        cases.append(dict(anchor=anchor, range_max=500, read=read))
    return maxdel, contig, cases


def key(kind, k, g, seed):
    return "%s k%d g%d seed%d" % (kind, k, g, seed)


def plain(ref_out):
    """a reference answer (refbind.Ref.realign) as it is stored: None, or the evidence list in returned order with
    cls / type / b1 / b2 and the three segment lists"""
    if ref_out is None:
        return None
    return json.loads(json.dumps([{f: e[f] for f in ("cls", "type", "b1", "b2", "aln1", "aln2", "aln3")} for e in ref_out]))
