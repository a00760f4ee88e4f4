"""realign_kernel's two lane layouts against the CPU oracle, every read of every batch: reads of up to 128 bases lie two
positions to a lane (staging, k-mer table, diagonal scans, merge), longer ones four, chosen per read inside one launch.

Lengths on both sides of every border the layouts have -- 5 and 6 (a piece shorter than k = 6 / exactly k), 7, 50, 100,
127, 128 (the last position of lane 63 at two per lane), 129, 130, 255 -- and one batch that mixes 100, 128, 129 and 255,
so that neighbouring workgroups of one grid take different paths.  One -k per instantiation: 6 (specialised direct table),
4 (direct table, mask at run time), 8 (prefix table), 14 (hash).  A piece shorter than k - 1 makes the reference's diagonal
count (src/alignment.c:403-404) wrap around as unsigned arithmetic; the batches keep to read lengths of at least k - 1, where
it does not, so -k 8 starts at 7 bases and -k 14 at 50.

Contigs of 4 to 8 kb and anchors drawn within range_max of either end as often as in between: the windows are clipped at 0
and at the contig's length.  Planted 1-50 bp deletions and insertions on either side of the read's middle (the second
piece then starts at a read offset other than 0, and either piece can be the one that starts the read), reads whose one end
is not from the contig at all (what an aligner emits soft-clipped), and unchanged reads.  The oracle alone must find at
least ten reads with evidence and ten without in every batch of reads of 50 bases or more: a batch that stops being a test
of both outcomes fails here, whatever the kernel does."""
import random

import numpy as np
import pytest

from tests.support import gpucmp, oraclebind as ob

pytestmark = pytest.mark.gpu

LENGTHS = (5, 6, 7, 50, 100, 127, 128, 129, 130, 255)
MIXED = (100, 128, 129, 255)
RANGE_MAX = 705
N_READS = 240


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _batch(seed, lengths, n=N_READS):
    """(contig, cases): one contig of 4..8 kb, n reads of the given lengths in turn"""
    rng = random.Random(seed)
    clen = rng.randint(4000, 8000)
    contig = _rand(rng, clen)
    cases = []
    for i in range(n):
        L = lengths[i % len(lengths)]
        where = rng.random()
        if where < 0.3:
            anchor = rng.randint(0, RANGE_MAX // 2)                    # the windows are clipped at 0
        elif where < 0.6:
            anchor = rng.randint(clen - 1 - RANGE_MAX // 2, clen - 1)  # ... at the contig's length
        else:
            anchor = rng.randint(0, clen - 1)
        p = max(0, min(clen - L - 60, anchor + rng.randint(-RANGE_MAX + 60, RANGE_MAX - L - 60)))
        cut = rng.randint(min(12, L // 2), max(L - 12, L // 2))
        typ = rng.random()
        if typ < 0.36:
            d = rng.randint(1, 50)
            read = contig[p:p + cut] + contig[p + cut + d:p + cut + d + (L - cut)]
        elif typ < 0.62:
            read = (contig[p:p + cut] + _rand(rng, rng.randint(1, 50)) + contig[p + cut:p + L])[:L]
        elif typ < 0.72:
            read = contig[p:p + cut] + _rand(rng, L - cut)             # soft-clipped tail
        elif typ < 0.82:
            read = _rand(rng, cut) + contig[p + cut:p + L]             # soft-clipped head
        else:
            read = contig[p:p + L]
        read = "".join((rng.choice("ACGT") if rng.random() < 0.005 else ch) for ch in read)
        assert len(read) == L
        cases.append(dict(anchor=anchor, range_max=RANGE_MAX, read=read))
    return contig, cases


def _low_complexity(seed, L):
    from tests.support import lowcomplexity as lc
    contig, cases, share = lc.realign_cases(seed, n=N_READS, clen=6000, lengths=(L,))
    assert share >= 0.4, share
    return contig, cases


def _batches(k):
    """[(tag, seed, lengths or None for a low-complexity batch)] of one -k; the seeds were chosen on the oracle alone"""
    out = [("L%d" % L, 5000 + 10 * L + k, (L,)) for L in LENGTHS if L >= k - 1]
    out.append(("mixed", 9000 + k, MIXED))
    if k == 6:
        out += [("lowc100", 7100, None), ("lowc128", 7128, None)]
    return out


def _compare(ctx, kw, contig, cases):
    """every read of the batch against the oracle; returns (oracle statuses, oracle results, differing reads)"""
    from indelminer_amd import capi
    cb = contig.encode()
    ctx.set_reference([cb])
    rc, out = ctx.realign_batch(capi.params(**kw), [c["read"].encode() for c in cases], np.zeros(len(cases), np.int32),
                                np.array([c["anchor"] for c in cases], np.int32),
                                np.array([c["range_max"] for c in cases], np.int32), allow=(capi.E_ABORT,))
    P = ob.params(**kw)
    sts, ress, bad = [], [], []
    for i, c in enumerate(cases):
        st, res = ob.realign(P, cb, len(cb), c["anchor"], c["range_max"], c["read"])
        sts.append(st); ress.append(res)
        msg = gpucmp.hip_vs_oracle(out[i], st, res)
        if msg:
            bad.append((i, msg, c["anchor"], c["range_max"], c["read"]))
    return sts, ress, bad


@pytest.mark.parametrize("k", [6, 4, 8, 14])
def test_both_lane_layouts_match_oracle(gpu_ctx, k):
    kw = dict(klength=k, numgaps=0, maxdelsize=1000, ethreshold=max(k, 10))
    first_is_head = first_is_tail = offset_second = 0
    for tag, seed, lengths in _batches(k):
        if lengths is None:
            contig, cases = _low_complexity(seed, int(tag[4:]))
        else:
            contig, cases = _batch(seed, lengths)
        sts, ress, bad = _compare(gpu_ctx, kw, contig, cases)
        n_ev = sum(1 for st in sts if st == 1)
        print("k %d %s: %d reads, %d with evidence, %d differ" % (k, tag, len(cases), n_ev, len(bad)))
        if min(len(c["read"]) for c in cases) >= 50:
            assert n_ev >= 10 and len(cases) - n_ev >= 10, (k, tag, n_ev, len(cases))
        assert not bad, "k %d %s: %d of %d differ, first: %r" % (k, tag, len(bad), len(cases), bad[:3])
        for st, res, c in zip(sts, ress, cases):
            if st == 1 and len(c["read"]) <= 128:
                # which piece the first alignment is: the one that starts the read (the second search then takes read[f, L),
                # a piece at an offset) or the one that ends it
                if res.piece[0].q1 == 0:
                    first_is_head += 1
                    offset_second += 1 if res.piece[1].q1 > 0 else 0
                else:
                    first_is_tail += 1
    assert first_is_head >= 10 and first_is_tail >= 10 and offset_second >= 10, (first_is_head, first_is_tail, offset_second)
