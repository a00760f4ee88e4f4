"""im_dev_flush_groupby at the sizes where its three launches take another path: flush lists around the 64 descriptors a
workgroup holds whole, candidate counts around a workgroup and below the launch bound, slots behind the count that must
not be seen, clusters whose members lie inside and beyond the stretch of slots a wave fetches ahead, paired-read entries
alone, and call after call on one scratch.  consumed[] is held against imo_flush_cut applied flush by flush, the clusters
against a plain group-by (bit-exact, member order included)."""
import numpy as np
import pytest

from indelminer_amd import capi
from tests.support import oraclebind as ob

pytestmark = pytest.mark.gpu

E = capi.MAX_EV
CAP, CAP_PE, CAP_FL = 4096, 128, 160
BIG = 32768                     # candidates of the hand-made cluster layout (131 072 slots)
INT_MAX = 2**31 - 1
UNTOUCHED = -7                  # consumed[] behind the count and behind the paired-read entries, as uploaded


@pytest.fixture(scope="module")
def pipe(gpu_ctx):
    return capi.Pipeline(gpu_ctx, 1, 64, cap_cand=CAP, n_pe=CAP_PE, n_flushes=CAP_FL)


def _case(rng, n_cand, fl_per_ctg, n_pe, pinned=False):
    """slot arrays, candidate records, paired-read entries and a flush list with exactly fl_per_ctg[c] flushes in contig c, the
    way the product builds them: records ascend, a contig's flushes share rec0, its markers never decrease, INT_MAX at its end"""
    n_ctg = len(fl_per_ctg)
    rec = np.cumsum(rng.integers(1, 40, n_cand)).astype(np.int32)
    n_rec = int(rec[-1]) + 1
    ctg_start = [0] + sorted(int(x) for x in rng.choice(np.arange(1, n_rec), n_ctg - 1, replace=False)) + [n_rec]
    pos_of_rec = np.zeros(n_rec, np.int64)
    for c in range(n_ctg):
        a, b = ctg_start[c], ctg_start[c + 1]
        pos_of_rec[a:b] = np.sort(rng.integers(0, 2_000_000, b - a))
    cls = np.full(n_cand * E, -1, np.int32); b1 = np.zeros(n_cand * E, np.int32); b2 = np.zeros(n_cand * E, np.int32)
    pool = rng.integers(-600, 600, 64)                                   # few distinct offsets: clusters with several members
    for j in range(E):
        live = rng.random(n_cand) < (0.9 if j == 0 else 0.15)
        s = np.maximum(pos_of_rec[rec] // 200 * 200 + pool[rng.integers(0, 64, n_cand)], 0)
        cls[j::E] = np.where(live, rng.integers(0, 2, n_cand), -1)
        b1[j::E] = s
        b2[j::E] = s + np.where(rng.random(n_cand) < 0.6, rng.integers(1, 900, n_cand) // 50 * 50, 0)
    cls[0] = 0                                                           # a count of one still holds a live slot
    pe_rec = np.sort(rng.integers(0, n_rec, n_pe))
    pe_b1 = np.maximum(pos_of_rec[pe_rec] + rng.integers(-500, 500, n_pe), 0).astype(np.int32)
    pe_b2 = (pe_b1 + rng.integers(100, 5000, n_pe)).astype(np.int32)
    flushes = []
    for c in range(n_ctg):
        a, b = ctg_start[c], ctg_start[c + 1]
        floor = int(rng.integers(0, 100_000)) if pinned else INT_MAX
        mk = -1
        for r1 in np.sort(rng.integers(a, b + 1, fl_per_ctg[c] - 1)):
            here = int(pos_of_rec[r1 - 1]) if r1 > a else 0
            mk = max(mk, min(floor, here - int(rng.integers(0, 3000))))
            flushes.append((a, int(r1), int(np.searchsorted(pe_rec, r1)), mk))
        flushes.append((a, b, int(np.searchsorted(pe_rec, b)), INT_MAX))
    assert len(flushes) == sum(fl_per_ctg)
    return rec, cls, b1, b2, pe_b1, pe_b2, flushes


def _check(pipe, case, n_cand=None, tie=0, cand_bound=None):
    """one call on the first n_cand candidates of `case`; every slot behind them holds an entry that would win every cut if it
    were seen (class 0, b1 0, b2 INT_MAX - 1, record 0).  Returns (entries consumed, clusters)."""
    rec, cls, b1, b2, pe_b1, pe_b2, flushes = case
    cap = pipe.cap_cand
    n_cand = len(rec) if n_cand is None else n_cand
    ns, n_pe, base = n_cand * E, len(pe_b1), cap * E
    rec, cls, b1, b2 = rec[:n_cand], cls[:ns], b1[:ns], b2[:ns]
    up = lambda a, fill, n: np.concatenate([a, np.full(n - len(a), fill, np.int32)]).astype(np.int32)
    pipe.d_cls.upload(up(cls, 0, base)); pipe.d_b1.upload(up(b1, 0, base)); pipe.d_b2.upload(up(b2, INT_MAX - 1, base))
    pipe.d_cand_rec.upload(up(rec, 0, cap))
    pipe.d_consumed.upload(np.full(pipe.n_slots, UNTOUCHED, np.int32))
    pipe.n_pe = n_pe
    pipe.set_pe(pe_b1, pe_b2)
    cnt = np.zeros(8, np.int32); cnt[0] = n_cand
    pipe.d_counters.upload(cnt)
    pipe.flush_groupby(flushes, tie_desc=tie, cand_bound=cap if cand_bound is None else cand_bound)
    pipe.sync()
    a_b1 = np.concatenate([b1, pe_b1]).astype(np.int32); a_b2 = np.concatenate([b2, pe_b2]).astype(np.int32)
    want = np.zeros(ns + n_pe, np.int32)
    for k, (r0, r1, pe_hi, marker) in enumerate(flushes):
        lo, hi = int(np.searchsorted(rec, r0)), int(np.searchsorted(rec, r1))
        vis = np.full(ns + n_pe, -1, np.int32)
        vis[lo * E:hi * E] = cls[lo * E:hi * E]; vis[ns:ns + pe_hi] = 2
        ob.flush_cut(vis, a_b1, a_b2, want, marker, k + 1)
    got = pipe.d_consumed.download(np.int32, pipe.n_slots)
    assert np.array_equal(got[:ns], want[:ns]), int((got[:ns] != want[:ns]).sum())
    assert np.array_equal(got[base:base + n_pe], want[ns:])
    assert np.all(got[ns:base] == UNTOUCHED) and np.all(got[base + n_pe:] == UNTOUCHED)
    groups = {}
    for s in np.nonzero((cls >= 0) & (cls < 2) & (want[:ns] > 0))[0]:
        groups.setdefault((int(want[s]), int(cls[s]), int(b1[s]), int(b2[s])), []).append(int(s))
    key, first, count, order = pipe.clusters()
    assert int(count.sum()) == len(order) == sum(len(v) for v in groups.values())
    seen = {tuple(int(x) for x in key[c]): [int(x) for x in order[first[c]:first[c] + count[c]]] for c in range(len(key))}
    assert len(seen) == len(key)
    assert seen == ({k: v[::-1] for k, v in groups.items()} if tie else groups)
    return int((want > 0).sum()), len(groups)


def _split(total, n_ctg):
    n_ctg = min(n_ctg, total)           # every contig ends in a flush: a list of one or two flushes has as many contigs at most
    return [total // n_ctg] * (n_ctg - 1) + [total - total // n_ctg * (n_ctg - 1)]


@pytest.mark.parametrize("n_ctg", [1, 3])
@pytest.mark.parametrize("n_fl", [1, 2, 63, 64, 65, 130])
def test_list_sizes_at_the_window_edge(pipe, n_fl, n_ctg):
    """the whole list in LDS up to 64 flushes, the window behind a search from 65 on; `last` at a contig's end inside and
    outside the window; markers free and pinned low"""
    rng = np.random.default_rng(1000 * n_fl + n_ctg)
    consumed, clusters = _check(pipe, _case(rng, 3000, _split(n_fl, n_ctg), 100, pinned=n_fl in (63, 130)), tie=n_fl & 1)
    assert consumed > 1000 and clusters > 100


@pytest.fixture(scope="module")
def cap_case():
    return _case(np.random.default_rng(5), CAP, [9, 4, 12], 40)


@pytest.mark.parametrize("bound_is_cap", [True, False])
@pytest.mark.parametrize("n_cand", [0, 1, 255, 256, 257, CAP])
def test_candidate_counts_below_the_launch_bound(pipe, cap_case, n_cand, bound_is_cap):
    """the launch covers cand_bound candidates, the device's count says how many there are"""
    consumed, clusters = _check(pipe, cap_case, n_cand=n_cand, tie=n_cand & 1, cand_bound=CAP if bound_is_cap else max(n_cand, 1))
    assert consumed >= 40 + (n_cand > 0)                   # the paired-read entries, and slot 0 of the first candidate
    assert clusters > 0 if n_cand else clusters == 0       # without candidates there is nothing to cluster
    if n_cand >= 255:
        assert clusters > 50


def test_poison_behind_the_count(pipe, cap_case):
    """a thousand candidates of a buffer of 4 096: what lies behind them would cut every flush at (0, INT_MAX - 1) -- nothing
    but the contigs' ends would consume -- and must come through the call as it went in"""
    consumed, clusters = _check(pipe, cap_case, n_cand=1000)
    assert consumed > 500 and clusters > 100


def test_paired_read_entries_alone(pipe):
    for n_pe in (1, 63, 64, 70):
        rng = np.random.default_rng(n_pe)
        consumed, clusters = _check(pipe, _case(rng, 500, [3, 2], n_pe), n_cand=0)
        assert consumed == n_pe and clusters == 0


def test_two_shapes_on_one_scratch(pipe):
    """a large call, a small one, the large one again: the table and the tree leave every call clean"""
    large = _case(np.random.default_rng(21), CAP, [70, 60], 120, pinned=True)
    small = _case(np.random.default_rng(22), 50, [2], 3)
    a = _check(pipe, large)
    b = _check(pipe, small, tie=1)
    assert _check(pipe, large) == a
    assert a[0] > 2000 and a[1] > 200 and b[0] > 10 and b[1] > 5


def _layout(n_cand):
    """hand-made clusters in the slots of n_cand candidates, consumed by one flush at the contig's end: (slot -> key)"""
    ns = n_cand * E
    key_of = {}
    # 64 firsts inside one 64-slot stretch, each with a member inside the stretches fetched ahead and one beyond them
    for k in range(64):
        for s in (640 + k, 704 + (63 - k), 640 + 64 * 7 + k):
            key_of[s] = 2000 + k
    # two firsts inside one stretch, one closed within the stretches ahead, one not
    key_of.update({2048: 3000, 2048 + 65: 3000, 2050: 3001, 2050 + 400: 3001, 2050 + 401: 3001})
    # one cluster of several hundred members 1, 63, 64, 65, 255, 256, 257 and about 1 000 slots apart
    s, gaps, big = 4101, (1, 63, 64, 65, 255, 256, 257, 1003), 0
    while s < ns - 1:
        key_of[s] = 1000; big += 1
        s += gaps[big % len(gaps)]
    key_of[ns - 1] = 4000                                                # a first in the last slot
    return key_of, big


def test_clusters_against_the_prefetch(gpu_ctx):
    """members inside and beyond the slots a wave fetches ahead, 2 and 64 firsts in one stretch, a first in the last slot, both
    member orders; then fewer candidates on the same buffers, with the first call's table positions still behind the count"""
    p = capi.Pipeline(gpu_ctx, 1, 64, cap_cand=BIG, n_pe=1, n_flushes=4)
    none = np.zeros(0, np.int32)
    for n_cand, tie in ((BIG, 0), (BIG, 1), (20_000, 0), (20_000, 1)):
        key_of, big = _layout(n_cand)
        assert big > (250 if n_cand == BIG else 150)
        cls = np.full(n_cand * E, -1, np.int32); b1 = np.zeros(n_cand * E, np.int32)
        for s, k in key_of.items():
            cls[s] = k & 1; b1[s] = k
        case = (np.arange(n_cand, dtype=np.int32), cls, b1, b1 + 7, none, none, [(0, n_cand, 0, INT_MAX)])
        consumed, clusters = _check(p, case, tie=tie)
        assert consumed == len(key_of) and clusters == len(set(key_of.values())) == 68
