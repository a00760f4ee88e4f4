"""Parity of the HIP split-read cluster kernels with the CPU oracle (bit-exact)."""
import os

import numpy as np
import pytest

from tests.test_oracle_golden import _cluster_oracle

pytestmark = pytest.mark.gpu


def _random_evidence(seed, n, span):
    rng = np.random.default_rng(seed)
    nsite = max(1, n // 12)
    site_b1 = rng.integers(0, span, nsite)
    site_len = rng.integers(0, 60, nsite)          # 0 -> insertion (b1 == b2)
    pick = rng.integers(0, nsite, n)
    b1 = site_b1[pick].astype(np.int32)
    b2 = (site_b1[pick] + site_len[pick]).astype(np.int32)
    noise = rng.random(n) < 0.2
    b1[noise] = rng.integers(0, span, noise.sum())
    b2[noise] = b1[noise] + rng.integers(0, 60, noise.sum())
    cls = (b2 > b1).astype(np.int32)
    return cls, b1, b2


@pytest.mark.parametrize("n,span,marker,tie", [
    (1, 100, 2**31 - 1, 0), (7, 50, 2**31 - 1, 1), (300, 2000, 2**31 - 1, 0), (5000, 100000, 60000, 0),
    (5000, 100000, 60000, 1), (70000, 5000000, 2**31 - 1, 0), (70000, 5000000, 2500000, 1), (2049, 300, 200, 0),
])
def test_cluster_matches_oracle(gpu_ctx, n, span, marker, tie):
    cls, b1, b2 = _random_evidence(n * 31 + tie, n, span)
    o_order, o_first, o_count, o_used, o_k = _cluster_oracle(cls, b1, b2, marker, tie)
    h_order, h_first, h_count, h_used, h_k = gpu_ctx.cluster_sr(cls, b1, b2, marker, tie)
    assert h_k == o_k
    assert np.array_equal(h_used, o_used)
    assert np.array_equal(h_first, o_first)
    assert np.array_equal(h_count, o_count)
    m = int(o_used.sum())
    assert np.array_equal(h_order[:m], o_order[:m])


def test_cluster_empty(gpu_ctx):
    order, first, count, used, k = gpu_ctx.cluster_sr([], [], [])
    assert k == 0 and len(order) == 0


def test_cluster_sortedness_and_grouping_large(gpu_ctx):
    """Size-independent properties at 2M records: clusters ascend in (b1,b2), members share
    a key and ascend in arrival, every record is placed exactly once."""
    n = 2_000_000
    cls, b1, b2 = _random_evidence(5, n, 50_000_000)
    order, first, count, used, k = gpu_ctx.cluster_sr(cls, b1, b2)
    assert used.all() and int(count.sum()) == n
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.int32))
    kb1, kb2 = b1[order], b2[order]
    key = kb1.astype(np.int64) << 32 | kb2.astype(np.int64)
    assert (np.diff(key) >= 0).all()
    same = np.diff(key) == 0
    assert (np.diff(order)[same] > 0).all()
    heads = np.zeros(n, bool); heads[first] = True
    assert np.array_equal(heads[1:], ~same)


def _cut_and_group(ctx, n_slots, d, marker, tie):
    """One flush (id 1) over slots [0, n_slots) through im_dev_flush_cut, then im_dev_cluster_groupby (asynchronous)."""
    from indelminer_amd import capi
    L = capi.lib()
    st = ctx.stream
    ctx._check(L.im_dev_memset(ctx.h, d["consumed"].ptr, 0, 4 * n_slots, st))
    ctx._check(L.im_dev_memset(ctx.h, d["cut"].ptr, 0xFF, 8, st))
    ctx._check(L.im_dev_flush_cut(ctx.h, d["cls"].ptr, d["b1"].ptr, d["b2"].ptr, d["consumed"].ptr, 0, n_slots, 0, 0, marker, 1,
                                  d["cut"].ptr, st))
    ctx._check(L.im_dev_cluster_groupby(ctx.h, n_slots, d["cls"].ptr, d["b1"].ptr, d["b2"].ptr, d["consumed"].ptr, tie,
                                        d["order"].ptr, d["key"].ptr, d["first"].ptr, d["count"].ptr, d["counts"].ptr,
                                        d["gs"].ptr, d["gs_bytes"], st))


def _slot_buffers(ctx, cls, b1, b2):
    from indelminer_amd import capi
    L = capi.lib()
    n = len(cls)
    d = {k: capi.DevBuf(ctx, 4 * n).upload(np.ascontiguousarray(v, np.int32)) for k, v in (("cls", cls), ("b1", b1), ("b2", b2))}
    for k in ("consumed", "order", "first", "count"):
        d[k] = capi.DevBuf(ctx, 4 * n)
    d["key"] = capi.DevBuf(ctx, 16 * n); d["counts"] = capi.DevBuf(ctx, 64); d["cut"] = capi.DevBuf(ctx, 64)
    d["gs_bytes"] = L.im_dev_groupby_scratch_bytes(n)
    d["gs"] = capi.DevBuf(ctx, d["gs_bytes"])
    ctx._check(L.im_dev_groupby_scratch_init(ctx.h, n, d["gs"].ptr, d["gs_bytes"], ctx.stream))
    return d


def _clusters_by_key(d):
    """counts, and the group-by's clusters ordered by (b1, b2, cls): keys [k, 4], firsts, counts"""
    counts = d["counts"].download(np.int32, 2)
    k = int(counts[0])
    key = d["key"].download(np.int32, 4 * k).reshape(k, 4)
    perm = np.lexsort((key[:, 1], key[:, 3], key[:, 2]))
    return counts, key[perm], d["first"].download(np.int32, k)[perm], d["count"].download(np.int32, k)[perm]


def test_cluster_slots_matches_oracle(gpu_ctx):
    """Slot form (empty slots = cls -1) through im_dev_flush_cut + im_dev_cluster_groupby: same clusters as the oracle
    on the compacted records once ordered by key, order[] in slot indices, used[] from consumed[]; the group-by scratch
    must come back clean (3 calls, then a replay from a captured launch graph)."""
    from indelminer_amd import capi
    L = capi.lib()
    for seed, n_slots, live_frac, marker, tie in [(1, 4000, 0.5, 2**31 - 1, 0), (2, 30000, 0.25, 2**31 - 1, 1),
                                                  (3, 9000, 0.9, 40000, 0), (4, 50, 0.5, 2**31 - 1, 0),
                                                  (5, 40000, 0.5, 2**31 - 1, 0)]:
        rng = np.random.default_rng(seed)
        cls, b1, b2 = _random_evidence(seed, n_slots, 80000)
        live = rng.random(n_slots) < live_frac
        cls_s = np.where(live, cls, -1).astype(np.int32)
        idx = np.nonzero(live)[0]
        o_order, o_first, o_count, o_used, o_k = _cluster_oracle(cls[idx], b1[idx], b2[idx], marker, tie)
        d = _slot_buffers(gpu_ctx, cls_s, b1, b2)
        for _round in range(3):     # the table cleans itself: identical answers call after call
            _cut_and_group(gpu_ctx, n_slots, d, marker, tie)
        # ... and once more replayed from a captured launch graph (im_capture_* / im_graph_launch)
        with capi.Graph.capture(gpu_ctx) as g:
            _cut_and_group(gpu_ctx, n_slots, d, marker, tie)
        g.launch()
        gpu_ctx._check(L.im_stream_sync(gpu_ctx.h, gpu_ctx.stream))
        g.close()
        counts, key, first, count = _clusters_by_key(d)
        m = int(o_used.sum())
        assert counts[0] == o_k and counts[1] == m
        order = d["order"].download(np.int32, n_slots)
        got = np.concatenate([order[f:f + c] for f, c in zip(first, count)]) if o_k else np.zeros(0, np.int32)
        assert np.array_equal(got, idx[o_order[:m]])
        assert np.array_equal(np.cumsum(count) - count, o_first)
        assert np.array_equal(count, o_count)
        used = d["consumed"].download(np.int32, n_slots) != 0
        want = np.zeros(n_slots, bool); want[idx[o_used.astype(bool)]] = True
        assert np.array_equal(used, want)


def test_cluster_records_and_rccl_allgather_world1(gpu_ctx):
    """The gathered unit (16 B cluster records, packed on the host from the group-by's clusters) and the RCCL
    all-gather entry point with one rank."""
    from indelminer_amd import capi
    from tests.support import gathered as shard
    L = capi.lib()
    n = 3000
    cls, b1, b2 = _random_evidence(77, n, 40000)
    o_order, o_first, o_count, o_used, o_k = _cluster_oracle(cls, b1, b2, 2**31 - 1, 0)
    d = _slot_buffers(gpu_ctx, cls, b1, b2)
    _cut_and_group(gpu_ctx, n, d, 2**31 - 1, 0)
    gpu_ctx._check(L.im_stream_sync(gpu_ctx.h, gpu_ctx.stream))
    counts, key, _, count = _clusters_by_key(d)
    cap = 4096
    recs = shard.pack_records(3, key[:, 2], key[:, 3], key[:, 1], count, int(counts[1]), cap)
    d_recs = capi.DevBuf(gpu_ctx, 16 * cap).upload(recs); d_all = capi.DevBuf(gpu_ctx, 16 * cap)
    st = gpu_ctx.stream
    comm = capi.Comm(gpu_ctx, capi.comm_unique_id(), 0, 1)
    comm.allgather(d_recs.ptr, d_all.ptr, 16 * cap, st)
    gpu_ctx._check(L.im_stream_sync(gpu_ctx.h, st))
    got, trunc = shard.merge_gathered(d_all.download(np.int32, 4 * cap), cap)
    heads = o_order[o_first]
    want = shard.pack_records(3, b1[heads], b2[heads], cls[heads], o_count, n, cap)
    want, _ = shard.merge_gathered(want.reshape(-1), cap)
    assert not trunc and np.array_equal(got, want)
    comm.close()


def test_depth_matches_numpy(gpu_ctx):
    """Region depth (DP=): difference array + device scan + range sums vs numpy, incl. segments
    clipped at both contig ends and a contig longer than one scan tile."""
    rng = np.random.default_rng(11)
    for clen, nseg in ((5000, 800), (100_000, 60_000), (3_000_000, 900_000)):
        start = rng.integers(-50, clen + 20, nseg).astype(np.int32)
        ln = rng.integers(1, 101, nseg).astype(np.int32)
        gpu_ctx.depth_build(clen, start, ln)
        diff = np.zeros(clen + 1, np.int64)
        a = np.clip(start.astype(np.int64), 0, clen); b = np.clip(start.astype(np.int64) + ln, 0, clen)
        ok = a < b
        np.add.at(diff, a[ok], 1); np.add.at(diff, b[ok], -1)
        depth = np.cumsum(diff)[:clen]
        csum = np.concatenate([[0], np.cumsum(depth)])
        qb = rng.integers(0, clen - 1, 500).astype(np.int32)
        qe = np.minimum(qb + rng.integers(1, 1200, 500), clen).astype(np.int32)
        got = gpu_ctx.depth_query(qb, qe)
        want = (csum[qe] - csum[qb]).astype(np.uint32)
        assert np.array_equal(got, want)


def _depth_case(ctx, rng, clen, nseg):
    """one im_depth_build on ctx against numpy: every position, the whole contig, and range sums clipped at both ends"""
    start = rng.integers(-50, clen + 20, nseg).astype(np.int32)
    ln = rng.integers(1, 101, nseg).astype(np.int32)
    ctx.depth_build(clen, start, ln)
    diff = np.zeros(clen + 1, np.int64)
    a = np.clip(start.astype(np.int64), 0, clen); b = np.clip(start.astype(np.int64) + ln, 0, clen)
    ok = a < b
    np.add.at(diff, a[ok], 1); np.add.at(diff, b[ok], -1)
    depth = np.cumsum(diff)[:clen]
    csum = np.concatenate([[0], np.cumsum(depth)])
    p = np.arange(clen, dtype=np.int32)
    assert np.array_equal(ctx.depth_query(p, p + 1), depth.astype(np.uint32)), clen
    qb = np.concatenate([rng.integers(-300, clen + 300, 500), [-5, -40, 0, clen - 1, clen, clen + 3, -9]])
    qe = np.concatenate([qb[:500] + rng.integers(0, 1200, 500), [clen + 7, 30, clen, clen + 1, clen + 50, clen + 90, -2]])
    ca, cb = np.clip(qb, 0, clen), np.clip(qe, 0, clen)
    want = np.where(ca < cb, csum[cb] - csum[ca], 0).astype(np.uint32)
    assert np.array_equal(ctx.depth_query(qb.astype(np.int32), qe.astype(np.int32)), want), clen
    return start, ln, depth


def test_depth_build_contigs_in_sequence_and_tile_edges():
    """im_depth_build call after call on ONE context, exact against numpy: contigs that grow, shrink and grow again (the array is
    reallocated, and a shorter contig's arrival counters lie where a longer one's tile offsets were), clen + 1 a multiple of the
    scan's 8192-position tile, 32 / 33 / 1025 tiles (the edges of the two-level arrival count and of the 1024-wide offset pass),
    an empty build, and the same build three times over."""
    from indelminer_amd import capi
    rng = np.random.default_rng(12)
    ctx = capi.Context(0)
    try:
        for clen, nseg in ((5000, 800), (3_000_000, 900_000), (100, 40), (3_000_001, 900_000),
                           (8191, 3000), (32 * 8192 - 1, 80_000), (32 * 8192, 80_000), (1024 * 8192, 1_200_000), (70_000, 0)):
            _depth_case(ctx, rng, clen, nseg)
        clen = 33 * 8192 - 1
        start, ln, depth = _depth_case(ctx, rng, clen, 90_000)
        p = np.arange(clen, dtype=np.int32)
        for _again in range(3):
            ctx.depth_build(clen, start, ln)
            assert np.array_equal(ctx.depth_query(p, p + 1), depth.astype(np.uint32))
    finally:
        ctx.close()


def test_support_sw_matches_oracle(gpu_ctx):
    """Annotate-mode SW (K7): forward-carried path statistics vs the oracle's full-matrix DP +
    traceback on random target/query pairs (planted indels, substitutions, lengths up to 255 x 1500)."""
    import ctypes as C
    from tests.support import oraclebind as ob
    L = ob.lib()
    rng = np.random.default_rng(5)
    targets, queries = [], []
    for it in range(460):
        len1 = int(rng.choice([40, 120, 200, 260, 700, 1500]))
        len2 = int(rng.choice([20, 64, 65, 100, 100, 128, 150, 255]))
        if it >= 400:                  # reads of up to IM_MAX_READ bases: the packed path statistics (11 + 11 + 10 bits) at their widest
            len1, len2 = int(rng.choice([1200, 2500, 4000])), int(rng.choice([256, 300, 600, 1020, 1020]))
        t = rng.choice(list(b"ACGT"), size=len1).astype(np.uint8)
        p = int(rng.integers(0, max(1, len1 - len2 // 2)))
        q = t[p:p + len2].copy()
        if len(q) < len2:
            q = np.concatenate([q, rng.choice(list(b"ACGT"), size=len2 - len(q)).astype(np.uint8)])
        typ = rng.random()
        if typ < 0.35 and len2 > 20:
            cut = int(rng.integers(5, len2 - 5)); d = int(rng.integers(1, 12))
            q = np.concatenate([q[:cut], q[cut + d:], rng.choice(list(b"ACGT"), size=d).astype(np.uint8)])
        elif typ < 0.7 and len2 > 20:
            cut = int(rng.integers(5, len2 - 5)); d = int(rng.integers(1, 12))
            q = np.concatenate([q[:cut], rng.choice(list(b"ACGT"), size=d).astype(np.uint8), q[cut:]])[:len2]
        elif typ < 0.8:
            q = rng.choice(list(b"ACGT"), size=len2).astype(np.uint8)
        sub = rng.random(len(q)) < rng.choice([0, 0.02, 0.1, 0.3] if it >= 400 else [0, 0.02, 0.1])
        q[sub] = rng.choice(list(b"ACGT"), size=int(sub.sum())).astype(np.uint8)
        if it % 17 == 0:
            q[len(q) // 2] = ord("N")
        if it % 23 == 0:
            t[len(t) // 3] = ord("N")
        targets.append(t.tobytes()); queries.append(q.tobytes())
    targets.append(b"ACGTACGT"); queries.append(b"TTTT")        # nothing positive... (a T matches)
    targets.append(b"AAAA"); queries.append(b"CCCC")            # all-nonpositive matrix
    got = gpu_ctx.support_batch(targets, queries)
    for k, (t, q) in enumerate(zip(targets, queries)):
        s, i, a = C.c_int32(), C.c_int32(), C.c_int32()
        L.imo_sw_indel(t, len(t), q, len(q), C.byref(s), C.byref(i), C.byref(a))
        assert tuple(got[k][:3]) == (s.value, i.value, a.value), (k, len(t), len(q), tuple(got[k]), (s.value, i.value, a.value))


def test_support_sw_long_windows_and_queries(gpu_ctx):
    """Windows beyond IM_MAX_SW_TARGET and queries beyond IM_MAX_READ (the reference takes any, src/variant.c:1246-1424): the
    support kernel's second form -- boundary row in device memory, 64-bit packed statistics -- in one batch with tasks of the LDS form"""
    import ctypes as C
    from indelminer_amd import capi
    from tests.support import oraclebind as ob
    L = ob.lib()
    rng = np.random.default_rng(77)
    targets, queries = [], []
    shapes = [(4096, 100), (5100, 100), (13000, 150), (9000, 300), (3000, 1021), (6000, 1500), (2000, 2600), (200, 100), (1500, 255), (4095, 1020), (20000, 64)]
    for it in range(40):
        len1, len2 = shapes[it % len(shapes)]
        t = rng.choice(list(b"ACGT"), size=len1).astype(np.uint8)
        p = int(rng.integers(0, max(1, len1 - len2)))
        q = t[p:p + len2].copy()
        if len(q) < len2:
            q = np.concatenate([q, rng.choice(list(b"ACGT"), size=len2 - len(q)).astype(np.uint8)])
        if it % 3 == 0:
            cut = int(rng.integers(5, len2 - 5)); d = int(rng.integers(1, 30))
            q = np.concatenate([q[:cut], q[cut + d:], rng.choice(list(b"ACGT"), size=d).astype(np.uint8)])
        elif it % 3 == 1:
            cut = int(rng.integers(5, len2 - 5)); d = int(rng.integers(1, 30))
            q = np.concatenate([q[:cut], rng.choice(list(b"ACGT"), size=d).astype(np.uint8), q[cut:]])[:len2]
        sub = rng.random(len(q)) < rng.choice([0, 0.02, 0.1])
        q[sub] = rng.choice(list(b"ACGT"), size=int(sub.sum())).astype(np.uint8)
        targets.append(t.tobytes()); queries.append(q.tobytes())
    got = gpu_ctx.support_batch(targets, queries)
    n_big = 0
    for k, (t, q) in enumerate(zip(targets, queries)):
        s, i, a = C.c_int32(), C.c_int32(), C.c_int32()
        L.imo_sw_indel(t, len(t), q, len(q), C.byref(s), C.byref(i), C.byref(a))
        assert tuple(got[k][:3]) == (s.value, i.value, a.value) and got[k][3] == capi.ST_EVIDENCE, (k, len(t), len(q), tuple(got[k]), (s.value, i.value, a.value))
        n_big += len(t) > 4095 or len(q) > capi.MAX_READ
    assert n_big >= 20


def test_cluster_kernels_match_reference_process_evidence(gpu_ctx):
    """the device cluster path against vectors the reference's own process_evidence produced (tests/golden/units_cluster.json)"""
    import json
    from tests.test_oracle_units import reference_clusters
    cases = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "units_cluster.json")))["cases"]
    for case in cases:
        cls, b1, b2 = case["cls"], case["b1"], case["b2"]
        for tie in (0, 1):
            order, first, count, used, k = gpu_ctx.cluster_sr(cls, b1, b2, case["marker"], tie)
            got = []
            for f, c in zip(first, count):
                m = [int(x) for x in order[f:f + c]]
                got.append(((cls[m[0]], b1[m[0]], b2[m[0]]), m))
            want = reference_clusters(case)
            assert got == (want if tie == 0 else [(key, m[::-1]) for key, m in want]), case["seed"]
            assert [int(x) for x in used] == case["used"]


def test_support_kernel_matches_reference_realign_with_indel(gpu_ctx):
    """the annotate-mode Smith-Waterman against vectors the reference's own realign_with_indel produced"""
    import json
    from tests.test_oracle_units import variant_window
    cases = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "units_sw.json")))["cases"]
    targets = [variant_window(c) for c in cases]
    queries = [c["read"][c["qstart"]:c["qstop"]].encode() for c in cases]
    got = gpu_ctx.support_batch(targets, queries)
    for k, c in enumerate(cases):
        assert [int(x) for x in got[k][:3]] == c["expect"], (k, c["expect"], tuple(got[k]))


def _sw_oracle(t, q):
    import ctypes as C
    from tests.support import oraclebind as ob
    s, i, a = C.c_int32(), C.c_int32(), C.c_int32()
    ob.lib().imo_sw_indel(t, len(t), q, len(q), C.byref(s), C.byref(i), C.byref(a))
    return [s.value, i.value, a.value]


def test_support_kernel_on_low_complexity_variants(gpu_ctx):
    """variants inside or at the edge of homopolymers and short tandem repeats, whole repeat units among them
    (tests/support/lowcomplexity.py: sw_cases): where equal-score paths are the norm the forward-carried path statistics must
    follow the path the reference's traceback prefers.  Against the reference's own realign_with_indel answers
    (tests/golden/ref_lowcomplexity.json) and against the oracle."""
    import json
    from tests.support import lowcomplexity as lc
    from tests.test_oracle_units import variant_window
    cases = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", lc.GOLDEN_NAME)))["sw"]
    assert len(cases) == 300 and sum(c["expect"][1] > 0 for c in cases) >= 100
    targets = [variant_window(c) for c in cases]
    queries = [c["read"][c["qstart"]:c["qstop"]].encode() for c in cases]
    got = gpu_ctx.support_batch(targets, queries)
    for k, c in enumerate(cases):
        assert [int(x) for x in got[k][:3]] == c["expect"], (k, c["expect"], tuple(got[k]))
        assert _sw_oracle(targets[k], queries[k]) == c["expect"], k


def test_support_sw_second_form_on_low_complexity(gpu_ctx):
    """the second form (windows beyond IM_MAX_SW_TARGET, queries beyond IM_MAX_READ) on targets of alternating random and repeat
    stretches; every query carries a deletion or an expansion of whole repeat units inside a repeat"""
    from indelminer_amd import capi
    from tests.support import lowcomplexity as lc
    shapes = [(4096, 100), (5100, 150), (9000, 300), (3000, 1021), (2000, 2600), (1500, 255)] * 4
    targets, queries = lc.support_pairs(88, shapes)
    assert [(len(t), len(q)) for t, q in zip(targets, queries)] == shapes
    got = gpu_ctx.support_batch(targets, queries)
    n_big = n_indel = 0
    for k, (t, q) in enumerate(zip(targets, queries)):
        want = _sw_oracle(t, q)
        assert [int(x) for x in got[k][:3]] == want and got[k][3] == capi.ST_EVIDENCE, (k, len(t), len(q), tuple(got[k]), want)
        n_big += len(t) > 4095 or len(q) > capi.MAX_READ
        n_indel += want[1] > 0
    assert 2 * n_big >= len(shapes) and n_indel >= len(shapes) // 3


def test_support_sw_hand_made_ties(gpu_ctx):
    """nothing but ties: a query that fits a pure repeat at every period, with one unit deleted or inserted, each once more with
    an N in the middle of the query"""
    from indelminer_amd import capi
    pairs = [(b"A" * 200, b"A" * 90),
             (b"AC" * 100, b"AC" * 40 + b"AC" * 38),
             (b"CAG" * 60, b"CAG" * 20 + b"CAG" + b"CAG" * 15)]
    # the same between flanks of 25 bases that occur once and pin both ends (50 points each; a gap of six bases costs 10):
    # two units deleted, two units inserted -- six indels each, their place in the repeat open -- and six units inserted
    f1, f2 = b"GTTACGGATCCATTGACGTA" * 2, b"TCGGATACCTGAATCGTTCA" * 2
    pairs += [(f1 + b"CAG" * 30 + f2, f1[-25:] + b"CAG" * n + f2[:25]) for n in (28, 32, 36)]
    targets, queries = [], []
    for t, q in pairs:
        targets += [t, t]
        queries += [q, q[:len(q) // 2] + b"N" + q[len(q) // 2 + 1:]]
    got = gpu_ctx.support_batch(targets, queries)
    indels = []
    for k, (t, q) in enumerate(zip(targets, queries)):
        want = _sw_oracle(t, q)
        assert [int(x) for x in got[k][:3]] == want and got[k][3] == capi.ST_EVIDENCE, (k, tuple(got[k]), want)
        indels.append(want[1])
    assert indels[6:10] == [6, 6, 6, 6], indels


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 50001, 600_001])
def test_compact_results_packs_exactly_the_records_with_evidence(gpu_ctx, n):
    """im_dev_compact_results: status and place of every read, the records with status == IM_ST_EVIDENCE and n_ev > 0 packed whole
    (any order), nothing else; also with the batch size read from device memory.  600 001 is more than the 8 x 256 CUs x 256 records of
    one grid: compact_results_kernel's workgroups take a second tile in their loop"""
    import ctypes as C
    from indelminer_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(n)
    res = np.frombuffer(rng.integers(0, 256, size=512 * max(n, 1), dtype=np.uint8).tobytes(), dtype=capi.RESULT_DTYPE).copy()
    res["status"] = rng.choice([0, 1, 1, -1, -2, -3], size=len(res))
    res["n_ev"] = rng.choice([0, 1, 2, 4], size=len(res))
    for n_live in ([n] if n < 100 else [n, n - 37]):
        d_res = capi.DevBuf(gpu_ctx, 512 * max(n, 1)).upload(res)
        d_stat, d_slot = capi.DevBuf(gpu_ctx, 4 * max(n, 1)), capi.DevBuf(gpu_ctx, 4 * max(n, 1))
        d_comp, d_cnt = capi.DevBuf(gpu_ctx, 512 * max(n, 1)), capi.DevBuf(gpu_ctx, 256)
        d_n = capi.DevBuf(gpu_ctx, 256).upload(np.array([n_live], np.int32))
        gpu_ctx._check(L.im_dev_compact_results(gpu_ctx.h, d_res.ptr, n, d_n.ptr if n_live != n else None, d_stat.ptr, d_slot.ptr, d_comp.ptr, d_cnt.ptr, gpu_ctx.stream))
        gpu_ctx._check(L.im_stream_sync(gpu_ctx.h, gpu_ctx.stream))
        cnt = int(d_cnt.download(np.int32, 1)[0])
        want = (res["status"][:n_live] == 1) & (res["n_ev"][:n_live] > 0)
        assert cnt == int(want.sum())
        if n_live:
            stat, slot = d_stat.download(np.int32, n_live), d_slot.download(np.int32, n_live)
            assert np.array_equal(stat, res["status"][:n_live])
            assert np.array_equal(slot >= 0, want)
            assert sorted(slot[want].tolist()) == list(range(cnt))
            if cnt:
                comp = d_comp.download(capi.RESULT_DTYPE, cnt)
                assert comp[slot[want]].tobytes() == res[:n_live][want].tobytes()
        for b in (d_res, d_stat, d_slot, d_comp, d_cnt, d_n):
            b.free()
