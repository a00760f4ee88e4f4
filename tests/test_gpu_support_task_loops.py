"""The Smith-Waterman kernels of im_support.hip past one grid.  Every one of them gives a workgroup of one wave to a task and takes task
+ gridDim.x in the same workgroup: support_kernel<false> and support_count_kernel past 2^20 workgroups, support_kernel<true> and
support_count_big_kernel past 2 048, or past fewer where the 2 GiB budget of the boundary rows cuts the grid.  A second task in a
workgroup meets what the first left: the window in LDS, the parked boundary row (rowV, rowF, rowS -- in device memory for the big
forms, where the first task's row may be longer than the second's window), the running best.

The yardstick is the CPU checker's imo_sw_indel, called once per DISTINCT pair; a batch is those pairs tiled, and the expected rows are
the distinct rows tiled the same way with numpy.  Everything is an integer and every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SENTINEL = 0x77777777
GRID_LDS, GRID_BIG = 1 << 20, 2048             # launch_support, support_big_scratch_bytes (im_support.hip)


def make_pair(rng, len1, len2, indel=None):
    """(window, query): len1 random bases and a query of len2 cut from them (with random bases around the window where it is the
    shorter one), a deletion or an insertion of 1 .. 12 bases in the query's middle, and one substitution"""
    t = rng.choice(ACGT, len1)
    if len2 <= len1:
        p = int(rng.integers(0, len1 - len2 + 1))
        q = t[p:p + len2].copy()
    else:
        more = len2 - len1
        q = np.concatenate([rng.choice(ACGT, more // 2), t, rng.choice(ACGT, more - more // 2)])
    cut, d = len(q) // 2, int(rng.integers(1, max(2, min(13, len(q) // 3))))
    if indel == "del":
        q = np.concatenate([q[:cut], q[cut + d:], rng.choice(ACGT, d)])
    elif indel == "ins":
        q = np.concatenate([q[:cut], rng.choice(ACGT, d), q[cut:]])[:len2]
    q[len(q) // 3] = ACGT[int(rng.integers(0, 4))]
    assert len(t) == len1 and len(q) == len2
    return t.tobytes(), q.tobytes()


def rows_of(pairs):
    """int32 [n, 4] the checker gives for every pair: subs, indels, aligned, IM_ST_EVIDENCE"""
    from tests.support import knowncounts as kc
    return np.array([kc.sw_stats(t, q) + (1,) for t, q in pairs], np.int32)


def packed(parts):
    """(bytes one after another with 8 more behind them, int64 offsets [n + 1]) of a list of bytes"""
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(x) for x in parts], out=off[1:])
    return np.frombuffer(b"".join(parts) + b"\0" * 8, np.uint8).copy(), off


def raw_batch(ctx, n, t, t_off, q, q_off):
    """im_support_batch itself over an output full of SENTINEL"""
    from indelminer_amd import capi
    out = np.full((n, 4), SENTINEL, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().im_support_batch(ctx.h, n, p(t), p(t_off), p(q), p(q_off), p(out))
    assert rc == 0, capi.lib().im_last_error(ctx.h).decode()
    return out


def check_rows(got, want, grid):
    bad = np.nonzero((got != want).any(axis=1))[0][:6]
    # (task, its workgroup, its trip, got, expected) of the first rows that differ
    assert len(bad) == 0 and got.shape == want.shape, [(int(i), int(i) % grid, int(i) // grid, got[i].tolist(), want[i].tolist()) for i in bad]


def batch_of(ctx, pool, idx):
    """the batch whose task i is pool[idx[i]], through the C entry; returns (rows, the pool's expected rows tiled)"""
    t, t_off = packed([pool[k][0] for k in idx])
    q, q_off = packed([pool[k][1] for k in idx])
    return raw_batch(ctx, len(idx), t, t_off, q, q_off), rows_of(pool)[np.asarray(idx)]


@pytest.fixture()
def ctx():
    from indelminer_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def test_a_second_big_task_in_one_workgroup(ctx):
    """support_kernel<true>: 2 112 tasks over a grid of 2 048; tasks i and i + 2 048, i < 64, are both beyond the LDS form, one by its
    window (4 096 .. 5 000 bases against 80 .. 150) and one by its query (1 021 .. 1 400 against a window of 40 .. 400), in either order:
    the second meets a parked row longer than its window, or shorter.  Every other task is of the LDS form, from 16 distinct pairs"""
    rng = np.random.default_rng(2112)
    n = 2_112
    by_window = lambda k: make_pair(rng, int(rng.integers(4_096, 5_001)), int(rng.integers(80, 151)), (None, "del", "ins")[k % 3])
    by_query = lambda k: make_pair(rng, int(rng.integers(40, 401)), int(rng.integers(1_021, 1_401)), (None, "del", "ins")[k % 3])
    pool = [make_pair(rng, int(rng.integers(60, 400)), int(rng.integers(40, 150)), (None, "del", "ins")[k % 3]) for k in range(16)]
    idx = [k % 16 for k in range(n)]
    for i in range(64):
        first, second = (by_window(i), by_query(i)) if i % 2 == 0 else (by_query(i), by_window(i))
        idx[i], idx[i + GRID_BIG] = len(pool), len(pool) + 1
        pool += [first, second]
    big = lambda p: len(p[0]) > 4_095 or len(p[1]) > 1_020
    assert n > GRID_BIG and all(big(pool[idx[i]]) and big(pool[idx[i + GRID_BIG]]) for i in range(64)) and sum(big(pool[k]) for k in idx) == 128
    longer = [len(pool[idx[i]][0]) > len(pool[idx[i + GRID_BIG]][0]) for i in range(64)]
    assert sum(longer) == 32 and max(len(p[0]) for p in pool) * 16 * GRID_BIG < 2 << 30            # both orders; the budget does not cut this grid
    got, want = batch_of(ctx, pool, idx)
    assert len({tuple(r) for r in want[:64].tolist()}) > 50 and (want[:, 1] > 0).sum() > n // 3
    check_rows(got, want, GRID_BIG)


def test_the_lds_form_past_two_to_the_twenty_workgroups(ctx):
    """support_kernel<false>: 2^20 + 130 tasks.  Tasks 0 .. 129 are real-sized (windows of 250 .. 400, reads of 100 .. 150); the last
    130, the second trips of the same workgroups, are real-sized but shorter, half with a deletion and half with an insertion; the middle
    is 251 distinct tiny pairs going round, one of them all-nonpositive and one with an N"""
    rng = np.random.default_rng(1 << 20)
    n = GRID_LDS + 130
    first = [make_pair(rng, int(rng.integers(250, 401)), int(rng.integers(100, 151)), (None, "del", "ins")[k % 3]) for k in range(130)]
    last = [make_pair(rng, int(rng.integers(120, 241)), int(rng.integers(50, 100)), ("del", "ins")[k % 2]) for k in range(130)]
    tiny = [make_pair(rng, int(rng.integers(6, 41)), int(rng.integers(4, 31)), (None, "del", "ins")[k % 3]) for k in range(251)]
    tiny[7] = (b"AAAAAA", b"CCCC")
    tiny[19] = (tiny[19][0], tiny[19][1][:2] + b"N" + tiny[19][1][3:])
    middle = n - 260
    reps, rest = divmod(middle, 251)
    assert middle > 0 and rest > 0 and all(len(a[0]) > len(b[0]) and len(a[1]) > len(b[1]) for a, b in zip(first, last))
    cols = []
    for k in (0, 1):
        parts = [x[k] for x in first], [x[k] for x in tiny], [x[k] for x in tiny[:rest]], [x[k] for x in last]
        blob = b"".join(parts[0]) + b"".join(parts[1]) * reps + b"".join(parts[2]) + b"".join(parts[3]) + b"\0" * 8
        lens = np.concatenate([[len(x) for x in parts[0]], np.tile([len(x) for x in parts[1]], reps), [len(x) for x in parts[2]], [len(x) for x in parts[3]]])
        off = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        assert off[n] + 8 == len(blob)
        cols += [np.frombuffer(blob, np.uint8).copy(), off]
    rows = [rows_of(first), rows_of(tiny), rows_of(last)]
    want = np.concatenate([rows[0], np.tile(rows[1], (reps, 1)), rows[1][:rest], rows[2]])
    assert tuple(rows[1][7][:3]) == (0, 0, 1) and len(want) == n and (rows[2][:, 1] > 0).sum() > 100
    got = raw_batch(ctx, n, *cols)
    check_rows(got, want, GRID_LDS)


def test_the_grid_the_scratch_budget_cuts(ctx):
    """support_kernel<true> with fewer workgroups than tasks because of ONE long window: 2 048 tasks, one of 70 000 bases, 2 GiB of
    boundary rows at 16 bytes per base of the longest window rounded up -- 1 917 workgroups; big tasks sit at i and i + 1 917, i < 32.
    The grid is not handed out by any entry: the assert below guards this test's own copy of support_big_scratch_bytes' rule, which has
    to be kept in step with im_support.hip by hand"""
    n, longest = 2_048, 70_000
    cap = (longest + 4) & ~3                                        # support_big_scratch_bytes: the row capacity ..
    grid = min(n, GRID_BIG, (2 << 30) // (16 * cap))                # .. V, F and the 64-bit statistics per base, within 2 GiB
    assert grid == 1_917 < n                                        # the copy of the rule: tasks i and i + grid share a workgroup
    rng = np.random.default_rng(1917)
    pool = [make_pair(rng, int(rng.integers(60, 400)), int(rng.integers(40, 150)), (None, "del", "ins")[k % 3]) for k in range(16)]
    idx = [k % 16 for k in range(n)]
    for i in range(32):
        for at in (i, i + grid):
            idx[at] = len(pool)
            if at == 5:
                pool.append(make_pair(rng, longest, 100, "del"))
            elif (i + (at >= grid)) % 2:
                pool.append(make_pair(rng, int(rng.integers(4_096, 5_001)), int(rng.integers(80, 151)), ("del", "ins")[i % 2]))
            else:
                pool.append(make_pair(rng, int(rng.integers(40, 401)), int(rng.integers(1_021, 1_401)), ("del", "ins")[i % 2]))
    assert max(len(p[0]) for p in pool) == longest and 31 + grid < n and len(pool) == 16 + 64
    got, want = batch_of(ctx, pool, idx)
    check_rows(got, want, grid)


def _variants(rng, contig, ins_size=None):
    """(variants, alts): six known variants 2 500 bases apart, insertions and deletions by turns, of 3 .. 20 bases (ins_size: the insertions')"""
    from indelminer_amd import capi
    from tests.support import knowncounts as kc
    variants, alts = [], b""
    for v in range(6):
        typ = kc.DEL if v % 2 else kc.INS
        size = ins_size if typ == kc.INS and ins_size else int(rng.integers(3, 21))
        start = 2_500 + 2_500 * v
        alt = contig[start - 1:start] + (bytes(rng.choice(ACGT, size)) if typ == kc.INS else b"")
        variants.append((0, start, start + size + 1 if typ == kc.DEL else start + 1, typ, len(alts), len(alt)))
        alts += alt
    return np.array(variants, dtype=capi.KNOWN_VARIANT_DTYPE), alts


def _tasks(rng, contig, variants, alts, n_distinct, q_lens, q_base=0):
    """(the distinct tasks, their query bytes, whether each supports): n_distinct reads across the variants, their queries from q_base
    on; a read's own numbers are one below, at or one above what the checker gives for its window, so that a count moves with any
    statistic that comes out differently"""
    from indelminer_amd import capi
    from tests.support import knowncounts as kc
    tasks, queries, ok = [], b"", []
    for j in range(n_distinct):
        k = variants[j % 6]
        alt = alts[k["alt_off"]:k["alt_off"] + k["alt_len"]]
        typ, start, stop = int(k["type"]), int(k["start"]), int(k["stop"])
        size = stop - start - 1 if typ == kc.DEL else int(k["alt_len"]) - 1
        want_len = int(rng.integers(*q_lens))
        lo = start - want_len // 2
        with_variant = kc.window(contig, typ, start, stop, alt, lo, lo + want_len + size)
        q = bytearray((with_variant if j % 3 else contig[lo:lo + want_len + size])[:want_len])
        q[len(q) // 4] = ord("ACGT"[j % 4])
        rstart, rstop = lo - size, lo + want_len + 2 * size
        s, d, a = kc.sw_stats(kc.window(contig, typ, start, stop, alt, rstart, rstop), bytes(q))
        own = (s + int(rng.integers(-1, 2)), d + int(rng.integers(-1, 2)), a + int(rng.integers(-1, 2)))
        ok.append(s <= own[0] and d <= own[1] and a >= own[2])
        tasks.append((j % 6, rstart, rstop, q_base + len(queries), len(q)) + own + (int(rng.integers(0, 4)) << 1,))
        queries += bytes(q)
    return np.array(tasks, dtype=capi.COUNT_TASK_DTYPE), queries, np.array(ok)


def _expected_counts(capi, tasks, ok, idx):
    """[6, 3] from the per-distinct verdict times the multiplicity"""
    mult = np.bincount(idx, minlength=len(tasks))
    want = np.zeros((6, 3), np.int64)
    for t, good, m in zip(tasks, ok, mult):
        if good:
            want[t["variant"], 0] += m
            if t["flags"] & capi.SC_MAPQ_OK:
                want[t["variant"], 1] += m
                if t["flags"] & capi.SC_SPANS:
                    want[t["variant"], 2] += m
    return want


def test_support_count_past_both_grids():
    """support_count_kernel: 2^20 + 130 tasks tiled from 64 distinct ones that share their query bytes, with tasks that support
    directly among the first 130 and the last 130 -- a continue in front of the barriers of the workgroup's next task;
    support_count_big_kernel: 2 112 tasks beyond the LDS form by their query (1 021 .. 1 300 bases) tiled from 16, between short ones.
    64 and 16 divide the grids, so the tiling goes on by an odd step at every trip: the second task of a workgroup is another task
    than its first, of the other kind of variant (a deletion behind an insertion and the other way round), of another length"""
    from indelminer_amd import capi
    rng = np.random.default_rng(64)
    contig = bytes(rng.choice(ACGT, 20_000))
    ctx = capi.Context(0)
    try:
        ctx.set_reference([contig])
        # the LDS form
        variants, alts = _variants(rng, contig)
        tasks, queries, ok = _tasks(rng, contig, variants, alts, 64, (40, 121))
        direct = tasks[:4].copy()
        direct["flags"] = [capi.SC_DIRECT | f for f in (0, capi.SC_MAPQ_OK, capi.SC_MAPQ_OK | capi.SC_SPANS, capi.SC_SPANS)]
        direct["own_subs"], direct["own_aligned"] = -1, 1 << 20            # numbers no alignment meets: only the flag lets them count
        pool, ok = np.concatenate([tasks, direct]), np.concatenate([ok, [True] * 4])
        n = GRID_LDS + 130
        at = np.arange(n)
        idx = (at + 7 * (at // GRID_LDS)) % 64                           # 64 divides the grid: the second trips go on by an odd 7 ..
        idx[[3, 77, 129, n - 130, n - 66, n - 1]] = [64, 65, 66, 67, 64, 65]
        one, two = pool[idx[:130]], pool[idx[GRID_LDS:]]                 # .. so a workgroup's two tasks differ: the other kind of variant
        assert (idx[:130] != idx[GRID_LDS:]).all() and ((variants["type"][one["variant"]] != variants["type"][two["variant"]]) | (idx[:130] >= 64) | (idx[GRID_LDS:] >= 64)).all()
        span = lambda t: t["rstop"] - t["rstart"]
        assert (span(one) > span(two)).sum() > 30 and (span(one) < span(two)).sum() > 30 and (one["q_len"] != two["q_len"]).sum() > 100
        want = _expected_counts(capi, pool, ok, idx)
        assert 8 < ok[:64].sum() < 56 and (want[:, 0] > 0).all() and (want[:, 0] > want[:, 1]).any() and want[:, 2].sum() > 0 and want[:, 0].sum() < n
        got = ctx.support_count(variants, alts, pool[idx], queries).astype(np.int64)
        assert np.array_equal(got, want), (got.tolist(), want.tolist())
        # the form beyond it: the insertions are of 300 bases
        variants, alts = _variants(rng, contig, ins_size=300)
        big, queries, ok_big = _tasks(rng, contig, variants, alts, 16, (1_021, 1_301))
        short, queries_s, ok_short = _tasks(rng, contig, variants, alts, 16, (40, 121), q_base=len(queries))
        assert big["q_len"].min() > capi.MAX_READ and short["q_len"].max() <= capi.MAX_READ
        pool, ok = np.concatenate([big, short]), np.concatenate([ok_big, ok_short])
        n_big, n_short = 2_112, 500
        is_short = np.zeros(n_big + n_short, bool)
        is_short[np.arange(n_short) * 5 + 2] = True                      # every fifth task of the first 2 500 is a short one
        idx = np.empty(n_big + n_short, np.int64)
        b = np.arange(n_big)
        of_big = (b + 5 * (b // GRID_BIG)) % 16                          # 16 divides the grid: the second trips go on by an odd 5
        idx[~is_short], idx[is_short] = of_big, 16 + np.arange(n_short) % 16
        one, two = big[of_big[:n_big - GRID_BIG]], big[of_big[GRID_BIG:]]   # the two big tasks of the workgroups that take two
        assert n_big > GRID_BIG and (~is_short).sum() == n_big and (of_big[:n_big - GRID_BIG] != of_big[GRID_BIG:]).all()
        assert (variants["type"][one["variant"]] != variants["type"][two["variant"]]).all() and (one["q_len"] != two["q_len"]).all()
        assert (one["q_len"] > two["q_len"]).sum() > 10 and (one["q_len"] < two["q_len"]).sum() > 10
        want = _expected_counts(capi, pool, ok, idx)
        got = ctx.support_count(variants, alts, pool[idx], queries + queries_s).astype(np.int64)
        assert 0 < ok_big.sum() < 16 and np.array_equal(got, want), (got.tolist(), want.tolist())
    finally:
        ctx.close()
