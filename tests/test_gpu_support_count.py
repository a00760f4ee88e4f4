"""im_support_count (seam 4, counting form) against the restatement: per known variant the number of tasks that pass
check_for_indel's verdict, {N_all, AS, DC}.  The windows are built here in Python (tests/support/knowncounts.py: window), their
Smith-Waterman statistics come from the CPU checker (imo_sw_indel) and, a second time, from im_support_batch on those windows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _contigs(rng):
    out = []
    for n in (60_000, 9_000):
        a = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
        for _ in range(n // 700):                                   # lower-case stretches: the score folds case, the substitution count does not
            p = int(rng.integers(0, n - 80)); ln = int(rng.integers(5, 80))
            a[p:p + ln] |= 0x20
        out.append(a.tobytes())
    return out


def _expected(capi, kc, contigs, variants, alts, tasks, queries, stats_of):
    want = np.zeros((len(variants), 3), np.int64)
    need = [i for i, t in enumerate(tasks) if not t["flags"] & capi.SC_DIRECT]
    wins = []
    for i in need:
        t, v = tasks[i], variants[tasks[i]["variant"]]
        alt = alts[v["alt_off"]:v["alt_off"] + v["alt_len"]]
        wins.append(kc.window(contigs[v["tid"]], int(v["type"]), int(v["start"]), int(v["stop"]), alt, int(t["rstart"]), int(t["rstop"])))
    stats = dict(zip(need, stats_of(wins, [queries[tasks[i]["q_off"]:tasks[i]["q_off"] + tasks[i]["q_len"]] for i in need])))
    for i, t in enumerate(tasks):
        ok = bool(t["flags"] & capi.SC_DIRECT)
        if not ok:
            s, d, a = stats[i]
            ok = s <= t["own_subs"] and d <= t["own_indels"] and a >= t["own_aligned"]
        if ok:
            want[t["variant"], 0] += 1
            if t["flags"] & capi.SC_MAPQ_OK:
                want[t["variant"], 1] += 1
                if t["flags"] & capi.SC_SPANS:
                    want[t["variant"], 2] += 1
    return want, wins


def _check(ctx, capi, kc, contigs, variants, alts, tasks, queries):
    got = ctx.support_count(variants, alts, tasks, queries).astype(np.int64)
    want_cpu, wins = _expected(capi, kc, contigs, variants, alts, tasks, queries, lambda ws, qs: [kc.sw_stats(w, q) for w, q in zip(ws, qs)])
    want_dev, _ = _expected(capi, kc, contigs, variants, alts, tasks, queries, lambda ws, qs: [tuple(int(x) for x in r[:3]) for r in ctx.support_batch(ws, qs)])
    assert np.array_equal(want_cpu, want_dev)
    bad = np.nonzero((got != want_cpu).any(axis=1))[0]
    assert len(bad) == 0, (bad[:10], got[bad[:10]], want_cpu[bad[:10]])
    return got, wins


def _mutate(rng, q, rate):
    q = np.frombuffer(q, np.uint8).copy()
    hit = rng.random(len(q)) < rate
    q[hit] = rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), int(hit.sum()))
    return q.tobytes()


def test_support_count_random_tasks():
    from indelminer_amd import capi
    from tests.support import knowncounts as kc
    rng = np.random.default_rng(20)
    contigs = _contigs(rng)
    ctx = capi.Context(0)
    ctx.set_reference(contigs)
    variants, alts = [], b""
    for v in range(120):
        tid = v % 2
        clen = len(contigs[tid])
        typ = kc.DEL if v % 3 else kc.INS
        size = int(rng.integers(1, 60))
        # the first and last few variants sit at the contig's ends: their reads' stretches are clipped there
        start = int(rng.integers(1, 40)) if v < 6 else (clen - int(rng.integers(1, 40)) - (size if typ == kc.DEL else 0) if v >= 114 else int(rng.integers(300, clen - 400)))
        alt = contigs[tid][start - 1:start] + (bytes(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), size)) if typ == kc.INS else b"")
        stop = start + size + 1 if typ == kc.DEL else start + 1
        variants.append((tid, start, stop, typ, len(alts), len(alt)))
        alts += alt
    variants = np.array(variants, dtype=capi.KNOWN_VARIANT_DTYPE)
    tasks, queries = [], b""
    for i in range(4000):
        v = int(rng.integers(0, 118)) if i >= 80 else (118 if i < 40 else 119)
        k = variants[v]
        clen = len(contigs[k["tid"]])
        size = k["stop"] - k["start"] - 1 if k["type"] == kc.DEL else k["alt_len"] - 1
        rs0 = int(k["start"]) - int(rng.integers(5, 140)); re0 = int(k["stop"]) + int(rng.integers(5, 140))
        rstart, rstop = max(rs0 - size, 0), min(re0 + size, clen)
        flags = int(rng.integers(0, 8)) & ~capi.SC_DIRECT | (capi.SC_DIRECT if rng.random() < 0.1 else 0)
        src = rng.random()
        alt = alts[k["alt_off"]:k["alt_off"] + k["alt_len"]]
        with_variant = kc.window(contigs[k["tid"]], int(k["type"]), int(k["start"]), int(k["stop"]), alt, max(rs0, 0), min(re0, clen))
        plain = contigs[k["tid"]][max(rs0, 0):min(re0, clen)]
        q = _mutate(rng, with_variant if src < 0.6 else plain, float(rng.choice([0, 0.01, 0.05])))
        if rng.random() < 0.3:
            q = q.upper()
        own = (int(rng.integers(0, 6)), int(rng.integers(0, 70)), len(q) - int(rng.integers(0, 12)))
        if v == 118:                                        # every read supports
            own = (5000, 5000, 0)
        if v == 119:                                        # none does
            own = (0, 0, 100000); flags &= ~capi.SC_DIRECT
        tasks.append((v, rstart, rstop, len(queries), len(q)) + own + (flags,))
        queries += q
    tasks = np.array(tasks, dtype=capi.COUNT_TASK_DTYPE)
    got, wins = _check(ctx, capi, kc, contigs, variants, alts, tasks, queries)
    assert {int(t) for t in variants["type"]} == {kc.INS, kc.DEL}
    assert {int(f) for f in tasks["flags"]} == set(range(8))
    assert got[119, 0] == 0 and got[118, 0] == 40
    assert 0 < got[:118, 0].sum() < 3920 and got[:, 2].sum() > 0 and (got[:, 1] < got[:, 0]).any()
    assert any(t["rstart"] == 0 for t in tasks) and any(t["rstop"] == len(contigs[variants[t["variant"]]["tid"]]) for t in tasks)
    assert any(w != w.upper() for w in wins)
    # a second call on the same context, another order: integer adds, the same counts
    perm = rng.permutation(len(tasks))
    assert np.array_equal(ctx.support_count(variants, alts, tasks[perm], queries), got)
    # a variant without tasks, no tasks at all
    assert np.array_equal(ctx.support_count(variants, alts, tasks[:0], b""), np.zeros((120, 3), np.int32))
    ctx.close()


def test_support_count_mixes_lds_form_tasks_with_tasks_beyond_it():
    """a known deletion of 2500 bases whose reads' stretches make windows beyond IM_MAX_SW_TARGET, a query above IM_MAX_READ, and
    ordinary tasks, in one batch"""
    from indelminer_amd import capi
    from tests.support import knowncounts as kc
    rng = np.random.default_rng(21)
    contigs = _contigs(rng)
    ctx = capi.Context(0)
    ctx.set_reference(contigs)
    c0 = contigs[0]
    alts = c0[19999:20000] + c0[29999:30000] + c0[39999:40000] + b"ACGTTGCA" * 40
    variants = np.array([(0, 20000, 20000 + 2501, kc.DEL, 0, 1), (0, 30000, 30006, kc.DEL, 1, 1), (0, 40000, 40001, kc.INS, 2, 321)], dtype=capi.KNOWN_VARIANT_DTYPE)
    tasks, queries = [], b""

    def add(v, rstart, rstop, q, own, flags):
        nonlocal queries
        tasks.append((v, rstart, rstop, len(queries), len(q)) + own + (flags,))
        queries += q
    for i in range(24):
        k = variants[0]
        lo = 20000 - int(rng.integers(40, 90)); hi = 22501 + int(rng.integers(40, 90))
        alt = alts[0:1]
        good = kc.window(c0, kc.DEL, 20000, 22501, alt, lo, hi)
        q = _mutate(rng, good if i % 2 else c0[lo:lo + len(good)], 0.01)
        add(0, lo - 2500, hi + 2500, q, (3, 2500, len(q) - 3), int(rng.integers(0, 8)) & ~capi.SC_DIRECT)          # window of about 5.3 kb
    for i in range(60):
        lo = 30000 - int(rng.integers(20, 120)); hi = 30006 + int(rng.integers(20, 120))
        good = kc.window(c0, kc.DEL, 30000, 30006, alts[1:2], lo, hi)
        q = _mutate(rng, good if i % 3 else c0[lo:hi], 0.01)
        add(1, lo - 5, hi + 5, q, (2, 5, len(q) - 2), int(rng.integers(0, 8)))
    for i in range(6):
        lo, hi = 40000 - 500, 40000 + 400
        good = kc.window(c0, kc.INS, 40000, 40001, alts[2:323], lo, hi)          # 1220 bases: a query above IM_MAX_READ
        q = _mutate(rng, good if i % 2 else c0[lo:lo + 1100], 0.005)
        add(2, lo - 320, hi + 320, q, (12, 320, len(q) - 10), capi.SC_MAPQ_OK | (capi.SC_SPANS if i < 3 else 0))
    tasks = np.array(tasks, dtype=capi.COUNT_TASK_DTYPE)
    got, wins = _check(ctx, capi, kc, contigs, variants, alts, tasks, queries)
    assert sum(len(w) > 4095 for w in wins) >= 24 and max(int(t["q_len"]) for t in tasks) > capi.MAX_READ
    assert (got[:, 0] > 0).all(), got
    ctx.close()


def test_support_count_on_whole_repeat_unit_variants():
    """known variants that delete or expand whole repeat units inside a homopolymer or a short tandem repeat
    (tests/support/lowcomplexity.py: sw_cases), every read's own numbers one below, at or one above what the Smith-Waterman gives
    for it, so that a count moves with any path statistic that comes out differently among the equal-score paths of a repeat"""
    import json
    import os
    from indelminer_amd import capi
    from tests.support import knowncounts as kc, lowcomplexity as lc
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", lc.GOLDEN_NAME)))["sw"]
    made = lc.sw_cases(lc.SW_SEED, lc.SW_N)
    rng = np.random.default_rng(22)
    contig, variants, alts, tasks, queries = b"", [], b"", [], b""
    for c, g in zip(made, gold):
        assert lc.sw_inputs(c) == {k: v for k, v in g.items() if k != "expect"}
        if not (c["in_repeat"] and c["whole_units"]):
            continue
        base = len(contig)                                          # the cases' stretches one after another: one contig
        contig += c["contig"].encode()
        typ = kc.DEL if c["is_deletion"] else kc.INS
        alt = c["alternate"].encode()
        variants.append((0, base + c["vstart"], base + (c["vstop"] if typ == kc.DEL else c["vstart"] + 1), typ, len(alts), len(alt)))
        alts += alt
        q = c["read"][c["qstart"]:c["qstop"]].encode()
        for _ in range(3):
            own = tuple(int(x) + int(rng.integers(-1, 2)) for x in g["expect"])
            tasks.append((len(variants) - 1, base + c["rstart"], base + c["rstop"], len(queries), len(q)) + own + (int(rng.integers(0, 8)) & ~capi.SC_DIRECT,))
        queries += q
    assert len(variants) >= 60
    variants = np.array(variants, dtype=capi.KNOWN_VARIANT_DTYPE)
    tasks = np.array(tasks, dtype=capi.COUNT_TASK_DTYPE)
    ctx = capi.Context(0)
    ctx.set_reference([contig])
    got, wins = _check(ctx, capi, kc, [contig], variants, alts, tasks, queries)
    assert {int(t) for t in variants["type"]} == {kc.INS, kc.DEL}
    assert 0 < got[:, 0].sum() < len(tasks) and got[:, 2].sum() > 0
    ctx.close()
