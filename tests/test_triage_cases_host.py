"""The inputs of tests/test_gpu_triage_shapes.py reach what they claim to reach: every generator of tests/support/triagecases.py
through the CPU oracle alone.  A generator that misses its target fails here, not silently on the GPU."""
import struct

import numpy as np

from tests.support import oraclebind as ob
from tests.support import triagecases as tc


def _tri(recs, names=("generic",), ranges=(700,), **kw):
    raw, off = tc.batch(recs)
    return ob.triage_records(raw, off, list(names), list(ranges), **kw)


def test_length_cases_give_both_strands_at_every_length():
    cases = tc.length_cases()
    tri = _tri([r for r, _ in cases])
    seen = {}
    for (r, m), (t, b) in zip(cases, tri):
        assert tc.l_seq_of(r) == m["L"]
        if m["kind"] == "unmapped":
            assert t.cls == 2 and bool(t.revcomp) == m["revcomp"] and len(b) == m["L"]
        else:
            assert t.cls == (3 if m["cand"] else 1)
        if t.cls in (2, 3):
            seen.setdefault(m["L"], set()).add((t.cls, bool(t.revcomp)))
    for L in tc.LENGTHS:
        assert {(2, False), (2, True)} <= seen[L], L
        if L >= 12:
            assert {(3, False), (3, True)} <= seen[L], L
    assert sorted(seen) == sorted(tc.LENGTHS) and tc.LENGTHS[-1] < 4096
    # bases of all five letters
    assert set(b"".join(b for t, b in tri if b)) == set(b"ACGTN")


def test_length_layout_waves_differ():
    recs, waves = tc.length_layout(tc.length_cases())
    assert [k for k, _ in waves].count("one129") == 6 and {lane for k, lane in waves if k == "one129"} == {0, 7, 8, 15, 16, 63}
    for w, (kind, lane) in enumerate(waves):
        wave = recs[64 * w:64 * w + 64]
        ls = [tc.l_seq_of(r) for r in wave]
        if kind == "short":
            assert max(ls) <= 128
        elif kind == "one129":
            assert ls[lane] == 129 and tc.sweeps(wave[lane]) and max(l for k, l in enumerate(ls) if k != lane) <= 128
        elif kind == "one257":
            assert ls[lane] > 256 and tc.sweeps(wave[lane]) and max(l for k, l in enumerate(ls) if k != lane) <= 128
        else:
            assert min(ls) > 128 and max(ls) > 256 and all(tc.sweeps(r) for r in wave)
    # every case is in the batch
    assert set(r for r, _ in tc.length_cases()) <= set(recs)


def test_base_cases_put_every_refused_code_at_every_position():
    cases = tc.base_cases()
    tri = _tri([r for r, _ in cases])
    for (r, m), (t, _) in zip(cases, tri):
        assert t.cls == m["expect"], (m, t.cls)
    for L in tc.BASE_LENGTHS:
        want = {(p, c) for p in set(q for q in tc.BASE_POSITIONS if q < L) | {L - 1} for c in tc.REFUSED}
        got = set()
        for r, m in cases:
            if m["kind"] == "one" and m["L"] == L:
                # read the nibble back from the record itself
                o = 32 + r[8] + 4 * struct.unpack_from("<H", r, 12)[0]
                code = (r[o + (m["p"] >> 1)] >> (0 if m["p"] & 1 else 4)) & 15
                assert code == m["code"]
                got.add((m["p"], code))
        assert got == want, L
    kinds = {(m["kind"], m["L"]) for _, m in cases}
    for L in tc.BASE_LENGTHS:
        for k in ("two", "op", "in_clip", "in_ins", "past_lseq", "past_record"):
            assert (k, L) in kinds
        assert ((("padding", L) in kinds)) == bool(L & 1)
    ops = {(m["op"], m["d"], m["expect"]) for _, m in cases if m["kind"] == "op"}
    assert ops == {(op, d, 20 if d < 0 else 18) for op in (3, 5, 6, 9) for d in (-1, 0, 1)}
    assert {(m["k"], m["expect"]) for _, m in cases if m["kind"] == "past_lseq"} == {(k, e) for k in (1, 6, 20) for e in (1, 20)}
    assert {m["expect"] for _, m in cases if m["kind"] == "past_record"} == {1, 20}
    # the layout: cases at lane 0 and lane 63, and some in the last, partly filled wave of a partly filled workgroup
    recs = tc.base_layout(cases)
    mine = set(r for r, _ in cases)
    assert sum(1 for k in range(0, len(recs), 64) if recs[k] in mine and all(r not in mine for r in recs[k + 1:k + 63])) >= 20
    assert sum(1 for k in range(63, len(recs), 64) if recs[k] in mine and all(r not in mine for r in recs[k - 62:k])) >= 20
    assert len(recs) % 256 > 128 and 0 < len(recs) % 64 < 10 and all(r in mine for r in recs[len(recs) // 64 * 64:])


def test_aux_cases_cover_every_prefix_length_and_type():
    cases = tc.aux_cases()
    tri = _tri([r for r, _ in cases], tc.AUX_NAMES, tc.AUX_RANGES)
    assert {m["T"] for _, m in cases if m["kind"] == "prefix"} >= set(range(61))
    for T in range(61):
        assert {m["tail"] for _, m in cases if m["kind"] == "prefix" and m["T"] == T} == {"rg", "mq", "rg_mq", "mq_rg"}
    types = {t for _, m in cases for t, _, _ in m["parts"]}
    assert set("AcCsSiIfdZH") <= types and {"B" + e for e in "cCsSiIfdA"} <= types
    zlens = {s - 4 for _, m in cases for t, _, s in m["parts"] if t in "ZH"}
    assert set(range(31)) <= zlens
    # the terminator of a string on every offset of a 24-byte window, whether the window stands at the aux area's start or anywhere behind
    term = {(o + s - 1) % 24 for _, m in cases for t, o, s in m["parts"] if t in "ZH"}
    assert term == set(range(24))
    assert {n for _, m in cases for t, _, s in m["parts"] if t[0] == "B" for n in [(s - 8) // tc.FIXED[t[1]]]} >= {0, 1, 5, 40}
    # what the walk finds is visible: with whole fields in front, RG gives range 500 and MQ makes the record a candidate
    for (r, m), (t, _) in zip(cases, tri):
        if m["kind"] == "prefix" and (m["T"] == 0 or m["T"] >= 4):
            assert t.cls == 3, m
            assert t.range_max == (700 if m["tail"] == "mq" else 500), m
        elif m["kind"] in ("b_over", "unknown_type") or m["kind"] == "prefix":
            assert (t.cls, t.range_max) == ((3, 700) if m["tail"] == "rg" else (1, 700)), (m, t.cls, t.range_max)
    assert {"b_over", "unknown_type"} <= {m["kind"] for _, m in cases}


def test_rg_name_and_mq_cases():
    names, ranges = tc.rg_name_table()
    cases = tc.rg_name_cases()
    tri = _tri([r for r, _ in cases], names, ranges)
    hit = {}
    for (r, m), (t, _) in zip(cases, tri):
        hit.setdefault(m["kind"], {}).setdefault(m["k"], set()).add(t.cls)
    assert all(hit["rg_present"][k] == {3} and hit["rg_present_H"][k] == {3} and hit["rg_absent"][k] == {16} for k in range(1, 41))
    assert sorted(hit["rg_prefix"]) == list(range(1, 40))
    assert {c for v in hit["rg_prefix"].values() for c in v} == {3, 16}      # a prefix answers only from its own bin
    # a present name of length k gets ITS range unless an older name it is a prefix of shares its bin
    own = sum(1 for (r, m), (t, _) in zip(cases, tri) if m["kind"] == "rg_present" and t.range_max == ranges[m["k"] - 1])
    assert own >= 60
    cases = tc.mq_cases()
    tri = _tri([r for r, _ in cases], tc.AUX_NAMES, tc.AUX_RANGES)
    seen = {}
    for (r, m), (t, _) in zip(cases, tri):
        assert len(r) % 4 == 0
        seen.setdefault(m["kind"], set()).add((m.get("type"), t.cls))
    assert {ty for ty, _ in seen["mq_proper"]} == set("cCsSiIZfAHdB")
    for ty in "cCsSiI":
        assert {(ty, 1), (ty, 3)} <= seen["mq_proper"] and {(ty, 1), (ty, 2)} <= seen["mq_unmapped"], ty      # below and above -q
    for ty in "ZfAHdB":
        assert (ty, 17) in seen["mq_unmapped"] and (ty, 1) in seen["mq_proper"]
    assert {(m["type"], m["have"]) for _, m in cases if m["kind"] == "mq_cut"} == {(t, h) for t, s in zip("cCsSiI", (1, 1, 2, 2, 4, 4)) for h in range(s)}
    assert {c for _, c in seen["mq_cut"]} == {1} and {c for _, c in seen["mq_cut_unmapped"]} <= {1, 2}
    got = [(t.cls, t.range_max) for (r, m), (t, _) in zip(cases, tri) if m["kind"] in ("second_rg", "second_mq")]
    assert got == [(3, 500), (3, 600), (3, 500), (1, 700), (16, 0)], got
    pads = {}
    for (r, m), (t, _) in zip(cases, tri):
        if m["kind"] == "padding_spells":
            assert tc.l_seq_of(r) % 4 == 0
            pads.setdefault(m["npad"], set()).add((t.cls, t.range_max))
    assert sorted(pads) == [0, 1, 2, 3] and all(v == {(3, 700), (3, 500)} for v in pads.values()), pads


def test_rg_tables_sit_on_both_sides_of_the_lds_limit():
    for target in (2048, 2052, 6144):
        names, ranges = tc.rg_table(target)
        # 4 * (20 + 3 n) + sum(len + 1) + 8, rounded up to 4 (im_set_insert_ranges)
        assert (4 * (20 + 3 * len(names)) + sum(len(x) + 1 for x in names) + 8 + 3) // 4 * 4 == target
        cases = tc.rg_table_cases(names)
        tri = _tri([r for r, _ in cases], names, ranges)
        assert {m["bin"] for _, m in cases if m["kind"] == "rg_bin"} == set(range(16))
        for (r, m), (t, _) in zip(cases, tri):
            if m["kind"] == "rg_bin":
                assert t.cls == 3
            if m["kind"] == "rg_query" and m["name"] == "pfx":
                # the older, longer name of the same bin answers
                assert names.index(names[0]) < names.index("pfx") and names[0].startswith("pfx") and t.range_max == ranges[0]
            if m["kind"] in ("rg_absent", "rg_type"):
                assert t.cls == 16
            if m["kind"] == "no_rg":
                assert (t.cls, t.range_max) == (3, ranges[names.index("generic")])
    assert tc.RG_LDS == 2048
    # without "generic", and with no names at all
    names, ranges = tc.rg_table(2048)
    cases = tc.rg_table_cases(names)
    k = names.index("generic")
    tri = _tri([r for r, _ in cases], names[:k] + names[k + 1:], ranges[:k] + ranges[k + 1:])
    assert all(t.cls == 16 for (r, m), (t, _) in zip(cases, tri) if m["kind"] == "no_rg")
    assert any(t.cls == 3 for t, _ in tri)
    assert all(t.cls in (16,) for t, _ in _tri([r for r, _ in cases], [], []))


def test_defer_cases():
    names, ranges = tc.rg_table(2048)
    cases = tc.rg_table_cases(names) + tc.defer_cases()
    tri = _tri([r for r, _ in cases], names, ranges, defer=True)
    plain = _tri([r for r, _ in cases], names, ranges)
    n4 = 0
    for (r, m), (t, _), (u, _) in zip(cases, tri, plain):
        assert t.range_max == 0
        assert (t.cls == 16) == (m["kind"] == "rg_type" or b"RGAx" in r)
        if m["kind"] == "pe":
            want = 0 < abs(m["isize"]) < 1000000 and m["opposite"] and b"RGAx" not in r
            assert (t.cls == 4) == want, m
            n4 += want
            if m["isize"] == 0:
                assert t.cls != 4
    assert n4 >= 10 and any(u.cls == 16 and t.cls != 16 for (t, _), (u, _) in zip(tri, plain))


def test_tile_templates_and_patterns():
    tpl = tc.tile_templates()
    for role, want in (("cand", {2, 3}), ("counted", {1}), ("skip", {0}), ("err", {16, 17, 18, 20})):
        tri = _tri(tpl[role], eth_vcf=0)
        assert {t.cls for t, _ in tri} == want, role
        assert all(8 <= tc.l_seq_of(r) <= 12 for r in tpl[role])
    tri = _tri(tpl["cand"], eth_vcf=0)
    assert {bool(t.revcomp) for t, _ in tri} == {False, True} and {t.n_ev for t, _ in tri} == {0, 1}
    assert {t.l_seq % 4 for t, _ in tri} == {0, 1, 2, 3}
    assert tc.TILE_COUNTS == [1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 16389]
    assert -(-8192 // 256) == 32 and -(-16389 // 256) == 65          # one group of 32 workgroups, and a third group of one
    for n in (257, 8193):
        for name in tc.TILE_PATTERNS:
            role, sub = tc.tile_pattern(name, n, tpl)
            cand = role == 0
            if name == "all":
                assert cand.all()
            if name == "none":
                assert not cand.any() and set(role) == {1, 2}
            if name == "first":
                assert list(np.nonzero(cand)[0]) == [0]
            if name == "last":
                assert list(np.nonzero(cand)[0]) == [n - 1]
            if name == "lane255":
                assert list(np.nonzero(cand)[0]) == list(range(255, n, 256))
            if name == "err_counted":
                assert (role[:256] == 3).all() and (role[256:512] == 1).all()
            if name == "mix":
                assert 0.4 < cand.mean() < 0.6 and set(role) == {0, 1, 2, 3}
            assert all(sub[role == k].max(initial=0) < len(tpl[key]) for k, key in enumerate(("cand", "counted", "skip", "err")))


def test_every_class_is_seen():
    recs = [r for r, _ in tc.length_cases() + tc.base_cases() + tc.mq_cases() + tc.defer_cases()]
    recs += tc.edge_records()
    raw, off = tc.batch(recs)
    tri = ob.triage_records(raw, off, tc.AUX_NAMES, tc.AUX_RANGES)
    seen = {21 if t.cls == 3 and t.n_ev > 4 else t.cls for t, _ in tri}
    assert seen >= {0, 1, 2, 3, 4, 16, 17, 18, 19, 20, 21}, seen
    assert set(tc.edge_records()) <= set(tc.aux_layout(tc.aux_cases()))


def test_append_batch_chunks():
    recs = tc.append_batch()
    assert 2500 <= len(recs) <= 3000
    tri = _tri(recs, tc.AUX_NAMES, tc.AUX_RANGES)
    bounds = np.concatenate([[0], np.cumsum(tc.APPEND_CHUNKS), [len(recs)]])
    assert list(np.diff(bounds)[:6]) == [1, 255, 256, 257, 700, 1] and bounds[-1] - bounds[-2] > 256
    per = [sum(1 for t, _ in tri[a:b] if t.want) for a, b in zip(bounds[:-1], bounds[1:])]
    assert per[5] == 0 and all(x > 0 for x in per[1:5] + per[6:]), per
    assert {t.cls for t, _ in tri} >= {1, 2, 3, 16, 17, 18, 20}
    assert max(t.l_seq for t, _ in tri) == 2600


def test_depth_cases_meet_every_condition():
    recs = tc.depth_cases()
    facts = tc.depth_facts(recs)
    assert tc.DEPTH_FACTS <= facts, sorted(tc.DEPTH_FACTS - facts)
    raw, off = tc.batch(recs)
    for tid, clen in enumerate(tc.DEPTH_CONTIGS):
        d = ob.depth_of(raw, off, tid, clen)
        assert d.max() >= 256 if tid == 1 else d.max() > 0
        assert d[0] > 0 and d[clen - 1] > 0
