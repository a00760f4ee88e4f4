"""The inputs of tests/test_gpu_triage_wave.py reach what they claim to reach: every generator of tests/support/wavecases.py through
the CPU oracle alone, and the constants they are derived from are the ones im_triage.hip holds."""
import os
import re

import numpy as np

from tests.support import oraclebind as ob
from tests.support import triagecases as tc
from tests.support import wavecases as wc

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "indelminer_amd", "csrc", "im_triage.hip")


def _constant(name):
    with open(HIP) as f:
        m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
    assert m, name
    return int(m.group(1))


def test_constants_are_the_kernels():
    assert (wc.WG, wc.GROUP, wc.DEPTH_WIN, wc.RG_LDS, wc.SCAN_AHEAD) == tuple(
        _constant(k) for k in ("kClsBlock", "kTriGroup", "kDepthWin", "kClsRgLds", "kAhead"))
    assert wc.SCAN_LANES == wc.WG
    # the LDS a classify workgroup holds fits the hole one realign wave leaves
    assert wc.WG * 24 + wc.WG * 4 + wc.DEPTH_WIN * 4 + wc.RG_LDS <= _constant("kClsLdsBudget") == 6400


def test_counts_sit_around_the_workgroup_the_group_and_the_scan():
    assert wc.TILE_COUNTS == [1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049]
    blocks = lambda n: -(-n // wc.WG)
    groups = lambda n: -(-blocks(n) // wc.GROUP)
    assert [groups(n) for n in (2047, 2048, 2049)] == [1, 1, 2] and [blocks(n) for n in (63, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]
    # the scan: 64 groups a round, eight rounds a fetch -- one group behind the first round, one behind the first fetch
    assert [groups(n) for n in wc.SCAN_COUNTS] == [65, 513] and [groups(n - 1) for n in wc.SCAN_COUNTS] == [64, 512]
    # an emit workgroup (256 records) is four classify workgroups of one group
    assert 256 % wc.WG == 0 and wc.GROUP % (256 // wc.WG) == 0


def test_patterns():
    tpl = tc.tile_templates()
    assert "lane255" not in wc.TILE_PATTERNS and "lane63" in wc.TILE_PATTERNS and set(wc.TILE_PATTERNS) - {"lane63"} == set(tc.TILE_PATTERNS) - {"lane255"}
    for n in (65, 2049):
        role, sub = wc.tile_pattern("lane63", n, tpl)
        assert list(np.nonzero(role == 0)[0]) == list(range(63, n, 64)) and set(role) == {0, 1}
        assert sub[role == 0].max() < len(tpl["cand"]) and sub[role == 1].max() < len(tpl["counted"])
        role, _ = wc.tile_pattern("err_counted", n, tpl)
        assert (role[:64] == 3).all()                    # a workgroup of 64 error records
        role, _ = wc.tile_pattern("all", n, tpl)
        assert (role == 0).all()                         # 64 candidates in every full workgroup
    role, _ = wc.tile_pattern("mix", wc.SCAN_COUNTS[0], tpl)
    assert set(role) == {0, 1, 2, 3} and (role[-1:] >= 0).all()
    # every record of the tile batches takes at most 64 bytes
    assert max(len(r) for k in tpl for r in tpl[k]) <= 64


def test_depth_cases_meet_every_condition():
    recs = wc.depth_cases()
    facts = wc.depth_facts(recs)
    assert wc.DEPTH_FACTS <= facts, sorted(wc.DEPTH_FACTS - facts)
    assert "chunk_cut_inside_a_workgroup" not in facts
    cut = wc.depth_facts(recs, [0, wc.DEPTH_CHUNK_CUT, len(recs)])
    assert "chunk_cut_inside_a_workgroup" in cut and wc.DEPTH_CHUNK_CUT % wc.WG and len(recs) % wc.WG
    raw, off = tc.batch(recs)
    for tid, clen in enumerate(wc.DEPTH_CONTIGS):
        d = ob.depth_of(raw, off, tid, clen)
        assert d.max() >= (64 if tid == 1 else 1) and d[0] > 0 and d[clen - 1] > 0
    # the runs im_depth_reset clears: whole 16-byte stores and a tail, and one shorter than 16 bytes
    runs = [4 * (clen + 1) for clen in wc.DEPTH_CONTIGS]
    assert all(r % 16 for r in runs) and min(runs) < 16 < max(runs)


def test_chunks_and_tables():
    recs = wc.append_batch()
    b = wc.append_bounds(len(recs))
    assert list(np.diff(b)[:8]) == [1, 63, 64, 65, 1, 63, 64, 65] and b[-1] == len(recs) and len(b) > 12
    raw, off = tc.batch(recs)
    tri = ob.triage_records(raw, off, tc.AUX_NAMES, tc.AUX_RANGES)
    per = [sum(1 for t, _ in tri[a:c] if t.want) for a, c in zip(b[:-1], b[1:])]
    assert sum(1 for x in per if x == 0) >= 1 and sum(1 for x in per if x > 0) >= 8        # chunks with and without candidates
    assert {t.cls for t, _ in tri} >= {1, 2, 3}
    for target in (wc.RG_LDS, wc.RG_LDS + 4):
        names, ranges = tc.rg_table(target)
        assert tc.table_bytes(names) == target and "generic" in names
        cases = tc.rg_table_cases(names)
        tri = ob.triage_records(*tc.batch([r for r, _ in cases]), names, ranges)
        for (r, m), (t, _) in zip(cases, tri):
            if m["kind"] == "no_rg":
                assert (t.cls, t.range_max) == (3, ranges[names.index("generic")])
            if m["kind"] == "rg_bin":
                assert t.cls == 3
