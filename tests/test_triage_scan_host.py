"""The inputs of tests/test_gpu_triage_scan.py reach what they claim to reach: the record counts of tests/support/scancases.py follow
from the constants im_triage.hip holds, and every pattern puts candidates where its case needs them (the CPU oracle alone)."""
import os
import re

import numpy as np

from tests.support import oraclebind as ob
from tests.support import scancases as sc
from tests.support import triagecases as tc
from tests.support import wavecases as wc

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "indelminer_amd", "csrc", "im_triage.hip")


def _constant(name):
    with open(HIP) as f:
        m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
    assert m, name
    return int(m.group(1))


def test_constants_are_the_kernels():
    assert (sc.WG, sc.EMIT, sc.GROUP, sc.SCAN_LANES, sc.AHEAD) == tuple(
        _constant(k) for k in ("kClsBlock", "kTriBlock", "kTriGroup", "kScanLanes", "kAhead"))
    # at most 256 lanes in the scan workgroup; a lane's kAhead emit workgroups are one group, 256 bytes of 8-byte words
    assert sc.SCAN_LANES <= 256 and sc.AHEAD * (sc.EMIT // sc.WG) == sc.GROUP and sc.GROUP * 8 == 256
    assert sc.PASS_BLOCKS == 8192


def test_counts_sit_on_every_edge_of_the_scan_launch():
    assert sc.EMIT_COUNTS == [1, 255, 256, 257] and [sc.emits(n) for n in sc.EMIT_COUNTS] == [1, 1, 1, 2]
    assert sc.GROUP_COUNTS == [2047, 2048, 2049] and [sc.groups(n) for n in sc.GROUP_COUNTS] == [1, 1, 2]
    assert [sc.blocks(n) for n in sc.GROUP_COUNTS] == [sc.GROUP, sc.GROUP, sc.GROUP + 1]
    assert [sc.groups(n) for n in sc.WAVE_COUNTS] == [64, 64, 65]                   # lane 63 of the first wave, lane 0 of the second
    S, B = sc.SCAN_LANES, sc.GROUP
    assert [sc.blocks(n) for n in sc.PASS_COUNTS] == [S * B - 1, S * B, S * B + 1]
    assert [sc.passes(n) for n in sc.PASS_COUNTS] == [1, 1, 2] and sc.passes(sc.PASS_COUNTS[2] - 1) == 1
    # S * B - 1 workgroups: the pass's last lane holds 31 words of its launch and one that is not, in its last emit workgroup
    assert sc.groups(sc.PASS_COUNTS[0]) == S and sc.blocks(sc.PASS_COUNTS[0]) % B == B - 1
    # the counts of the existing wave tests: the second wave of the scan, and its third pass
    assert sc.groups(wc.SCAN_COUNTS[0]) == 65 and sc.passes(wc.SCAN_COUNTS[1]) == 3
    # chunks and the reused scratch
    assert sc.CHUNKS == [1, 63, 65]
    assert sc.emits(sc.REUSE_SMALL) == 2 and sc.blocks(sc.REUSE_SMALL) % (sc.EMIT // sc.WG) == 1 and sc.groups(sc.REUSE_LARGE) > sc.groups(sc.REUSE_SMALL)


def test_patterns_put_candidates_where_the_case_needs_them():
    tpl = tc.tile_templates()
    keys = ["cand", "counted", "skip", "err"]
    flat = [r for k in keys for r in tpl[k]]
    first = np.cumsum([0] + [len(tpl[k]) for k in keys])[:4]
    tri = ob.triage_records(*tc.batch(flat), ["generic"], [700], eth_vcf=0)
    want = np.array([t.want != 0 for t, _ in tri])
    assert max(len(r) for r in flat) <= 64
    assert want[:len(tpl["cand"])].all() and not want[len(tpl["cand"]):].any()
    for n in (sc.EMIT + 1, sc.GROUP_RECORDS + 1, sc.WAVE_COUNTS[0]):
        per_block = {}
        for name in sc.PATTERNS:
            role, sub = sc.pattern(name, n, tpl)
            cand = want[first[role] + sub]
            per_block[name] = np.add.reduceat(cand.astype(np.int64), np.arange(0, n, sc.WG))
        full = n // sc.WG
        assert per_block["none"].sum() == 0
        assert (per_block["all"][:full] == sc.WG).all() and per_block["all"].sum() == n
        assert (per_block["lane63"][:full] == 1).all() and per_block["lane63"].sum() == full
        assert (per_block["last_block"][:-1] == 0).all() and per_block["last_block"][-1] == n - (n - 1) // sc.WG * sc.WG >= 1


def test_the_chunked_batch_has_candidates_in_every_part():
    recs = wc.append_batch(sum(sc.CHUNKS))
    assert len(recs) == sum(sc.CHUNKS)
    tri = ob.triage_records(*tc.batch(recs), tc.AUX_NAMES, tc.AUX_RANGES)
    b = np.cumsum([0] + sc.CHUNKS)
    per = [sum(1 for t, _ in tri[a:c] if t.want) for a, c in zip(b[:-1], b[1:])]
    assert per[1] > 0 and per[2] > 0 and sum(per) >= 3, per
