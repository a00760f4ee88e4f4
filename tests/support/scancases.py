"""Inputs for the triage's scan launch (triage_scan_kernel in im_triage.hip): record counts around every edge of the launch, and
candidate patterns that put known totals into the classify workgroups' words.  Built on tests/support/triagecases.py and
wavecases.py.  tests/test_triage_scan_host.py proves on the CPU that the counts are what they claim, from the constants im_triage.hip
holds; tests/test_gpu_triage_scan.py runs them through the kernels."""
import numpy as np

from tests.support import wavecases as wc

WG = 64                 # kClsBlock: records of a classify workgroup, one word of blk[] each
EMIT = 256              # kTriBlock: records of an emit workgroup, one base entry each
GROUP = 32              # kTriGroup: classify workgroups a lane of the scan takes per pass
SCAN_LANES = 256        # kScanLanes: lanes of the one scan workgroup
AHEAD = 8               # kAhead: emit workgroups of a group, whose words a lane fetches together

GROUP_RECORDS = GROUP * WG                      # 2 048
PASS_BLOCKS = SCAN_LANES * GROUP                # S * B: classify workgroups of a pass of the scan, 8 192
EMIT_COUNTS = [1, EMIT - 1, EMIT, EMIT + 1]     # one emit workgroup and its base entry, and the second
GROUP_COUNTS = [GROUP_RECORDS - 1, GROUP_RECORDS, GROUP_RECORDS + 1]            # the scan's first lane, whole, and the second lane
WAVE_COUNTS = [64 * GROUP_RECORDS - 1, 64 * GROUP_RECORDS, 64 * GROUP_RECORDS + 1]      # the scan's first wave, whole, and the second (totals through LDS)
# S * B - 1, S * B and S * B + 1 classify workgroups: the pass's last lane has 31 of its 32 words, all of them, and the second pass
# begins with one record.  The last is also the smallest launch that fetches a second time.
PASS_COUNTS = [(PASS_BLOCKS - 1) * WG, PASS_BLOCKS * WG, PASS_BLOCKS * WG + 1]
COUNTS = EMIT_COUNTS + GROUP_COUNTS + WAVE_COUNTS + PASS_COUNTS
PATTERNS = ["none", "all", "lane63", "last_block"]


def blocks(n):
    return -(-n // WG)


def emits(n):
    return -(-n // EMIT)


def groups(n):
    return -(-blocks(n) // GROUP)


def passes(n):
    return -(-groups(n) // SCAN_LANES)


def pattern(name, n, tpl, seed=0):
    """role of each of n records (0 cand, 1 counted, 2 skip, 3 err) and the template index inside the role"""
    if name != "last_block":
        return wc.tile_pattern(name, n, tpl, seed)
    rng = np.random.default_rng(3000 + seed + n)
    role = np.where(np.arange(n) >= (n - 1) // WG * WG, 0, 1)
    sub = np.where(role == 0, rng.integers(0, len(tpl["cand"]), n), rng.integers(0, len(tpl["counted"]), n))
    return role, sub


# chunk after chunk: 1, 63 and 65 records
CHUNKS = [1, 63, 65]
# a larger launch, then a smaller one on the same scratch: the smaller one's last emit workgroup has one classify workgroup; the
# words behind it in its group, and the base entries behind its two, are whatever the larger launch left there
REUSE_LARGE, REUSE_SMALL = 2 * GROUP_RECORDS + 1, EMIT + 1
