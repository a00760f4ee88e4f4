"""Inputs for the classify kernel's one-wave workgroups (im_triage.hip): record counts around the 64-record workgroup and the
group of 32 of them, counts that take the scan of the groups' totals into its second round and into its second fetch, pileup
segments around the 1024-position depth window with the first eligible record in lane 0, 1 and 63, and read-group tables on both
sides of the LDS copy's limit.  Built on tests/support/triagecases.py.  tests/test_triage_wave_host.py proves on the CPU that
the generators reach what they name; tests/test_gpu_triage_wave.py runs them through the kernels."""
import struct

import numpy as np

from tests.support import triagecases as tc

WG = 64                 # kClsBlock
GROUP = 32              # kTriGroup: classify workgroups per group
SCAN_LANES = 64         # groups the scanning wave takes per round
SCAN_AHEAD = 8          # rounds whose totals are fetched together (kAhead)
DEPTH_WIN = 1024        # kDepthWin
RG_LDS = 448            # kClsRgLds

GROUP_RECORDS = WG * GROUP
TILE_COUNTS = [1, WG - 1, WG, WG + 1, 2 * WG - 1, 2 * WG, 2 * WG + 1, GROUP_RECORDS - 1, GROUP_RECORDS, GROUP_RECORDS + 1]
TILE_PATTERNS = [p for p in tc.TILE_PATTERNS if p != "lane255"] + ["lane63"]
# one group more than a round of the scan holds (65 groups), and one more than a fetch of SCAN_AHEAD rounds holds (513 groups: a
# million records -- no smaller input reaches the second fetch, and the 32 MB chunks of tests/test_gpu_large.py do not either)
SCAN_COUNTS = [SCAN_LANES * GROUP_RECORDS + 1, SCAN_AHEAD * SCAN_LANES * GROUP_RECORDS + 1]
CHUNK_CUTS = [1, WG - 1, WG, WG + 1]


def tile_pattern(name, n, tpl, seed=0):
    if name != "lane63":
        return tc.tile_pattern(name, n, tpl, seed)
    rng = np.random.default_rng(2000 + seed + n)
    role = np.where(np.arange(n) % WG == WG - 1, 0, 1)
    sub = np.where(role == 0, rng.integers(0, len(tpl["cand"]), n), rng.integers(0, len(tpl["counted"]), n))
    return role, sub


# ---- the depth feed ----------------------------------------------------------------------------------------------------------------

# (len + 1) * 4 bytes per run: 20 004 and 36 004 are no multiples of 16, 12 is shorter than 16
DEPTH_CONTIGS = [5000, 9000, 2]
W = DEPTH_WIN


def depth_cases():
    """workgroups of 64 records; position in the list = record index"""
    d = tc._drec
    M = lambda n: ((n, 0),)
    un = lambda: d(0, 50, M(30), 0x4)                      # unmapped, with a position and a CIGAR: not piled up

    def fill(wg, rec_):
        return wg + [rec_(k) for k in range(WG - len(wg))]
    base = 100
    # A: the first eligible record in lane 0 (window base 100 on contig 0); starts and ends at W - 1, W, W + 1 from the base
    a = [d(0, base, M(50))]
    a += [d(0, base + W - 1, M(10)), d(0, base + W, M(10)), d(0, base + W + 1, M(10))]
    a += [d(0, base + W - 1 - 50, M(50)), d(0, base + W - 50, M(50)), d(0, base + W + 1 - 50, M(50))]
    a += [d(0, 4970, M(30)), d(0, 4971, M(30)), d(0, 4990, M(500))]                    # ends at clen, at clen + 1, far past it
    a += [d(0, 20, M(2600))]                                                           # in front of the window base, and long
    a = fill(a, lambda k: d(0, base + 3 * k, M(40)))
    # B: lane 0 is not eligible, lane 1 decides (contig 1, base 200); the second contig of the workgroup goes to memory
    b = [un(), d(1, 200, M(20)), d(1, 200 + W - 1, M(1)), d(1, 200 + W, M(1)), d(1, 200 + W + 1, M(1))]
    b += [d(1, 200 + 10, ((5, 4), (10, 0), (3, 1), (10, 7), (4, 2), (10, 8), (7, 3), (10, 0), (2, 6), (5, 5)))]
    b += [d(2, 0, M(2)), d(2, 1, M(5)), d(0, 300, M(25)), d(3, 10, M(10)), d(-1, 10, M(10))]
    b += [d(1, 10, M(10), 0x100), d(1, 10, M(10), 0x200), d(1, 10, M(10), 0x400)]
    b = fill(b, lambda k: d(1, 230 + k, M(15)))
    # C: only lane 63 is eligible
    c = [un() for _ in range(WG - 1)] + [d(1, 3000, M(10))]
    # D: no eligible record at all
    dd = [un() for _ in range(32)] + [d(-1, 10, M(10)) for _ in range(16)] + [d(1, 10, M(10), 0x400) for _ in range(16)]
    # E: the first eligible record starts in front of the contig (window base 0); 64 minus a few records at one position
    e = [d(1, -20, M(50)), d(1, -1, M(20)), d(1, -5, ((10, 2), (10, 0))), d(1, W - 1, M(2)), d(1, W, M(2)), d(1, 8970, M(30)), d(1, 8971, M(30)),
         d(1, 8999, M(1)), d(1, 9000, M(5)), d(1, 500, ((10, 0), (2000, 2), (10, 0)))]
    e = fill(e, lambda k: d(1, 700, M(10)))
    # F: 64 records at one position
    f = [d(1, 4000, M(10)) for _ in range(WG)]
    tail = [d(0, 2500, M(100), 0x10), d(1, 2500, M(100)), d(0, 0, M(5000)), d(1, 0, M(9000)), d(2, 0, M(2))] + [d(0, 7 * k, M(33)) for k in range(20)]
    return a + b + c + dd + e + f + tail


DEPTH_CHUNK_CUT = 3 * WG + 17     # inside workgroup D of the one-chunk run


def depth_facts(recs, bounds=None):
    """what the window logic meets on these records, per 64-record workgroup of every chunk"""
    facts = set()
    n_ctg = len(DEPTH_CONTIGS)
    bounds = bounds or [0, len(recs)]
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        if c0 % WG:
            facts.add("chunk_cut_inside_a_workgroup")
        for w0 in range(c0, c1, WG):
            info = []
            for r in recs[w0:min(w0 + WG, c1)]:
                tid, pos = struct.unpack_from("<ii", r, 0)
                l_qname, n_cig, flag = r[8], struct.unpack_from("<H", r, 12)[0], tc.flag_of(r)
                cig = [struct.unpack_from("<I", r, 32 + l_qname + 4 * k)[0] for k in range(n_cig)]
                info.append((tid, pos, cig, 0 <= tid < n_ctg and not flag & (0x4 | 0x100 | 0x200 | 0x400)))
            first = next((k for k, x in enumerate(info) if x[3]), None)
            if first is None:
                facts.add("no_eligible_record" + ("" if len(info) == WG else "_partial"))
                continue
            facts.add("first_in_lane_%d" % first)
            wtid, wpos = info[first][0], max(info[first][1], 0)
            if info[first][1] < 0:
                facts.add("first_pos_negative")
            if len({x[0] for x in info if x[3]}) > 1:
                facts.add("two_contigs")
            same = {}
            for tid, pos, cig, elig in info:
                if not elig:
                    continue
                same[(tid, pos)] = same.get((tid, pos), 0) + 1
                clen = DEPTH_CONTIGS[tid]
                x = pos
                for cw in cig:
                    op, ln = cw & 15, cw >> 4
                    facts.add("op_%d" % op)
                    if op in (0, 7, 8):
                        if x + ln == clen:
                            facts.add("ends_at_clen")
                        if x + ln == clen + 1:
                            facts.add("ends_at_clen+1")
                        if tid == wtid and x >= 0:
                            for k in (-1, 0, 1):
                                if x - wpos == W + k:
                                    facts.add("starts_at_W%+d" % k)
                                if x + ln - wpos == W + k:
                                    facts.add("ends_at_W%+d" % k)
                            if x - wpos < 0:
                                facts.add("in_front_of_window")
                        x += ln
                    elif op in (2, 3):
                        x += ln
            if max(same.values()) == WG:
                facts.add("64_at_one_position")
    return facts


DEPTH_FACTS = {"first_in_lane_0", "first_in_lane_1", "first_in_lane_63", "no_eligible_record", "first_pos_negative", "two_contigs", "ends_at_clen",
               "ends_at_clen+1", "in_front_of_window", "64_at_one_position"} | {"op_%d" % k for k in range(9)} \
    | {"%s_at_W%+d" % (s, k) for s in ("starts", "ends") for k in (-1, 0, 1)}


# ---- one mixed batch for the chunked run -------------------------------------------------------------------------------------------

def append_batch(n=700):
    """the first records of triagecases.append_batch: every kind of section 1 to 3, interleaved"""
    return tc.append_batch()[:n]


def append_bounds(n):
    """chunks of 1, 63, 64 and 65 records, over and over"""
    b = [0]
    k = 0
    while b[-1] < n:
        b.append(min(b[-1] + CHUNK_CUTS[k % len(CHUNK_CUTS)], n))
        k += 1
    return b
