"""The waves of tests/support/mixedwaves.py hold what they claim: every class and every exit of the rule cascade, every CIGAR length
with its refused ops and bases, the pileup's window and width edges, every aux size -- through the CPU oracle alone.  Where a case
is about 32-bit arithmetic, the oracle's answer is shown to differ from what wrapping 32-bit arithmetic would give."""
import os
import re
import struct

import numpy as np

from tests.support import mixedwaves as mw
from tests.support import oraclebind as ob
from tests.support import triagecases as tc

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "indelminer_amd", "csrc")


def _constant(name, file="im_triage.hip"):
    with open(os.path.join(HIP, file)) as f:
        m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
    assert m, name
    return int(m.group(1))


def _classes(recs, names=mw.NAMES, ranges=mw.RANGES, **kw):
    return [t for t, _ in ob.triage_records(*tc.batch(recs), names, ranges, **kw)]


def test_constants_are_the_kernels():
    assert (mw.WAVE, mw.DEPTH_WIN) == (_constant("kClsBlock"), _constant("kDepthWin"))
    assert _constant("kAuxWin", "im_rg.hpp") == 24      # the aux sizes sit around one and two windows
    assert {0, 3, 4, 5, 23, 24, 25, 47, 48, 49, 100} == set(mw.AUX_SIZES)


def test_cascade_records_reach_every_exit():
    cases = mw.cascade_records()
    tri = _classes([r for _, _, r in cases])
    got = {name: t.cls for (name, _, _), t in zip(cases, tri)}
    assert got == {name: cls for name, cls, _ in cases}
    assert set(got.values()) == mw.CASCADE_CLASSES
    by = {name: t for (name, _, _), t in zip(cases, tri)}
    # the ranges name the read group that was found
    assert (by["no_rg"].range_max, by["rg_known"].range_max, by["rg_known_H"].range_max, by["pe_rg_range"].range_max) == (700, 600, 500, 500)
    # both strands of the `three` case, and both reverse-complement outcomes of either candidate class
    assert {(by[k].cls, by[k].revcomp) for k in ("proper_clip_5p_fwd", "proper_clip_5p_rev", "proper_ins")} == {(3, 0), (3, 1)}
    assert {by[k].revcomp for k in ("unmapped_mapq_above", "unmapped_mapq_at")} == {0, 1}
    # without "generic" in the table a record without an RG tag is an error; the others keep their class
    tri2 = _classes([r for _, _, r in cases], mw.NAMES_NO_GENERIC, mw.RANGES_NO_GENERIC)
    for (name, cls, rec), t in zip(cases, tri2):
        has_rg = b"RG" in rec[-16:]
        assert t.cls == (cls if has_rg or cls in (0, 21) else 16), name
    # deferred ranges: no look-up, only a refused RG type is an error; the pair test runs against range 0
    tri3 = _classes([r for _, _, r in cases], defer=True)
    d = {name: t.cls for (name, _, _), t in zip(cases, tri3)}
    assert (d["rg_type"], d["rg_type_int"], d["rg_not_in_table"], d["rg_longer_than_stored"], d["pe_inside_range"], d["pe_rg_range_in"]) == (16, 16, 3, 3, 4, 4)
    assert all(t.range_max == 0 for t in tri3)


def test_cascade_waves_hold_every_record_in_different_lanes():
    n = len(mw.cascade_records())
    waves = [mw.cascade_wave(seed) for seed in (1, 2, 3)]
    for w in waves:
        assert len(w) == mw.WAVE and len({bytes(r) for r in w}) == n
        assert {t.cls for t in _classes(w)} == mw.CASCADE_CLASSES
    assert waves[0] != waves[1] != waves[2]
    for lane in mw.ODD_LANES:
        recs = mw.odd_lane_waves(lane)
        assert len(recs) == 2 * n * mw.WAVE
        for k in range(0, len(recs), mw.WAVE):
            w = recs[k:k + mw.WAVE]
            others = {bytes(r) for j, r in enumerate(w) if j != lane}
            assert len(others) == 1
    cls = [t.cls for t in _classes(mw.odd_lane_waves(31)[:2 * mw.WAVE])]
    assert cls[0] == 1 and cls[mw.WAVE] == 0            # the two waves of one class


def test_cigar_records():
    cases = mw.cigar_records()
    tri = _classes([r for _, _, r in cases])
    for (name, cls, _), t in zip(cases, tri):
        assert t.cls == cls, (name, t.cls, cls)
    names = [n for n, _, _ in cases]
    n_ops = {struct.unpack_from("<H", r, 12)[0] for _, _, r in cases}
    assert set(mw.CIGAR_LENGTHS) <= n_ops and 19 in n_ops
    for n in mw.CIGAR_LENGTHS[1:]:
        for where in ("first", "mid", "last") + (("beyond4",) if n > 4 else ()):
            assert any(x.startswith("len%d_%s_op" % (n, where)) for x in names), (n, where)
            if where != "last":                          # behind the last op's offset there may be no base left
                assert "len%d_%s_base+0" % (n, where) in names
            if where != "first" and n > 1:
                assert "len%d_%s_base-1" % (n, where) in names
    # a refused op in a word that comes from memory (index >= 4)
    for name, _, r in cases:
        if "beyond4" in name:
            l_qname = r[8]
            ops = [struct.unpack_from("<I", r, 32 + l_qname + 4 * k)[0] & 15 for k in range(struct.unpack_from("<H", r, 12)[0])]
            assert all(o in (0, 1, 2, 4) for o in ops[:4]) and any(o in mw.REFUSED_OPS for o in ops[4:])
    assert {"past_lseq_1_in", "past_lseq_1_out", "past_record", "inner_clip"} <= set(names)
    wave = mw.cigar_wave(5)
    assert len(wave) % mw.WAVE == 0 and len(wave) <= 3 * mw.WAVE
    first = [struct.unpack_from("<H", r, 12)[0] for r in wave[:mw.WAVE]]
    assert len(set(first)) >= 6                          # lengths mixed inside one wave


def test_read_offsets_at_2_pow_32_differ_between_the_widths():
    for name, cls, rec, wrapped in mw.wide_offset_records():
        l_qname, n = rec[8], struct.unpack_from("<H", rec, 12)[0]
        cig = [struct.unpack_from("<I", rec, 32 + l_qname + 4 * k)[0] for k in range(n)]
        k_bad = next(k for k, cw in enumerate(cig) if cw & 15 == 3)
        q = sum(cw >> 4 for cw in cig[:k_bad] if cw & 15 in (0, 1, 4, 7, 8))
        assert q == 2 ** 32 and q % 2 ** 32 == 0
        assert _classes([rec])[0].cls == cls
    (_, cls, _, wrapped) = mw.wide_offset_records()[0]
    assert cls != wrapped                                # 64 bits: a bad base in front of the op; wrapped to 0: behind it


def test_pileup_waves():
    waves = mw.pileup_waves()
    elig = lambda r: 0 <= struct.unpack_from("<i", r, 0)[0] < len(mw.CONTIGS) and not tc.flag_of(r) & (0x4 | 0x100 | 0x200 | 0x400)   # noqa: E731
    assert sum(elig(r) for r in waves["one"]) == 1 and sum(elig(r) for r in waves["none"]) == 0
    win = waves["window"]
    first = next(k for k, r in enumerate(win) if elig(r))
    wtid, wpos = struct.unpack_from("<ii", win[first], 0)
    assert (first, wtid, wpos) == (1, 0, 300)
    starts, ends, tids, neg = set(), set(), set(), 0
    for r in win:
        if not elig(r):
            continue
        tid, pos = struct.unpack_from("<ii", r, 0)
        tids.add(tid)
        neg += pos < 0
        l_qname = r[8]
        x = pos
        for k in range(struct.unpack_from("<H", r, 12)[0]):
            cw = struct.unpack_from("<I", r, 32 + l_qname + 4 * k)[0]
            if cw & 15 in (0, 7, 8) and tid == wtid:
                starts.add(x - wpos); ends.add(x + (cw >> 4) - wpos)
                if x + (cw >> 4) == mw.CONTIGS[0]:
                    ends.add("clen")
                if x + (cw >> 4) > mw.CONTIGS[0]:
                    ends.add("past")
            if cw & 15 in (0, 2, 3, 7, 8):
                x += cw >> 4
    W = mw.DEPTH_WIN
    assert {W - 1, W, 2000, -1} <= starts and {W - 1, W, "clen", "past", 0, 1} <= ends and tids == {0, 1} and neg >= 4
    raw, off = tc.batch(win)
    assert all(ob.depth_of(raw, off, t, clen).max() > 0 for t, clen in enumerate(mw.CONTIGS))
    assert {t.cls for t in _classes(win)} >= {0, 3, 18}  # lanes that pile up whatever their class


def test_pileup_width_edges_differ_between_the_widths():
    clen = mw.CONTIGS[0]
    differ = 0
    for name, rec, wide, narrow in mw.width_edge_records():
        raw, off = tc.batch([rec])
        want = ob.depth_of(raw, off, 0, clen)
        d64, d32 = mw.depth_model(rec, 0, clen, 64), mw.depth_model(rec, 0, clen, 32)
        assert np.array_equal(want, d64), name
        exp = np.zeros(clen, np.int32); exp[wide[0]:wide[1]] = 1
        assert np.array_equal(want, exp), name
        exp32 = np.zeros(clen, np.int32); exp32[narrow[0]:narrow[1]] = 1
        assert np.array_equal(d32, exp32), name
        differ += not np.array_equal(d64, d32)
    assert differ >= 2
    edges = mw.pileup_waves()["edges"]
    assert sum(1 for _, rec, _, _ in mw.width_edge_records() if any(rec == r for r in edges)) == len(mw.width_edge_records())


def test_aux_records():
    cases = mw.aux_records()
    sizes = {}
    for name, T, rec in cases:
        assert mw.aux_bytes(rec) == T and len(rec) % 4 == 0, name
        sizes.setdefault(T, []).append(name)
    assert set(sizes) == set(mw.AUX_SIZES)
    tri = _classes([r for _, _, r in cases])
    got = {name: t for (name, _, _), t in zip(cases, tri)}
    for T in (23, 24, 25, 47, 48, 49, 100):
        # RG found first and last: the range is lib1's; MQ found: the mapq-0 record is a candidate
        assert got["aux%d_rg_first" % T].range_max == got["aux%d_rg_last" % T].range_max == 500
        assert got["aux%d_mq_first" % T].cls == got["aux%d_mq_last" % T].cls == 3
        assert got["aux%d_mq_last_unmapped" % T].cls == 2
        assert got["aux%d_absent" % T].range_max == 700 and got["aux%d_absent" % T].cls == 3
        assert got["aux%d_rg_refused_last" % T].cls == 16 and got["aux%d_rg_unknown_last" % T].cls == 16
        assert got["aux%d_mq_refused_last_unmapped" % T].cls == 17 and got["aux%d_mq_refused_last" % T].cls == 1
        assert (got["aux%d_rg_mq_last" % T].cls, got["aux%d_rg_mq_last" % T].range_max) == (3, 500)
    assert got["aux4_mq_first"].cls == 3 and got["aux5_mq_refused_first_unmapped"].cls == 17 and got["aux3_no_field"].cls == 3
    assert (got["aux48_long_name"].cls, got["aux48_long_name"].range_max) == (3, 900)
    assert (got["aux100_long_name_behind"].cls, got["aux100_long_name_behind"].range_max) == (3, 900)
    assert got["aux47_B_front"].range_max == 500 and got["aux24_B_over"].range_max == 700      # behind a B array; behind one that stops the walk
    wave = mw.aux_wave(3)
    assert len(wave) % mw.WAVE == 0 and len(wave) <= 4 * mw.WAVE
    assert mw.aux_bytes(wave[-1]) == max(mw.aux_bytes(r) for r in wave) == 100
    per_wave = [{mw.aux_bytes(r) for r in wave[k:k + mw.WAVE]} for k in range(0, len(wave), mw.WAVE)]
    assert all(len(s) >= 6 for s in per_wave[1:])        # sizes mixed inside a wave
