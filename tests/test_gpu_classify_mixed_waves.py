"""The classify kernel (im_triage.hip) on waves that mix what its straight-line form must keep apart: every class and exit of the
rule cascade in one wave, CIGARs of 0 to 40 ops in one wave, pileup lanes beside lanes that do not pile up, aux areas of 0 to 100
bytes in one wave (tests/support/mixedwaves.py; tests/test_classify_mixed_waves_host.py proves the cases on the CPU).  Every
output is compared exactly with the CPU oracle: the class array, the per-record info word (class and reverse-complement bit) and
range of the scratch, the counters, the workgroups' packed totals (blk[]), the candidates' outputs and the depth array.  Each
launch is a few waves; the odd-lane test is one launch of two waves per record of the cascade."""
import struct

import numpy as np
import pytest

from indelminer_amd import capi
from tests.support import mixedwaves as mw
from tests.support import oraclebind as ob
from tests.support import triagecases as tc
from tests.test_gpu_triage import _compare_triage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def depth_ctx():
    """a context of its own with the two contigs of the pileup cases and the depth array"""
    ctx = capi.Context(0)
    ctx.set_reference([b"A" * mw.CONTIGS[0], b"C" * mw.CONTIGS[1]])
    ctx.set_insert_ranges(mw.NAMES, mw.RANGES)
    ctx.depth_enable()
    yield ctx
    ctx.close()


def _up(x):
    return (x + 255) // 256 * 256


def _scratch(pipe, n):
    """info[n], rmax[n] and blk[classify workgroups] of the triage scratch (launch_triage's layout: 256 fixed bytes, then the arrays)"""
    words = pipe.d_ts.download(np.uint32, pipe.ts_bytes // 4)
    at = 64
    info = words[at:at + n]; at += _up(4 * n) // 4
    rmax = words[at:at + n].view(np.int32); at += _up(4 * n) // 4
    blk = words[at:at + 2 * (-(-n // mw.WAVE))].reshape(-1, 2)
    return info, rmax, blk


def _expected(tri, recs):
    """per record what classify itself leaves: its class (emit and decode change a candidate's class later: 19, 20, 21 on a record
    the oracle wanted), the reverse-complement bit, the range"""
    n = len(tri)
    final = np.array([21 if (t.cls == 3 and t.n_ev > capi.MAX_EV) else t.cls for t in tri], np.uint8)
    want = np.array([t.want for t in tri], np.uint8)
    stage = np.where(want != 0, want, final)
    emit_err = (want != 0) & np.isin(final, (19, 21))     # emit writes its error into info
    info_cls = np.where(emit_err, final, stage)
    rev = np.zeros(n, bool)
    for k, (t, r) in enumerate(zip(tri, recs)):
        f = tc.flag_of(r)
        if t.want == 2:
            rev[k] = not f & 0x20
        elif t.want == 3:
            rev[k] = bool(f & 0x10) == bool(f & 0x20)
        if t.cls in (2, 3):
            assert rev[k] == bool(t.revcomp)
    return final, stage, info_cls, rev, np.array([t.range_max for t in tri], np.int32)


def _check(ctx, recs, names=mw.NAMES, ranges=mw.RANGES, defer=False, want_depth=False, candidates=True):
    raw, off = tc.batch(recs)
    n = len(recs)
    tri_b = ob.triage_records(raw, off, names, ranges, defer=defer)
    tri = [t for t, _ in tri_b]
    final, stage, info_cls, rev, o_rmax = _expected(tri, recs)
    ctx.set_insert_ranges(names, ranges)
    pipe = capi.Pipeline(ctx, n, len(raw), cap_cand=n, read_len_max=max(tc.l_seq_of(r) for r in recs if len(r) >= 32), want_depth=want_depth)
    if candidates and not defer and not want_depth:
        _compare_triage(pipe, raw, off, names, ranges, tri=tri_b)      # every candidate output, with and without qualities
    pipe.upload(raw, off)
    if defer:
        pipe.d_counters.upload(np.full(64, 0x7F, np.uint8))
        pipe.triage_append(n, 0, restart=True, defer=True)
    else:
        pipe.triage()
    c = pipe.fetch_counts()
    got = pipe.d_class.download(np.uint8, n)
    print(n, c[:5], np.bincount(final, minlength=22)[[0, 1, 2, 3, 4, 16, 17, 18, 19, 20, 21]])
    assert np.array_equal(got, final), [(int(k), int(got[k]), int(final[k])) for k in np.nonzero(got != final)[0][:8]]
    m = int(np.isin(stage, (2, 3)).sum())
    pad = sum((tc.l_seq_of(r) + 3) // 4 * 4 for r, s in zip(recs, stage) if s in (2, 3))
    assert list(c[:5]) == [m, pad, int((final != 0).sum()), int((final >= 16).sum()), 0], c[:5]
    info, rmax, blk = _scratch(pipe, n)
    assert np.array_equal(info & 255, info_cls), np.nonzero((info & 255) != info_cls)[0][:8]
    assert np.array_equal((info >> 8) != 0, rev), np.nonzero(((info >> 8) != 0) != rev)[0][:8]
    assert np.array_equal(rmax, o_rmax), [(int(k), int(rmax[k]), int(o_rmax[k])) for k in np.nonzero(rmax != o_rmax)[0][:8]]
    for w in range(-(-n // mw.WAVE)):
        s = stage[w * mw.WAVE:(w + 1) * mw.WAVE]
        lens = [tc.l_seq_of(r) for r, x in zip(recs[w * mw.WAVE:(w + 1) * mw.WAVE], s) if x in (2, 3)]
        word = int(np.isin(s, (2, 3)).sum()) | int((s != 0).sum()) << 9 | int((s >= 16).sum()) << 18
        assert (int(blk[w, 0]), int(blk[w, 1])) == (word, sum((x + 3) // 4 * 4 for x in lens)), w
    if want_depth:
        for t, clen in enumerate(mw.CONTIGS):
            want = ob.depth_of(raw, off, t, clen).astype(np.int64)
            ctx.depth_scan(t)
            p = np.arange(clen, dtype=np.int32)
            got_d = ctx.depth_query_tid(t, p, p + 1).astype(np.int64)
            bad = np.nonzero(got_d != want)[0]
            assert len(bad) == 0, (t, bad[:8], got_d[bad[:8]], want[bad[:8]])
        for t in range(len(mw.CONTIGS)):
            ctx._check(capi.lib().im_depth_reset(ctx.h, t, ctx.stream))
        pipe.sync()


@pytest.mark.parametrize("want_depth", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_class_in_one_wave(depth_ctx, seed, want_depth):
    _check(depth_ctx, mw.cascade_wave(seed), want_depth=want_depth)


@pytest.mark.parametrize("want_depth", [False, True])
def test_every_class_in_one_wave_without_generic_and_with_deferred_ranges(depth_ctx, want_depth):
    wave = mw.cascade_wave(4)
    _check(depth_ctx, wave, mw.NAMES_NO_GENERIC, mw.RANGES_NO_GENERIC, want_depth=want_depth)
    _check(depth_ctx, wave, defer=True, want_depth=want_depth)
    _check(depth_ctx, wave, mw.NAMES_NO_GENERIC, mw.RANGES_NO_GENERIC, defer=True, want_depth=want_depth)


@pytest.mark.parametrize("lane", mw.ODD_LANES)
def test_one_odd_lane_in_a_wave_of_one_class(depth_ctx, lane):
    recs = mw.odd_lane_waves(lane)
    _check(depth_ctx, recs, candidates=False)
    _check(depth_ctx, recs, want_depth=True)


@pytest.mark.parametrize("want_depth", [False, True])
@pytest.mark.parametrize("seed", [5, 6])
def test_cigar_lengths_mixed_in_one_wave(depth_ctx, seed, want_depth):
    _check(depth_ctx, mw.cigar_wave(seed), want_depth=want_depth)


@pytest.mark.parametrize("name", ["one", "none", "window", "edges"])
def test_pileup_waves(depth_ctx, name):
    wave = mw.pileup_waves()[name]
    _check(depth_ctx, wave, want_depth=True)
    _check(depth_ctx, wave, want_depth=False)
    if name == "window":
        # the same lanes behind a wave without an eligible lane, and in reverse order (another window base)
        _check(depth_ctx, mw.pileup_waves()["none"] + wave + wave[::-1], want_depth=True)


@pytest.mark.parametrize("want_depth", [False, True])
@pytest.mark.parametrize("seed", [3, 4])
def test_aux_areas_mixed_in_one_wave(depth_ctx, seed, want_depth):
    wave = mw.aux_wave(seed)
    assert mw.aux_bytes(wave[-1]) == 100                  # the longest aux area is the last thing in the chunk
    _check(depth_ctx, wave, want_depth=want_depth)
    if not want_depth:
        _check(depth_ctx, wave, defer=True)
