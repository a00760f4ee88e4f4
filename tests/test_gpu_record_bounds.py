"""The four realign kernels at the bounds of the result record: IM_MAX_OPS = 64 segment words and IM_MAX_EV = 4 evidence
records per read (include/indelminer_amd.h), which the reference does not have.  The batches come from
tests/support/recordbounds.py: per route, reads whose oracle result has exactly 59 .. 67 segments or 2 .. 6 indels, shuffled
among ordinary reads, an overflow read first and last (tests/test_record_bounds_host.py proves that much on the CPU).
The rule is gpucmp.hip_vs_oracle_at_bounds: a result that fits is compared field for field, one beyond a bound must come back
IM_ST_OVERFLOW with the oracle's band bookkeeping -- and must leave its neighbours, the bytes behind the results and the
evidence slots alone (ops[] is the record's last field: ops[64] of read i is the status of read i + 1).

Which bound a route can reach: the segment bound on realign_long_kernel and realign_any_kernel only (a list grows by at most
2 words per ~12 bases: the densest list of a 255-base read has 33 words), the indel bound on realign_band_kernel and
realign_any_kernel only (numgaps == 0 leaves one indel per read).  Lists of 62, 64 and 66 words come from recordbounds.even."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.support import gpucmp, recordbounds as rb

pytestmark = pytest.mark.gpu

ROUTES = sorted(rb.ROUTES)
SEED = 77               # what the evidence slots hold before a launch, as test_general_pass_on_the_device_entry seeds them
GUARD = 0xA5


DUMP_DIR = os.environ.get("INDELMINER_TEST_DUMPS", "mismatch_dumps")       # where the reads of a failed comparison go


def _dump(tag, bad, B):
    os.makedirs(DUMP_DIR, exist_ok=True)
    with open(os.path.join(DUMP_DIR, "mismatch_record_bounds_%s.txt" % tag), "w") as fh:
        fh.write(rb.report(B) + "\n")
        for i, msg in bad:
            c, info = B.cases[i], B.info[i]
            fh.write(repr((i, msg, c["label"], info.n_ops, info.n_ev, c["anchor"], c["range_max"], c["read"])) + "\n")


def _check_records(B, out, tag, idx=None):
    """every record against the rule; idx: the batch positions the records belong to (default: all, in order)"""
    idx = range(len(B.cases)) if idx is None else idx
    bad = []
    for rec, i in zip(out, idx):
        msg = gpucmp.hip_vs_oracle_at_bounds(rec, B.info[i].st, B.info[i].res)
        if msg:
            bad.append((i, msg))
    if bad:
        _dump(tag, bad, B)
    assert not bad, "%s: %d of %d differ, first: read %d (%s, oracle n_ops %d n_ev %d): %s" % (
        tag, len(bad), len(out), bad[0][0], B.cases[bad[0][0]]["label"], B.info[bad[0][0]].n_ops, B.info[bad[0][0]].n_ev, bad[0][1])


def _content(rec):
    """what a record says, without the words behind n_ops / n_ev (nobody writes them)"""
    return (int(rec["status"]), int(rec["ref_start"]), int(rec["n_ops"]), int(rec["n_ev"]), int(rec["n_band"]), rec["band"].tobytes(),
            rec["ev"][:int(rec["n_ev"])].tobytes(), rec["ops"][:int(rec["n_ops"])].tobytes())


def _host_run(ctx, capi, B, idx):
    cases = [B.cases[i] for i in idx]
    ctx.set_reference([B.contig])
    return ctx.realign_batch(capi.params(**B.kw), [c["read"].encode() for c in cases], np.zeros(len(cases), np.int32),
                             np.array([c["anchor"] for c in cases], np.int32), np.array([c["range_max"] for c in cases], np.int32),
                             allow=(capi.E_OVERFLOW,))


@pytest.mark.parametrize("name", ROUTES)
def test_host_entry_every_record_and_the_neighbours(gpu_ctx, name):
    """im_realign_batch: every record passes the rule; IM_E_OVERFLOW when and only when the batch holds an overflow read, with
    every record filled and im_last_error naming a read that did overflow; the ordinary reads come out exactly as in a batch
    without the bound reads"""
    from indelminer_amd import capi
    B = rb.select(name)
    n = len(B.cases)
    rc, out = _host_run(gpu_ctx, capi, B, range(n))
    _check_records(B, out, name + "_host")
    over = [i for i in range(n) if B.info[i].overflow]
    assert rc == (capi.E_OVERFLOW if over else capi.IM_OK), (rc, rb.report(B))
    if over:
        err = capi.lib().im_last_error(gpu_ctx.h).decode()
        m = re.match(r"read (\d+): ", err)
        assert m and int(m.group(1)) in over and "IM_MAX_OPS" in err, err
        assert over[0] == 0 and over[-1] == n - 1
    plain = [i for i in range(n) if B.cases[i]["label"] is None]
    rc2, alone = _host_run(gpu_ctx, capi, B, plain)
    assert rc2 == capi.IM_OK
    _check_records(B, alone, name + "_host_plain", plain)
    differ = [i for j, i in enumerate(plain) if _content(alone[j]) != _content(out[i])]
    assert not differ, "ordinary reads that change beside the bound reads: %r" % differ[:8]
    assert int((alone["status"] == 1).sum()) >= len(plain) // 2


class _DeviceRun:
    """one im_dev_realign_n / im_dev_realign_keep launch over a batch, the caller owning every buffer: one guard record behind
    the results and 64 guard bytes behind each slot array"""

    def __init__(self, ctx, capi, B, entry):
        self.bufs = []
        reads = [c["read"].encode() for c in B.cases]
        n = self.n = len(reads)
        ctx.set_reference([B.contig])
        ctx.expect_read_length(max(len(r) for r in reads))
        offs = np.zeros(n + 1, np.int64)
        np.cumsum([(len(r) + 3) & ~3 for r in reads], out=offs[1:])
        bases = np.zeros(int(offs[-1]) + 16, np.uint8)
        for i, r in enumerate(reads):
            bases[offs[i]:offs[i] + len(r)] = np.frombuffer(r, np.uint8)

        def dev(arr):
            arr = np.ascontiguousarray(arr)
            b = capi.DevBuf(ctx, max(arr.nbytes, 16)).upload(arr)
            self.bufs.append(b)
            return b
        d_bases, d_off = dev(bases), dev(offs[:n].copy())
        d_len, d_tid = dev(np.array([len(r) for r in reads], np.int32)), dev(np.zeros(n, np.int32))
        d_anchor = dev(np.array([c["anchor"] for c in B.cases], np.int32))
        d_range = dev(np.array([c["range_max"] for c in B.cases], np.int32))
        rsz = capi.RESULT_DTYPE.itemsize
        self.d_res = dev(np.full((n + 1) * rsz, GUARD, np.uint8))
        slots = np.full(n * capi.MAX_EV + 16, SEED, np.int32)
        self.d_slots = [dev(slots) for _ in range(3)]
        d_n = dev(np.array([n], np.int32))
        batch = capi.DevBatch(n, d_bases.ptr, d_off.ptr, d_len.ptr, d_tid.ptr, d_anchor.ptr, d_range.ptr, self.d_res.ptr,
                              *[d.ptr for d in self.d_slots])
        P = capi.params(**B.kw)
        L = capi.lib()
        if entry == "keep":
            ctx._check(L.im_dev_realign_keep(ctx.h, C.byref(P), C.byref(batch), ctx.stream))
        else:
            ctx._check(L.im_dev_realign_n(ctx.h, C.byref(P), C.byref(batch), d_n.ptr, 1 if entry == "n_keep" else 0, ctx.stream))
        ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
        raw = self.d_res.download(np.uint8, (n + 1) * rsz)
        self.out = raw[:n * rsz].view(capi.RESULT_DTYPE)
        self.guard = raw[n * rsz:]
        got = [d.download(np.int32, n * capi.MAX_EV + 16) for d in self.d_slots]
        self.cls, self.b1, self.b2 = [g[:n * capi.MAX_EV].reshape(n, capi.MAX_EV) for g in got]
        self.slot_guards = [g[n * capi.MAX_EV:] for g in got]

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("entry", ["n_clear", "n_keep", "keep"])
@pytest.mark.parametrize("name", ROUTES)
def test_device_entry_guards_and_evidence_slots(gpu_ctx, name, entry):
    """im_dev_realign_n (clearing and keeping form) and im_dev_realign_keep on buffers the test owns: every record by the rule,
    the record behind the last read (an overflow read's, where the route has any) and the 64 bytes behind each slot array
    untouched; a fitting read's slots hold ranks 0 .. n_ev - 1 and -1 behind them, an overflow read's hold -1 four times in the
    clearing form and what they held before in the keeping form"""
    from indelminer_amd import capi
    B = rb.select(name)
    run = _DeviceRun(gpu_ctx, capi, B, entry)
    try:
        _check_records(B, run.out, "%s_dev_%s" % (name, entry))
        assert (run.guard == GUARD).all(), "bytes behind the last record written: %r" % np.nonzero(run.guard != GUARD)[0][:8]
        for g in run.slot_guards:
            assert (g == SEED).all()
        keep = entry != "n_clear"
        bad = []
        for i, info in enumerate(B.info):
            cls, b1, b2 = ([int(x) for x in a[i]] for a in (run.cls, run.b1, run.b2))
            if info.fits:
                ev = [info.res.ev[k] for k in range(info.n_ev)]
                pad = capi.MAX_EV - info.n_ev
                want = ([e.cls for e in ev] + [-1] * pad, [e.b1 for e in ev] + [0] * pad, [e.b2 for e in ev] + [0] * pad)
            elif keep:
                want = ([SEED] * 4,) * 3
            else:
                want = ([-1] * 4, [0] * 4, [0] * 4)
            if (cls, b1, b2) != want:
                bad.append((i, B.cases[i]["label"], info.st, info.n_ev, (cls, b1, b2), want))
        assert not bad, "%d reads with wrong evidence slots, first: %r" % (len(bad), bad[0])
    finally:
        run.free()


@pytest.mark.parametrize("name", ROUTES)
def test_compact_results_leaves_overflow_reads_out(gpu_ctx, name):
    """im_dev_compact_results over such a batch: overflow reads are not packed and their status says IM_ST_OVERFLOW, the
    evidence reads are packed whole -- 64 segment words included, where the route has such a list"""
    from indelminer_amd import capi
    B = rb.select(name)
    run = _DeviceRun(gpu_ctx, capi, B, "n_clear")
    n = run.n
    d = [capi.DevBuf(gpu_ctx, 4 * n), capi.DevBuf(gpu_ctx, 4 * n), capi.DevBuf(gpu_ctx, 512 * n), capi.DevBuf(gpu_ctx, 256)]
    try:
        L = capi.lib()
        gpu_ctx._check(L.im_dev_compact_results(gpu_ctx.h, run.d_res.ptr, n, None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, gpu_ctx.stream))
        gpu_ctx._check(L.im_stream_sync(gpu_ctx.h, gpu_ctx.stream))
        cnt = int(d[3].download(np.int32, 1)[0])
        stat, slot = d[0].download(np.int32, n), d[1].download(np.int32, n)
        comp = d[2].download(capi.RESULT_DTYPE, n)[:cnt]
        want_stat = [gpucmp.expected_status(i.st, i.res) for i in B.info]
        assert [int(x) for x in stat] == want_stat
        fits = [i for i in range(n) if B.info[i].fits]
        assert cnt == len(fits) and sorted(int(slot[i]) for i in fits) == list(range(cnt))
        assert all(int(slot[i]) == -1 for i in range(n) if not B.info[i].fits)
        _check_records(B, [comp[int(slot[i])] for i in fits], name + "_compact", fits)
        assert all(comp[int(slot[i])].tobytes() == run.out[i].tobytes() for i in fits)
        if "ops" in B.reaches and name != "any_g3":
            assert max(int(r["n_ops"]) for r in comp) == capi.MAX_OPS
        if "ev" in B.reaches:
            assert max(int(r["n_ev"]) for r in comp) == capi.MAX_EV
    finally:
        run.free()
        for b in d:
            b.free()
