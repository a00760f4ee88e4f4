#!/usr/bin/env python3
"""The three per-chunk launches of a -G -P run on the configs[1] chunk (300 000 records without qualities), eight times each, for
rocprofv3 --kernel-trace --stats: the triage, span_scatter_kernel, pair_scatter_kernel.  python profiles/pairspan_probe.py
AUX=1: every record carries what an aligner writes in front of MQ / RG (31 bytes) and an RG:Z tag."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from indelminer_amd import capi, rawrec, synth  # noqa: E402

L = capi.lib()
refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
ctx = capi.Context(0)
ctx.set_reference([refs[0].tobytes()])
ctx.set_insert_ranges(["generic"], [rd.range_max])
ctx.depth_enable()
ctx.span_enable(10, 10)
ctx.pairspan_enable(10, 10)
AUX = os.environ.get("AUX") == "1"
raw, off = rawrec.records(rd, qual=False, rg="generic" if AUX else None,
                          aux_prefix=(b"NMC\x00" + b"MDZ100\x00" + b"ASC\x64" + b"XSC\x00" + b"MCZ100M\x00") if AUX else b"")
pipe = capi.Pipeline(ctx, rd.n, len(raw), cap_cand=max(4096, rd.n // 8), read_len_max=100, want_depth=True)
pipe.upload(raw, off)
tp = capi.TriageParams(pipe.tp.qthreshold, pipe.tp.ethreshold_vcfcheck, pipe.tp.maxpedelsize, 1, 0, 1)
tm = capi.Timer(ctx)
for name, call in (("triage (3 launches)", lambda: L.im_dev_triage(ctx.h, C.byref(tp), C.byref(pipe.recs), C.byref(pipe.cands), pipe.d_ts.ptr, pipe.ts_bytes, ctx.stream)),
                   ("span scatter", lambda: L.im_dev_span_scatter(ctx.h, C.byref(pipe.recs), ctx.stream)),
                   ("pair scatter", lambda: L.im_dev_pairspan_scatter(ctx.h, C.byref(pipe.recs), ctx.stream))):
    ts = []
    for _ in range(8):
        ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
        tm.start(ctx.stream)
        ctx._check(call())
        tm.stop(ctx.stream)
        ts.append(tm.elapsed_ms())
    print("%-20s aux=%d records %7d  bytes %9d  %7.1f us (HIP events, median of 6)" % (name, AUX, rd.n, len(raw), float(np.median(ts[2:])) * 1e3), flush=True)
ctx.pairspan_scan(0)
ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
p = np.arange(0, len(refs[0]), 997, dtype=np.int32)
print("pspan / 8 at every 997th position: median %d" % int(np.median(ctx.pairspan_query_tid(0, p, p)) // 8))
ctx.close()
