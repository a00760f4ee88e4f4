#!/usr/bin/env python3
"""Where a wave of triage_classify_kernel spends its life, from the diagnostic (-DIM_STAMPS) build: six readings of the shader clock
per wave (im_triage.hip, IM_TRI_STAMP), one record per workgroup, read back through im_debug_tri_stamps_read.  Three settings on
bench.py's default shape: one buffer set's triage alone on the chip, the triage of the four sets overlapped, and the whole step
overlapped (four streams, graphs replayed back to back as in the bench; profiles/step_probe.py).  A record holds the last launch
that wrote it, whichever set's that was.

    INDELMINER_AMD_LIB=indelminer_amd/libindelminer_amd_stamps.so python profiles/triage_stamps.py [steps]

Clock ticks and shares only -- the stamped build is slower than the product and its run time is never quoted."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import bench  # noqa: E402
from indelminer_amd import capi, synth  # noqa: E402

PHASES = ["entry -> core arrived", "-> CIGAR / aux / sweep arrived", "-> classification done", "-> window written out", "-> publication done"]

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
ctx = capi.Context(0)
ctx.set_reference([refs[0].tobytes()] * bench.PIPELINE_DEPTH)
ctx.set_insert_ranges(["generic"], [rd.range_max])
ps = bench.PipeStep(ctx, rd, bench.PIPELINE_DEPTH)
ps.step(); ps.sync()                      # every buffer set holds a complete pass: partial passes below re-use what is there
for _ in range(bench.PIPELINE_DEPTH):
    ps.step()
ps.sync()
L = capi.lib()
L.im_debug_tri_stamps_read.argtypes = [C.c_void_p, C.c_int, C.c_int]
n_waves = -(-rd.n // 64)
full = [list(s["calls"]) for s in ps.sets]
kinds = [[getattr(fn, "__name__", "?") for fn, _ in calls] for calls in full]


def read(reset):
    buf = np.zeros((n_waves, 8), np.uint64)
    assert L.im_debug_tri_stamps_read(buf.ctypes.data_as(C.c_void_p), n_waves, 1 if reset else 0) == 0
    return buf[:, :6].astype(np.int64)


def table(t):
    # a record two launches wrote at once mixes their clocks: out of order, or a life of more than 10 M ticks -- dropped
    ok = (t[:, 0] > 0) & (np.diff(t, axis=1) >= 0).all(axis=1) & (t[:, 5] - t[:, 0] < 10_000_000)
    t = t[ok]
    d = np.diff(t, axis=1)
    life = t[:, 5] - t[:, 0]
    out = {"waves": int(len(t)), "life_mean": float(life.mean()), "life_median": float(np.median(life)), "phases": {}}
    for k, name in enumerate(PHASES):
        out["phases"][name] = {"mean": float(d[:, k].mean()), "median": float(np.median(d[:, k])), "share_of_life": float(d[:, k].sum() / life.sum())}
    return out


def capture(keep):
    for s, calls, kd in zip(ps.sets, full, kinds):
        s["calls"] = [c for c, k in zip(calls, kd) if keep(k)]
        s["graph"] = None
    ps.capture()


out = {"records": rd.n, "classify_waves": n_waves}
# one set's triage, nothing else on the chip
capture(lambda k: k in ("im_depth_reset", "im_dev_triage"))
one = ps.sets[0]
for k in range(12):
    if k == 11:
        read(True)
    ctx._check(L.im_graph_launch(one["graph"], one["stream"]))
    ctx._check(L.im_stream_sync(ctx.h, one["stream"]))
out["alone"] = table(read(True))
for name, keep in (("only triage, four sets overlapped", lambda k: k in ("im_depth_reset", "im_dev_triage")), ("whole step, four sets overlapped", lambda k: True)):
    capture(keep)
    for _ in range(20):
        ps.step()
    ps.sync()
    read(True)
    for _ in range(steps):
        ps.step()
    ps.sync()
    out[name] = table(read(True))
print(json.dumps(out, indent=1))
