"""What tests/test_gpu_depth_median.py, tests/test_gpu_depth_evidence.py and tests/test_depth_evidence_host.py share: the plain
restatement of the median query and of the -D fields, written from the definitions in include/indelminer_amd.h and DESIGN.md
section 4.5d, not from the code under test.  tests/test_depth_evidence_host.py pins it to cases worked by hand (no GPU needed)."""
import numpy as np

NONE = 0xFFFFFFFF       # the answer for an interval without positions
CAP = 4095              # a deeper position counts as this
MIN_LEN, FLANK = 50, 1000


def medians(depth, beg, end):
    """per query the lower median of min(depth, CAP) over [beg, end) clipped to the contig: sort, element (n - 1) // 2"""
    clen = len(depth)
    out = []
    for a, b in zip(beg, end):
        a, b = max(int(a), 0), min(int(b), clen)
        if a >= b:
            out.append(NONE)
            continue
        v = np.sort(np.minimum(depth[a:b], CAP))
        out.append(int(v[(len(v) - 1) // 2]))
    return np.array(out, np.int64)


def lower_median(depth, a, b):
    m = int(medians(depth, [a], [b])[0])
    return None if m == NONE else m


def evidence_of(depth, pos, end):
    """(DM text, DFC text) of a deletion with these printed coordinates"""
    inside, l, r = lower_median(depth, pos, end), lower_median(depth, pos - FLANK, pos), lower_median(depth, end, end + FLANK)
    if l is not None and r is not None:
        dfc = "." if l + r == 0 else str((2000 * inside + (l + r) // 2) // (l + r))
    elif l is not None or r is not None:
        f = l if l is not None else r
        dfc = "." if f == 0 else str((1000 * inside + f // 2) // f)
    else:
        dfc = "."
    return ",".join("." if x is None else str(x) for x in (inside, l, r)), dfc
