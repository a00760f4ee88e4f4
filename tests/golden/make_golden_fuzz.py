#!/usr/bin/env python3
"""The reference's answers to the inputs of tests/test_oracle_vs_ref.py (tests/support/refcases.py), made by the REFERENCE
compiled in place (oracle/_ref/libimref.so, oracle/Makefile): its evidence list for every read, or "abort" where the
oracle says the reference would exit inside the process (forceassert) and it is not called.  Commits data only."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.support import leftedge, oraclebind as ob, refbind, refcases  # noqa: E402


def answers(R, P, cb, buf, cases):
    out = []
    for c in cases:
        st, _ = ob.realign(P, cb, len(cb), c["anchor"], c["range_max"], c["read"])
        out.append("abort" if st == -1 else refcases.plain(R.realign(buf, c["anchor"], c["range_max"], c["read"])))
    return out


def main():
    if not refbind.available():
        sys.exit("oracle/_ref/libimref.so missing: run `make -C oracle ref` where the reference sources are")
    R = refbind.Ref()
    doc = {"made_by": "attempt_pe_alignment of the reference (oracle/_ref/libimref.so) on the inputs of tests/support/refcases.py",
           "cases": {}}
    for k, g, seed in refcases.FUZZ:
        maxdel, contig, cases = refcases.fuzz(seed)
        eth = max(k, 10)
        R.set_params(k, g, maxdel, eth)
        cb = contig.encode()
        doc["cases"][refcases.key("fuzz", k, g, seed)] = answers(R, ob.params(k, g, maxdel, eth), cb, C.create_string_buffer(cb), cases)
    for k, g, seed in refcases.LEFT_EDGE:
        contig, cases = leftedge.cases(seed)
        R.set_params(k, g, 1000, 10)
        cb = contig.encode()
        # one byte in front of the contig that never equals a base: what the reference reads for a window at the contig's start
        raw = C.create_string_buffer(b"#" + cb)
        buf = C.cast(C.addressof(raw) + 1, C.POINTER(C.c_char * (len(cb) + 1))).contents
        doc["cases"][refcases.key("left_edge", k, g, seed)] = answers(R, ob.params(k, g, 1000, 10), cb, buf, cases)
    path = os.path.join(ROOT, "tests", "golden", refcases.GOLDEN_NAME)
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
    print("%s: %d runs, %d bytes" % (path, len(doc["cases"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
