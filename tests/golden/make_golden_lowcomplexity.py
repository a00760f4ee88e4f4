#!/usr/bin/env python3
"""The reference's answers to the low-complexity inputs of tests/support/lowcomplexity.py, made by the REFERENCE compiled in
place (oracle/Makefile; build container only), stored in tests/golden/ref_lowcomplexity.json:

  realign   attempt_pe_alignment (oracle/_ref/libimref.so) on realign_cases for every (k, g, seed) of REALIGN_RUNS: the
            evidence list per read (segments without their bases: lowcomplexity.thin), or "abort" where the oracle says
            the reference would exit inside the process (forceassert) and it is not called.  One byte that never equals a
            base lies in front of the contig.
  sw        realign_with_indel (oracle/_ref/librefunits.so) on sw_cases: the inputs and the three counts, as units_sw.json

  python tests/golden/make_golden_lowcomplexity.py

Commits data only."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.support import lowcomplexity as lc, oraclebind as ob, refbind, refcases  # noqa: E402


def fronted(cb):
    """the contig as the reference gets it: a '#' in front of its first base (tests/test_oracle_vs_ref.py)"""
    raw = C.create_string_buffer(b"#" + cb)
    return raw, C.cast(C.addressof(raw) + 1, C.POINTER(C.c_char * (len(cb) + 1))).contents


def run_sw(L, c):
    s, i, a = C.c_int(), C.c_int(), C.c_int()
    L.imref_realign_with_indel(c["contig"].encode(), C.c_int(c["rstart"]), C.c_int(c["rstop"]), c["read"].encode(), C.c_int(c["qstart"]),
                               C.c_int(c["qstop"]), C.c_int(c["is_deletion"]), C.c_uint(c["vstart"]), C.c_uint(c["vstop"]),
                               c["alternate"].encode(), C.byref(s), C.byref(i), C.byref(a))
    return [s.value, i.value, a.value]


def main():
    units = os.path.join(ROOT, "oracle", "_ref", "librefunits.so")
    if not refbind.available() or not os.path.exists(units):
        sys.exit("oracle/_ref missing: run `make -C oracle ref` where the reference sources are")
    R = refbind.Ref()
    doc = {"made_by": "attempt_pe_alignment (oracle/_ref/libimref.so) and realign_with_indel (oracle/_ref/librefunits.so) of the "
                      "reference on the inputs of tests/support/lowcomplexity.py",
           "realign": {}, "sw": []}
    for k, g, seed in lc.REALIGN_RUNS:
        contig, cases, share = lc.realign_cases(seed)
        eth = max(k, 10)
        R.set_params(k, g, 1000, eth)
        P = ob.params(k, g, 1000, eth)
        cb = contig.encode()
        raw, buf = fronted(cb)
        out = []
        for c in cases:
            st, _ = ob.realign(P, cb, len(cb), c["anchor"], c["range_max"], c["read"])
            full = "abort" if st == -1 else refcases.plain(R.realign(buf, c["anchor"], c["range_max"], c["read"]))
            assert lc.with_bases(lc.thin(full), c["read"]) == full, c
            out.append(lc.thin(full))
        doc["realign"][refcases.key("lowc", k, g, seed)] = out
        print("k %2d g %2d seed %d: %d cases, in-repeat share %.3f, aborted %d, evidence %d"
              % (k, g, seed, len(cases), share, sum(o == "abort" for o in out), sum(len(o) for o in out if o not in (None, "abort"))))
    U = C.CDLL(units)
    made = lc.sw_cases(lc.SW_SEED, lc.SW_N)
    for c in made:
        d = lc.sw_inputs(c)
        d["expect"] = run_sw(U, d)
        doc["sw"].append(d)
    print("sw: %d cases, %d in or at a repeat, %d of whole repeat units, %d with indels on the best path"
          % (len(doc["sw"]), sum(c["in_repeat"] for c in made), sum(c["whole_units"] for c in made), sum(d["expect"][1] > 0 for d in doc["sw"])))
    path = os.path.join(ROOT, "tests", "golden", lc.GOLDEN_NAME)
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
    print("%s: %d realign runs, %d bytes" % (path, len(doc["realign"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
