#!/usr/bin/env python3
"""Generate tests/golden/range_ref.json from the REAL reference build (oracle/_ref).

tests/test_oracle_vs_reference_range.py holds the CPU oracle to the reference on the inputs of the range suites (tied corner
scores, non-finite tracks, pivot ties, degenerate two-view scenes, ragged BA windows, cut pose graphs, ...).  Where oracle/_ref is
not built that comparison cannot run, so the reference's results are recorded here: per case of tests/oracle_range_cases.py the
SHA-256 of its output arrays (every NaN first replaced by the canonical quiet NaN), with the shapes and the return codes in clear.
Digests only: no input and no output value is stored.  A case listed in UNDEFINED_IN_REFERENCE is not run on the reference; the
oracle's own record is stored for it and marked "source": "oracle".

The file is written with sorted keys, one case per line; it comes out byte-identical from a clean `make -C oracle ref`.
Run in the build container only:

    python tests/golden/make_range_golden.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helpers as H  # noqa: E402
import oracle_range_cases as C  # noqa: E402

PATH = os.path.join(HERE, "range_ref.json")


def dump(store):
    lines = [f" {json.dumps(k)}: {json.dumps(store[k], sort_keys=True, separators=(',', ':'))}" for k in sorted(store)]
    return "{\n" + ",\n".join(lines) + "\n}\n"


def main():
    r = H.ref()
    assert r is not None, "oracle/_ref/libsfmref.so missing: run `make -C oracle ref` in the build container"
    store = {}
    for c in C.all_cases():
        k = C.key(c)
        assert k not in store, f"duplicate case id {k}"
        if k in C.UNDEFINED_IN_REFERENCE:
            store[k] = dict(C.record(c.run(H.oracle(), "orc")), source="oracle")
        else:
            store[k] = C.record(c.run(r, "ref"))
    with open(PATH, "w") as f:
        f.write(dump(store))
    per = {}
    for k in store:
        per[k.split("/")[0]] = per.get(k.split("/")[0], 0) + 1
    print("wrote range_ref.json:", len(store), "cases", per, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
