#!/usr/bin/env python3
"""Generates tests/golden/reference_frprmn.json: what the reference's own nrc::Frprmn (minimize_nrc.h, built as
oracle/_ref by oracle/Makefile where the reference tree is present) returns on the minimiser cases of
tests/test_oracle.py -- the reason code, the end point, the end value and the iteration count of every case, and the
start it was given.  tests/test_oracle.py holds the restated minimiser to these where oracle/_ref cannot be built, and
checks them against the live reference where it can.

    python tests/golden/make_reference_frprmn.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402


def main():
    if not O.ref_available():
        sys.exit("oracle/_ref is not built: the reference tree is needed to record its results")
    spec = importlib.util.spec_from_file_location("test_oracle", os.path.join(ROOT, "tests", "test_oracle.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    out = {}

    def record(key, f, g, x0, maxiters):
        rc, x, fret, it = O.ref_frprmn(f, g, x0, maxiters, 3e-8)
        out[key] = {"maxiters": maxiters, "x0": [float(v) for v in x0], "reason": int(rc), "x": [float(v) for v in x],
                    "fret": float(fret), "iter": int(it)}
    for maxiters in (1, 2, 7, 25, 400):
        for k, (f, g, x0) in enumerate(T._minimiser_cases(maxiters)):
            record("maxiters_%d_case_%d" % (maxiters, k), f, g, x0, maxiters)
    f, g, x0 = T._ba_minimiser_case()
    record("ladybug_5_30", f, g, x0, 25)
    with open(os.path.join(HERE, "reference_frprmn.json"), "w") as fh:   # one case a line
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main()
