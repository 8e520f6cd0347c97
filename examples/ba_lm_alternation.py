#!/usr/bin/env python3
"""Camera / point alternation of full ladybug (49 cameras, 7776 points) with Levenberg-Marquardt as the subspace solver
(the reference's LMSubspaceOptimizer, optBA with useCGD=false), every half-round one call: the points fixed, the
components that are left -- 49 cameras of 9 unknowns -- come from rdis_hip_components and are solved by one
rdis_hip_lm_batch call; then the cameras fixed, 7776 points of 3 unknowns, likewise.  Residual model 2 (the two pixel
residuals of an observation, trial points kept inside the domains).  Prints the objective after every half-round.

  python examples/ba_lm_alternation.py [rounds] [iterations per half-round]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdis_amd import capi, problems as P  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    pp = P.load_bal()
    ncams = pp.meta["ncams"]
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = {}
    for name, fixed in (("cameras", slice(9 * ncams, None)), ("points", slice(0, 9 * ncams))):
        assigned = np.zeros(pp.nvars, dtype=np.uint8)
        assigned[fixed] = 1                                   # the other kind of block is constant in this half-round
        plans[name] = g.components(assigned)
        print("%s free: %d components" % (name, len(plans[name][0]) - 1))
    f = g.eval()
    print("start                        %.6f" % f)
    for r in range(rounds):
        for name in ("cameras", "points"):
            t = time.perf_counter()
            res = g.lm_batch(*plans[name], maxiters=iters, model=2, history=1)
            ms = (time.perf_counter() - t) * 1e3
            fn = g.eval()
            stops = np.bincount([q.stop for q in res], minlength=8)
            print("round %d, %-7s free: %14.6f   (%.2f ms; stop codes %s)" % (
                r + 1, name, fn, ms, ", ".join("%d x %d" % (n, s) for s, n in enumerate(stops) if n)))
            assert fn <= f, "a half-round raised the objective"
            f = fn


if __name__ == "__main__":
    main()
