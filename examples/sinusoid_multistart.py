#!/usr/bin/env python3
"""RDIS's random restarts (sampleRandomState, reference src/RDISOptimizer.cpp:1196-1216) on optSinusoid's function
(BASELINE config 2: 121 variables, 362 nonlinear-product factors, one component), on the device: K starts drawn uniformly
in the variables' domains, every one of them solved by CGD (25 iterations) in ONE call of the multi-start entry -- one
workgroup of the plain solver per start.  Then the same with the root variable held constant: three independent subtrees,
each of which keeps its own best start, as an RDIS node does with its children.

  python examples/sinusoid_multistart.py [nstarts] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdis_amd import capi, problems as P  # noqa: E402


def report(title, plan, ms, wall):
    kernel_ms, launches = plan.last_kernel_ms()
    print(f"{title}: {ms.fret.shape[0]} starts x {plan.ncomp} component(s), {wall * 1e3:.2f} ms "
          f"({launches} launch(es), {kernel_ms:.2f} ms on the device)")
    for c in range(plan.ncomp):
        f = ms.fret[:, c]
        ok = np.isfinite(f)
        distinct = np.unique(np.round(f[ok] / 1e-6).astype(np.int64)).shape[0]
        print(f"  component {c}: best f = {np.min(f[ok]):.6f} (start {int(ms.best[c])}), "
              f"{distinct} distinct end values to 1e-6, {int(np.sum(~ok))} not finite")
    print(f"  sum of the best per component = {plan.objective():.6f}")


def main():
    nstarts = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    pp = P.make_high_dim_sinusoid().single_component()
    starts = np.random.default_rng(seed).uniform(pp.lo, pp.hi, size=(nstarts, pp.nvars))

    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plan = capi.Plan(g)
    plan.set_start(pp.x0); plan.solve(25, 3e-8); plan.fetch()          # (tables, first launch)
    t = time.perf_counter()
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    report("all variables free", plan, ms, time.perf_counter() - t)
    print(f"  the problem is left at the best start's result: f = {g.eval():.6f}")

    # the root assigned (to the value the best start found): its three subtrees are independent components
    assigned = np.zeros(pp.nvars, np.uint8)
    assigned[0] = 1
    comps = g.components(assigned)
    sub = capi.Plan(g, *comps)
    t = time.perf_counter()
    sub.solve_starts(starts[:, comps[1]], 25, 3e-8)
    ms = sub.fetch_starts()
    report(f"root held at {g.get_x([0])[0]:.6f}", sub, ms, time.perf_counter() - t)
    print(f"  starts kept per subtree: {ms.best.tolist()}; the whole function there: f = {g.eval():.6f}")


if __name__ == "__main__":
    main()
