#!/usr/bin/env python3
"""A node's random restarts with Levenberg-Marquardt as the subspace solver (RDISOptimizer.cpp:1087-1094 with optBA's
useCGD=false): ladybug 5 cameras / 30 points.  Every round draws `starts` rows of start values on the device
(Population.sample, the round as the stream), then the point plan and the camera plan each solve every one of their components
from every row in one solve_starts_population call and leave the problem at the best start per component -- the other plan's
variables, the constants of the solve, come from the problem's x, so a half-round builds on the one before.  The drawn values
never leave the device.  After every half-round the plan's objective -- the sum of its winners' values, which is the whole
objective here because every factor belongs to exactly one point component and to exactly one camera component -- is summed on
the device and printed; the script exits with an error if the last one is not the problem's value or not below the start's.

  python examples/ba_lm_restarts.py [starts] [rounds] [iterations per half-round] [seed]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdis_amd import capi, problems as P  # noqa: E402


def sampling_intervals(pp, ncams):
    """around the start: 1e-2 of a variable's size; the two distortion coefficients of a camera stay where they are"""
    typ = np.concatenate([np.arange(9 * ncams) % 9, 9 + np.arange(pp.nvars - 9 * ncams) % 3])
    half = np.where((typ == 7) | (typ == 8), 0.0, 1e-2 * (1.0 + np.abs(pp.x0)))
    return pp.x0 - half, pp.x0 + half


def main():
    starts = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    seed = int(sys.argv[4]) if len(sys.argv) > 4 else 0x5D15
    pp = P.load_bal(ncams=5, npts=30)
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = {}
    for kind, fixed in (("points", slice(0, 45)), ("cameras", slice(45, None))):
        assigned = np.zeros(pp.nvars, dtype=np.uint8)
        assigned[fixed] = 1
        plans[kind] = capi.LmPlan(g, *g.components(assigned), model=2, history=1)
    f0 = g.eval()
    pop = capi.Population(g, nmembers=starts)
    pop.set_sampling(*sampling_intervals(pp, 5))
    print(f"{starts} starts a round, {rounds} rounds of point plan + camera plan ({plans['points'].ncomp} + {plans['cameras'].ncomp} components, "
          f"{iters} iterations each); f(x0) = {f0:.6f}")
    f = f0
    for r in range(rounds):
        pop.sample(seed, r)                                  # restartValue(seed, node = r, restart = the row, variable)
        line = []
        for kind, plan in plans.items():
            plan.solve_starts_population(pop, maxiters=iters)
            f = plan.objective()                             # (summed on the device; eight bytes are read)
            _, best = plan.fetch_starts()
            line.append(f"{kind} {f:.6f} ({len(set(best.tolist()))} distinct winners)")
        print(f"  round {r}: " + ", ".join(line))
    fx = g.eval()
    print(f"  the problem is left at f = {fx:.6f} ({plans['cameras'].info('launches')} solver launch(es) a camera half-round of "
          f"{plans['cameras'].info('members_per_launch')} starts)")
    if not (abs(f - fx) <= 1e-12 * fx and fx < f0):
        sys.exit("the last objective is not the problem's value, or no better than the start's")


if __name__ == "__main__":
    main()
