#!/usr/bin/env python3
"""optBA's sample loop WITH the decomposition (reference src/bundleadjust/optBA.cpp:198-224; sampleRandomState,
src/RDISOptimizer.cpp:1196-1216), on the device: S whole states of ladybug 5 cameras / 30 points drawn from the sampling
intervals live in a population, and every round runs the camera plan (points fixed) and then the point plan (cameras fixed)
on ALL of them -- two launches a round, no host traffic in between: a member's constants are its own cameras / points.  After
every round the members are evaluated (one launch) and the best one selected on the device, and at the end it is assigned to the problem.  For comparison the
same loop runs one member at a time on the problem itself (set_x, set_start(None), solve, get_x), the way without populations.

  python examples/ba_population.py [members] [rounds] [seed]

Full ladybug (49 cameras, 7776 points) is examples/ba_population_full.py: its 7776 three-variable point components stay on the
tiny-component solver (plan option "population_tiny" = 1), its camera plan is kept on the LDS-resident solver by
"coop_min_factors" = 0 and "coop_group_min_factors" = 0.  The options below keep every component of the small problem on the
LDS-resident solver; the script checks "components_lds" before it solves."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rdis_amd import capi, problems as P  # noqa: E402
from ba_multistart import sampling_intervals  # noqa: E402

OPTIONS = {"row_min_components": 1 << 40, "coop_min_factors": 0, "coop_group_min_factors": 0}


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    lo, hi = sampling_intervals(pp)
    X = np.random.default_rng(seed).uniform(lo, hi, size=(members, pp.nvars))

    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
    for plan in plans:
        for k, v in OPTIONS.items():
            plan.set_option(k, v)
        if plan.info("components_lds") != plan.ncomp:
            sys.exit("a component of the plan does not fit the LDS-resident solver: no population solve")
        plan.set_start(None); plan.solve(25, 3e-8); plan.fetch()       # (tables, first launch)
    g.set_x(pp.x0)

    pop = capi.Population(g, x=X)
    t = time.perf_counter()
    best = []
    for _ in range(rounds):
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8)
        pop.eval_device()                          # (all members in one launch, the values stay on the device)
        best.append(pop.best()[0])                 # (selected there; kept per round for the line below: the round's one wait)
    pop.assign_best()
    x_pop = pop.get_x()
    together = time.perf_counter() - t
    f = pop.eval()

    t = time.perf_counter()
    x_seq = np.empty_like(X)
    for s in range(members):
        g.set_x(X[s])
        for _ in range(rounds):
            for plan in plans:
                plan.set_start(None)
                plan.solve(25, 3e-8)
        x_seq[s] = g.get_x()
    sequential = time.perf_counter() - t
    pop.assign_best()

    ok = np.isfinite(f)
    print(f"{members} members from the sampling intervals, {rounds} rounds of camera plan + point plan, 25 CG iterations a solve "
          f"({int(np.sum(~ok))} members not finite)")
    print(f"best member per round: {best}; f = {f[best[-1]]:.6f} (x0 itself: {capi.Problem(ctx, pp).eval():.6f})")
    print(f"population : {together * 1e3:8.2f} ms  ({2 * rounds} solver launches, {rounds} evaluations)")
    print(f"one by one : {sequential * 1e3:8.2f} ms  -> {sequential / together:.1f} x; the same bytes of x: {x_pop.tobytes() == x_seq.tobytes()}")
    print(f"the problem is left at the best member: f = {g.eval():.6f}")


if __name__ == "__main__":
    main()
