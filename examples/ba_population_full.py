#!/usr/bin/env python3
"""optBA's sample loop with the decomposition on FULL ladybug (49 cameras, 7776 points, 31843 observations), on the device: S
whole states drawn from the sampling intervals live in a population, and every round runs the camera plan (points fixed: 49
components of hundreds of factors, on the LDS-resident solver) and then the point plan (cameras fixed: 7776 components of three
variables, on the tiny-component solver, sixteen lanes a point) on ALL of them.  The point plan takes the plan option
"population_tiny" = 1 (solver_quad_population.hpp): every member's blocks walk that member's points, with rotation records of
the member's own cameras.  After every round the members are evaluated (one launch) and the best one selected on the device; at the end it is assigned to the
problem.  For comparison the same loop runs one member at a time on the problem itself (set_x, set_start(None), solve, get_x)
with the same plan options.

  python examples/ba_population_full.py [members] [rounds] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rdis_amd import capi, problems as P  # noqa: E402
from ba_multistart import sampling_intervals  # noqa: E402

CAMERA_OPTIONS = {"coop_min_factors": 0, "coop_group_min_factors": 0}   # (by default cameras of hundreds of factors go to the cooperative solver)
POINT_OPTIONS = {"population_tiny": 1}


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    pp = P.load_bal()
    cams, pts = P.ba_alternation_plans(pp)
    lo, hi = sampling_intervals(pp)
    X = np.random.default_rng(seed).uniform(lo, hi, size=(members, pp.nvars))

    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
    for plan, options in zip(plans, (CAMERA_OPTIONS, POINT_OPTIONS)):
        for k, v in options.items():
            plan.set_option(k, v)
        plan.set_start(None); plan.solve(25, 3e-8); plan.fetch()       # (tables, first launch)
    if plans[0].info("components_lds") != plans[0].ncomp or plans[1].info("components_tiny") != plans[1].ncomp:
        sys.exit("the camera plan is not on the LDS-resident solver or the point plan not on the tiny-component solver")
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
    print(f"full ladybug, {members} members from the sampling intervals, {rounds} rounds of camera plan ({plans[0].ncomp} components, LDS-resident "
          f"solver) + point plan ({plans[1].ncomp} components, tiny-component solver, {plans[1].info('population_tiny_blocks')} blocks a member), "
          f"25 CG iterations a solve ({int(np.sum(~ok))} members not finite)")
    print(f"best member per round: {best}; f = {f[best[-1]]:.6f} (x0 itself: {capi.Problem(ctx, pp).eval():.6f})")
    print(f"population : {together * 1e3:8.2f} ms  ({2 * rounds} solver launches, {rounds} evaluations)")
    print(f"one by one : {sequential * 1e3:8.2f} ms  -> {sequential / together:.1f} x; the same bytes: {x_pop.tobytes() == x_seq.tobytes()}")
    print(f"the problem is left at the best member: f = {g.eval():.6f}")


if __name__ == "__main__":
    main()
