#!/usr/bin/env python3
"""optBA's sample loop with ONE CGD call over everything, on the device: full ladybug (49 cameras, 7776 points, 31843
observations) as a single component, S whole states drawn from the sampling intervals in a population, and one launch that runs
CGD on all of them -- a workgroup of 768 lanes of the point-major streaming solver per member (cameras in LDS, the member's point
blocks streamed from its replica of the point records; plan options "population_point_major" = 1 and "ptm_group" = 1:
solver_ptm_population.hpp).  Then the members are evaluated in one launch, the best one is selected on the device and assigned to
the problem.  For comparison the same members are solved one at a time on the problem itself (set_x, set_start(None), solve,
get_x) with the same plan options, and the example prints whether the bytes agree.

  python examples/ba_population_whole.py [members] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rdis_amd import capi, problems as P  # noqa: E402
from ba_multistart import sampling_intervals  # noqa: E402

# (by default one component of this size is shared by the workgroups of a cooperative or a wide group: other sums, other bits)
OPTIONS = {"coop_min_factors": 0, "coop_group_min_factors": 0, "ptm_stream": 2, "ptm_group": 1, "population_point_major": 1}


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    pp = P.load_bal().single_component()
    lo, hi = sampling_intervals(pp)
    X = np.random.default_rng(seed).uniform(lo, hi, size=(members, pp.nvars))

    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plan = capi.Plan(g)
    for k, v in OPTIONS.items():
        plan.set_option(k, v)
    plan.set_start(None); plan.solve(25, 3e-8); plan.fetch()       # (tables, first launch)
    if plan.info("components_point_major") != 1 or plan.info("point_major_group") != 1:
        sys.exit("the component is not on the point-major solver as one workgroup")
    g.set_x(pp.x0)

    pop = capi.Population(g, x=X)
    t = time.perf_counter()
    plan.solve_population(pop, 25, 3e-8)           # every sample's CGD call, one launch
    pop.eval_device()                              # (all members in one launch, the values stay on the device)
    pop.assign_best()                              # (selected there)
    best, f_best = pop.best()                      # (the one wait)
    together = time.perf_counter() - t
    x_pop = pop.get_x()
    x_best = g.get_x()
    launches = plan.last_kernel_ms()[1]

    t = time.perf_counter()
    x_seq = np.empty_like(X)
    for s in range(members):
        g.set_x(X[s])
        plan.set_start(None)
        plan.solve(25, 3e-8)
        x_seq[s] = g.get_x()
    sequential = time.perf_counter() - t
    pop.assign_best()

    f = pop.eval()
    print(f"full ladybug as one component ({pp.nvars} variables, {pp.nfac} factors), {members} members from the sampling intervals, "
          f"25 CG iterations: {launches} launch of {members} workgroups of {plan.info('population_point_major_threads')} lanes "
          f"({int(np.sum(~np.isfinite(f)))} members not finite)")
    print(f"best member: {best}; f = {f_best:.6f} (x0 itself: {capi.Problem(ctx, pp).eval():.6f})")
    print(f"population : {together * 1e3:8.2f} ms  (one solver launch, one evaluation, the selection)")
    print(f"one by one : {sequential * 1e3:8.2f} ms  -> {sequential / together:.1f} x; the same bytes: {x_pop.tobytes() == x_seq.tobytes()}")
    print(f"the problem is left at the best member: {x_best.tobytes() == x_seq[best].tobytes()}, f = {g.eval():.6f}")


if __name__ == "__main__":
    main()
