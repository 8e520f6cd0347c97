#!/usr/bin/env python3
"""RDIS's random restarts WITH the decomposition (sampleRandomState, reference src/RDISOptimizer.cpp:1196-1216; a node's
restarts :1087-1094) on optSinusoid's function (BASELINE config 2: 121 variables, 362 nonlinear-product factors), on the
device: S whole states drawn uniformly in the variables' domains live in a population, and every round runs the root plan
(variable 0 free, the subtrees constants) and then the three-subtree plan (the root constant) on ALL of them -- two launches a
round, one workgroup of the plain solver per (component, member), no host traffic in between: a member's constants are its own
earlier results, which examples/sinusoid_multistart.py, with the root at one value for all starts, cannot do.  After the rounds
the members are evaluated (one launch), the lowest is selected on the device, and that member is assigned to the problem.  For comparison
the same loop runs one member at a time on the problem itself (set_x, set_start(None), solve, get_x), the way without
populations.

  python examples/sinusoid_population.py [members] [rounds] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdis_amd import capi, problems as P  # noqa: E402


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    pp = P.make_high_dim_sinusoid()
    X = np.random.default_rng(seed).uniform(pp.lo, pp.hi, size=(members, pp.nvars))

    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    only_root = np.ones(pp.nvars, np.uint8)
    only_root[0] = 0
    plans = [capi.Plan(g, *g.components(only_root)), capi.Plan(g, *g.components(1 - only_root))]
    for plan in plans:
        plan.set_option("population_plain", 1)                         # (nonlinear-product plans: opt-in)
        if plan.info("components_plain") != plan.ncomp:
            sys.exit("a component of the plan does not run on the plain batch solver: no population solve")
        plan.set_start(None); plan.solve(25, 3e-8); plan.fetch()       # (tables, first launch)
    g.set_x(pp.x0)

    pop = capi.Population(g, x=X)
    t = time.perf_counter()
    for _ in range(rounds):
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8)
    pop.eval_device()                              # (all members in one launch, the values stay on the device)
    pop.assign_best()                              # (the lowest is selected and assigned there: nothing waited for)
    x_pop = pop.get_x()
    together = time.perf_counter() - t
    best, _ = pop.best()
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
    print(f"{members} uniform members, {rounds} rounds of root plan ({plans[0].ncomp} component) + subtree plan "
          f"({plans[1].ncomp} components), 25 CG iterations a solve ({int(np.sum(~ok))} members not finite)")
    print(f"best member: {best}, f = {f[best]:.6f}; {np.unique(np.round(f[ok] / 1e-6).astype(np.int64)).shape[0]} distinct end values to 1e-6")
    print(f"population : {together * 1e3:8.2f} ms  ({2 * rounds} solver launches, 1 evaluation)")
    print(f"one by one : {sequential * 1e3:8.2f} ms  -> {sequential / together:.1f} x; the same bytes of x: {x_pop.tobytes() == x_seq.tobytes()}")
    print(f"the problem is left at the best member: f = {g.eval():.6f}")


if __name__ == "__main__":
    main()
