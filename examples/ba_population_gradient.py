#!/usr/bin/env python3
"""Which members of a population have converged?  The camera / point alternation of examples/ba_population.py on ladybug 5
cameras / 30 points, 64 members from the sampling intervals; after every round all members' values AND gradients are formed in
one call (rdis_hip_population_eval_grad_device: the member a grid dimension, three or four kernels for the whole population)
and every row's largest gradient entry is reduced on the device (rdis_hip_population_grad_max).  Per round: f and max |g| per
quartile of the members, and how many members' gradient maximum fell below the round before.  At the end three members are
checked against the member-by-member route (population_assign + rdis_hip_eval_grad): the same bytes.

  python examples/ba_population_gradient.py [members] [rounds] [seed]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rdis_amd import capi, problems as P  # noqa: E402
from ba_multistart import sampling_intervals  # noqa: E402

OPTIONS = {"row_min_components": 1 << 40, "coop_min_factors": 0, "coop_group_min_factors": 0}


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
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
    pop = capi.Population(g, x=X)

    def quartiles(v):
        return "  ".join(f"{q:11.4e}" for q in np.nanquantile(v, [0.0, 0.25, 0.5, 0.75, 1.0]))

    print(f"{members} members from the sampling intervals, camera plan + point plan a round, 25 CG iterations a solve")
    print("round   f: min / quartiles / max                                          max |g|: min / quartiles / max"
          "                                   fell")
    before = None
    for r in range(rounds + 1):
        if r > 0:
            for plan in plans:
                plan.solve_population(pop, 25, 3e-8)
        fd, _ = pop.eval_grad_device()                 # (enqueued behind the solves: nothing waited for)
        gmax = pop.grad_max()                          # (the round's one wait: members doubles come back)
        f = np.frombuffer(ctx.copy_to_host(fd, 8 * members), dtype=np.float64)
        fell = "" if before is None else f"{int(np.sum(gmax < before)):4d} of {members}"
        print(f"{r:5d}   {quartiles(f)}   {quartiles(gmax)}   {fell}")
        before = gmax
    print(f"kernels of the last gradient call: {pop.info('grad_launches')} for {pop.info('grad_members_per_launch')} members a round")

    f, gr = pop.eval_grad()
    same = True
    for s in sorted({0, members // 2, members - 1}):
        pop.assign(s)
        fs, gs = g.eval_grad()
        same = same and np.float64(fs).tobytes() == f[s].tobytes() and gs.tobytes() == gr[s].tobytes()
    print(f"against population_assign + eval_grad member by member, the same bytes: {same}")


if __name__ == "__main__":
    main()
