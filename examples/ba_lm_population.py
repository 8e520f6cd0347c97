#!/usr/bin/env python3
"""A population of restarts with Levenberg-Marquardt as the subspace solver (the reference's LMSubspaceOptimizer, optBA with
useCGD=false): ladybug 5 cameras / 30 points, `members` states drawn on the device from the sampling intervals, then rounds of
the camera / point alternation through two LmPlans -- every round two solve_population calls, six launches at most, all
members at once -- then the members' values (eval_device) and the best member assigned to the problem.  Residual model 2.
The plans' tables are built and uploaded once; nothing travels between host and device from the first round to the final
read; the script exits with an error if the loop took as long to enqueue as the result took to arrive (a call in it waited
for the device) or if the problem is not left at the best member.

  python examples/ba_lm_population.py [members] [rounds] [iterations per half-round] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rdis_amd import capi, problems as P  # noqa: E402
from ba_multistart import sampling_intervals  # noqa: E402


def alternation(plans, pop, rounds, iters):
    """nothing in it waits for the device"""
    for _ in range(rounds):
        for plan in plans:
            plan.solve_population(pop, maxiters=iters)
    pop.eval_device()
    pop.assign_best()


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    seed = int(sys.argv[4]) if len(sys.argv) > 4 else 0x5D15
    pp = P.load_bal(ncams=5, npts=30)
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = []
    for fixed in (slice(45, None), slice(0, 45)):            # the points constant: 5 camera components; the cameras constant: 30 points
        assigned = np.zeros(pp.nvars, dtype=np.uint8)
        assigned[fixed] = 1
        plans.append(capi.LmPlan(g, *g.components(assigned), model=2, history=1))
    f0 = g.eval()
    pop = capi.Population(g, nmembers=members)
    pop.set_sampling(*sampling_intervals(pp))
    pop.sample(seed, 0)
    pop.set_x(pp.x0, first=0, count=1)                       # member 0: the problem's own start
    start = pop.eval()
    alternation(plans, pop, rounds, iters)                   # (first launches, buffers)
    ctx.synchronize()
    pop.sample(seed, 0)
    pop.set_x(pp.x0, first=0, count=1)
    t = time.perf_counter()
    alternation(plans, pop, rounds, iters)
    enqueued = time.perf_counter() - t
    x = g.get_x()                                            # the final read: the one wait
    done = time.perf_counter() - t
    b, fb = pop.best()
    f = pop.eval()
    print(f"{members} members, {rounds} rounds of camera plan + point plan ({plans[0].ncomp} + {plans[1].ncomp} components, {iters} iterations each), "
          f"{plans[1].info('launches')} launch(es) a point half-round of {plans[1].info('members_per_launch')} members")
    print(f"  values at the start: best {np.nanmin(start):.6f}, median {np.nanmedian(start):.6f}   (x0 itself: {f0:.6f})")
    print(f"  values at the end:   best {np.nanmin(f):.6f}, median {np.nanmedian(f):.6f}; {int(np.sum(f < start))} of {members} members improved")
    print(f"  enqueued in {enqueued * 1e3:.2f} ms, result read after {done * 1e3:.2f} ms: "
          f"{'nothing but the final read waited' if enqueued < 0.5 * done else 'THE LOOP WAITED for the device'}")
    print(f"  the problem is left at member {b}, f = {fb:.6f}")
    if not enqueued < 0.5 * done:
        sys.exit("a call of the loop waited for the device")
    if not (x.tobytes() == pop.get_x(b).tobytes() and fb == g.eval() == np.nanmin(f)):
        sys.exit("the problem was not left at the best member")


if __name__ == "__main__":
    main()
