#!/usr/bin/env python3
"""Successive halving on the device: 256 states of ladybug 5 cameras / 30 points are drawn ON the device from the sampling
intervals (Population.sample: restartValue's counter-based draw), and four rounds follow of camera plan + point plan on the
members 0 .. k-1 only (Plan.solve_population(first=0, count=k)), evaluation of all members (eval_device), ranking (sort: the
members put into the order of their values) and k //= 2 -- 256, 128, 64, 32 members solved.  At the end the best member is
assigned to the problem.  Then the same loop again with the worse half REDRAWN each round (sample with stream = round) instead
of dropped.  Everything is enqueued on one stream and the result is read once, at the end; the script checks that nothing but
that read waited: the whole loop is enqueued in a fraction of the time after which the result arrives (a call that waited
for the device would make the two times equal).

  python examples/ba_population_halving.py [members] [rounds] [seed]

The plans and their options are examples/ba_population.py's."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rdis_amd import capi, problems as P  # noqa: E402
from ba_multistart import sampling_intervals  # noqa: E402
from ba_population import OPTIONS  # noqa: E402


def halving(plans, pop, members, rounds, seed, redraw):
    """one loop; nothing in it waits for the device.  Returns the address of f after each round's sort (read by the caller
    afterwards, if at all)"""
    pop.sample(seed, 0)
    k = members
    for r in range(rounds):
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8, first=0, count=k)
        pop.eval_device()
        pop.sort(want_order=False)
        if redraw:
            pop.sample(seed, r + 1, first=members // 2)   # the worse half: new states, another stream every round
        else:
            k = max(1, k // 2)
    if redraw:
        pop.eval_device()
    pop.assign_best()


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0x5D15
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    lo, hi = sampling_intervals(pp)

    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
    for plan in plans:
        for k, v in OPTIONS.items():
            plan.set_option(k, v)
        if plan.info("components_lds") != plan.ncomp:
            sys.exit("a component of the plan does not fit the LDS-resident solver: no population solve")
    f0 = g.eval()

    for redraw in (False, True):
        pop = capi.Population(g, nmembers=members)
        pop.set_sampling(lo, hi)
        halving(plans, pop, members, rounds, seed, redraw)            # (tables, buffers, first launches)
        ctx.synchronize()
        # per round the best value, from a loop that reads it (one wait a round) ...
        pop.sample(seed, 0)
        k, best = members, []
        for r in range(rounds):
            for plan in plans:
                plan.solve_population(pop, 25, 3e-8, first=0, count=k)
            pop.eval_device()
            pop.sort(want_order=False)
            best.append(pop.best()[1])
            if redraw:
                pop.sample(seed, r + 1, first=members // 2)
            else:
                k = max(1, k // 2)
        # ... and the loop as it is meant: enqueued as a whole, the host far ahead of the device when it returns
        t = time.perf_counter()
        halving(plans, pop, members, rounds, seed, redraw)
        enqueued = time.perf_counter() - t
        x = g.get_x()                                                  # the final read: the one wait
        done = time.perf_counter() - t
        b, fb = pop.best()
        what = "the worse half redrawn each round" if redraw else "the worse half dropped each round (%s members solved)" % \
            ", ".join(str(max(1, members >> r)) for r in range(rounds))
        print(f"{members} members drawn on the device, {rounds} rounds, {what}")
        print("  best value per round: " + ", ".join(f"{v:.6f}" for v in best) + f"   (x0 itself: {f0:.6f})")
        print(f"  enqueued in {enqueued * 1e3:.2f} ms, result read after {done * 1e3:.2f} ms: "
              f"{'nothing but the final read waited' if enqueued < 0.5 * done else 'THE LOOP WAITED for the device'}")
        print(f"  the problem is left at member {b} of the last order, f = {fb:.6f}; its x is that row: {x.tobytes() == pop.get_x(0).tobytes()}")
        if not (b == 0 and x.tobytes() == pop.get_x(0).tobytes() and fb == g.eval()):
            sys.exit("the problem was not left at the best member")
        pop.close()


if __name__ == "__main__":
    main()
