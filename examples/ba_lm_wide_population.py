#!/usr/bin/env python3
"""A population of restarts with one joint Levenberg-Marquardt solve each: ladybug 49 cameras / 300 points as ONE component of
49 camera blocks -- the wide class of the batched solver (LmPlan(..., wide=True): 17 to 64 cameras, one workgroup a member,
the reduced system of 441 unknowns in the member's workspace) -- on `members` states drawn on the device from the sampling
intervals.  One solve_population call, one launch for all members, then the members' values (eval_device) and the best member
assigned to the problem.  Residual model 2.  Nothing travels between host and device from the solve to the final read; the
script exits with an error if the calls took as long to enqueue as the result took to arrive (one of them waited for the
device), if the solve was split into more than one launch, or if the problem is not left at the best member.
(examples/ba_lm_population.py alternates camera and point plans on small blocks instead.)

  python examples/ba_lm_wide_population.py [members] [iterations] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rdis_amd import capi, problems as P  # noqa: E402
from ba_multistart import sampling_intervals  # noqa: E402


def joint_solve(plan, pop, iters):
    """nothing in it waits for the device"""
    plan.solve_population(pop, maxiters=iters)
    pop.eval_device()
    pop.assign_best()


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0x5D15
    pp = P.load_bal(ncams=49, npts=300)
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    whole = (np.array([0, pp.nvars], dtype=np.int64), np.arange(pp.nvars, dtype=np.int64),
             np.array([0, pp.nfac], dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))
    plan = capi.LmPlan(g, *whole, model=2, history=1, wide=True)
    f0 = g.eval()

    def draw():
        pop.sample(seed, 0)
        pop.set_x(pp.x0, first=0, count=1)                   # member 0: the problem's own start

    pop = capi.Population(g, nmembers=members)
    pop.set_sampling(*sampling_intervals(pp))
    draw()
    start = pop.eval()
    joint_solve(plan, pop, iters)                            # (first launch, buffers)
    ctx.synchronize()
    draw()
    t = time.perf_counter()
    joint_solve(plan, pop, iters)
    enqueued = time.perf_counter() - t
    x = g.get_x()                                            # the final read: the one wait
    done = time.perf_counter() - t
    b, fb = pop.best()
    f = pop.eval()
    launches, per = plan.info("launches"), plan.info("members_per_launch")
    print(f"{members} members, one joint solve each of {pp.nvars} unknowns ({pp.meta['ncams']} cameras, {pp.nfac} factors, at most {iters} iterations): "
          f"{launches} launch(es) of {per} members, {plan.info('member_workspace_bytes')} bytes of workspace a member")
    print(f"  values at the start: best {np.nanmin(start):.6f}, median {np.nanmedian(start):.6f}   (x0 itself: {f0:.6f})")
    print(f"  values at the end:   best {np.nanmin(f):.6f}, median {np.nanmedian(f):.6f}; {int(np.sum(f < start))} of {members} members improved")
    print(f"  enqueued in {enqueued * 1e3:.2f} ms, result read after {done * 1e3:.2f} ms: "
          f"{'nothing but the final read waited' if enqueued < 0.5 * done else 'THE CALLS WAITED for the device'}")
    print(f"  the problem is left at member {b}, f = {fb:.6f}")
    if launches != 1:
        sys.exit("the solve was split into %d launches" % launches)
    if not enqueued < 0.5 * done:
        sys.exit("a call waited for the device")
    if not (x.tobytes() == pop.get_x(b).tobytes() and fb == g.eval() == np.nanmin(f)):
        sys.exit("the problem was not left at the best member")


if __name__ == "__main__":
    main()
