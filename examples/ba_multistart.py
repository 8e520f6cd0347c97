#!/usr/bin/env python3
"""optBA's sample loop (reference src/bundleadjust/optBA.cpp:198-224) on ladybug 5 cameras / 30 points, on the device:
256 starts drawn uniformly from the variables' sampling intervals (BundleAdjustmentFunction.cpp:402-477: rotations in
[-pi, pi], translations, points and the focal length within 100 of their initial value, k1 within 1e-4, k2 within 1e-6),
every one of them solved by CGD (SSmaxit 25) -- in ONE call of the multi-start entry, and one by one for comparison.

  python examples/ba_multistart.py [nstarts] [seed]"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdis_amd import capi, problems as P  # noqa: E402


def sampling_intervals(pp):
    nc = int(pp.meta["ncams"])
    typ = np.concatenate([np.arange(9 * nc) % 9, 9 + np.arange(pp.nvars - 9 * nc) % 3])
    half = np.select([typ < 3, typ == 7, typ == 8], [math.pi, 1e-4, 1e-6], default=100.0)
    centre = np.where(typ < 3, 0.0, pp.x0)
    return centre - half, centre + half


def main():
    nstarts = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    pp = P.load_bal(ncams=5, npts=30).single_component()
    lo, hi = sampling_intervals(pp)
    starts = np.random.default_rng(seed).uniform(lo, hi, size=(nstarts, pp.nvars))

    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plan = capi.Plan(g)
    plan.set_start(pp.x0); plan.solve(25, 3e-8); plan.fetch()          # (tables, first launch)

    t = time.perf_counter()
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    together = time.perf_counter() - t
    kernel_ms, launches = plan.last_kernel_ms()

    t = time.perf_counter()
    one_by_one = np.empty(nstarts)
    for s in range(nstarts):
        plan.set_start(starts[s])
        plan.solve(25, 3e-8)
        one_by_one[s] = plan.fetch().fret[0]
    sequential = time.perf_counter() - t

    f = ms.fret[:, 0]
    ok = np.isfinite(f)
    q = np.quantile(f[ok], [0.25, 0.5, 0.75])
    print(f"{nstarts} starts from the sampling intervals, 25 CG iterations each ({int(np.sum(~ok))} not finite)")
    print(f"best f = {np.min(f[ok]):.6f} (start {int(ms.best[0])}); quartiles {q[0]:.4g} / {q[1]:.4g} / {q[2]:.4g}")
    print(f"one call : {together * 1e3:8.2f} ms  ({launches} launch(es), {kernel_ms:.2f} ms on the device)")
    print(f"one by one: {sequential * 1e3:8.2f} ms  -> {sequential / together:.1f} x; the same bits: {one_by_one.tobytes() == f.tobytes()}")
    print(f"the problem is left at the best start's result: f = {g.eval():.6f}")


if __name__ == "__main__":
    main()
