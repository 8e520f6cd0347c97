#!/usr/bin/env python3
"""The wide class of rdis_hip_lm_batch / rdis_hip_lm_plan (RDIS_HIP_LM_WIDE: components of 17 to 64 cameras, one workgroup
each) measured against rdis_hip_lm_optimize, the host-driven solver such components went to before (the yardstick: it is
not touched by the wide class), with the same iteration limit.

  python tools/bench_lm_wide.py [--repeats 5] [--case a|b|c] [--members 64] [--iters 6]

  a  ladybug 49 cameras / 300 points as one component: one wide lm_batch call -- against one lm_optimize call
  b  full ladybug (49 cameras, 7776 points, 31843 factors) as one wide component: the same pair
  c  `--members` perturbed starts of ladybug 49 / 300: one solve_population of a wide plan and a wait -- against the loop over
     the members of set_x and lm_optimize

Both ways are timed at the C ABI (ctypes calls, arrays allocated beforehand, no history, the start re-assigned outside the
timed window): a host clock around work that ends synchronised.  One warm-up of each way, then `--repeats` rounds that
alternate the two ways; the best and the median of each are printed, one JSON line per case, with the objective both ways
end at and whether they agree to 1e-9; if they do not, the tool stops there with an error.  Model 2."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rdis_amd import capi, problems as P  # noqa: E402

MODEL = 2


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def whole(pp):
    return (np.array([0, pp.nvars], dtype=np.int64), np.arange(pp.nvars, dtype=np.int64),
            np.array([0, pp.nfac], dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))


def measure(name, what, ways, reset, end, repeats, extra):
    """ways: {label: run}; reset(): the start re-assigned (not timed); end(label): the objective a way ended at (not timed)"""
    ends, ms = {}, {k: [] for k in ways}
    for k, run in ways.items():      # warm-up: code objects, workspaces
        reset()
        run()
        ends[k] = end(k)
    for _ in range(repeats):
        for k, run in ways.items():
            reset()
            t = time.perf_counter()
            run()
            ms[k].append((time.perf_counter() - t) * 1e3)
    rec = {"case": name, "what": what, "repeats": repeats}
    for k in ways:
        rec[k + "_ms_best"] = round(min(ms[k]), 4)
        rec[k + "_ms_median"] = round(float(np.median(ms[k])), 4)
        rec[k + "_end"] = ends[k]
    a, b = (ends[k] for k in ("wide", "optimize"))
    rec["ends_agree"] = bool(abs(a - b) <= 1e-9 * abs(b))
    rec["optimize_over_wide"] = round(rec["optimize_ms_best"] / rec["wide_ms_best"], 3)
    rec.update(extra())
    print(json.dumps(rec), flush=True)
    if not rec["ends_agree"]:
        sys.exit("case %s: the two ways ended at different objectives (%r, %r)" % (name, a, b))


def single_pair(ctx, pp, iters):
    """(problem, {way: run}) for one component that is the whole problem"""
    g = capi.Problem(ctx, pp)
    lib, check = ctx.lib, ctx.check
    fp, fv, jp, fj = lists = whole(pp)
    out = np.zeros(2)

    def wide():
        check(lib.rdis_hip_lm_batch(g.h, 1, _p(fp), _p(fv), _p(jp), _p(fj), None, iters, 3e-8, MODEL | capi.LM_WIDE, None, None, None, None, 0, None))

    def optimize():
        check(lib.rdis_hip_lm_optimize(g.h, pp.nvars, _p(fv), pp.nfac, _p(fj), None, iters, 3e-8, MODEL, _p(out), None, None, None, 0, None))
    return g, lists, {"wide": wide, "optimize": optimize}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--case", default="abc")
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--iters", type=int, default=6)
    a = ap.parse_args()
    ctx = capi.Context(0)
    lib, check = ctx.lib, ctx.check
    for case, pp, what in (("a", lambda: P.load_bal(ncams=49, npts=300), "ladybug 49/300 as one component"),
                           ("b", P.load_bal, "full ladybug as one component")):
        if case not in a.case:
            continue
        pp = pp()
        g, _, ways = single_pair(ctx, pp, a.iters)
        measure(case, "%s (%d factors), model %d, %d iterations" % (what, pp.nfac, MODEL, a.iters), ways,
                lambda: g.set_x(pp.x0), lambda k: g.eval(), a.repeats, dict)
    if "c" in a.case:
        pp = P.load_bal(ncams=49, npts=300)
        g, lists, ways = single_pair(ctx, pp, a.iters)
        S_n = a.members
        rng = np.random.default_rng(2000)
        X = np.clip(pp.x0 + 1e-3 * (1.0 + np.abs(pp.x0)) * rng.standard_normal((S_n, pp.nvars)), pp.lo, pp.hi)
        X[0] = pp.x0
        pop = capi.Population(g, x=X)
        plan = capi.LmPlan(g, *lists, model=MODEL, history=0, wide=True)
        finals = np.zeros((S_n, pp.nvars))        # the loop's results, kept for the comparison of the ends (warm-up only)
        keep = [False]

        def wide_population():
            check(lib.rdis_hip_lm_plan_solve_population(plan.h, pop.h, 0, S_n, a.iters, 3e-8))
            check(lib.rdis_hip_synchronize(ctx.h))

        def optimize_loop():
            for s in range(S_n):
                check(lib.rdis_hip_set_x(g.h, pp.nvars, None, _p(X[s])))
                ways["optimize"]()
                if keep[0]:
                    finals[s] = g.get_x()

        def end(k):
            if k == "wide":
                return float(np.sum(pop.eval()))
            keep[0] = True
            optimize_loop()
            keep[0] = False
            return float(np.sum(capi.Population(g, x=finals).eval()))

        measure("c", "ladybug 49/300, %d members, one joint solve each, model %d, %d iterations" % (S_n, MODEL, a.iters),
                {"wide": wide_population, "optimize": optimize_loop}, lambda: pop.set_x(X), end, a.repeats,
                lambda: {"members_per_launch": plan.info("members_per_launch"), "launches": plan.info("launches"),
                         "member_workspace_bytes": plan.info("member_workspace_bytes")})


if __name__ == "__main__":
    main()
