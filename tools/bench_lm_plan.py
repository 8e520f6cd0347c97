#!/usr/bin/env python3
"""rdis_hip_lm_plan measured against the same work done with rdis_hip_lm_batch calls (the yardstick: it checks its lists,
builds and uploads its tables, downloads and waits in every call).

  python tools/bench_lm_plan.py [--repeats 5] [--case a|b|c] [--members 256]

  a  full ladybug, 5 rounds of the camera / point alternation, 5 iterations a half-round, model 2: two plans, ten solves
     enqueued, one wait at the end -- against ten lm_batch calls
  b  full ladybug, the point plan alone (7776 components): one solve and a wait -- against one lm_batch call
  c  ladybug 5 cameras / 30 points, a population of `--members` perturbed starts, one alternation round: two
     solve_population calls and a wait -- against a loop over the members of set_x and two lm_batch calls

Both ways are timed at the C ABI (ctypes calls, arrays allocated beforehand, no history, the start re-assigned outside the
timed window): a host clock around work that ends synchronised.  One warm-up of each way, then `--repeats` rounds that
alternate the two ways; the best and the median of each are printed, one JSON line per case, with the objective both ways
end at and whether they agree to 1e-9; if they do not, the tool stops there with an error."""
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


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def lists_of(g, pp, ncams):
    """(camera lists, point lists): the components left with the points / the cameras constant"""
    out = []
    for fixed in (slice(9 * ncams, None), slice(0, 9 * ncams)):
        assigned = np.zeros(pp.nvars, dtype=np.uint8)
        assigned[fixed] = 1
        out.append(g.components(assigned))
    return out


def batch_call(g, lists, iters, model):
    fp, fv, jp, fj = lists
    nc = len(fp) - 1
    lib, check = g.ctx.lib, g.ctx.check

    def run():
        check(lib.rdis_hip_lm_batch(g.h, nc, _p(fp), _p(fv), _p(jp), _p(fj), None, iters, 3e-8, model, None, None, None, None, 0, None))
    return run


def measure(name, what, ways, reset, end, repeats, extra):
    """ways: {label: run}; reset(): the start re-assigned (not timed); end(label): the objective a way ended at (not timed);
    extra(): further fields of the record, asked after the runs"""
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
    a, b = (ends[k] for k in ("plan", "batch"))
    rec["ends_agree"] = bool(abs(a - b) <= 1e-9 * abs(b))
    rec["batch_over_plan"] = round(rec["batch_ms_best"] / rec["plan_ms_best"], 2)
    rec.update(extra())
    print(json.dumps(rec), flush=True)
    if not rec["ends_agree"]:
        sys.exit("case %s: the two ways ended at different objectives (%r, %r)" % (name, a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--case", default="abc")
    ap.add_argument("--members", type=int, default=256)
    a = ap.parse_args()
    ctx = capi.Context(0)
    lib, check = ctx.lib, ctx.check
    if "a" in a.case or "b" in a.case:
        pp = P.load_bal()
        ncams = pp.meta["ncams"]
        g = capi.Problem(ctx, pp)
        cams, pts = lists_of(g, pp, ncams)
        pc, pq = capi.LmPlan(g, *cams, model=2, history=0), capi.LmPlan(g, *pts, model=2, history=0)
        bc, bq = batch_call(g, cams, 5, 2), batch_call(g, pts, 5, 2)
        sizes = {"camera_plan_member_workspace_bytes": pc.info("member_workspace_bytes"), "point_plan_member_workspace_bytes": pq.info("member_workspace_bytes")}
        for k in list(sizes):
            sizes[k.replace("member_workspace_bytes", "members_per_launch_1GiB")] = min((1 << 30) // sizes[k], 65535)

        def plan_rounds():
            for _ in range(5):
                check(lib.rdis_hip_lm_plan_solve(pc.h, 5, 3e-8))
                check(lib.rdis_hip_lm_plan_solve(pq.h, 5, 3e-8))
            check(lib.rdis_hip_synchronize(ctx.h))

        def batch_rounds():
            for _ in range(5):
                bc()
                bq()

        def plan_points():
            check(lib.rdis_hip_lm_plan_solve(pq.h, 5, 3e-8))
            check(lib.rdis_hip_synchronize(ctx.h))

        if "a" in a.case:
            measure("a", "full ladybug, 5 alternation rounds (49 camera / 7776 point components), model 2, 5 iterations a half-round",
                    {"plan": plan_rounds, "batch": batch_rounds}, lambda: g.set_x(pp.x0), lambda k: g.eval(), a.repeats, lambda: sizes)
        if "b" in a.case:
            measure("b", "full ladybug, the point plan alone (7776 components), model 2, 5 iterations",
                    {"plan": plan_points, "batch": bq}, lambda: g.set_x(pp.x0), lambda k: g.eval(), a.repeats, dict)
    if "c" in a.case:
        pp = P.load_bal(ncams=5, npts=30)
        g = capi.Problem(ctx, pp)
        cams, pts = lists_of(g, pp, 5)
        S_n = a.members
        rng = np.random.default_rng(2000)
        X = np.clip(pp.x0 + 1e-3 * (1.0 + np.abs(pp.x0)) * rng.standard_normal((S_n, pp.nvars)), pp.lo, pp.hi)
        X[0] = pp.x0
        pop = capi.Population(g, x=X)
        pc, pq = capi.LmPlan(g, *cams, model=2, history=0), capi.LmPlan(g, *pts, model=2, history=0)
        bc, bq = batch_call(g, cams, 5, 2), batch_call(g, pts, 5, 2)
        finals = np.zeros((S_n, pp.nvars))        # the loop's results, kept for the comparison of the ends (warm-up only)
        keep = [False]

        def plan_round():
            check(lib.rdis_hip_lm_plan_solve_population(pc.h, pop.h, 0, S_n, 5, 3e-8))
            check(lib.rdis_hip_lm_plan_solve_population(pq.h, pop.h, 0, S_n, 5, 3e-8))
            check(lib.rdis_hip_synchronize(ctx.h))

        def batch_loop():
            for s in range(S_n):
                check(lib.rdis_hip_set_x(g.h, pp.nvars, None, _p(X[s])))
                bc()
                bq()
                if keep[0]:
                    finals[s] = g.get_x()

        def end(k):
            if k == "plan":
                return float(np.sum(pop.eval()))
            keep[0] = True
            batch_loop()
            keep[0] = False
            return float(np.sum(capi.Population(g, x=finals).eval()))

        measure("c", "ladybug 5/30, %d members, one alternation round (5 camera / 30 point components), model 2, 5 iterations a half-round" % S_n,
                {"plan": plan_round, "batch": batch_loop}, lambda: pop.set_x(X), end, a.repeats,
                lambda: {"members_per_launch": pq.info("members_per_launch"), "launches_a_half_round": pq.info("launches")})


if __name__ == "__main__":
    main()
