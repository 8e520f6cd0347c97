#!/usr/bin/env python3
"""rdis_hip_lm_plan_solve_starts measured against the loop it replaces: per start set_x + rdis_hip_lm_plan_solve +
rdis_hip_lm_plan_fetch (a wait and two copies a start), the ranking on the host, and set_x of the winners.

  python tools/bench_lm_starts.py [--repeats 5] [--case a|b|c]

  a  ladybug 5 cameras / 30 points, the point plan (30 components), 64 starts
  b  ladybug 5 cameras / 30 points, the camera plan (5 components), 64 starts
  c  full ladybug, the point plan (7776 components), 16 starts

Model 2, 5 iterations, no history.  The starts move every free variable by 1e-3 of its size (row 0: the problem's start).  The
method is tools/bench_lm_plan.py's: both ways timed at the C ABI (ctypes calls, arrays allocated beforehand, the start
re-assigned outside the timed window), a host clock around work that ends synchronised -- the one call ends with
rdis_hip_synchronize, the loop with its last set_x and a synchronize.  One warm-up of each way, then `--repeats` rounds that
alternate the two ways; the best and the median of each are printed, one JSON line per case, with the objective both ways end at;
if the two differ in a bit, or the winners differ, the tool stops there with an error."""
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


def select(fret):
    """the library's rule on fret[nstarts, ncomp] without NaNs: the lowest value, the lowest index on a tie"""
    return np.argmin(fret, axis=0)


def case(ctx, name, what, pp, lists, nstarts, repeats):
    lib, check = ctx.lib, ctx.check
    g = capi.Problem(ctx, pp)
    fp, fv = lists[0], lists[1]
    nc, nfree = len(fp) - 1, len(fv)
    plan = capi.LmPlan(g, *lists, model=2, history=0)
    rng = np.random.default_rng(3000)
    starts = pp.x0[fv] + 1e-3 * (1.0 + np.abs(pp.x0[fv])) * rng.standard_normal((nstarts, nfree))
    starts = np.ascontiguousarray(np.clip(starts, pp.lo[fv], pp.hi[fv]))
    starts[0] = pp.x0[fv]
    xs, fret, win = np.zeros((nstarts, nfree)), np.zeros((nstarts, nc)), np.zeros(nfree)
    comp_of, cols = np.repeat(np.arange(nc), np.diff(fp)), np.arange(nfree)
    best = {"starts": np.zeros(nc, dtype=np.int32), "loop": None}

    def one_call():
        check(lib.rdis_hip_lm_plan_solve_starts(plan.h, nstarts, _p(starts), 5, 3e-8))
        check(lib.rdis_hip_synchronize(ctx.h))

    def loop():
        for s in range(nstarts):
            check(lib.rdis_hip_set_x(g.h, nfree, _p(fv), _p(starts[s])))
            check(lib.rdis_hip_lm_plan_solve(plan.h, 5, 3e-8))
            check(lib.rdis_hip_lm_plan_fetch(plan.h, _p(xs[s]), _p(fret[s]), None, None, None, None))
        b = select(fret)
        win[:] = xs[b[comp_of], cols]
        check(lib.rdis_hip_set_x(g.h, nfree, _p(fv), _p(win)))
        check(lib.rdis_hip_synchronize(ctx.h))
        best["loop"] = b

    ways = {"starts": one_call, "loop": loop}
    ends, ms = {}, {k: [] for k in ways}
    for k, run in ways.items():
        g.set_x(pp.x0)
        run()
        ends[k] = g.eval()
    check(lib.rdis_hip_lm_plan_solve_starts(plan.h, nstarts, _p(starts), 5, 3e-8))
    check(lib.rdis_hip_lm_plan_fetch_starts(plan.h, None, None, None, None, None, None, _p(best["starts"])))
    info = {"members_per_launch": plan.info("members_per_launch"), "launches": plan.info("launches"), "device_bytes": plan.info("device_bytes")}
    for _ in range(repeats):
        for k, run in ways.items():
            g.set_x(pp.x0)
            t = time.perf_counter()
            run()
            ms[k].append((time.perf_counter() - t) * 1e3)
    rec = {"case": name, "what": what, "starts": nstarts, "components": nc, "repeats": repeats}
    for k in ways:
        rec[k + "_ms_best"] = round(min(ms[k]), 4)
        rec[k + "_ms_median"] = round(float(np.median(ms[k])), 4)
        rec[k + "_end"] = ends[k]
    rec["same_winners"] = bool(np.array_equal(best["starts"], best["loop"]))
    rec["ends_equal"] = bool(ends["starts"] == ends["loop"])
    rec["distinct_winners"] = int(len(set(best["starts"].tolist())))
    rec["loop_over_starts"] = round(rec["loop_ms_best"] / rec["starts_ms_best"], 2)
    rec.update(info)
    print(json.dumps(rec), flush=True)
    if not (rec["same_winners"] and rec["ends_equal"]):
        sys.exit("case %s: the two ways ended differently (%r, %r)" % (name, ends["starts"], ends["loop"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--case", default="abc")
    a = ap.parse_args()
    ctx = capi.Context(0)
    if "a" in a.case or "b" in a.case:
        pp = P.load_bal(ncams=5, npts=30)
        cams, pts = lists_of(capi.Problem(ctx, pp), pp, 5)
        if "a" in a.case:
            case(ctx, "a", "ladybug 5/30, the point plan (30 components), 64 starts, model 2, 5 iterations", pp, pts, 64, a.repeats)
        if "b" in a.case:
            case(ctx, "b", "ladybug 5/30, the camera plan (5 components), 64 starts, model 2, 5 iterations", pp, cams, 64, a.repeats)
    if "c" in a.case:
        pp = P.load_bal()
        cams, pts = lists_of(capi.Problem(ctx, pp), pp, pp.meta["ncams"])
        case(ctx, "c", "full ladybug, the point plan (7776 components), 16 starts, model 2, 5 iterations", pp, pts, 16, a.repeats)


if __name__ == "__main__":
    main()
