#!/usr/bin/env python3
"""Multi-start solves measured: rdis_hip_plan_solve_starts against the same starts solved one by one.

  python tools/bench_multistart.py            # both steps, one JSON line
  python tools/bench_multistart.py --step config3|config5s|config2|population|population-nlp|population-tiny|population-eval|population-point-major|population-halving|population-grad   # one step, in this process

config3   BASELINE config 3 (ladybug 5 cameras / 30 points, one component): 320 one-ulp starts -- those of the end-value fixture,
          tests/golden/end_values.json -- in one call, and the same 320 by set_start / solve / fetch on the same plan.
config5s  BASELINE config 5-S (1000 components of 3 cameras x 40 points) x 8 starts, likewise.
config2   BASELINE config 2 (the 121-variable sinusoid, one component on the plain solver: one workgroup of 512 lanes a solve) from
          1024 starts drawn uniformly in the domains (seed 2), likewise.
population  ladybug 5 / 30, 256 members drawn from the sampling intervals (examples/ba_multistart.py), one alternation round -- camera
          plan, then point plan -- as two population launches (rdis_hip_plan_solve_population), against the same round member by
          member through set_x / set_start(None) / solve / get_x on the problem: the baseline is the way without populations.
population-nlp  the 121-variable sinusoid, 256 members drawn uniformly in the domains (seed 0), one round -- the root plan (variable 0
          free), then the three-subtree plan (the root constant: 3 x 40 variables, 3 x 120 factors) -- as two population launches on the
          plain solver (plan option population_plain; the subtree launch is 768 workgroups of 128 lanes), against the same round member
          by member through set_x / set_start(None) / solve / get_x.
population-tiny  full ladybug, 64 members drawn from the sampling intervals, the POINT plan only (7776 components of three variables),
          after one camera step on the population so that the members' cameras differ: (a) on the tiny-component solver (plan option
          population_tiny), sixteen lanes a point; (b) the same with four lanes (quad_min_components = 1); (c) the way before that
          option: row_min_components = 1 << 40, a 64-lane workgroup of the LDS-resident solver per point and member; (d) member by member
          through set_x / set_start(None) / solve / get_x.  (a) again with 2 and 4 times the resident blocks (tiny_population_fill).
population-eval  the step that closes a round: 256 members of ladybug 5 / 30 and 64 members of full ladybug from the sampling intervals,
          after one camera step on the population so that the members' cameras differ.  (a) the wall time of rdis_hip_population_eval
          with the population option eval_batched = 1 (the member a grid dimension: two or three launches) against eval_batched = 0
          (member by member, two or three launches each: the path before that option), and of one member's rdis_hip_eval; (b) one
          round -- camera plan, point plan -- ending in eval_device + assign_best + best() against the round ending in eval()
          (eval_batched = 0) + the host's argmin + assign(); whether the bytes of f, the member chosen and the problem's x agree.
population-point-major  full ladybug as ONE component (what optBA's sample loop runs per sample when it calls CGD on everything) on the
          point-major streaming solver, one workgroup of 768 lanes a member (plan options population_point_major = 1, ptm_group = 1):
          64 and 256 members from the sampling intervals, 25 iterations, one population launch each, against the same members one by
          one through set_x / set_start(None) / solve / get_x; last_kernel_ms of the population launch in units of one ordinary
          solve's (cgd_ptm_kernel, whose code and registers are the parent commit's); whether both routes left the same bytes.
          Not part of the run without --step (it is asked for by name).
population-halving  ladybug 5 / 30, 256 members DRAWN ON THE DEVICE from the sampling intervals (rdis_hip_population_sample), four rounds of
          camera plan + point plan on the members 0 .. k-1, evaluation, ranking, k //= 2 (256, 128, 64, 32 members solved): (a) through
          rdis_hip_plan_solve_population_range / _population_eval_device / _population_sort, one read at the end; (b) the same halving
          the way before those entries: eval, the host's sort by the same rule, get_x of the survivors, a new population from them;
          (c) all 256 members in all four rounds (context).  The ways alternate within the job.  Wall time and summed kernel ms of each,
          whether (a) and (b) end with the same order and the same bytes in the surviving rows, the best value of (a) and (c).  Then the
          wall time of sort alone (between two synchronisations) at 256, 4096 and 65535 members, and of sample of 256 whole members of
          full ladybug against the host's draw + set_x of the same 48.7 MB.  Asked for by name, like population-point-major.
population-grad  the members' gradients: 256 members of ladybug 5 / 30 and 64 members of full ladybug from the sampling intervals, after one
          camera step.  The wall time of rdis_hip_population_eval_grad_device + one synchronisation (the member a grid dimension: three
          or four launches), of the member-by-member route -- population_assign(s) + rdis_hip_eval_grad_device for every s, then one
          synchronisation: code the batched path does not touch -- and of one member's rdis_hip_eval_grad_device; the launches; whether
          f and g have the same bytes both ways.  Asked for by name, like population-point-major.
Every step runs in a child process under a time limit of its own; a step that fails ends the run.  Wall times are the median of
`--repeats` calls after one warm-up call; kernel_ms is rdis_hip_plan_last_kernel_ms of the last call."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = {"config3": 240, "config5s": 240, "config2": 240, "population": 240, "population-nlp": 240, "population-tiny": 240, "population-eval": 240,
                "population-point-major": 420, "population-halving": 420, "population-grad": 240}
STEPS = ("config3", "config5s", "config2", "population", "population-nlp", "population-tiny", "population-eval")


def ulp_perturbed(x0, rng):
    return np.nextafter(x0, np.where(rng.random(x0.shape) < 0.5, -np.inf, np.inf))


def measure(pp, starts, repeats):
    from rdis_amd import capi
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plan = capi.Plan(g)
    ns = starts.shape[0]

    def together():
        t = time.perf_counter()
        plan.solve_starts(starts, 25, 3e-8)
        r = plan.fetch_starts()
        return time.perf_counter() - t, r

    def one_by_one():
        t = time.perf_counter()
        fret, x = [], []
        for row in starts:
            plan.set_start(row)
            plan.solve(25, 3e-8)
            r = plan.fetch()
            fret.append(r.fret.copy()); x.append(r.x.copy())
        return time.perf_counter() - t, np.array(fret), np.array(x)

    plan.set_start(starts[0]); plan.solve(25, 3e-8); plan.fetch()
    single_ms = plan.last_kernel_ms()[0]
    together()
    tt = []
    for _ in range(repeats):
        dt, ms = together()
        tt.append(dt)
    kernel_ms, launches = plan.last_kernel_ms()
    one_by_one()
    ts = []
    for _ in range(repeats):
        dt, fret, x = one_by_one()
        ts.append(dt)
    same = bool(fret.tobytes() == ms.fret.tobytes() and x.tobytes() == ms.x.tobytes())
    wall, seq = float(np.median(tt)), float(np.median(ts))
    return {"starts": ns, "components": plan.ncomp, "components_lds": plan.info("components_lds"),
            "components_plain": plan.info("components_plain"),
            "starts_per_launch": plan.info("starts_per_launch"), "launches": launches,
            "wall_ms": 1e3 * wall, "sequential_wall_ms": 1e3 * seq, "speedup": seq / wall,
            "last_kernel_ms": kernel_ms, "one_solve_kernel_ms": single_ms, "kernel_in_single_solves": kernel_ms / single_ms,
            "starts_per_second": ns / wall, "sequential_starts_per_second": ns / seq, "bits_equal_sequential": same,
            "best_fret_sum": float(np.sum(np.min(ms.fret, axis=0))),
            "device_bytes": plan.device_bytes()}


def measure_population(repeats, members=256):
    """one alternation round on a population against the same round member by member on the problem"""
    from rdis_amd import capi, problems as P
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from ba_multistart import sampling_intervals
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    lo, hi = sampling_intervals(pp)
    X = np.random.default_rng(0).uniform(lo, hi, size=(members, pp.nvars))
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
    assert all(p.info("components_lds") == p.ncomp for p in plans)
    pop = capi.Population(g, members)

    def together():
        pop.set_x(X)
        t = time.perf_counter()
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8)
        ctx.synchronize()
        return time.perf_counter() - t, pop.get_x()

    def kernel_times():   # (the problem's timing events belong to its last solve: read after each launch, outside the timed round)
        pop.set_x(X)
        out = []
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8)
            out.append(plan.last_kernel_ms())
        return [ms for ms, _ in out], sum(n for _, n in out)

    def one_by_one():
        out = np.empty_like(X)
        t = time.perf_counter()
        for s in range(members):
            g.set_x(X[s])
            for plan in plans:
                plan.set_start(None)
                plan.solve(25, 3e-8)
            out[s] = g.get_x()
        return time.perf_counter() - t, out

    g.set_x(X[0]); plans[1].set_start(None); plans[1].solve(25, 3e-8); plans[1].fetch()
    single_ms = plans[1].last_kernel_ms()[0]
    together()
    tt = []
    for _ in range(repeats):
        dt, xt = together()
        tt.append(dt)
    kernel_ms, launches = kernel_times()
    one_by_one()
    ts = []
    for _ in range(repeats):
        dt, xs = one_by_one()
        ts.append(dt)
    f = pop.eval()
    wall, seq = float(np.median(tt)), float(np.median(ts))
    return {"members": members, "camera_components": plans[0].ncomp, "point_components": plans[1].ncomp,
            "members_per_launch": plans[1].info("starts_per_launch"), "launches_per_round": 2,
            "wall_ms": 1e3 * wall, "sequential_wall_ms": 1e3 * seq, "speedup": seq / wall,
            "last_kernel_ms": kernel_ms, "last_kernel_launches": launches, "one_member_point_solve_kernel_ms": single_ms,
            "point_kernel_in_single_solves": kernel_ms[1] / single_ms,
            "bits_equal_sequential": bool(xt.tobytes() == xs.tobytes()), "finite_members": int(np.sum(np.isfinite(f))),
            "best_f": float(np.nanmin(f)) if np.any(np.isfinite(f)) else None,
            "device_bytes": [p.device_bytes() for p in plans]}


def measure_population_nlp(repeats, members=256):
    """one root / subtrees round of the sinusoid on a population (plain solver) against the same round member by member"""
    from rdis_amd import capi, problems as P
    pp = P.make_high_dim_sinusoid()
    X = np.random.default_rng(0).uniform(pp.lo, pp.hi, size=(members, pp.nvars))
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    only_root = np.ones(pp.nvars, np.uint8)
    only_root[0] = 0
    plans = [capi.Plan(g, *g.components(only_root)), capi.Plan(g, *g.components(1 - only_root))]
    for plan in plans:
        plan.set_option("population_plain", 1)
    assert plans[0].nfree == 1 and plans[1].ncomp == 3 and all(p.info("components_plain") == p.ncomp for p in plans)
    pop = capi.Population(g, members)

    def together():
        pop.set_x(X)
        t = time.perf_counter()
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8)
        ctx.synchronize()
        return time.perf_counter() - t, pop.get_x()

    def kernel_times():   # (the problem's timing events belong to its last solve: read after each launch, outside the timed round)
        pop.set_x(X)
        out = []
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8)
            out.append(plan.last_kernel_ms())
        return [ms for ms, _ in out], sum(n for _, n in out)

    def one_by_one():
        out = np.empty_like(X)
        t = time.perf_counter()
        for s in range(members):
            g.set_x(X[s])
            for plan in plans:
                plan.set_start(None)
                plan.solve(25, 3e-8)
            out[s] = g.get_x()
        return time.perf_counter() - t, out

    # one member's subtree solve, the device time of its launch (three workgroups of 128 lanes): the median over a few members
    singles = []
    for s in range(min(members, 9)):
        g.set_x(X[s]); plans[1].set_start(None); plans[1].solve(25, 3e-8); plans[1].fetch()
        singles.append(plans[1].last_kernel_ms()[0])
    single_ms = float(np.median(singles[1:])) if len(singles) > 1 else singles[0]
    together()
    tt = []
    for _ in range(repeats):
        dt, xt = together()
        tt.append(dt)
    kernel_ms, launches = kernel_times()
    one_by_one()
    ts = []
    for _ in range(repeats):
        dt, xs = one_by_one()
        ts.append(dt)
    f = pop.eval()
    wall, seq = float(np.median(tt)), float(np.median(ts))
    return {"members": members, "root_components": plans[0].ncomp, "subtree_components": plans[1].ncomp,
            "subtree_workgroups": members * plans[1].ncomp,
            "members_per_launch": plans[1].info("starts_per_launch"), "launches_per_round": 2,
            "wall_ms": 1e3 * wall, "sequential_wall_ms": 1e3 * seq, "speedup": seq / wall,
            "last_kernel_ms": kernel_ms, "last_kernel_launches": launches, "one_member_subtree_solve_kernel_ms": single_ms,
            "subtree_kernel_in_single_solves": kernel_ms[1] / single_ms,
            "bits_equal_sequential": bool(xt.tobytes() == xs.tobytes()), "finite_members": int(np.sum(np.isfinite(f))),
            "best_f": float(np.nanmin(f)) if np.any(np.isfinite(f)) else None,
            "device_bytes": [p.device_bytes() for p in plans]}


def measure_population_tiny(repeats, members=64):
    """full ladybug's point plan on a population: the tiny-component solver (16 and 4 lanes) against a workgroup of the
    LDS-resident solver per point and against one member at a time"""
    from rdis_amd import capi, problems as P
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from ba_multistart import sampling_intervals
    pp = P.load_bal()
    cams, pts = P.ba_alternation_plans(pp)
    lo, hi = sampling_intervals(pp)
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    pop = capi.Population(g, x=np.random.default_rng(0).uniform(lo, hi, size=(members, pp.nvars)))
    plan_c = capi.Plan(g, *cams)
    for k in ("coop_min_factors", "coop_group_min_factors"):
        plan_c.set_option(k, 0)
    plan_c.solve_population(pop, 25, 3e-8)                 # one camera step: every member its own cameras
    X = pop.get_x()
    ways = {"tiny16": {"population_tiny": 1}, "tiny4": {"population_tiny": 1, "quad_min_components": 1},
            "lds_workgroup_per_point": {"row_min_components": 1 << 40},
            "tiny16_fill2": {"population_tiny": 1, "tiny_population_fill": 2}, "tiny16_fill4": {"population_tiny": 1, "tiny_population_fill": 4}}
    out = {"members": members, "point_components": len(pts[0]) - 1}
    rows = {}
    for name, opts in ways.items():
        plan = capi.Plan(g, *pts)
        for k, v in opts.items():
            plan.set_option(k, v)
        tt = []
        for it in range(repeats + 1):                      # (the first call is the warm-up)
            pop.set_x(X)
            t = time.perf_counter()
            plan.solve_population(pop, 25, 3e-8)
            ctx.synchronize()
            tt.append(time.perf_counter() - t)
        ms, launches = plan.last_kernel_ms()
        rows[name] = pop.get_x()
        out[name] = {"wall_ms": 1e3 * float(np.median(tt[1:])), "last_kernel_ms": ms, "launches": launches,
                     "components_tiny": plan.info("components_tiny"), "components_lds": plan.info("components_lds"),
                     "members_per_launch": plan.info("starts_per_launch"), "blocks_per_member": plan.info("population_tiny_blocks"),
                     "device_bytes": plan.device_bytes()}
        plan.close()
    plan = capi.Plan(g, *pts)

    def one_by_one():
        res = np.empty_like(X)
        t = time.perf_counter()
        for s in range(members):
            g.set_x(X[s])
            plan.set_start(None)
            plan.solve(25, 3e-8)
            res[s] = g.get_x()
        return time.perf_counter() - t, res

    one_by_one()
    ts = []
    for _ in range(repeats):
        dt, xs = one_by_one()
        ts.append(dt)
    out["member_by_member"] = {"wall_ms": 1e3 * float(np.median(ts)), "one_member_kernel_ms": plan.last_kernel_ms()[0],
                               "components_tiny": plan.info("components_tiny")}
    out["tiny16_bits_equal_member_by_member"] = bool(rows["tiny16"].tobytes() == xs.tobytes())
    out["fill_changes_no_bit"] = bool(rows["tiny16"].tobytes() == rows["tiny16_fill2"].tobytes() == rows["tiny16_fill4"].tobytes())
    base = out["lds_workgroup_per_point"]["last_kernel_ms"]
    out["kernel_speedup_over_lds_workgroups"] = {k: base / out[k]["last_kernel_ms"] for k in ways if k != "lds_workgroup_per_point"}
    return out


def measure_population_point_major(repeats, sizes=(64, 256)):
    """full ladybug as one component: S workgroups of the point-major solver in one launch against S ordinary solves"""
    from rdis_amd import capi, problems as P
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from ba_multistart import sampling_intervals
    pp = P.load_bal().single_component()
    lo, hi = sampling_intervals(pp)
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plan = capi.Plan(g)
    for k, v in {"coop_min_factors": 0, "coop_group_min_factors": 0, "ptm_stream": 2, "ptm_group": 1, "ptm_threads": 768,
                 "population_point_major": 1}.items():
        plan.set_option(k, v)
    Xall = np.random.default_rng(0).uniform(lo, hi, size=(max(sizes), pp.nvars))
    out = {"factors": int(pp.nfac), "variables": int(pp.nvars), "maxiters": 25}
    # the unit: one ordinary solve from x0 and from the first member (their iteration counts differ)
    unit = {}
    for name, x in (("x0", pp.x0), ("member_0", Xall[0])):
        kk = []
        for _ in range(repeats + 1):
            g.set_x(x)
            plan.set_start(None)
            plan.solve(25, 3e-8)
            r = plan.fetch()
            kk.append(plan.last_kernel_ms()[0])
        unit[name] = {"last_kernel_ms": float(np.median(kk[1:])), "nfeval": int(r.nfeval[0]), "iters": int(r.iters[0])}
    out["one_ordinary_solve"] = unit
    out["components_point_major"] = plan.info("components_point_major")
    out["point_major_threads"] = plan.info("point_major_threads")
    for members in sizes:
        X = Xall[:members]
        pop = capi.Population(g, x=X)
        tt, kk = [], []
        for _ in range(repeats + 1):                       # (the first call is the warm-up)
            pop.set_x(X)
            ctx.synchronize()
            t = time.perf_counter()
            plan.solve_population(pop, 25, 3e-8)
            ctx.synchronize()
            tt.append(time.perf_counter() - t)
            kk.append(plan.last_kernel_ms()[0])
        xt = pop.get_x()
        pr = plan.fetch_population(want_x=False)

        def one_by_one():
            res = np.empty_like(X)
            km = 0.0
            t = time.perf_counter()
            for s in range(members):
                g.set_x(X[s])
                plan.set_start(None)
                plan.solve(25, 3e-8)
                res[s] = g.get_x()
                km += plan.last_kernel_ms()[0]
            return time.perf_counter() - t, res, km

        one_by_one()
        ts, ks = [], []
        for _ in range(repeats):
            dt, xs, km = one_by_one()
            ts.append(dt)
            ks.append(km)
        kernel, seq_kernel = float(np.median(kk[1:])), float(np.median(ks))
        out["members_%d" % members] = {
            "wall_ms": 1e3 * float(np.median(tt[1:])), "last_kernel_ms": kernel, "launches": plan.last_kernel_ms()[1],
            "members_per_launch": plan.info("starts_per_launch"), "threads": plan.info("population_point_major_threads"),
            "sequential_wall_ms": 1e3 * float(np.median(ts)), "sequential_kernel_ms_summed": seq_kernel,
            "speedup_wall": float(np.median(ts)) / float(np.median(tt[1:])),
            "kernel_in_ordinary_solves_of_member_0": kernel / unit["member_0"]["last_kernel_ms"],
            "kernel_in_mean_member_solves": kernel / (seq_kernel / members),
            "nfeval_min_max": [int(pr.nfeval.min()), int(pr.nfeval.max())],
            "bits_equal_member_by_member": bool(xt.tobytes() == xs.tobytes()), "device_bytes": plan.device_bytes()}
        pop.close()
    return out


def measure_population_eval(repeats):
    """the evaluation of a population, batched against member by member, and a round that ends on the device against one that
    ends on the host"""
    from rdis_amd import capi, problems as P
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from ba_multistart import sampling_intervals
    ctx = capi.Context(0)

    def median_ms(call):
        call()                                             # (warm-up)
        tt = []
        for _ in range(repeats):
            t = time.perf_counter()
            call()
            tt.append(time.perf_counter() - t)
        return 1e3 * float(np.median(tt))

    def shape(pp, members, cam_opts, pt_opts):
        cams, pts = P.ba_alternation_plans(pp)
        lo, hi = sampling_intervals(pp)
        g = capi.Problem(ctx, pp)
        plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
        for plan, opts in zip(plans, (cam_opts, pt_opts)):
            for k, v in opts.items():
                plan.set_option(k, v)
        pop = capi.Population(g, x=np.random.default_rng(0).uniform(lo, hi, size=(members, pp.nvars)))
        plans[0].solve_population(pop, 25, 3e-8)           # one camera step: every member its own cameras
        X = pop.get_x()
        out = {"members": members, "factors": int(pp.nfac)}
        f = {}
        for batched in (1, 0):
            pop.set_option("eval_batched", batched)
            out["eval_batched_%d_wall_ms" % batched] = median_ms(lambda: f.__setitem__(batched, pop.eval()))
            out["eval_batched_%d_launches" % batched] = pop.info("eval_launches")
        pop.set_option("eval_batched", 1)
        pop.eval()
        out["members_per_launch"] = pop.info("eval_members_per_launch")
        g.set_x(X[0])
        out["one_member_eval_wall_ms"] = median_ms(g.eval)
        out["eval_speedup"] = out["eval_batched_0_wall_ms"] / out["eval_batched_1_wall_ms"]
        out["batched_eval_in_single_evals"] = out["eval_batched_1_wall_ms"] / out["one_member_eval_wall_ms"]
        out["f_bytes_equal"] = bool(f[1].tobytes() == f[0].tobytes())
        res = {}

        def round_device():
            pop.set_x(X)
            t = time.perf_counter()
            for plan in plans:
                plan.solve_population(pop, 25, 3e-8)
            pop.eval_device()
            pop.assign_best()
            res["device"] = pop.best()
            return time.perf_counter() - t

        def round_host():
            pop.set_x(X)
            t = time.perf_counter()
            for plan in plans:
                plan.solve_population(pop, 25, 3e-8)
            fh = pop.eval()
            b = int(np.nanargmin(fh)) if not np.all(np.isnan(fh)) else 0      # (the lowest, the first of equals, no NaN unless all are)
            pop.assign(b)
            ctx.synchronize()
            dt = time.perf_counter() - t
            res["host"] = (b, float(fh[b]))
            return dt

        for name, call, batched in (("round_on_device_wall_ms", round_device, 1), ("round_on_host_wall_ms", round_host, 0)):
            pop.set_option("eval_batched", batched)
            call()                                         # (warm-up)
            out[name] = 1e3 * float(np.median([call() for _ in range(repeats)]))
            res[name] = g.get_x()
        out["round_speedup"] = out["round_on_host_wall_ms"] / out["round_on_device_wall_ms"]
        out["best_member"], out["best_f"] = res["device"]
        out["round_results_equal"] = bool(res["device"][0] == res["host"][0] and np.float64(res["device"][1]).tobytes() == np.float64(res["host"][1]).tobytes()
                                          and res["round_on_device_wall_ms"].tobytes() == res["round_on_host_wall_ms"].tobytes())
        for o in plans + [pop, g]:
            o.close()
        return out

    lds = {"coop_min_factors": 0, "coop_group_min_factors": 0}
    return {"ladybug_5_30": shape(P.load_bal(ncams=5, npts=30), 256, {}, {}),
            "ladybug_full": shape(P.load_bal(), 64, lds, {"population_tiny": 1})}


def measure_population_grad(repeats):
    """every member's value and gradient in one call (rdis_hip_population_eval_grad_device) against the member-by-member route
    (population_assign(s) + rdis_hip_eval_grad_device for every s -- code the batched path does not touch), device forms
    followed by one synchronisation"""
    from rdis_amd import capi, problems as P
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from ba_multistart import sampling_intervals
    ctx = capi.Context(0)

    def median_ms(call):
        call()                                             # (warm-up; a list's tables are built at its first use)
        tt = []
        for _ in range(repeats):
            t = time.perf_counter()
            call()
            ctx.synchronize()
            tt.append(time.perf_counter() - t)
        return 1e3 * float(np.median(tt))

    def shape(pp, members, cam_opts):
        cams, pts = P.ba_alternation_plans(pp)
        lo, hi = sampling_intervals(pp)
        g = capi.Problem(ctx, pp)
        plan = capi.Plan(g, *cams)
        for k, v in cam_opts.items():
            plan.set_option(k, v)
        pop = capi.Population(g, x=np.random.default_rng(0).uniform(lo, hi, size=(members, pp.nvars)))
        plan.solve_population(pop, 25, 3e-8)               # one camera step: every member its own cameras
        ctx.synchronize()

        def one_by_one():
            for s in range(members):
                pop.assign(s)
                g.eval_grad_device()

        out = {"members": members, "factors": int(pp.nfac), "variables": int(pp.nvars)}
        out["batched_wall_ms"] = median_ms(pop.eval_grad_device)
        out["batched_launches"] = pop.info("grad_launches")
        out["members_per_launch"] = pop.info("grad_members_per_launch")
        out["grad_branch"] = pop.info("grad_branch")
        out["member_by_member_wall_ms"] = median_ms(one_by_one)
        pop.assign(0)
        out["one_member_wall_ms"] = median_ms(g.eval_grad_device)
        out["speedup"] = out["member_by_member_wall_ms"] / out["batched_wall_ms"]
        out["batched_in_single_calls"] = out["batched_wall_ms"] / out["one_member_wall_ms"]
        f, gr = pop.eval_grad()
        same = True
        for s in range(members):
            pop.assign(s)
            fs, gs = g.eval_grad()
            same = same and np.float64(fs).tobytes() == f[s].tobytes() and gs.tobytes() == gr[s].tobytes()
        out["f_and_g_bytes_equal"] = bool(same)
        for o in (plan, pop, g):
            o.close()
        return out

    return {"ladybug_5_30": shape(P.load_bal(ncams=5, npts=30), 256, {}),
            "ladybug_full": shape(P.load_bal(), 64, {"coop_min_factors": 0, "coop_group_min_factors": 0})}


def measure_population_halving(repeats, members=256, rounds=4):
    """successive halving on the device against the way without sample / sort / a member range, and the three pieces alone"""
    from rdis_amd import capi, problems as P
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from ba_multistart import sampling_intervals
    from ba_population import OPTIONS
    seed = 0x5D15
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    lo, hi = sampling_intervals(pp)
    ctx = capi.Context(0)
    g = capi.Problem(ctx, pp)
    plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
    for plan in plans:
        for k, v in OPTIONS.items():
            plan.set_option(k, v)
        assert plan.info("components_lds") == plan.ncomp
    pop = capi.Population(g, members)
    pop.set_sampling(lo, hi)
    pop.sample(seed, 0)
    X0 = pop.get_x()

    def rule_order(f):
        return np.array(sorted(range(len(f)), key=lambda s: (f[s] != f[s], 0.0 if f[s] != f[s] else f[s], s)), dtype=np.int64)

    def on_device(halve=True, read_orders=False, kernel_ms=None):
        """(a), or with halve=False (c): all members in every round"""
        t = time.perf_counter()
        pop.sample(seed, 0)
        k, ids = members, np.arange(members)
        for _ in range(rounds):
            for plan in plans:
                plan.solve_population(pop, 25, 3e-8, first=0, count=k)
                if kernel_ms is not None:
                    kernel_ms.append(plan.last_kernel_ms()[0])
            pop.eval_device()
            order = pop.sort(want_order=read_orders)
            if read_orders:
                ids = ids[order]
            if halve:
                k //= 2
        pop.assign_best()
        x = g.get_x()                                       # the one read
        return time.perf_counter() - t, x, ids, k

    def on_host(kernel_ms=None):
        """(b): eval, the host's sort by the same rule, get_x of the survivors, a new Population from them"""
        t = time.perf_counter()
        part, ids = capi.Population(g, x=X0), np.arange(members)
        for _ in range(rounds):
            for plan in plans:
                plan.solve_population(part, 25, 3e-8)
                if kernel_ms is not None:
                    kernel_ms.append(plan.last_kernel_ms()[0])
            keep = rule_order(part.eval())[:part.nmembers // 2]
            rows = part.get_x()[keep]
            ids = ids[keep]
            part.close()
            part = capi.Population(g, x=rows)
        part.assign(0)
        x = g.get_x()
        dt = time.perf_counter() - t
        part.close()
        return dt, x, ids, rows

    on_device(); on_host(); on_device(halve=False)          # (warm-up: tables, buffers, first launches)
    ta, tb, tc = [], [], []
    for _ in range(repeats):                                # the ways alternate within the job
        ta.append(on_device()[0]); tb.append(on_host()[0]); tc.append(on_device(halve=False)[0])
    ka, kb, kc = [], [], []
    _, xa, ids_a, k_end = on_device(read_orders=True, kernel_ms=ka)
    rows_a = pop.get_x(first=0, count=k_end)
    fa = pop.best()[1]
    _, xb, ids_b, rows_b = on_host(kernel_ms=kb)
    on_device(halve=False, kernel_ms=kc)
    fc = pop.best()[1]
    out = {"members": members, "rounds": rounds, "survivors": k_end,
           "device_wall_ms": 1e3 * float(np.median(ta)), "device_wall_ms_all": [1e3 * t for t in ta], "device_kernel_ms": float(sum(ka)),
           "host_wall_ms": 1e3 * float(np.median(tb)), "host_wall_ms_all": [1e3 * t for t in tb], "host_kernel_ms": float(sum(kb)),
           "all_members_wall_ms": 1e3 * float(np.median(tc)), "all_members_kernel_ms": float(sum(kc)),
           "same_order": bool(ids_a[:k_end].tolist() == ids_b.tolist()), "same_surviving_rows": bool(rows_a.tobytes() == rows_b.tobytes()),
           "same_x": bool(xa.tobytes() == xb.tobytes()), "best_f_halving": fa, "best_f_all_members": fc}
    out["host_over_device"] = out["host_wall_ms"] / out["device_wall_ms"]
    out["device_faster_beyond_host_spread"] = bool(out["host_wall_ms"] - out["device_wall_ms"] > 1e3 * (max(tb) - min(tb)))
    pop.close()

    # sort alone: eval once, then sort (enqueued) + synchronize, the wall time between two synchronisations
    sort_ms = {}
    for n in (256, 4096, 65535):
        q = capi.Population(g, n)
        q.set_sampling(lo, hi)
        q.sample(seed, 1)
        q.eval_device()
        q.sort(want_order=False)                            # (the second buffer, the first launch)
        ts = []
        for r in range(5):
            q.sample(seed, 2 + r)
            q.eval_device()
            ctx.synchronize()
            t = time.perf_counter()
            q.sort(want_order=False)
            ctx.synchronize()
            ts.append(time.perf_counter() - t)
        sort_ms[str(n)] = 1e3 * float(np.median(ts))
        q.close()
    out["sort_wall_ms_by_members"] = sort_ms

    # sample alone: 256 whole members of full ladybug against the host's draw + set_x of the same bytes
    pf = P.load_bal()
    gf = capi.Problem(ctx, pf)
    flo, fhi = sampling_intervals(pf)
    q = capi.Population(gf, 256)
    q.set_sampling(flo, fhi)
    rng = np.random.default_rng(0)

    def draw_device():
        t = time.perf_counter()
        q.sample(seed, 0)
        ctx.synchronize()
        return time.perf_counter() - t

    def draw_host():
        t = time.perf_counter()
        q.set_x(rng.uniform(flo, fhi, size=(256, pf.nvars)))
        return time.perf_counter() - t

    draw_device(); draw_host()
    out["sample_full_ladybug"] = {"members": 256, "bytes": 256 * pf.nvars * 8,
                                  "device_wall_ms": 1e3 * float(np.median([draw_device() for _ in range(5)])),
                                  "host_draw_set_x_wall_ms": 1e3 * float(np.median([draw_host() for _ in range(5)]))}
    return out


def step(name, repeats):
    from rdis_amd import problems as P
    if name == "population-halving":
        return measure_population_halving(repeats)
    if name == "population-eval":
        return measure_population_eval(repeats)
    if name == "population-grad":
        return measure_population_grad(repeats)
    if name == "population-tiny":
        return measure_population_tiny(repeats)
    if name == "population-point-major":
        return measure_population_point_major(repeats)
    if name == "population":
        return measure_population(repeats)
    if name == "population-nlp":
        return measure_population_nlp(repeats)
    if name == "config3":
        with open(os.path.join(ROOT, "tests", "golden", "end_values.json")) as fh:
            seed = json.load(fh)["seed"]
        pp = P.load_bal(ncams=5, npts=30).single_component()
        starts = np.stack([ulp_perturbed(pp.x0, np.random.default_rng([seed, 100000 + k])) for k in range(320)])
    elif name == "config2":
        pp = P.make_high_dim_sinusoid().single_component()
        starts = np.random.default_rng(2).uniform(pp.lo, pp.hi, size=(1024, pp.nvars))
    else:
        pp = P.make_synthetic_ba(1000, 3, 40)
        rng = np.random.default_rng(17)
        starts = np.stack([pp.x0] + [ulp_perturbed(pp.x0, rng) for _ in range(7)])
    return measure(pp, starts, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.step:
        print(json.dumps({a.step: step(a.step, a.repeats)}))
        return 0
    out = {"tool": "bench_multistart", "maxiters": 25, "ftol": 3e-8}
    try:
        out["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        out["commit"] = None
    for name in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--repeats", str(a.repeats)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            out[name] = {"error": f"time limit of {STEP_LIMIT_S[name]} s"}
            break
        if p.returncode != 0:
            out[name] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            break   # (nothing more is started on a device that a step has just failed on)
        out.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0 if all("error" not in out.get(k, {"error": 1}) for k in STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
