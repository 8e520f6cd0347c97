#!/usr/bin/env python3
"""The level driver's two subspace optimisers measured on full ladybug (49 cameras, 7776 points) through rdis_optba_run,
schedule 0 (sweeps over the levels), SSmaxit 25: what optBA's --useCGD switch costs and buys.

  python tools/bench_lm_levels.py [--rounds 5] [--sweeps 5] [--out profiles/lm_levels_bench.json] [--design DESIGN.md]
  python tools/bench_lm_levels.py --table-from profiles/lm_levels_bench.json --design DESIGN.md     (no GPU: the table only)

Configurations (each a complete rdis_optba_run: load, upload, decomposition, maxSweeps sweeps; the time is out[5], the seconds
in the optimisation alone):
  cgd          useCGD 1
  lm1, lm2     useCGD 0 with LMmodel 1 / 2, every other option at its default       (a) the switch itself
  lm1-{plan,single}-{summary,detail}   LMmodel 1 with both remaining options spelled out:
               plan / single    LMsingleMinFactors 0 / just below the separator's factor count: the 46-camera separator step as
                                a wide component of the level's plan / by rdis_hip_lm_optimize on its own           (c)
               summary / detail lmStepDetail 0 / 1: the 128-byte summary alone / a full fetch and host mirror a step  (b)
One warm-up of every configuration, then `--rounds` rounds that run the configurations one after the other (alternating, so
drift hits all alike); best and median per configuration.  The objective after every sweep comes from runs with maxSweeps
1, 2, ... (the run is deterministic: the test suite pins it bit for bit).  --design splices the table between the markers
'<!-- lm_levels_bench:begin -->' and '<!-- lm_levels_bench:end -->' of that file."""
import argparse
import ctypes as C
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEPARATOR_FACTORS = 30594          # full ladybug's depth-0 separator: 46 cameras + 1 point
CONFIGS = {
    "cgd": {"useCGD": 1.0},
    "lm1": {"useCGD": 0.0, "LMmodel": 1.0},                   # the defaults of lmStepDetail and LMsingleMinFactors
    "lm2": {"useCGD": 0.0, "LMmodel": 2.0},
    "lm1-plan-summary": {"useCGD": 0.0, "LMmodel": 1.0, "LMsingleMinFactors": 0.0, "lmStepDetail": 0.0},
    "lm1-plan-detail": {"useCGD": 0.0, "LMmodel": 1.0, "LMsingleMinFactors": 0.0, "lmStepDetail": 1.0},
    "lm1-single-summary": {"useCGD": 0.0, "LMmodel": 1.0, "LMsingleMinFactors": float(SEPARATOR_FACTORS - 594), "lmStepDetail": 0.0},
    "lm1-single-detail": {"useCGD": 0.0, "LMmodel": 1.0, "LMsingleMinFactors": float(SEPARATOR_FACTORS - 594), "lmStepDetail": 1.0},
}
BEGIN, END = "<!-- lm_levels_bench:begin -->", "<!-- lm_levels_bench:end -->"


def _entry():
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                   C.c_int32, C.c_void_p, C.c_void_p]
    return lib.rdis_optba_run


def run(entry, path, opts):
    names, vals = [k.encode() for k in opts], list(opts.values())
    out = np.zeros(10)
    rc = entry(path, 0, 0, 0, len(names), (C.c_char_p * len(names))(*names), (C.c_double * len(vals))(*vals), 0, out.ctypes.data_as(C.c_void_p), None)
    if rc != 0:
        raise RuntimeError("rdis_optba_run returned %d for %r" % (rc, opts))
    print("  %r: %.6f after %d sweep(s), %.4f s" % (opts, out[0], int(out[9]), out[5]), file=sys.stderr, flush=True)
    return out


def measure(rounds, sweeps):
    from rdis_amd import problems as P
    entry = _entry()
    tmp = tempfile.mkdtemp()
    try:
        path = os.path.join(tmp, "ladybug.txt")
        with gzip.open(P.LADYBUG_PATH, "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        path = path.encode()
        base = {"SSmaxit": 25.0, "maxSweeps": float(sweeps)}
        rows = {}
        for name, extra in CONFIGS.items():                       # warm-up, and what does not depend on the round
            out = run(entry, path, dict(base, **extra))
            rows[name] = {"options": extra, "initial": out[1], "final": out[0], "sweeps_done": int(out[9]), "launches": int(out[4]),
                          "calls": int(out[2]), "iterations": int(out[3]), "residual_evaluations": int(out[8]), "seconds": []}
        for _ in range(rounds):
            for name, extra in CONFIGS.items():
                out = run(entry, path, dict(base, **extra))
                assert out[0] == rows[name]["final"], name        # the same run every time
                rows[name]["seconds"].append(out[5])
        for name in ("cgd", "lm1", "lm2"):                        # the objective after every sweep
            per, done = [], rows[name]["sweeps_done"]
            for k in range(1, done + 1):
                per.append(run(entry, path, dict(base, maxSweeps=float(k), **CONFIGS[name]))[0])
            rows[name]["objective_after_sweep"] = per
        for r in rows.values():
            r["best_s"], r["median_s"] = min(r["seconds"]), statistics.median(r["seconds"])
            r["spread_s"] = max(r["seconds"]) - min(r["seconds"])
        return {"problem": "ladybug-49-7776", "schedule": 0, "SSmaxit": 25, "maxSweeps": sweeps, "rounds": rounds,
                "separator_factors": SEPARATOR_FACTORS, "configs": rows}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


CROSSOVER_SHAPES = [(3, 100), (6, 300), (6, 2000), (12, 150), (16, 300), (16, 1500), (17, 100), (17, 400), (21, 300), (32, 300), (32, 1000), (49, 300),
                    (49, 1000), (49, 3000), (49, 7776)]


def crossover(rounds, iters=10):
    """--crossover: one component alone -- the first nc cameras and npts points of ladybug, everything free -- as the only
    component of a resident plan (solve + summary) against rdis_hip_lm_optimize, the same start, `iters` iterations at most,
    model 1; host clock around calls that end synchronised, the start re-assigned outside the window.  What the default of
    LMsingleMinFactors is read from."""
    import time
    from rdis_amd import capi, problems as P
    ctx = capi.Context(0)
    rows = []
    for nc, npnt in CROSSOVER_SHAPES:
        pp = P.load_bal(ncams=nc, npts=npnt)
        g = capi.Problem(ctx, pp)
        fv, fc = np.arange(pp.nvars, dtype=np.int64), np.arange(pp.nfac, dtype=np.int64)
        plan = capi.LmPlan(g, [0, pp.nvars], fv, [0, pp.nfac], fc, model=1, history=1, wide=True)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        out, info = np.zeros(2), np.zeros(8)

        def by_plan():
            plan.solve(iters, 3e-8)
            return plan.summary()[2]

        def by_call():
            g.ctx.check(g.ctx.lib.rdis_hip_lm_optimize(g.h, fv.shape[0], vp(fv), fc.shape[0], vp(fc), None, iters, 3e-8, 1, vp(out), C.c_void_p(out.ctypes.data + 8),
                                                       vp(info), None, 0, None))
            return info[0]
        t = {"plan": [], "call": []}
        done = {}
        for r in range(rounds + 1):
            for name, fn in (("plan", by_plan), ("call", by_call)):
                g.set_x(pp.x0)
                ctx.synchronize()
                t0 = time.perf_counter()
                done[name] = int(fn())
                if r > 0:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        row = {"cameras": nc, "points": npnt, "factors": int(pp.nfac), "plan_ms": statistics.median(t["plan"]), "call_ms": statistics.median(t["call"]),
               "plan_spread_ms": max(t["plan"]) - min(t["plan"]), "call_spread_ms": max(t["call"]) - min(t["call"]), "plan_iterations": done["plan"],
               "call_iterations": done["call"]}
        print("  %r" % row, file=sys.stderr, flush=True)
        rows.append(row)
        plan.close(); g.close()
    return rows


def crossover_table(rows):
    lines = ["| cameras | points | factors | plan (wide or LDS class) ms | single call ms | iterations plan / call |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %d | %d | %.3f | %.3f | %d / %d |" % (r["cameras"], r["points"], r["factors"], r["plan_ms"], r["call_ms"], r["plan_iterations"],
                                                                 r["call_iterations"]))
    return "\n".join(lines)


def table(res):
    c = res["configs"]
    lines = ["| configuration | options | sweeps | LM / CG iterations | final objective | best s | median s | spread s |", "|---|---|---|---|---|---|---|---|"]
    for name, r in c.items():
        opts = ", ".join("%s %g" % kv for kv in r["options"].items())
        lines.append("| %s | %s | %d | %d | %.6f | %.4f | %.4f | %.4f |" % (name, opts, r["sweeps_done"], r["iterations"], r["final"], r["best_s"],
                                                                          r["median_s"], r["spread_s"]))
    lines.append("")
    lines.append("Objective after every sweep (initial %.6f):" % c["cgd"]["initial"])
    lines.append("")
    for name in ("cgd", "lm1", "lm2"):
        lines.append("- %s: %s" % (name, ", ".join("%.6f" % f for f in c[name]["objective_after_sweep"])))
    if res.get("crossover"):
        lines += ["", "One component alone, in a plan against a call of its own (10 iterations at most, model 1):", "", crossover_table(res["crossover"])]

    def verdict(a, b, what):
        d = c[a]["median_s"] - c[b]["median_s"]
        noise = max(c[a]["spread_s"], c[b]["spread_s"])
        return "- %s: %s median %.4f s against %s %.4f s: a difference of %+.4f s, the larger spread between rounds %.4f s -- %s." % (
            what, a, c[a]["median_s"], b, c[b]["median_s"], d, noise, "beyond the spread" if abs(d) > noise else "within the spread")
    lines.append("")
    lines.append(verdict("lm1-plan-detail", "lm1-plan-summary", "(b) lmStepDetail 1 against the summary, the separator a wide plan component"))
    lines.append(verdict("lm1-single-detail", "lm1-single-summary", "(b) the same with the separator solved by a call of its own"))
    lines.append(verdict("lm1-single-summary", "lm1-plan-summary", "(c) the separator by a call of its own against a wide plan component"))
    return "\n".join(lines)


def splice(design, text):
    with open(design) as fh:
        s = fh.read()
    a, b = s.index(BEGIN) + len(BEGIN), s.index(END)
    with open(design, "w") as fh:
        fh.write(s[:a] + "\n" + text + "\n" + s[b:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_levels_bench.json"))
    ap.add_argument("--table-from", default=None)
    ap.add_argument("--design", default=None)
    ap.add_argument("--crossover", action="store_true", help="also time single components of growing size both ways")
    a = ap.parse_args()
    if a.table_from:
        with open(a.table_from) as fh:
            res = json.load(fh)
    else:
        res = measure(a.rounds, a.sweeps)
        if a.crossover:
            res["crossover"] = crossover(a.rounds)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    text = table(res)
    print(text)
    if a.design:
        splice(a.design, text)


if __name__ == "__main__":
    main()
