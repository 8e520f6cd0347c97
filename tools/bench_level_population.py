#!/usr/bin/env python3
"""optBA's sample loop as one population run (HipRDISLevelOptimizer::optimizePopulation) against the loop it replaces: assignAll +
optimize() member by member on one driver object.  Schedule 0, the members drawn as rdis_optba_run_samples draws them.

  python tools/bench_level_population.py [--rounds 5] [--out profiles/level_population_bench.json] [--design DESIGN.md]
  python tools/bench_level_population.py --table-from profiles/level_population_bench.json --design DESIGN.md   (no GPU: the table only)
  python tools/bench_level_population.py --cooperative [--out profiles/level_population_cooperative_bench.json] [--design DESIGN.md]

Cases: ladybug 5 / 30 with 16, 64 and 256 members, CGD and Levenberg-Marquardt model 2; full ladybug (49 / 7776) with 8 and 32
members, Levenberg-Marquardt model 2, and CGD where the population entry takes its tree (else the refusal is recorded).
One warm-up of both, then `--rounds` rounds that run the loop and the population run one after the other (alternating, so drift
hits both alike); the median of each and the ratio of the medians.  The decomposition is outside both timings; the plans each run
makes are inside (the population run makes them once, optimize() once per member).  The seconds inside
rdis_hip_population_permute (which moves all S rows) are reported on their own.  --design splices the table between the markers
'<!-- level_population_bench:begin -->' and '<!-- level_population_bench:end -->' of that file.
--cooperative reruns the two rows the population entry refuses (full ladybug, CGD, 8 and 32 members) with the level option
populationCooperative = 1 (a cooperative group per member: rdis_hip_plan_solve_population_cooperative), reports the members a launch
held, writes profiles/level_population_cooperative_bench.json and splices between the markers '<!-- level_population_cooperative_bench:begin -->'
and '<!-- level_population_cooperative_bench:end -->'.
The C++ side is tools/level_population_bench.cpp, compiled here against rdis_amd/lib/librdis_host.so."""
import argparse
import ctypes as C
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SSMAXIT, SWEEPS, SEED = 10, 3, 20240611
# (name, cameras, points (0: all), use_cgd, model, members)
CASES = [("ladybug-5-30", 5, 30, u, 2, s) for u in (1, 0) for s in (16, 64, 256)] + \
        [("ladybug-49-7776", 0, 0, u, 2, s) for u in (0, 1) for s in (8, 32)]
COOPERATIVE_CASES = [("ladybug-49-7776", 0, 0, 1, 2, s) for s in (8, 32)]
BEGIN, END = "<!-- level_population_bench:begin -->", "<!-- level_population_bench:end -->"
COOP_BEGIN, COOP_END = "<!-- level_population_cooperative_bench:begin -->", "<!-- level_population_cooperative_bench:end -->"


def _helper(tmp):
    lib = os.path.join(ROOT, "rdis_amd", "lib")
    out = os.path.join(tmp, "liblevel_population_bench.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", out, os.path.join(ROOT, "tools", "level_population_bench.cpp"),
                           "-L" + lib, "-lrdis_host", "-lrdis_hip", "-Wl,-rpath," + lib])
    return C.CDLL(out)


def measure(rounds, cooperative=False):
    from rdis_amd import problems as P
    tmp = tempfile.mkdtemp()
    try:
        h = _helper(tmp)
        path = os.path.join(tmp, "ladybug.txt")
        with gzip.open(P.LADYBUG_PATH, "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        path = path.encode()
        rows = []
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        for name, nc, npnt, use_cgd, model, members in (COOPERATIVE_CASES if cooperative else CASES):
            loop, pop, perm, info = np.zeros(rounds), np.zeros(rounds), np.zeros(rounds), np.zeros(9)
            msg = C.create_string_buffer(2048)
            rc = h.bench_level_population_option(path, C.c_longlong(nc), C.c_longlong(npnt), use_cgd, SSMAXIT, SWEEPS, model, C.c_longlong(members),
                                                 C.c_ulonglong(SEED), rounds, 1 if cooperative else 0, p(loop), p(pop), p(perm), p(info), msg,
                                                 C.c_longlong(len(msg)))
            row = {"problem": name, "optimiser": "cgd" if use_cgd else "lm%d" % model, "members": members}
            if cooperative:
                row["populationCooperative"] = 1
            if rc == 1:
                row["refused"] = msg.value.decode()
            elif rc != 0:
                raise RuntimeError("bench_level_population returned %d for %r" % (rc, row))
            else:
                row.update({"loop_s": loop.tolist(), "population_s": pop.tolist(), "permute_s": perm.tolist(),
                            "loop_median_s": statistics.median(loop), "population_median_s": statistics.median(pop),
                            "loop_spread_s": float(loop.max() - loop.min()), "population_spread_s": float(pop.max() - pop.min()),
                            "permute_median_s": statistics.median(perm), "members_whose_final_value_differs": int(info[0]),
                            "best_loop": info[1], "best_population": info[2], "sweeps_of_all_members": int(info[3]), "most_sweeps": int(info[4]),
                            "permutes": int(info[5]), "launches_a_sweep": int(info[6]), "members_not_finite": int(info[7])})
                row["loop_over_population"] = row["loop_median_s"] / row["population_median_s"]
                if cooperative:
                    row["members_a_launch"] = int(info[8])
            print("  %r" % row, file=sys.stderr, flush=True)
            rows.append(row)
        res = {"schedule": 0, "SSmaxit": SSMAXIT, "maxSweeps": SWEEPS, "seed": SEED, "rounds": rounds, "cases": rows}
        if cooperative:
            res["populationCooperative"] = 1
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def table(res):
    coop = bool(res.get("populationCooperative"))
    lines = ["| problem | optimiser | members | loop median s (spread) | population run median s (spread) | loop / population | in permutes s (share) | "
             "permutes | sweeps of all members | finals that differ |" + (" members a launch |" if coop else ""),
             "|---|---|---|---|---|---|---|---|---|---|" + ("---|" if coop else "")]
    for r in res["cases"]:
        if "refused" in r:
            lines.append("| %s | %s | %d | refused: %s | | | | | | |" % (r["problem"], r["optimiser"], r["members"], r["refused"]) + (" |" if coop else ""))
            continue
        lines.append("| %s | %s | %d | %.4f (%.4f) | %.4f (%.4f) | %.2f | %.5f (%.1f %%) | %d | %d | %d |" % (
            r["problem"], r["optimiser"], r["members"], r["loop_median_s"], r["loop_spread_s"], r["population_median_s"], r["population_spread_s"],
            r["loop_over_population"], r["permute_median_s"], 100.0 * r["permute_median_s"] / r["population_median_s"], r["permutes"],
            r["sweeps_of_all_members"], r["members_whose_final_value_differs"]) + (" %d |" % r["members_a_launch"] if coop else ""))
    return "\n".join(lines)


def splice(design, text, begin=BEGIN, end=END):
    with open(design) as fh:
        s = fh.read()
    a, b = s.index(begin) + len(begin), s.index(end)
    with open(design, "w") as fh:
        fh.write(s[:a] + "\n" + text + "\n" + s[b:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cooperative", action="store_true")
    ap.add_argument("--table-from", default=None)
    ap.add_argument("--design", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "level_population_cooperative_bench.json" if a.cooperative else "level_population_bench.json")
    if a.table_from:
        with open(a.table_from) as fh:
            res = json.load(fh)
    else:
        res = measure(a.rounds, a.cooperative)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    text = table(res)
    print(text)
    if a.design:
        coop = bool(res.get("populationCooperative"))
        splice(a.design, text, COOP_BEGIN if coop else BEGIN, COOP_END if coop else END)


if __name__ == "__main__":
    main()
