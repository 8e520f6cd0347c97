#!/usr/bin/env python3
"""rdis_hip_lm_batch measured: a batch of small Levenberg-Marquardt components in one call against the same components one
by one through rdis_hip_lm_optimize (the only way before the batch entry), same start, same iteration limit.

  python tools/bench_lm_batch.py [--repeats 5] [--case a|b|c]

  a  ladybug 5 cameras / 30 points, the cameras constant: 30 point components of 3 unknowns, model 1, 3 iterations
  b  full ladybug, the cameras constant: 7776 point components (rdis_hip_components), model 2, 5 iterations
  c  the synthetic batch of 6 x (3 cameras, 40 points), each component whole, model 1, 5 iterations; rdis_hip_lm_optimize
     wants the cameras below the points, so the sequential loop runs every component as a problem of its own

Both ways are timed at the C ABI (ctypes calls with arrays allocated beforehand, no history, the start re-assigned
outside the timed window): a host clock around calls that end synchronised.  One warm-up of each way, then `--repeats`
rounds that alternate the two ways; the best and the median of each are printed, one JSON line per case, with whether
both ways ended at the same objective (to 1e-9)."""
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


def _csr(comps):
    fp = np.concatenate([[0], np.cumsum([len(f) for f, _ in comps])]).astype(np.int64)
    jp = np.concatenate([[0], np.cumsum([len(j) for _, j in comps])]).astype(np.int64)
    return fp, np.concatenate([f for f, _ in comps]).astype(np.int64), jp, np.concatenate([j for _, j in comps]).astype(np.int64)


def batch_call(g, comps, iters, model):
    fp, fv, jp, fj = _csr(comps)
    fret = np.zeros(len(comps))

    def run():
        g.ctx.check(g.ctx.lib.rdis_hip_lm_batch(g.h, len(comps), _p(fp), _p(fv), _p(jp), _p(fj), None, iters, 3e-8, model,
                                                _p(fret), None, None, None, 0, None))
        return float(np.sum(fret))
    return run


def sequential_call(items, iters, model):
    """items: (problem, free, fac) per component"""
    items = [(g, np.ascontiguousarray(f, dtype=np.int64), np.ascontiguousarray(j, dtype=np.int64)) for g, f, j in items]
    out = np.zeros(1)

    def run():
        total = 0.0
        for g, free, fac in items:
            g.ctx.check(g.ctx.lib.rdis_hip_lm_optimize(g.h, free.shape[0], _p(free), fac.shape[0], _p(fac), None, iters, 3e-8, model,
                                                       _p(out), None, None, None, 0, None))
            total += out[0]
        return total
    return run


def measure(name, what, ways, reset, repeats):
    """ways: {label: run}; reset(): the start re-assigned (not timed)"""
    ends, ms = {}, {k: [] for k in ways}
    for k, run in ways.items():      # warm-up: code objects, workspaces
        reset()
        ends[k] = run()
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
    a, b = (ends[k] for k in ways)
    rec["ends_agree"] = bool(abs(a - b) <= 1e-9 * abs(b))
    rec["sequential_over_batch"] = round(rec["sequential_ms_best"] / rec["batch_ms_best"], 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--case", default="abc")
    a = ap.parse_args()
    ctx = capi.Context(0)
    if "a" in a.case:
        pp = P.load_bal(ncams=5, npts=30)
        g = capi.Problem(ctx, pp)
        comps = [(45 + 3 * p + np.arange(3), np.where(pp.pt_vid0 == 45 + 3 * p)[0]) for p in range(30)]
        measure("a", "ladybug 5/30, 30 point components, model 1, 3 iterations",
                {"batch": batch_call(g, comps, 3, 1), "sequential": sequential_call([(g, f, j) for f, j in comps], 3, 1)},
                lambda: g.set_x(pp.x0), a.repeats)
    if "b" in a.case:
        pp = P.load_bal()
        g = capi.Problem(ctx, pp)
        assigned = np.zeros(pp.nvars, dtype=np.uint8)
        assigned[:9 * 49] = 1
        fp, fv, jp, fj = g.components(assigned)
        comps = [(fv[fp[c]:fp[c + 1]], fj[jp[c]:jp[c + 1]]) for c in range(len(fp) - 1)]
        measure("b", "full ladybug, %d point components, model 2, 5 iterations" % len(comps),
                {"batch": batch_call(g, comps, 5, 2), "sequential": sequential_call([(g, f, j) for f, j in comps], 5, 2)},
                lambda: g.set_x(pp.x0), a.repeats)
    if "c" in a.case:
        pp = P.make_synthetic_ba(6, 3, 40, first_comp=7)
        g = capi.Problem(ctx, pp)
        nv, nf = pp.nvars // 6, pp.nfac // 6
        comps = [(c * nv + np.arange(nv), c * nf + np.arange(nf)) for c in range(6)]
        singles = []
        for free, fac in comps:
            q = P.PackedProblem(kind=pp.kind, x0=pp.x0[free].copy(), lo=pp.lo[free].copy(), hi=pp.hi[free].copy(),
                                cam_vid0=pp.cam_vid0[fac] - free[0], pt_vid0=pp.pt_vid0[fac] - free[0], obs=pp.obs[fac].copy())
            singles.append((capi.Problem(ctx, q), q))

        def reset():
            g.set_x(pp.x0)
            for s, q in singles:
                s.set_x(q.x0)
        measure("c", "synthetic 6 x (3 cameras, 40 points), model 1, 5 iterations",
                {"batch": batch_call(g, comps, 5, 1),
                 "sequential": sequential_call([(s, np.arange(q.nvars), np.arange(q.nfac)) for s, q in singles], 5, 1)}, reset, a.repeats)


if __name__ == "__main__":
    main()
