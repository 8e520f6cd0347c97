"""The level driver on Levenberg-Marquardt plans (optBA's useCGD = false) on the device: a plan's step summary
(rdis_hip_lm_plan_summary) against a numpy restatement of its stated order; the driver's sweeps against the alternation built by
hand from capi.LmPlan / Problem.lm_optimize over the same lists -- with ==: LmPlan is pinned to oracle/lm_oracle.py by the
Levenberg-Marquardt suites, this file pins the driver to LmPlan --; HipLMSubspaceOptimizer::optimizeBatch against
Problem.lm_batch; the reference schedule against oracle/levels.py's replay; the C entry's useCGD switch.
The C++ side is tests/cpp/harness_lm_levels.cpp, built by this file's fixture."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import levels as LV
from oracle import oracle as O
from rdis_amd import capi, problems as P

import lm_levels_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTOL, STEPTOL = 3e-8, 1e-4      # SubspaceOptimizer's and the level driver's defaults
TRACE_COLS = 12
v = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rdis_amd", "host")], stdout=subprocess.DEVNULL)
    out = os.path.join(ROOT, "tests", "cpp", "libharness_lm_levels.so")
    src = os.path.join(ROOT, "tests", "cpp", "harness_lm_levels.cpp")
    deps = [src, os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so")]
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", out, src, "-L" + os.path.join(ROOT, "rdis_amd", "lib"),
                               "-lrdis_host", "-lrdis_hip", "-Wl,-rpath,$ORIGIN/../../rdis_amd/lib"])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def bal_path(tmp_path_factory):
    dst = tmp_path_factory.mktemp("bal") / "ladybug.txt"
    with gzip.open(P.LADYBUG_PATH, "rb") as src, open(dst, "wb") as out:
        shutil.copyfileobj(src, out)
    return str(dst).encode()


# ---- the summary kernel ---------------------------------------------------------------------------------------------------
def _device_sum(a):
    """the stated order: 256 lanes, a lane's stride over the components in component order, a butterfly over each wave of 64,
    then the four waves in wave order"""
    a = np.asarray(a, dtype=np.float64)
    acc = np.zeros(256)
    for c0 in range(0, len(a), 256):
        part = a[c0:c0 + 256]
        acc[:len(part)] = acc[:len(part)] + part
    w = acc.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    s = 0.0
    for k in range(4):
        s = s + w[k, 0]
    return s


def _summary_of(rows):
    fret = np.array([r.fret for r in rows])
    want = np.zeros(16)
    want[0] = _device_sum(fret)
    want[1] = _device_sum([r.delta for r in rows])
    for k, name in ((2, "iters"), (3, "nfev"), (4, "njev"), (5, "nsolve")):
        want[k] = _device_sum([getattr(r, name) for r in rows])
    for code in range(1, 8):
        want[5 + code] = _device_sum([1.0 if r.stop == code else 0.0 for r in rows])
    want[13] = _device_sum([0.0 if np.isfinite(f) else 1.0 for f in fret])
    return want


def _point_plan_lists(g, pp):
    """every point on its own, the cameras held: the point plan of the hand-built alternation"""
    assigned = np.zeros(pp.nvars, np.uint8)
    assigned[:int(pp.pt_vid0.min())] = 1
    return g.components(assigned)


def _fetch_bytes(rows):
    return b"".join(r.x.tobytes() + np.array([r.fret, r.delta, r.iters, r.stop, r.nfev, r.njev, r.nsolve, r.mu]).tobytes() + r.history.tobytes()
                    for r in rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", [("ladybug-5-30", "points"), ("ladybug-8-300", "points"), ("ladybug-20-120", "leaves")])
@pytest.mark.parametrize("model", [1, 2])
def test_summary_is_the_stated_sum_of_the_fetched_rows(name, which, model, gctx):
    pp = K.problem(name)
    g = capi.Problem(gctx, pp)
    lists = _point_plan_lists(g, pp) if which == "points" else K.plans(name)[1][3:]
    plan = capi.LmPlan(g, *lists, model=model, history=4, wide=True)
    ncomp = plan.ncomp
    assert ncomp == {"ladybug-5-30": 30, "ladybug-8-300": 300, "ladybug-20-120": 89}[name]
    with pytest.raises(capi.RdisHipError) as e:                      # before any solve
        plan.summary()
    assert e.value.code == -1
    plan.solve(5, FTOL)
    rows = plan.fetch()
    before = _fetch_bytes(rows)
    s = plan.summary()
    assert s[0] == plan.objective()
    want = _summary_of(rows)
    assert s.tobytes() == want.tobytes(), (s, want)
    assert s[6:13].sum() == ncomp and s[13] == 0 and s[14] == 0 and s[15] == 0 and s[1] < 0 and s[2] > 0
    assert _fetch_bytes(plan.fetch()) == before                     # nothing a fetch returns was written
    # after a multi-start solve: the winners' rows
    rng = np.random.default_rng(7)
    x0 = pp.x0[plan.free_vid]
    starts = np.stack([x0, x0 * (1.0 + 1e-3 * rng.standard_normal(x0.shape)), x0 + 1e-3 * rng.standard_normal(x0.shape)])
    g.set_x(pp.x0)
    plan.solve_starts(starts, 5, FTOL)
    winners = plan.fetch()
    s = plan.summary()
    assert s[0] == plan.objective() and s.tobytes() == _summary_of(winners).tobytes()
    srows, best = plan.fetch_starts()
    assert [w.fret for w in winners] == [srows[int(best[c])][c].fret for c in range(ncomp)]   # (the rows summed are the winners')
    print("%s %s, model %d: winners per start %s" % (name, which, model, np.bincount(best, minlength=3).tolist()))
    # after a population solve: refused, like the objective
    pop = capi.Population(g, 2)
    plan.solve_population(pop, 0, 2, 3, FTOL)
    with pytest.raises(capi.RdisHipError) as e:
        plan.summary()
    assert e.value.code == -1
    with pytest.raises(capi.RdisHipError):
        plan.objective()


@pytest.mark.gpu
def test_summary_counts_a_start_that_is_not_finite(gctx):
    """a NaN coordinate in one point: that component ends with code 7 and a value that is not finite -- [12] and [13] count it,
    [0] is not finite, and the entry still returns 0"""
    pp = K.problem("ladybug-5-30")
    g = capi.Problem(gctx, pp)
    plan = capi.LmPlan(g, *_point_plan_lists(g, pp), model=1, history=1, wide=True)
    x = pp.x0.copy()
    x[int(plan.free_vid[plan.free_ptr[3]])] = np.nan
    g.set_x(x)
    plan.solve(5, FTOL)
    s, rows = plan.summary(), plan.fetch()
    assert rows[3].stop == 7 and not np.isfinite(rows[3].fret)
    assert s[12] == 1 and s[13] == 1 and not np.isfinite(s[0]) and s[6:13].sum() == 30
    assert s[2] == sum(r.iters for r in rows) and s[3] == sum(r.nfev for r in rows)


# ---- schedule 0 against the hand-built alternation --------------------------------------------------------------------------
def _driver(h, path, nc, npnt, nvars, maxit, sweeps, pct=0.2, seppct=0.0, model=1, batch=1, detail=0, single_min=0.0):
    out, tr, x = np.zeros(5), np.zeros((4096, TRACE_COLS)), np.zeros(nvars)
    rc = h.harness_lm_level_driver(path, C.c_longlong(nc), C.c_longlong(npnt), maxit, sweeps, C.c_double(pct), C.c_double(seppct), model, batch,
                                   detail, C.c_double(single_min), v(out), v(tr), C.c_longlong(len(tr)), v(x))
    assert rc == 0, rc
    assert out[4] <= len(tr)
    return out, tr[:int(out[4])].copy(), x


def _cpp_lists(h, path, nc, npnt, pct, seppct):
    h.harness_lm_plan_lists.restype = C.c_longlong
    cap = 1 << 20
    buf = np.zeros(cap, dtype=np.int64)
    n = h.harness_lm_plan_lists(path, C.c_longlong(nc), C.c_longlong(npnt), C.c_double(pct), C.c_double(seppct), v(buf), C.c_longlong(cap))
    assert n > 0, n
    pos = [0]

    def take(k=None):
        if k is None:
            val = int(buf[pos[0]]); pos[0] += 1
            return val
        val = buf[pos[0]:pos[0] + k].copy(); pos[0] += k
        return val
    plans = []
    for _ in range(take()):
        depth, kind, nc_ = take(), take(), take()
        fp = take(nc_ + 1); fv = take(take()); cp = take(nc_ + 1); ci = take(take())
        plans.append((depth, kind, fp, fv, cp, ci))
    assert pos[0] == n
    return plans


def _route(pp, fv, nfac, single_min):
    """rdis_amd/host/lm_routing.h (tests/test_lm_levels_cpu.py pins the rule): True = a call of its own"""
    cams = len(np.unique(fv[fv < int(pp.pt_vid0.min())] // 9))
    return cams > capi.LM_WIDE_MAX_CAMERAS or (single_min > 0 and nfac >= single_min)


class _Launch:
    """one launch of a sweep as the driver runs it: a resident LmPlan for the components routed to it, the others one by one"""

    def __init__(self, g, pp, lists, model, single_min):
        self.g, self.model = g, model
        _d, _k, fp, fv, cp, ci = lists
        single = [_route(pp, fv[fp[c]:fp[c + 1]], int(cp[c + 1] - cp[c]), single_min) for c in range(len(fp) - 1)]
        self.singles = [(fv[fp[c]:fp[c + 1]], ci[cp[c]:cp[c + 1]]) for c in range(len(fp) - 1) if single[c]]
        keep = [c for c in range(len(fp) - 1) if not single[c]]
        self.plan = None
        if keep:
            vs, fs = [fv[fp[c]:fp[c + 1]] for c in keep], [ci[cp[c]:cp[c + 1]] for c in keep]
            self.plan = capi.LmPlan(g, np.concatenate([[0], np.cumsum([len(a) for a in vs])]), np.concatenate(vs),
                                    np.concatenate([[0], np.cumsum([len(a) for a in fs])]), np.concatenate(fs), model=model, history=1, wide=True)

    def step(self, maxit):
        """(sum of deltas, iterations) in the driver's order: the plan's summary, then the singles in list order"""
        if self.plan is not None:
            self.plan.solve(maxit, FTOL)
        rs = [self.g.lm_optimize(fv, fc, x=None, maxiters=maxit, ftol=FTOL, model=self.model) for fv, fc in self.singles]
        s = self.plan.summary() if self.plan is not None else np.zeros(16)
        dsum, iters = s[1], int(s[2])
        for r in rs:
            dsum = dsum + r.delta
            iters += r.iters
        return dsum, iters


def _replay(gctx, pp, plans, model, maxit, sweeps, single_min=0.0):
    g = capi.Problem(gctx, pp)
    launches = [_Launch(g, pp, lists, model, single_min) for lists in plans]
    every = np.arange(pp.nfac, dtype=np.int64)                      # (the factor list OptimizableFunction::eval hands over)
    f0 = g.eval(every)
    objective, steps, done = f0, [], 0
    for _ in range(sweeps):
        before = objective
        for L in launches:
            dsum, iters = L.step(maxit)
            objective = objective + dsum
            steps.append((objective, iters))
        done += 1
        if not (before - objective > STEPTOL):
            break
    return f0, steps, done, g.get_x(), g.eval(every), sum(len(L.singles) for L in launches)


def _check_against_replay(out, tr, x, rep, nplans):
    f0, steps, done, xr, fend, _ = rep
    assert out[1] == f0 and out[2] == done and out[3] == nplans and len(tr) == len(steps) == done * nplans
    for i, (obj, iters) in enumerate(steps):
        assert tr[i, 7] == obj and tr[i, 6] == iters, (i, tr[i, 7], obj, tr[i, 6], iters)
    assert x.tobytes() == xr.tobytes()
    assert out[0] == fend
    objs = np.concatenate([[f0], tr[:, 7]])
    assert np.all(np.diff(objs) <= 0)                                # non-increasing step by step
    assert abs(out[0] - tr[-1, 7]) <= len(tr) * 1e-12 * f0            # the running sum is the function value
    assert np.all(tr[:, 10] == 0) and np.all(tr[:, 11] == 0)         # nothing ended with invalid values


LEVEL_CASES = ["ladybug-5-30", "ladybug-8-30", "ladybug-20-120", "ladybug-20-120-pieces"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", LEVEL_CASES)
@pytest.mark.parametrize("model", [1, 2])
def test_sweeps_equal_the_hand_built_alternation(name, model, harness, bal_path, gctx):
    (_, nc, npnt), pct, seppct = K.CASES[name]
    pp = K.problem(name)
    plans = _cpp_lists(harness, bal_path, nc, npnt, pct, seppct)
    want = K.plans(name)                                             # (tests/test_host_dropin.py pins planLists to oracle/levels.py)
    assert len(plans) == len(want) and all(np.array_equal(a[3], b[4]) and np.array_equal(a[5], b[6]) for a, b in zip(plans, want))
    out, tr, x = _driver(harness, bal_path, nc, npnt, pp.nvars, 5, 3, pct, seppct, model)
    rep = _replay(gctx, pp, plans, model, 5, 3)
    print("%s, model %d: %.6f -> %.6f in %d sweep(s), %d launches" % (name, model, out[1], out[0], out[2], len(tr)))
    _check_against_replay(out, tr, x, rep, len(plans))
    assert np.all(tr[:, 8] == 0) and out[0] < out[1]
    if name == "ladybug-20-120-pieces":
        assert len(plans) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ladybug-5-30", "ladybug-20-120"])
def test_step_detail_changes_no_bit(name, harness, bal_path):
    (_, nc, npnt), pct, seppct = K.CASES[name]
    nvars = K.problem(name).nvars
    a = _driver(harness, bal_path, nc, npnt, nvars, 5, 3, pct, seppct, 1, detail=0)
    b = _driver(harness, bal_path, nc, npnt, nvars, 5, 3, pct, seppct, 1, detail=1)
    assert a[0][:5].tobytes() == b[0][:5].tobytes()
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()      # every step's record (no wall time in it), all of x


@pytest.mark.gpu
def test_unbatched_run_equals_one_call_per_component(harness, bal_path, gctx):
    """batch = 0: one HipLMSubspaceOptimizer::optimize -- rdis_hip_lm_optimize -- per component, in list order"""
    pp = K.problem("ladybug-5-30")
    plans = _cpp_lists(harness, bal_path, 5, 30, 0.2, 0.0)
    out, tr, x = _driver(harness, bal_path, 5, 30, pp.nvars, 5, 3, batch=0)
    g = capi.Problem(gctx, pp)
    every = np.arange(pp.nfac, dtype=np.int64)
    f0 = g.eval(every)
    objective, steps, done = f0, [], 0
    for _ in range(3):
        before = objective
        for _d, _k, fp, fv, cp, ci in plans:
            dsum, iters = 0.0, 0
            for c in range(len(fp) - 1):
                r = g.lm_optimize(fv[fp[c]:fp[c + 1]], ci[cp[c]:cp[c + 1]], x=None, maxiters=5, ftol=FTOL, model=1)
                dsum, iters = dsum + r.delta, iters + r.iters
            objective = objective + dsum
            steps.append((objective, iters))
        done += 1
        if not (before - objective > STEPTOL):
            break
    assert out[1] == f0 and out[2] == done and len(tr) == len(steps)
    assert [(t[7], t[6]) for t in tr] == steps
    assert x.tobytes() == g.get_x().tobytes() and out[0] == g.eval(every)


@pytest.mark.gpu
def test_a_separator_beyond_64_cameras_goes_the_single_call_way(harness, tmp_path, bal_path, gctx):
    name = "synthetic-160-400"
    pp = K.problem(name)
    path = str(tmp_path / "synthetic_160_400.txt")
    P.save_bal(pp, path)
    path = path.encode()
    plans = _cpp_lists(harness, path, 0, 0, 0.2, 0.0)
    want = K.plans(name)
    assert len(plans) == len(want) == 2 and all(np.array_equal(a[3], b[4]) and np.array_equal(a[5], b[6]) for a, b in zip(plans, want))
    out, tr, x = _driver(harness, path, 0, 0, pp.nvars, 3, 1)
    rep = _replay(gctx, pp, plans, 1, 3, 1)
    _check_against_replay(out, tr, x, rep, 2)
    assert rep[5] == 1 and tr[:, 8].tolist() == [1.0, 0.0]           # exactly one component: the 89-camera separator
    # ... and by option: a threshold at the separator's factor count sends ladybug 5/30's separator away, and only it
    lb = K.problem("ladybug-5-30")
    for t, singles in ((121.0, [1.0, 0.0]), (122.0, [0.0, 0.0])):
        out, tr, x = _driver(harness, bal_path, 5, 30, lb.nvars, 5, 1, single_min=t)
        rep = _replay(gctx, lb, _cpp_lists(harness, bal_path, 5, 30, 0.2, 0.0), 1, 5, 1, single_min=t)
        _check_against_replay(out, tr, x, rep, 2)
        assert tr[:, 8].tolist() == singles


# ---- optimizeBatch on its own -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("model", [1, 2])
def test_optimize_batch_equals_lm_batch_and_hits_the_plan_cache(model, harness, bal_path, gctx):
    pp = K.problem("ladybug-5-30")
    plans = _cpp_lists(harness, bal_path, 5, 30, 0.2, 0.0)
    ncomp = sum(len(p[2]) - 1 for p in plans)
    assert [len(p[2]) - 1 for p in plans] == [1, 29]
    out, res, xs = np.zeros(7), np.zeros((2 * ncomp, 6)), np.zeros(2 * pp.nvars)
    assert harness.harness_lm_optimize_batch(bal_path, C.c_longlong(5), C.c_longlong(30), 5, model, 8, 2, v(out), v(res), C.c_longlong(len(res)), v(xs),
                                             C.c_longlong(len(xs))) == 0
    assert out[0] == 4 and out[1] == 2 * ncomp and out[5] == 0
    assert (out[2], out[3], out[4]) == (2, 2, 2)                     # the second round's two calls found the first round's plans
    g = capi.Problem(gctx, pp)
    row, xpos, total = 0, 0, 0.0
    for _ in range(2):
        for _d, _k, fp, fv, cp, ci in plans:
            rs = g.lm_batch(fp, fv, cp, ci, x=g.get_x(fv), maxiters=5, ftol=FTOL, model=model, wide=True)
            part = 0.0
            for r in rs:
                assert (res[row, 0], res[row, 1], res[row, 2], res[row, 3], res[row, 4], res[row, 5]) == (r.fret, r.delta, r.iters, r.stop, r.nfev, r.njev)
                assert xs[xpos:xpos + len(r.x)].tobytes() == r.x.tobytes()
                part += r.fret
                row, xpos = row + 1, xpos + len(r.x)
            total += part
    assert out[6] == total
    # the cache switched off: the same bits, no entry kept
    out0, res0, xs0 = np.zeros(7), np.zeros_like(res), np.zeros_like(xs)
    assert harness.harness_lm_optimize_batch(bal_path, C.c_longlong(5), C.c_longlong(30), 5, model, 0, 2, v(out0), v(res0), C.c_longlong(len(res0)), v(xs0),
                                             C.c_longlong(len(xs0))) == 0
    assert res0.tobytes() == res.tobytes() and xs0.tobytes() == xs.tobytes() and out0[4] == 0 and out0[2] == 0
    assert harness.harness_lm_refuses_several_devices(bal_path) == 1


# ---- schedule 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_schedule_with_levenberg_marquardt(harness, bal_path):
    """the checker call of tests/test_host_dropin.py::test_reference_schedule_of_the_level_driver on the run useCGD = 0 makes"""
    nc, npnt, pct, seppct, nrr, maxna, steptol = 5, 30, 0.2, 0.0, 2, 10, 1e-2
    pp = K.problem("ladybug-5-30")
    nodes = LV.build_tree(pp, O.OracleProblem(pp), blkpct=pct, seppct=seppct)
    slo, shi = LV.ba_sampling_intervals(pp, nc)
    out, tr, x = np.zeros(7), np.zeros((300000, 10)), np.zeros(pp.nvars)
    harness.harness_lm_level_reference.restype = C.c_longlong
    n = harness.harness_lm_level_reference(bal_path, C.c_longlong(nc), C.c_longlong(npnt), 25, 1, C.c_double(pct), C.c_double(seppct), nrr, maxna,
                                           C.c_double(12345.0), C.c_double(300000.0), C.c_double(steptol), v(out), v(tr), C.c_longlong(len(tr)), v(x))
    assert 0 < n < len(tr) and out[2] == len(nodes)
    tr = tr[:n]
    rows = [tuple(r[:8]) + (int(r[8]) << 32 | int(r[9]),) for r in tr]
    calls = LV.replay_reference_schedule(nodes, rows, pp, slo, shi, steptol=steptol, nrr_per_lvl=nrr, max_na_to_rr=maxna, seed=12345, max_calls=300000)
    kinds = np.bincount(tr[:, 1].astype(int), minlength=3)
    print("reference schedule with Levenberg-Marquardt, 5 cameras / 30 points: %d calls (%d initial, %d iterative improvement, %d random restarts) in %d "
          "launches, %d iterations, %d residual evaluations, %.6f -> %.6f" % (calls, kinds[0], kinds[1], kinds[2], out[6], out[4], out[5], out[1], out[0]))
    assert calls == len(tr)                                          # consumed to the last record, no mismatch on the way
    assert out[0] <= out[1] and out[4] > 0 and out[5] >= out[4] and 0 < out[6] < calls
    o = O.OracleProblem(pp)
    o.assign(np.arange(pp.nvars, dtype=np.int64), x)
    assert abs(o.eval() - out[0]) <= 1e-10 * abs(out[0])


# ---- the C entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_optba_entry_takes_the_switch(harness, bal_path):
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                   C.c_int32, C.c_void_p, C.c_void_p]

    def run(schedule, opts, x=None):
        names, vals = [k.encode() for k in opts], list(opts.values())
        out = np.zeros(10)
        rc = lib.rdis_optba_run(bal_path, 5, 30, schedule, len(names), (C.c_char_p * len(names))(*names), (C.c_double * len(vals))(*vals), 0, v(out),
                                None if x is None else v(x))
        return rc, out
    for model in (1, 2):
        x = np.zeros(135)
        rc, out = run(0, {"SSmaxit": 5.0, "maxSweeps": 3.0, "useCGD": 0.0, "LMmodel": float(model)}, x)
        assert rc == 0
        ho, tr, hx = _driver(harness, bal_path, 5, 30, 135, 5, 3, model=model)
        assert out[0] == ho[0] and out[1] == ho[1] and x.tobytes() == hx.tobytes()
        assert out[3] == tr[:, 6].sum() and out[8] == tr[:, 9].sum() and out[2] == tr[:, 3].sum() and out[4] == len(tr) and out[9] == ho[2]
        assert out[8] >= out[3] > 0
    # useCGD 1 is the run without the option
    rc1, a = run(0, {"SSmaxit": 5.0, "maxSweeps": 2.0, "useCGD": 1.0})
    rc2, b = run(0, {"SSmaxit": 5.0, "maxSweeps": 2.0})
    assert rc1 == rc2 == 0 and a[[0, 1, 2, 3, 4, 7, 8, 9]].tobytes() == b[[0, 1, 2, 3, 4, 7, 8, 9]].tobytes()
    # schedule 1 through the entry: LM iterations and residual evaluations
    rc, out = run(1, {"SSmaxit": 25.0, "steptol": 1e-2, "restartSeed": 12345.0, "useCGD": 0.0})
    assert rc == 0 and out[0] <= out[1] and out[3] > 0 and out[8] >= out[3] and out[2] == out[9] > 0
    for bad in ({"useCGD": 0.5}, {"useCGD": 2.0}, {"useCGD": 0.0, "LMmodel": 3.0}, {"useCGD": 0.0, "LMmodel": 1.5}, {"useCGD": 0.0, "LMsingleMinFactors": -1.0},
                {"useCGD": 0.0, "LMsingleMinFactors": 2.5}):
        assert run(0, bad)[0] == -3, bad
