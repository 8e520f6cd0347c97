"""Every exit of the Levenberg-Marquardt solvers, not only the iteration limit (tests/lm_exit_cases.py; the oracle's side is
pinned by tests/test_lm_exits_cpu.py), through every entry: Problem.lm_optimize (rdis_hip_lm_optimize: the host loop of
lm_solver.hip), Problem.lm_batch (the four classes of k_lm_batch), LmPlan.solve + fetch, LmPlan.solve_population with 3 members
of which member 1 holds the case, and LmPlan.solve_starts with 4 starts of which start 2 holds it.

  exact       stop, iterations and the counters equal the oracle's; history, x and fret by test_gpu_lm_batch._compare
  converged   stop 2 or 5 before the iteration limit; fret within 1e-8, x within 1e-7, the history up to the convergence point
  zero        one-observation points: no reference exists (test_lm_exits_cpu), properties only
  nonfinite   the contract of include/rdis_hip.h: a start whose objective is not finite ends with code 7 before anything is
              linearised, a NaN coordinate stays NaN, nobody else in the call notices

Every result of every test passes lm_exit_cases.check_identities; nfail (linear solves whose factorisation was refused) is
printed per case and entry: no finite case here reaches one."""
import math

import numpy as np
import pytest

from rdis_amd import capi

import lm_batch_shapes as S
import lm_exit_cases as E
import lm_starts_cases as K
from test_gpu_lm_batch import _compare, _deviations, _same

pytestmark = pytest.mark.gpu

HIST = 256            # history records fetched per component, by every entry: more than any case's linear solves
SEQUENTIAL = 3        # components of a case that are also solved one at a time by lm_optimize


def _same_nan(a, b):
    """_same for results that may hold NaN"""
    fa = np.array([a.fret, a.delta, a.mu, a.iters, a.stop, a.nfev, a.njev, a.nsolve, a.camera_blocks, a.point_blocks], dtype=np.float64)
    fb = np.array([b.fret, b.delta, b.mu, b.iters, b.stop, b.nfev, b.njev, b.nsolve, b.camera_blocks, b.point_blocks], dtype=np.float64)
    return (np.array_equal(fa, fb, equal_nan=True) and a.history.tobytes() == b.history.tobytes() and
            np.array_equal(a.x, b.x, equal_nan=True))


def _clamp(pp, vid, x):
    return np.minimum(np.maximum(x, pp.lo[vid]), pp.hi[vid])


def _problem(gctx, pp, x):
    g = capi.Problem(gctx, pp)
    g.set_x(x)
    return g


def _batch(gctx, c, x=None, comps=None):
    comps = c.comps if comps is None else comps
    g = _problem(gctx, c.pp, c.x if x is None else x)
    return g, g.lm_batch(*S.csr(comps), maxiters=c.maxiters, ftol=c.ftol, history=HIST, model=c.model, wide=c.wide)


def _plan(g, c):
    return capi.LmPlan(g, *S.csr(c.comps), model=c.model, history=HIST, wide=c.wide)


def _others(c, n):
    """n ordinary complete states for the other members / starts: the case's x -- a poisoned component's free variables
    replaced by the problem's -- with every component's free variables moved by about 1e-3 (lm_plan_members.members_of's rule)"""
    base = np.array(c.x)
    if c.kind == "nonfinite":
        for k in c.stop:
            base[c.comps[k][0]] = c.pp.x0[c.comps[k][0]]
    X = np.tile(base, (n, 1))
    for s in range(n):
        rng = np.random.default_rng(2000 + s)
        for free, _ in c.comps:
            X[s, free] = base[free] + 1e-3 * (1.0 + np.abs(base[free])) * rng.standard_normal(len(free))
    return np.clip(X, c.pp.lo, c.pp.hi)


def _entries(gctx, c, sequential=True):
    """{entry: results of the case's components} -- the case solved through every entry; lm_optimize: the first SEQUENTIAL
    components, where the problem lays its cameras out first (all but the two-block problem of unread/wide-block)"""
    fv = S.csr(c.comps)[1]
    out = {}
    out["lm_batch"] = _batch(gctx, c)[1]
    g = _problem(gctx, c.pp, c.x)
    plan = _plan(g, c)
    plan.solve(c.maxiters, c.ftol)
    out["plan.solve"] = plan.fetch()
    oth = _others(c, 3)
    pop = capi.Population(g, x=np.stack([oth[0], c.x, oth[1]]))
    plan.solve_population(pop, maxiters=c.maxiters, ftol=c.ftol)
    out["plan.solve_population"] = plan.fetch_population()[1]
    g.set_x(c.x)
    plan.solve_starts(np.stack([oth[0], oth[1], c.x, oth[2]])[:, fv], c.maxiters, c.ftol)
    out["plan.solve_starts"] = plan.fetch_starts()[0][2]
    if sequential and np.max(c.pp.cam_vid0) < np.min(c.pp.pt_vid0):        # cameras first: what rdis_hip_lm_optimize requires
        rs = []
        for free, fac in c.comps[:SEQUENTIAL]:
            rs.append(_problem(gctx, c.pp, c.x).lm_optimize(free, fac, maxiters=c.maxiters, ftol=c.ftol, history=HIST, model=c.model))
        out["lm_optimize"] = rs
    return out


def _report(c, entry, rs, ref):
    nfail = [E.check_identities(r, ro.finit, HIST) for r, ro in zip(rs, ref)]
    worst = np.max([_deviations(r, ro) for r, ro in zip(rs, ref)], axis=0)
    print("LM exits %s, %s, %d components against the oracle: exits (stop, iterations) %s, nfail %d; history %.1e, x %.1e, fret %.1e" % (
        (c.name, entry, len(rs), sorted(set((r.stop, r.iters) for r in rs)), max(nfail)) + tuple(worst)))
    return nfail


# ---- cases 1 and 2: exits decided far from rounding -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.EXACT_NAMES)
def test_exact_exits_equal_the_oracle(name, gctx):
    """small error (6) after at least one accepted step, small gradient (1) at iteration 0, and a free camera block that no
    listed factor reads beside active ones"""
    c = E.case(name)
    ref = E.oracle_reference(name)
    for entry, rs in _entries(gctx, c).items():
        ref_e = ref[:len(rs)]
        assert len(rs) == len(ref_e)
        _report(c, entry, rs, ref_e)
        for k, (r, ro) in enumerate(zip(rs, ref_e)):
            free = c.comps[k][0]
            assert (r.stop, r.iters, r.nsolve, r.nfev, r.njev, len(r.history)) == (ro.stop, ro.iters, ro.nsolve, ro.nfev, ro.njev, len(ro.history)), entry
            _compare(r, ro, cap=HIST)
            if k in c.stop:
                assert r.stop == c.stop[k], entry
            if r.stop == 6:
                assert r.iters >= 1
            if r.stop == 1:         # nothing was solved: the start comes back clamped, bit for bit, and fret is the start's value
                assert (r.iters, r.njev, r.nsolve, r.nfev, len(r.history)) == (0, 1, 0, 1, 0), entry
                assert r.x.tobytes() == _clamp(c.pp, free, c.x[free]).tobytes() and r.delta == 0.0, entry
        if name.startswith("idle/"):
            idle = E.idle_block(name)
            at = np.isin(c.comps[0][0], idle)
            assert int(np.sum(at)) == 9 and rs[0].x[at].tobytes() == c.x[idle].tobytes(), entry     # the idle block: the same bytes


# ---- case 3: converged runs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.CONVERGED_NAMES)
def test_converged_runs_stop_with_a_small_step(name, gctx):
    """stop 2 (or 5) with the iteration limit at least four times away; fret to 1e-8 of the oracle's, x to 1e-7 (_compare's
    bounds).  The history is compared with _compare's criteria (the same decisions; mu, |Dp|^2, f(trial) to 1e-7) over the
    records the oracle itself reproduces to 1e-9 under one-ulp changes of its start (lm_exit_cases.stable_history): near a
    converged point the gain ratio is rounding, and the oracle's own later records move by up to 2e-3 (test_lm_exits_cpu
    prints the counts).  From the problem's start (converged/points) that is nearly all of them, and _compare runs as it is."""
    c = E.case(name)
    ref = E.oracle_reference(name)
    stable = E.stable_history(name)
    for entry, rs in _entries(gctx, c).items():
        ref_e = ref[:len(rs)]
        assert len(rs) == len(ref_e)
        _report(c, entry, rs, ref_e)
        for r, ro, n in zip(rs, ref_e, stable):
            assert r.stop in (2, 5) and r.iters < c.maxiters, (entry, r.stop, r.iters)
            assert n <= len(r.history) < HIST
            for (mu, dp, ft, ok), (omu, odp, oft, ook) in list(zip(r.history, ro.history))[:n]:
                assert bool(ok) == bool(ook), entry
                assert abs(mu - omu) <= 1e-7 * omu and abs(dp - odp) <= 1e-7 * odp and abs(ft - oft) <= 1e-7 * abs(oft), entry
            assert abs(r.fret - ro.fret) <= 1e-8 * abs(ro.fret), entry
            assert np.max(np.abs(r.x - ro.x)) <= 1e-7 * (1.0 + np.max(np.abs(ro.x))), entry
            if name == "converged/points":
                _compare(r, ro, cap=HIST)
    print("LM exits %s: history records compared %d of %d" % (name, sum(stable), sum(len(ro.history) for ro in ref)))


def test_one_observation_points_reach_zero(gctx):
    """two residuals, three unknowns, ftol 0: the minimum is 0 and what the oracle returns there is rounding (tests/
    test_lm_exits_cpu.py), so: the identities, a stop by small step, by refused steps or at an exact 0, well inside the iteration
    limit, and a value below 1e-20 of the start's -- at stop 2 the step is below 1e-15 |x|, which leaves a residual of some
    1e-13 pixels, a value of 1e-25; the bound is 1e5 times that"""
    c = E.case(E.ZERO_NAMES[0])
    for entry, rs in _entries(gctx, c).items():
        stops = set()
        for r in rs:
            E.check_identities(r, cap=HIST)
            finit = r.fret - r.delta
            stops.add(r.stop)
            assert r.stop in (2, 5, 6) and 2 * r.iters < c.maxiters and 0.0 <= r.fret <= 1e-20 * finit, (entry, r.stop, r.iters, r.fret)
        print("LM exits %s, %s, %d components: stops %s, largest fret %.1e" % (c.name, entry, len(rs), sorted(stops), max(r.fret for r in rs)))


# ---- case 4: starts whose objective is not finite -------------------------------------------------------------------------------------
def _check_contract(c, k, r, name):
    """component k of the case, result r: code 7 before any linearisation, fret not finite, NaN stays NaN, the rest clamped"""
    free = c.comps[k][0]
    E.check_identities(r, cap=HIST)
    assert (r.stop, r.iters, r.njev, r.nsolve, r.nfev, len(r.history)) == (7, 0, 0, 0, 1, 0), (name, r)
    assert not math.isfinite(r.fret), (name, r.fret)
    start = c.x[free]
    nan = np.isnan(start)
    assert np.array_equal(np.isnan(r.x), nan), (name, r.x)
    assert r.x[~nan].tobytes() == _clamp(c.pp, free, start)[~nan].tobytes(), name


@pytest.mark.parametrize("name", E.NONFINITE_NAMES)
def test_nonfinite_start_in_a_batch_of_every_class(name, gctx):
    """lm_batch on the mixed batch (classes 3, 2, 1 and 0 in one call, each at least twice: the poisoned workgroup runs in one
    launch with a healthy one of its class) with one component's start poisoned: the contract for that component; every other
    component equals, with ==, what the call without the poisoned one returns, in both orders of the batch; no variable outside
    the component differs from that call's by a byte"""
    c = E.case(name)
    (k, _), = c.stop.items()
    ncomp = len(c.comps)
    g, rs = _batch(gctx, c)
    after = g.get_x()
    _check_contract(c, k, rs[k], name)
    rest = [j for j in range(ncomp) if j != k]
    gb, rb = _batch(gctx, c, comps=[c.comps[j] for j in rest])
    assert all(_same(rs[j], b) for j, b in zip(rest, rb))
    assert all(r.stop in (2, 3) and math.isfinite(r.fret) for r in rb)
    _, rr = _batch(gctx, c, comps=c.comps[::-1])
    assert all(_same_nan(a, b) for a, b in zip(rs, rr[::-1]))
    free = c.comps[k][0]
    outside = np.setdiff1d(np.arange(c.pp.nvars), free)
    assert after[outside].tobytes() == gb.get_x()[outside].tobytes()
    assert np.array_equal(after[free], rs[k].x, equal_nan=True)
    cls = [0 if r.camera_blocks == 0 else 1 if r.camera_blocks <= 6 else 2 if r.camera_blocks <= 16 else 3 for r in rs]
    classes = sorted(set(cls))
    nfail = [E.check_identities(r, cap=HIST) for r in rs]
    print("LM exits %s, lm_batch: component %d (%d cameras, %d points) stop %d, fret %r; %d neighbours of classes %s unchanged, nfail %d" % (
        name, k, rs[k].camera_blocks, rs[k].point_blocks, rs[k].stop, rs[k].fret, len(rest), classes, max(nfail)))
    assert classes == [0, 1, 2, 3]
    # the poisoned workgroup shares its class's launch with a healthy one
    assert cls.count(cls[k]) >= 2


@pytest.mark.parametrize("name", E.NONFINITE_NAMES)
def test_nonfinite_start_through_the_plans(name, gctx):
    """the same through LmPlan.solve, .solve_population (member 1 of 3 poisoned: members 0 and 2 equal lm_batch on their own x)
    and .solve_starts (start 2 of 4 poisoned in that component alone: never the winner; all four poisoned: best is 0)"""
    c = E.case(name)
    (k, _), = c.stop.items()
    fp, fv, jp, fj = S.csr(c.comps)
    free = c.comps[k][0]
    _, rs = _batch(gctx, c)
    g = _problem(gctx, c.pp, c.x)
    plan = _plan(g, c)
    plan.solve(c.maxiters, c.ftol)
    got = plan.fetch()
    _check_contract(c, k, got[k], name)
    assert all(_same_nan(a, b) for a, b in zip(got, rs))
    assert math.isnan(plan.objective()) or math.isinf(plan.objective())

    oth = _others(c, 3)
    X = np.stack([oth[0], c.x, oth[1]])
    pop = capi.Population(g, x=X)
    plan.solve_population(pop, maxiters=c.maxiters, ftol=c.ftol)
    rows = plan.fetch_population()
    _check_contract(c, k, rows[1][k], name)
    assert all(_same_nan(a, b) for a, b in zip(rows[1], rs))
    for s in (0, 2):
        want = _batch(gctx, c, x=X[s])[1]
        assert all(_same(a, b) for a, b in zip(rows[s], want)) and all(math.isfinite(r.fret) for r in want), s
    px = pop.get_x()
    outside = np.setdiff1d(np.arange(c.pp.nvars), fv)
    assert px[:, outside].tobytes() == X[:, outside].tobytes()
    assert np.array_equal(px[1, free], rs[k].x, equal_nan=True)

    # four starts; start 2 holds the poisoned values in component k alone (its other components: an ordinary start)
    g.set_x(c.x)
    base = g.get_x()
    Y = _others(c, 4)
    Y[2, free] = c.x[free]
    const = np.setdiff1d(np.arange(c.pp.nvars), fv)
    Y[:, const] = c.x[const]
    plan.solve_starts(Y[:, fv], c.maxiters, c.ftol)
    srows, best = plan.fetch_starts()
    _check_contract(c, k, srows[2][k], name)
    refs = [_batch(gctx, c, x=Y[s])[1] for s in range(4)]
    for s in range(4):
        assert all(_same_nan(a, b) for a, b in zip(srows[s], refs[s])), s
    want = K.select(np.array([[r.fret for r in row] for row in refs]))
    assert np.array_equal(best, want) and best[k] != 2
    winners = plan.fetch()
    assert all(_same(w, srows[best[j]][j]) for j, w in enumerate(winners))
    fret = [w.fret for w in winners]
    assert abs(plan.objective() - math.fsum(fret)) <= len(fret) * 2.0 ** -52 * math.fsum(abs(f) for f in fret)
    x = g.get_x()
    assert x[const].tobytes() == base[const].tobytes() and np.all(np.isfinite(x))
    assert x[fv].tobytes() == np.concatenate([w.x for w in winners]).tobytes()
    if "/nan-" in name:
        # all four starts poisoned in component k: a column of NaN, best is 0
        Z = Y.copy()
        Z[:, free] = np.where(np.isnan(c.x[free])[None, :], np.nan, Y[:, free])
        g.set_x(c.x)
        plan.solve_starts(Z[:, fv], c.maxiters, c.ftol)
        zrows, zbest = plan.fetch_starts()
        assert all(math.isnan(zrows[s][k].fret) and zrows[s][k].stop == 7 for s in range(4))
        assert zbest[k] == 0 and np.array_equal(np.delete(zbest, k), np.delete(best, k))
        assert math.isnan(plan.objective())
    print("LM exits %s, plans: solve, population member 1 of 3, start 2 of 4: stop 7; best %s of component %d" % (name, best[k], k))


@pytest.mark.parametrize("name", E.NONFINITE_SEQUENTIAL_NAMES)
def test_nonfinite_start_through_the_sequential_entry(name, gctx):
    """rdis_hip_lm_optimize and lm_batch on one component of ladybug: the same contract, the same record; nothing outside the
    component changes"""
    c = E.case(name)
    free, fac = c.comps[0]
    g = _problem(gctx, c.pp, c.x)
    before = g.get_x()
    r = g.lm_optimize(free, fac, maxiters=c.maxiters, ftol=c.ftol, history=HIST, model=c.model)
    _check_contract(c, 0, r, name)
    after = g.get_x()
    outside = np.setdiff1d(np.arange(c.pp.nvars), free)
    assert after[outside].tobytes() == before[outside].tobytes() and np.array_equal(after[free], r.x, equal_nan=True)
    _, rb = _batch(gctx, c)
    _check_contract(c, 0, rb[0], name)
    assert (r.stop, r.iters, r.nfev, r.njev, r.nsolve) == (rb[0].stop, rb[0].iters, rb[0].nfev, rb[0].njev, rb[0].nsolve)
    assert np.array_equal(r.x, rb[0].x, equal_nan=True)
    print("LM exits %s: lm_optimize stop %d, fret %r; lm_batch stop %d, fret %r" % (name, r.stop, r.fret, rb[0].stop, rb[0].fret))
