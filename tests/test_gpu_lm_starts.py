"""Multi-start solves of Levenberg-Marquardt plans (rdis_hip_lm_plan_solve_starts, rdis_hip_lm_plan_solve_starts_population;
capi.LmPlan.solve_starts): every component solved from each of S rows of start values on scratch rows of x, the problem left at
the best start per component.  The yardstick is rdis_hip_lm_batch on a fresh problem whose x is the start, as in
tests/test_gpu_lm_plan.py: every (start, component) must equal it with == -- every field, the history's and x's bytes -- and
the winners, the problem's x afterwards and the plan's ordinary outputs must be what the select rule, written with numpy, makes
of those results.  tests/test_lm_starts_cpu.py pins that the starts discriminate (distinct winners, no near ties) and checks the
rule's NaN cases; tests/test_gpu_lm_exits.py feeds them on the device (one NaN start among four, and all four)."""
import math

import numpy as np
import pytest

from rdis_amd import capi

import lm_batch_shapes as S
import lm_starts_cases as K
import lm_wide_shapes as W
from test_gpu_lm_batch import _same

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -5


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _plan(g, comps, model, history=64, wide=False):
    return capi.LmPlan(g, *S.csr(comps), model=model, history=history, wide=wide)


_REFS = {}


def _refs(gctx, key, pp, comps, X, iters, model, wide=False):
    """the yardstick, once per case: for every row of X, lm_batch on a fresh problem whose x is the problem's with the components'
    free variables from that row -> [(results per component, the whole x afterwards)]"""
    if key not in _REFS:
        fv = S.csr(comps)[1]
        out = []
        for s in range(len(X)):
            g = capi.Problem(gctx, pp)
            g.set_x(X[s, fv], vid=fv)
            out.append((g.lm_batch(*S.csr(comps), maxiters=iters, model=model, history=64, wide=wide), g.get_x()))
        _REFS[key] = out
    return _REFS[key]


def _expected_x(base, comps, refs, best):
    x = base.copy()
    for c, (free, _) in enumerate(comps):
        x[free] = refs[best[c]][1][free]
    return x


def _check_against(refs, comps, g, base, plan, rows, best):
    """everything section 1 asks of a finished multi-start solve"""
    assert len(rows) == len(refs)
    for s, (ref, _) in enumerate(refs):
        assert _all_same(rows[s], ref), "start %d" % s
    want = K.select(np.array([[r.fret for r in ref] for ref, _ in refs]))
    assert best.dtype == np.int32 and np.array_equal(best, want)
    assert g.get_x().tobytes() == _expected_x(base, comps, refs, best).tobytes()
    winners = plan.fetch()
    assert _all_same(winners, [rows[best[c]][c] for c in range(len(comps))])
    fv = S.csr(comps)[1]
    assert np.concatenate([r.x for r in winners]).tobytes() == g.get_x()[fv].tobytes()     # fetch's x is what was left assigned


# ---- 1. every row is lm_batch; the winners, x and the ordinary outputs follow from the rows ----------------------------------------
ROW_NAMES = ["ladybug-5-30-points", "ladybug-5-30-cameras", "ladybug-5-30-sub-block", "synthetic-2x16x60"]


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("name", ROW_NAMES)
def test_every_row_equals_lm_batch(name, model, gctx):
    """classes 0, 1, 1 with free variables inside a camera block next to constants, and 2; six starts.  On every shape of more than
    one component at least two distinct winners occur; with model 1 they are the oracle's (tests/test_lm_starts_cpu.py: gaps of
    1.6e-4 and more, against frets that agree to 1e-8)"""
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fv = S.csr(comps)[1]
    refs = _refs(gctx, (name, model), pp, comps, X, iters, model)
    g = capi.Problem(gctx, pp)
    base = g.get_x()
    plan = _plan(g, comps, model)
    plan.solve_starts(X[:, fv], iters)
    rows, best = plan.fetch_starts()
    _check_against(refs, comps, g, base, plan, rows, best)
    assert plan.info("members_per_launch") == K.NSTARTS
    assert plan.info("launches") == len({0 if r.camera_blocks == 0 else 1 if r.camera_blocks <= 6 else 2 for r in rows[0]})
    assert any(len(r.history) > 0 for r in rows[0])
    print("LM starts %s, model %d: winners %s" % (name, model, np.bincount(best, minlength=K.NSTARTS).tolist()))
    if len(comps) > 1:
        assert len(set(best.tolist())) >= 2
    if model == 1 and name in K.ORACLE_NAMES:
        assert np.array_equal(best, K.select(K.oracle_frets(name, 1)))


# ---- 2. the components listed in reverse: pos is not monotone ---------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("ladybug-5-30-points", 1), ("synthetic-6x3x40", 2)])
def test_component_order_changes_no_bit(name, model, gctx):
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fwd = _refs(gctx, (name, model), pp, comps, X, iters, model)
    rev = comps[::-1]
    fv = S.csr(rev)[1]
    assert np.any(np.diff(fv) < 0)
    g = capi.Problem(gctx, pp)
    base = g.get_x()
    plan = _plan(g, rev, model)
    plan.solve_starts(X[:, fv], iters)
    rows, best = plan.fetch_starts()
    refs = [(ref[::-1], x) for ref, x in fwd]                       # per component the same results, and the same x
    _check_against(refs, rev, g, base, plan, rows, best)
    assert len(set(best.tolist())) >= 2


# ---- 3. the wide class ---------------------------------------------------------------------------------------------------------------
def test_wide_class_rows_equal_wide_lm_batch(gctx):
    name, model = "synthetic-1x17x60", 2
    pp, comps, iters = W.shape(name)[:3]
    X = K.M.members_of(pp, comps, 3)
    fv = S.csr(comps)[1]
    refs = _refs(gctx, (name, model), pp, comps, X, iters, model, wide=True)
    g = capi.Problem(gctx, pp)
    base = g.get_x()
    plan = _plan(g, comps, model, wide=True)
    plan.solve_starts(X[:, fv], iters)
    rows, best = plan.fetch_starts()
    _check_against(refs, comps, g, base, plan, rows, best)
    assert rows[0][0].camera_blocks == 17 and plan.info("launches") == 1 and plan.info("members_per_launch") == 3


# ---- 4. launch splitting ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synthetic-2x16x60", "ladybug-5-30-points"])
def test_the_split_into_rounds_changes_no_bit(name, gctx):
    """workspace_bytes for one, two and all of five starts a launch (the last round of two is smaller); a start is charged its
    workspace slices and its row of x"""
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)[:5]
    fv = S.csr(comps)[1]
    g = capi.Problem(gctx, pp)
    base = g.get_x()
    plan = _plan(g, comps, 2)
    sb = plan.info("member_workspace_bytes") + 8 * pp.nvars
    classes = 1
    seen = []
    for budget, per in ((0, 1), (sb - 1, 1), (2 * sb, 2), (3 * sb - 1, 2), (5 * sb - 1, 4), (5 * sb, 5), (1 << 30, 5)):
        plan.set_option("workspace_bytes", budget)
        g.set_x(base)
        plan.solve_starts(X[:, fv], iters)
        assert plan.info("members_per_launch") == per and plan.info("launches") == classes * ((5 + per - 1) // per)
        rows, best = plan.fetch_starts()
        seen.append((rows, best.tobytes(), g.get_x().tobytes(), plan.fetch()))
    for rows, bb, xb, win in seen[1:]:
        assert bb == seen[0][1] and xb == seen[0][2] and _all_same(win, seen[0][3])
        assert all(_all_same(a, b) for a, b in zip(rows, seen[0][0]))
    assert xb != base.tobytes() and any(len(r.history) > 0 for r in seen[0][0][4])


# ---- 5. one start; ties ------------------------------------------------------------------------------------------------------------------
def test_one_start_equals_a_plain_solve_from_it(gctx):
    name, model = "synthetic-6x3x40", 2
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fv = S.csr(comps)[1]
    h = capi.Problem(gctx, pp)
    h.set_x(X[2, fv], vid=fv)
    ph = _plan(h, comps, model)
    ph.solve(iters)
    want = ph.fetch()
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, model)
    plan.solve_starts(X[2:3, fv], iters)
    rows, best = plan.fetch_starts()
    assert len(rows) == 1 and np.all(best == 0)
    assert _all_same(rows[0], want) and _all_same(plan.fetch(), want) and g.get_x().tobytes() == h.get_x().tobytes()


def test_a_tie_goes_to_the_lower_index(gctx):
    name, model = "ladybug-5-30-points", 1
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fv = S.csr(comps)[1]
    starts = X[[3, 3, 1, 3, 5], :][:, fv]                            # rows 0, 1 and 3 are one start
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, model)
    plan.solve_starts(starts, iters)
    rows, best = plan.fetch_starts()
    assert _all_same(rows[0], rows[1]) and _all_same(rows[0], rows[3])
    assert not np.any(best == 1) and not np.any(best == 3) and np.any(best == 0) and len(set(best.tolist())) >= 2


# ---- 6. the starts taken from a population ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("ladybug-5-30-points", 1), ("ladybug-5-30-sub-block", 2)])
def test_population_source_equals_host_starts(name, model, gctx):
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fv = S.csr(comps)[1]
    g = capi.Problem(gctx, pp)
    base = g.get_x()
    plan = _plan(g, comps, model)
    plan.solve_starts(X[:, fv], iters)
    rows, best = plan.fetch_starts()
    xs = g.get_x()
    assert xs.tobytes() != base.tobytes()

    g.set_x(base)
    pop = capi.Population(g, x=X)
    f0 = pop.eval()
    m0 = pop.best()
    plan.solve_starts_population(pop, maxiters=iters)
    rows2, best2 = plan.fetch_starts()
    assert all(_all_same(a, b) for a, b in zip(rows2, rows)) and best2.tobytes() == best.tobytes() and g.get_x().tobytes() == xs.tobytes()
    assert pop.get_x().tobytes() == X.tobytes()                      # the population is only read ...
    assert pop.info("eval_valid") == 1 and pop.best() == m0 and m0[1] == np.min(f0)   # ... and still answers from its last evaluation

    # a member range
    g.set_x(base)
    plan.solve_starts_population(pop, first=1, count=3, maxiters=iters)
    rows3, best3 = plan.fetch_starts()
    assert len(rows3) == 3 and all(_all_same(a, b) for a, b in zip(rows3, rows[1:4]))
    assert np.array_equal(best3, K.select(np.array([[r.fret for r in row] for row in rows[1:4]])))

    # the constants come from the problem: a population whose other columns differ gives the same results
    rest = np.setdiff1d(np.arange(pp.nvars), fv)
    assert len(rest) > 0
    Y = np.array(X)
    Y[:, rest] += 1.0 + np.arange(K.NSTARTS)[:, None]
    g.set_x(base)
    other = capi.Population(g, x=Y)
    plan.solve_starts_population(other, maxiters=iters)
    rows4, best4 = plan.fetch_starts()
    assert all(_all_same(a, b) for a, b in zip(rows4, rows)) and best4.tobytes() == best.tobytes() and g.get_x().tobytes() == xs.tobytes()
    assert other.get_x().tobytes() == Y.tobytes()


# ---- 7. no state leaks between solves ----------------------------------------------------------------------------------------------------------
def test_no_state_reaches_the_next_solve(gctx):
    name, model = "synthetic-6x3x40", 2
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fv = S.csr(comps)[1]
    g = capi.Problem(gctx, pp)
    base = g.get_x()
    plan = _plan(g, comps, model)
    plan.solve_starts(X[:, fv], iters)
    rows, best = plan.fetch_starts()
    xs = g.get_x()
    bytes0 = plan.info("device_bytes")
    for _ in range(2):
        g.set_x(base)
        plan.solve_starts(X[:, fv], iters)
        again, best2 = plan.fetch_starts()
        assert all(_all_same(a, b) for a, b in zip(again, rows)) and best2.tobytes() == best.tobytes() and g.get_x().tobytes() == xs.tobytes()
    assert plan.info("device_bytes") == bytes0 > 0                   # nothing was allocated after the first call
    # a solve() and a solve_population() after a multi-start solve are what a fresh plan returns
    fresh_g = capi.Problem(gctx, pp)
    fresh = _plan(fresh_g, comps, model)
    fresh.solve(iters)
    g.set_x(base)
    plan.solve(iters)
    assert _all_same(plan.fetch(), fresh.fetch()) and g.get_x().tobytes() == fresh_g.get_x().tobytes()
    assert plan.info("members_per_launch") == 1 and plan.info("launches") == 1
    pa, pb = capi.Population(g, x=X[:4]), capi.Population(fresh_g, x=X[:4])
    plan.solve_population(pa, maxiters=iters)
    fresh.solve_population(pb, maxiters=iters)
    assert all(_all_same(a, b) for a, b in zip(plan.fetch_population(), fresh.fetch_population()))
    assert pa.get_x().tobytes() == pb.get_x().tobytes()
    # ... and a multi-start solve after those
    g.set_x(base)
    plan.solve_starts(X[:, fv], iters)
    again, best2 = plan.fetch_starts()
    assert all(_all_same(a, b) for a, b in zip(again, rows)) and best2.tobytes() == best.tobytes() and g.get_x().tobytes() == xs.tobytes()


# ---- 8. the objective ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladybug-5-30-points", "synthetic-2x16x60"])
def test_objective_is_the_sum_of_the_ordinary_outputs(name, gctx):
    """within ncomp * 2^-52 * sum |fret| of math.fsum of the fetched fret: after solve() its rows, after solve_starts() the winners'"""
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fv = S.csr(comps)[1]
    g = capi.Problem(gctx, pp)
    base = g.get_x()
    plan = _plan(g, comps, 1)

    def check():
        fret = [r.fret for r in plan.fetch()]
        got = plan.objective()
        assert abs(got - math.fsum(fret)) <= len(comps) * 2.0 ** -52 * math.fsum(abs(f) for f in fret), (got, math.fsum(fret))
        return got

    plan.solve(iters)
    a = check()
    g.set_x(base)
    plan.solve_starts(X[:, fv], iters)
    b = check()
    rows, best = plan.fetch_starts()
    assert b <= min(math.fsum(r.fret for r in row) for row in rows) * (1 + 1e-12)     # the winners' sum is no worse than any start's
    assert a != b


# ---- 9. refusals: all before anything is launched, copied or marked ----------------------------------------------------------------------------
def _raises(code, call, *words):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(gctx):
    name, model = "ladybug-5-30-points", 2
    pp, comps, iters = S.shape(name)[:3]
    X = K.rows(name)
    fv = S.csr(comps)[1]
    starts = X[:, fv]
    g = capi.Problem(gctx, pp)
    before = g.get_x()
    plan = _plan(g, comps, model)
    pop = capi.Population(g, x=X)
    foreign = capi.Population(capi.Problem(gctx, pp), x=X)
    lib = gctx.lib

    def refused_solves():
        _raises(EINVAL, lambda: plan.solve_starts(starts[:0], iters), "nstarts")
        _raises(EINVAL, lambda: gctx.check(lib.rdis_hip_lm_plan_solve_starts(plan.h, -1, starts.ctypes.data, iters, 3e-8)), "nstarts")
        _raises(EINVAL, lambda: plan.solve_starts(None, iters), "x_starts")
        _raises(EINVAL, lambda: plan.solve_starts(starts, 0), "maxiters")
        _raises(ERANGE, lambda: gctx.check(lib.rdis_hip_lm_plan_solve_starts(plan.h, 1 << 40, starts.ctypes.data, iters, 3e-8)), "too many starts")
        _raises(EINVAL, lambda: plan.solve_starts_population(foreign, maxiters=iters), "another problem")
        for first, count in ((0, 0), (0, 7), (4, 3), (-1, 2), (6, 1), (1, -1)):
            _raises(EINVAL, lambda: plan.solve_starts_population(pop, first=first, count=count, maxiters=iters), "out of range")
        _raises(EINVAL, lambda: plan.solve_starts_population(pop, maxiters=0), "maxiters")

    refused_solves()
    _raises(EINVAL, plan.fetch_starts, "nothing was solved")          # no refused call counted as a solve
    _raises(EINVAL, plan.fetch, "nothing was solved")
    _raises(EINVAL, plan.objective, "nothing was solved")
    assert plan.info("launches") == 0 and g.get_x().tobytes() == before.tobytes()
    assert pop.get_x().tobytes() == X.tobytes() and foreign.get_x().tobytes() == X.tobytes()

    # the three fetch-kind mismatches, each leaving the right fetch working
    plan.solve(iters)
    _raises(EINVAL, plan.fetch_starts, "not a multi-start solve")
    ref = plan.fetch()
    plan.objective()
    plan.solve_population(pop, maxiters=iters)
    _raises(EINVAL, plan.fetch_starts, "not a multi-start solve")
    _raises(EINVAL, plan.objective, "population solve")
    prow = plan.fetch_population()
    assert _all_same(prow[0], ref)
    g.set_x(before)
    plan.solve_starts(starts, iters)
    _raises(EINVAL, plan.fetch_population, "not a population solve")
    rows, best = plan.fetch_starts()
    xs = g.get_x()
    # refused calls after a solve leave the plan, its outputs and x as they are
    refused_solves()
    rows2, best2 = plan.fetch_starts()
    assert all(_all_same(a, b) for a, b in zip(rows2, rows)) and best2.tobytes() == best.tobytes() and g.get_x().tobytes() == xs.tobytes()
    assert _all_same(plan.fetch(), [rows[best[c]][c] for c in range(len(comps))])

    # a plan of no component: 0, and nothing is done
    empty = capi.LmPlan(g, np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64), model=1)
    empty.solve_starts(np.zeros((3, 0)), iters)
    assert empty.info("launches") == 0 and g.get_x().tobytes() == xs.tobytes()
