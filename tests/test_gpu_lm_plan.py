"""Levenberg-Marquardt plans (rdis_hip_lm_plan; capi.LmPlan): rdis_hip_lm_batch's tables built and uploaded once, solves that
stay on the stream, on the problem's x or on the members of a population (the member is the grid's second dimension of
lm_batch.hip's kernel).  The yardstick is rdis_hip_lm_batch itself (tests/test_gpu_lm_batch.py checks it against the
oracle): a plan's solve, and every member of a population solve, must equal with == what lm_batch returns and leaves on a
problem whose x is that start -- every field, the history's and x's bytes.  That pins the member strides, the splitting of
a solve into launches, and that no state leaks between solves.  Members 1 to 3 are compared with the oracle directly as well
(tests/test_lm_plan_cpu.py pins the oracle's own sensitivity there)."""
import numpy as np
import pytest

from rdis_amd import capi, problems as P

import lm_batch_shapes as S
import lm_plan_members as M
from test_gpu_lm_batch import _compare, _same

pytestmark = pytest.mark.gpu

EINVAL, EOVERLAP, ERANGE = -1, -4, -5

SOLVE_NAMES = ["ladybug-5-30-whole", "ladybug-5-30-points", "ladybug-5-30-sub-block", "synthetic-6x3x40", "synthetic-2x16x60"]


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _batch_from(gctx, pp, comps, x, iters, model, history=64):
    """the yardstick: lm_batch on a fresh problem whose x is x; (results, the whole x afterwards)"""
    g = capi.Problem(gctx, pp)
    g.set_x(x)
    rs = g.lm_batch(*S.csr(comps), maxiters=iters, model=model, history=history)
    return rs, g.get_x()


def _plan(g, comps, model, history=64):
    return capi.LmPlan(g, *S.csr(comps), model=model, history=history)


# ---- 1. a plan's solve is lm_batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("name", SOLVE_NAMES)
def test_plan_solve_equals_lm_batch(name, model, gctx):
    pp, comps, iters = S.shape(name)[:3]
    ref, xref = _batch_from(gctx, pp, comps, pp.x0, iters, model)
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, model)
    plan.solve(iters)
    rs = plan.fetch()
    assert any(len(r.history) > 0 for r in ref)
    assert _all_same(rs, ref) and g.get_x().tobytes() == xref.tobytes()
    assert plan.info("members_per_launch") == 1 and plan.info("launches") == len({capi_class(r.camera_blocks) for r in ref})
    # twice more from a re-assigned start: no state of a solve reaches the next one
    bytes0 = plan.info("device_bytes")
    for _ in range(2):
        g.set_x(pp.x0)
        plan.solve(iters)
        assert _all_same(plan.fetch(), ref) and g.get_x().tobytes() == xref.tobytes()
    assert plan.info("device_bytes") == bytes0 > 0                   # nothing was allocated after the first solve


def capi_class(nca):
    """lm_batch.hpp's lm_batch_class"""
    return 0 if nca == 0 else 1 if nca <= 6 else 2


# ---- 2. the alternation, with nothing fetched in between ----------------------------------------------------------------------------
def test_camera_point_alternation_without_a_fetch_equals_lm_batch_calls(gctx):
    pp = P.load_bal(ncams=5, npts=30)
    g, h = capi.Problem(gctx, pp), capi.Problem(gctx, pp)
    lists = {}
    for kind, fixed in (("cameras", slice(45, None)), ("points", slice(0, 45))):
        assigned = np.zeros(pp.nvars, dtype=np.uint8)
        assigned[fixed] = 1
        lists[kind] = g.components(assigned)
    assert len(lists["cameras"][0]) - 1 == 5 and len(lists["points"][0]) - 1 == 30
    plans = {kind: capi.LmPlan(h, *lists[kind], model=2, history=8) for kind in lists}
    for _ in range(3):
        for kind in ("cameras", "points"):
            g.lm_batch(*lists[kind], maxiters=5, model=2, history=8)
            plans[kind].solve(5)
    assert h.get_x().tobytes() == g.get_x().tobytes() and h.eval() == g.eval()
    assert h.eval() < capi.Problem(gctx, pp).eval()
    last = g.lm_batch(*lists["points"], maxiters=5, model=2, history=8)      # a fourth point half-round on both sides, now fetched
    plans["points"].solve(5)
    assert _all_same(plans["points"].fetch(), last)


# ---- 3. population rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("name", M.NAMES)
def test_population_rows_equal_lm_batch_from_each_members_x(name, model, gctx):
    """every member of one population solve == lm_batch on a problem whose x is that member's: results, history, and the
    member's whole row afterwards (constants included).  The members differ, so a wrong stride of x, of the workspace or of the
    outputs cannot pass.  Members 1 to 3 also against the oracle from their own start (_compare's tolerances: histories 1e-7,
    x 1e-7, fret 1e-8), but for lm_plan_members.TOO_SENSITIVE."""
    pp, comps, iters = S.shape(name)[:3]
    X = M.members(name)
    g = capi.Problem(gctx, pp)
    before = g.get_x()
    pop = capi.Population(g, x=X)
    plan = _plan(g, comps, model)
    plan.solve_population(pop, maxiters=iters)
    rows = plan.fetch_population()
    assert len(rows) == M.NMEMBERS and plan.info("members_per_launch") == M.NMEMBERS
    for s in range(M.NMEMBERS):
        ref, xref = _batch_from(gctx, pp, comps, X[s], iters, model)
        assert _all_same(rows[s], ref), "member %d" % s
        assert pop.get_x(s).tobytes() == xref.tobytes(), "member %d" % s
    for s in range(1, M.NMEMBERS):                                   # the rows are not copies of one another
        assert all(a.fret != b.fret for a, b in zip(rows[s], rows[0]) if a.nfev > 0 and a.fret != 0.0)
    assert g.get_x().tobytes() == before.tobytes()                   # the problem's own x is not touched
    if (name, model) in M.ORACLE_CASES:
        for s in range(1, M.NMEMBERS):
            for r, ro in zip(rows[s], M.oracle_member_reference(name, model, s)):
                _compare(r, ro)


# ---- 4. launch splitting -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synthetic-2x16x60", "ladybug-5-30-points"])
def test_the_split_into_launches_changes_no_bit(name, gctx):
    """workspace_bytes for one member, two members and all four members a launch (class 2 and class 0)"""
    pp, comps, iters = S.shape(name)[:3]
    X = M.members(name)
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, 2)
    mb = plan.info("member_workspace_bytes")
    assert mb > 0 and plan.info("workspace_bytes") == 1 << 30
    seen = []
    for budget, per in ((0, 1), (mb - 1, 1), (2 * mb, 2), (3 * mb - 1, 2), (4 * mb, 4), (1 << 30, 4)):
        plan.set_option("workspace_bytes", budget)
        pop = capi.Population(g, x=X)
        plan.solve_population(pop, maxiters=iters)
        assert plan.info("members_per_launch") == per and plan.info("launches") == (M.NMEMBERS + per - 1) // per
        seen.append((plan.fetch_population(), pop.get_x().tobytes()))
    for rows, xb in seen[1:]:
        assert xb == seen[0][1] and all(_all_same(a, b) for a, b in zip(rows, seen[0][0]))
    assert any(len(r.history) > 0 for r in seen[0][0][3])


# ---- 5. a member range ------------------------------------------------------------------------------------------------------------------
def test_a_member_range_solves_its_rows_and_touches_no_other(gctx):
    name, model = "synthetic-6x3x40", 2
    pp, comps, iters = S.shape(name)[:3]
    X = M.members(name)
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, model)
    whole = capi.Population(g, x=X)
    plan.solve_population(whole, maxiters=iters)
    rows = plan.fetch_population()
    part = capi.Population(g, x=X)
    plan.solve_population(part, first=1, count=2, maxiters=iters)
    got = plan.fetch_population()
    assert len(got) == 2 and _all_same(got[0], rows[1]) and _all_same(got[1], rows[2])
    after = part.get_x()
    assert after[1:3].tobytes() == whole.get_x(first=1, count=2).tobytes()
    assert after[0].tobytes() == X[0].tobytes() and after[3].tobytes() == X[3].tobytes()
    assert after[1].tobytes() != X[1].tobytes()


# ---- 6. what a population solve does to the population's and the problem's state ---------------------------------------------------------
def test_population_values_are_stale_after_a_solve(gctx):
    name = "ladybug-5-30-whole"                                      # (every factor listed: the objective as a whole falls)
    pp, comps, iters = S.shape(name)[:3]
    g = capi.Problem(gctx, pp)
    before = g.get_x()
    pop = capi.Population(g, x=M.members(name))
    f0 = pop.eval()
    pop.best()
    plan = _plan(g, comps, 2)
    plan.solve_population(pop, maxiters=iters)
    with pytest.raises(capi.RdisHipError) as e:
        pop.best()
    assert e.value.code == EINVAL and "evaluate first" in str(e.value)
    assert pop.info("eval_valid") == 0
    f1 = pop.eval()
    m, f = pop.best()
    assert f == f1[m] == np.min(f1) and np.all(f1 < f0)
    assert g.get_x().tobytes() == before.tobytes()


def test_a_fetch_returns_the_solves_x_whatever_became_of_the_population_or_the_problem(gctx):
    """the plan keeps the solve's x in its own output block: a fetch after the population was closed, or after x was assigned
    anew, returns the results of the solve -- the plan holds no pointer to the population"""
    name, model = "synthetic-6x3x40", 2
    pp, comps, iters = S.shape(name)[:3]
    X = M.members(name)
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, model)
    pop = capi.Population(g, x=X)
    plan.solve_population(pop, maxiters=iters)
    want = plan.fetch_population()
    xs = pop.get_x()
    fv = S.csr(comps)[1]
    assert np.concatenate([r.x for r in want[2]]).tobytes() == xs[2, fv].tobytes()
    plan.solve_population(pop, first=1, count=3, maxiters=iters)      # rows 1 to 3 once more, from their results
    again = plan.fetch_population()
    pop.set_x(X)                                                      # the rows rewritten ...
    assert all(_all_same(a, b) for a, b in zip(plan.fetch_population(), again))
    pop.close()                                                       # ... and the population destroyed before the fetch
    gone = plan.fetch_population()
    assert len(gone) == 3 and all(_all_same(a, b) for a, b in zip(gone, again))
    plan.solve_population(capi.Population(g, x=X), maxiters=iters)    # a population nobody holds on to
    import gc
    gc.collect()
    assert all(_all_same(a, b) for a, b in zip(plan.fetch_population(), want))
    # the same for the problem's own x
    plan.solve(iters)
    ref = plan.fetch()
    g.set_x(pp.x0 + 1.0)
    assert _all_same(plan.fetch(), ref)


# ---- 7. refusals: all before any launch, nothing changed ---------------------------------------------------------------------------------
def _raises(code, call, *words):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(gctx):
    pp17 = P.make_synthetic_ba(1, 17, 60, obs_per_pt=6)
    whole = [(np.arange(pp17.nvars, dtype=np.int64), np.arange(pp17.nfac, dtype=np.int64))]
    _raises(ERANGE, lambda: _plan(capi.Problem(gctx, pp17), whole, 1), "lm_plan_create", "component 0", "17", "16")
    name = "ladybug-5-30-points"
    pp, pts, iters = S.shape(name)[:3]
    g = capi.Problem(gctx, pp)
    shared = [pts[0], (np.concatenate([pts[1][0], pts[0][0][:1]]), pts[1][1])]
    _raises(EOVERLAP, lambda: _plan(g, shared, 1), "lm_plan_create")
    _raises(EINVAL, lambda: _plan(g, pts[:2], 3), "lm_plan_create")
    _raises(EINVAL, lambda: _plan(g, [(np.array([45, 46, pp.nvars], dtype=np.int64), pts[0][1])], 1), "lm_plan_create")
    _raises(EINVAL, lambda: _plan(capi.Problem(gctx, P.load_poly()), [(np.array([0], dtype=np.int64), np.array([0], dtype=np.int64))], 1))

    X = M.members(name)
    plan = _plan(g, pts, 2)
    before = g.get_x()
    pop = capi.Population(g, x=X)
    _raises(EINVAL, plan.fetch, "nothing was solved")                                    # a fetch before any solve
    _raises(EINVAL, plan.fetch_population, "nothing was solved")
    other = capi.Problem(gctx, pp)
    foreign = capi.Population(other, x=X)
    _raises(EINVAL, lambda: plan.solve_population(foreign, maxiters=iters), "another problem")
    for first, count in ((0, 0), (0, 5), (3, 2), (-1, 2), (4, 1), (1, -1)):
        _raises(EINVAL, lambda: plan.solve_population(pop, first=first, count=count, maxiters=iters), "out of range")
    _raises(EINVAL, lambda: plan.solve_population(pop, maxiters=0))
    _raises(EINVAL, lambda: plan.solve(0))
    _raises(EINVAL, lambda: plan.set_option("workspace_bytes", -1), "workspace_bytes")
    _raises(EINVAL, lambda: plan.set_option("no_such_option", 1))
    _raises(EINVAL, lambda: plan.info("no_such_info"))
    assert plan.info("workspace_bytes") == 1 << 30 and plan.info("launches") == 0
    _raises(EINVAL, plan.fetch, "nothing was solved")                                    # ... still: no refused call counted as a solve
    assert pop.get_x().tobytes() == X.tobytes() and foreign.get_x().tobytes() == X.tobytes() and g.get_x().tobytes() == before.tobytes()
    pop.eval()
    pop.best()                                                                           # (a refused solve left the values current)
    # a fetch of the other kind than the last solve
    plan.solve(iters)
    _raises(EINVAL, plan.fetch_population, "rdis_hip_lm_plan_fetch")
    ref = plan.fetch()
    plan.solve_population(pop, maxiters=iters)
    _raises(EINVAL, plan.fetch, "rdis_hip_lm_plan_fetch_population")
    rows = plan.fetch_population()                                                       # ... refused, and the right one still works
    assert len(rows) == M.NMEMBERS and _all_same(rows[0], ref)


# ---- 8. all three classes in one plan ---------------------------------------------------------------------------------------------------
def test_a_plan_with_all_three_classes(gctx):
    """three components of one synthetic problem: 8 cameras and their points (class 2), 3 cameras of 8 and the points (class 1),
    the points alone (class 0); two members, == lm_batch per member; three launches for any number of members of a launch"""
    pp = P.make_synthetic_ba(3, 8, 40, first_comp=11)
    nv, nf = pp.nvars // 3, pp.nfac // 3
    fac = [c * nf + np.arange(nf, dtype=np.int64) for c in range(3)]
    comps = [(np.arange(nv, dtype=np.int64), fac[0]),
             (nv + np.concatenate([np.arange(27), 72 + np.arange(120)]).astype(np.int64), fac[1]),
             (2 * nv + 72 + np.arange(120, dtype=np.int64), fac[2])]
    X = M.members_of(pp, comps, 2)
    assert X[0].tobytes() != X[1].tobytes()
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, 2)
    for nmem in (1, 2):
        pop = capi.Population(g, x=X[:nmem])
        plan.solve_population(pop, maxiters=5)
        rows = plan.fetch_population()
        assert plan.info("launches") == 3 and plan.info("members_per_launch") == nmem
        assert [r.camera_blocks for r in rows[0]] == [8, 3, 0] and [r.point_blocks for r in rows[0]] == [40, 40, 40]
        for s in range(nmem):
            ref, xref = _batch_from(gctx, pp, comps, X[s], 5, 2)
            assert _all_same(rows[s], ref) and pop.get_x(s).tobytes() == xref.tobytes()
            assert all(r.delta < 0 and len(r.history) > 0 for r in rows[s])
    g.set_x(X[1])
    plan.solve(5)                                                    # ... and on the problem's own x
    assert plan.info("launches") == 3 and _all_same(plan.fetch(), rows[1]) and g.get_x().tobytes() == pop.get_x(1).tobytes()


# ---- 9. the six readers at every kind of last solve ---------------------------------------------------------------------------------------
def test_every_reader_at_every_kind_of_last_solve(gctx):
    """nothing solved -> solve -> solve_population (2 members) -> solve_starts (2 starts): at each stage the readers that
    tests/test_lm_rules_cpu.py's table allows succeed, every other returns EINVAL with the table's whole message as the context's
    last error; afterwards the plan solves and fetches what a fresh plan does"""
    import ctypes as C
    from test_lm_rules_cpu import REFUSALS
    name, model = "ladybug-5-30-whole", 2
    pp, comps, iters = S.shape(name)[:3]
    X = M.members(name)[:2]
    g = capi.Problem(gctx, pp)
    plan = _plan(g, comps, model)
    lib, h = gctx.lib, plan.h
    dev = C.c_void_p()
    readers = {
        "fetch": lambda: lib.rdis_hip_lm_plan_fetch(h, None, None, None, None, None, None),
        "fetch_population": lambda: lib.rdis_hip_lm_plan_fetch_population(h, None, None, None, None, None, None),
        "fetch_starts": lambda: lib.rdis_hip_lm_plan_fetch_starts(h, None, None, None, None, None, None, None),
        "objective_device": lambda: lib.rdis_hip_lm_plan_objective_device(h, C.byref(dev)),
        "summary_device": lambda: lib.rdis_hip_lm_plan_summary_device(h, C.byref(dev)),
        "summary_population_device": lambda: lib.rdis_hip_lm_plan_summary_population_device(h, C.byref(dev)),
    }
    assert list(readers) == [r[0] for r in REFUSALS]
    pop = capi.Population(g, x=X)
    free = S.csr(comps)[1]
    stages = [lambda: None, lambda: plan.solve(iters), lambda: plan.solve_population(pop, maxiters=iters),
              lambda: plan.solve_starts(X[:, free], maxiters=iters)]
    for kind, solve in enumerate(stages):
        solve()
        for reader, allowed, nothing, wrong in REFUSALS:
            rc = readers[reader]()
            if kind in allowed:
                assert rc == 0, (kind, reader, lib.rdis_hip_last_error(gctx.h).decode())
            else:
                assert rc == EINVAL, (kind, reader)
                assert lib.rdis_hip_last_error(gctx.h).decode() == (nothing if kind == 0 else wrong), (kind, reader)
    # the refusals left the plan usable: a solve and a fetch == a fresh plan's
    g.set_x(pp.x0)
    plan.solve(iters)
    got, xgot = plan.fetch(), g.get_x()
    g2 = capi.Problem(gctx, pp)
    fresh = _plan(g2, comps, model)
    fresh.solve(iters)
    assert any(len(r.history) > 0 for r in got)
    assert _all_same(got, fresh.fetch()) and xgot.tobytes() == g2.get_x().tobytes()
