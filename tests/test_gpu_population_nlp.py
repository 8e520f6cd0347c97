"""Population solves of nonlinear-product plans: rdis_hip_plan_solve_population with the plan option population_plain = 1, on
the plain one-workgroup solver (solver_wg_population.hpp) -- one workgroup per (component, member), working in the member's
own row of X (trial points included) with a replica of dir, and no replica of x.

Every (member, component) must be, bit for bit, what set_start(None) / solve / fetch returns on a fresh Problem whose assigned x
is that member's row ("sequential" below), the member's whole row afterwards must be that problem's x, and where stated both
must be what the CPU oracle's restatement of that solver returns (OracleProblem.device_wg_default on a problem whose x0 is the
member's row: the device's sine / cosine, RO_SUM_TOPOLOGY_WG).  Everything is compared with == / .tobytes(); nothing is timed;
maxiters 25 and ftol 3e-8 unless stated."""
import dataclasses
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval")


def sequential(gctx, pp, x, steps, maxiters=25):
    """the parent's path: a fresh Problem whose x is the member's row; per step (a decomposition) set_start(None), solve, fetch,
    get_x -- the x a step leaves is the row the next step starts from.  Returns [(BatchResult, x after the step)] per step."""
    g = capi.Problem(gctx, pp)
    g.set_x(x)
    plans = {}
    out = []
    for comps in steps:
        if id(comps) not in plans:
            plans[id(comps)] = capi.Plan(g, *comps)
        plan = plans[id(comps)]
        plan.set_start(None)
        plan.solve(maxiters, 3e-8)
        out.append((plan.fetch(), g.get_x()))
    g.close()
    return out


def assert_step_equals(pr, rows, seq_rows, where=""):
    """pr: fetch_population() after a step, rows: pop.get_x() after it; seq_rows[s] = (BatchResult, x) of member s's sequential run"""
    for s, (r, x_after) in enumerate(seq_rows):
        for name in FIELDS:
            a, b = getattr(pr, name)[s], getattr(r, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, s, name, a, b)
        assert pr.x[s].tobytes() == r.x.tobytes(), (where, s)
        assert rows[s].tobytes() == x_after.tobytes(), (where, s)


def assert_row_equals_oracle(pr, s, c, want, x_row):
    assert pr.fret[s, c] == want.fret and pr.delta[s, c] == want.delta and x_row.tobytes() == want.x.tobytes(), (s, c, pr.fret[s, c], want.fret)
    assert (int(pr.iters[s, c]), int(pr.status[s, c]), int(pr.nfeval[s, c]), int(pr.ngeval[s, c])) == \
           (want.iters, want.status, want.nfeval, want.ngeval), (s, c)


def oracle_component(pp, row, comps, c, maxiters=25):
    """component c of the decomposition solved by the oracle on a problem whose x0 -- start and constants -- is the member's row"""
    fp, fv, cp, ci = comps
    v, f = fv[fp[c]:fp[c + 1]], ci[cp[c]:cp[c + 1]]
    pq = dataclasses.replace(pp, x0=np.array(row, dtype=np.float64))
    return O.OracleProblem.device_wg_default(pq, free_vid=v, fac=f).cgd(free_vid=v, fac=f, x=row[v], maxiters=maxiters)


def population_plan(g, comps):
    plan = capi.Plan(g, *comps)
    plan.set_option("population_plain", 1)
    assert plan.info("components_plain") == plan.ncomp
    return plan


def run_steps(gctx, pp, X, steps, plans, pop, maxiters=25):
    """the alternation on the population, every step compared with the members' sequential runs; returns per step
    (fetch_population(), rows after the step)"""
    seq = [sequential(gctx, pp, X[s], steps, maxiters) for s in range(X.shape[0])]
    out = []
    for k, comps in enumerate(steps):
        plan = plans[id(comps)]
        plan.solve_population(pop, maxiters, 3e-8)
        pr = plan.fetch_population()
        assert pr.best is None and pr.x.shape == (X.shape[0], plan.nfree) and pr.fret.shape == (X.shape[0], plan.ncomp)
        rows = pop.get_x()
        assert_step_equals(pr, rows, [seq[s][k] for s in range(X.shape[0])], "step %d" % k)
        out.append((pr, rows))
    return out


def test_one_wave_constants_per_member(gctx):
    """testpoly (two variables, seven factors; 64 lanes, one wave), four members with different (x, y); plan A frees x only, plan B
    y only; A, B, A.  After each step every field of every member and the member's whole row == sequential; step B == the oracle
    on a problem whose x0 is the member's row (its x the result of step A); the members end in different minima, so the constant
    of the last step (y) differs by member."""
    pp = P.load_poly()
    X = np.array([[3.0, 3.0], [-3.0, -3.0], [-3.0, 3.0], [0.5, -1.0]])
    g = capi.Problem(gctx, pp)
    plan_a_comps = g.components(np.array([0, 1], np.uint8))
    plan_b_comps = g.components(np.array([1, 0], np.uint8))
    assert plan_a_comps[1].tolist() == [0] and plan_b_comps[1].tolist() == [1]
    plans = {id(plan_a_comps): population_plan(g, plan_a_comps), id(plan_b_comps): population_plan(g, plan_b_comps)}
    pop = capi.Population(g, x=X)
    steps = [plan_a_comps, plan_b_comps, plan_a_comps]
    done = run_steps(gctx, pp, X, steps, plans, pop)
    for plan in plans.values():
        assert plan.info("starts_per_launch") == 4 and plan.info("starts_launches") == 1
    (_, rows_a), (pr_b, rows_b), (_, rows_end) = done
    for s in range(4):
        assert_row_equals_oracle(pr_b, s, 0, oracle_component(pp, rows_a[s], plan_b_comps, 0), pr_b.x[s])
        assert rows_b[s, 0] == rows_a[s, 0] and rows_end[s, 1] == rows_b[s, 1]     # a step's constant is bit-unchanged by it
    assert rows_end[0].tobytes() != rows_end[1].tobytes() and rows_end[0, 1] != rows_end[1, 1]
    assert g.get_x().tobytes() == pp.x0.tobytes()


def _root_and_subtrees(gctx, pp=None):
    """the sinusoid's two decompositions: its root alone (1 variable, the others constants) and, the root constant, its three
    subtrees of 40 variables and 120 factors each (128 lanes)"""
    pp = P.make_high_dim_sinusoid() if pp is None else pp
    g = capi.Problem(gctx, pp)
    assigned = np.ones(pp.nvars, np.uint8)
    assigned[0] = 0
    root = g.components(assigned)
    sub = g.components(1 - assigned)
    assert root[1].tolist() == [0] and root[0].tolist() == [0, 1]
    assert np.diff(sub[0]).tolist() == [40, 40, 40] and np.diff(sub[2]).tolist() == [120, 120, 120]
    return pp, g, root, sub


def _uniform_members(pp, n=4, seed=7):
    return np.random.default_rng(seed).uniform(pp.lo, pp.hi, (n, pp.nvars))


def test_three_subtrees_and_the_root(gctx):
    """the 121-variable sinusoid, four uniform members, root / subtrees / root / subtrees: every step == sequential; the first
    subtree step == the oracle for all 12 (member, component) pairs, each on the member's own root; the root is bit-unchanged by
    the subtree plan and differs by member after the first root step"""
    pp, g, root, sub = _root_and_subtrees(gctx)
    X = _uniform_members(pp)
    plans = {id(root): population_plan(g, root), id(sub): population_plan(g, sub)}
    pop = capi.Population(g, x=X)
    done = run_steps(gctx, pp, X, [root, sub, root, sub], plans, pop)
    (pr_root, rows_root), (pr_sub, rows_sub) = done[0], done[1]
    assert len(set(rows_root[:, 0].tolist())) == 4 and np.all(rows_root[:, 0] != X[:, 0])
    assert rows_root[:, 1:].tobytes() == X[:, 1:].tobytes()                      # (the root plan's constants)
    assert rows_sub[:, 0].tobytes() == rows_root[:, 0].tobytes() and done[3][1][:, 0].tobytes() == done[2][1][:, 0].tobytes()
    fp = sub[0]
    for s in range(4):
        for c in range(3):
            assert_row_equals_oracle(pr_sub, s, c, oracle_component(pp, rows_root[s], sub, c), pr_sub.x[s, fp[c]:fp[c + 1]])
    assert np.all(np.isfinite(pr_sub.fret)) and np.all(pr_sub.delta < 0)
    assert g.get_x().tobytes() == pp.x0.tobytes()


def test_launch_splitting_and_no_replica_of_x(gctx):
    """the subtree plan, four uniform members: a budget for three replicas (3 + 1 launches), one byte (four launches on ONE replica)
    and the default budget leave the same bytes in every field and in X.  A replica, measured through device_bytes(), is at least
    dir and the recurrence's five vectors, 8 (N + 5 nfree), and less than 8 (2N + 5 nfree + ngfac): no replica of x is kept."""
    pp, g, root, sub = _root_and_subtrees(gctx)
    X = _uniform_members(pp)
    plan = population_plan(g, sub)
    nfree = int(sub[1].shape[0])
    free = np.zeros(pp.nvars, bool)
    free[sub[1]] = True
    ngfac = int(sum(np.count_nonzero(free[pp.vid[pp.rowptr[f]:pp.rowptr[f + 1]]]) for f in sub[3]))   # (one partial per listed slot of a free variable)
    # with a budget of one byte a launch holds one replica whatever the number of members: a second member adds its inputs and
    # outputs only
    plan.set_option("starts_workspace_bytes", 1)
    grow = [plan.device_bytes()]
    for n in (1, 2):
        few = capi.Population(g, x=X[:n])
        plan.solve_population(few, 25, 3e-8)
        plan.fetch_population(want_x=False)
        grow.append(plan.device_bytes())
        few.close()
    assert plan.info("starts_per_launch") == 1 and plan.info("starts_launches") == 2
    rep = (grow[1] - grow[0]) - (grow[2] - grow[1])
    assert 8 * (pp.nvars + 5 * nfree) <= rep < 8 * (2 * pp.nvars + 5 * nfree + ngfac), rep

    def run(budget, per_launch, launches):
        pop = capi.Population(g, x=X)
        plan.set_option("starts_workspace_bytes", budget)
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.info("starts_per_launch") == per_launch and plan.info("starts_launches") == launches
        assert plan.last_kernel_ms()[1] == launches
        rows = pop.get_x()
        pop.close()
        return pr, rows

    split, rows_split = run(3 * rep + rep // 2, 3, 2)
    single, rows_single = run(1, 1, 4)
    whole, rows_whole = run(1 << 30, 4, 1)
    for name in FIELDS + ("x",):
        assert getattr(whole, name).tobytes() == getattr(split, name).tobytes() == getattr(single, name).tobytes(), name
    assert rows_whole.tobytes() == rows_split.tobytes() == rows_single.tobytes()
    assert_step_equals(whole, rows_whole, [sequential(gctx, pp, X[s], [sub])[0] for s in range(4)])


def _sinusoid_from_the_committed_start():
    pp = P.make_high_dim_sinusoid()
    with open(os.path.join(os.path.dirname(__file__), "golden", "sinusoid_start.json")) as fh:
        pp.x0 = np.array(json.load(fh)["x0"])
    return pp.single_component()


def test_config_2_512_lanes(gctx):
    """BASELINE config 2 (the sinusoid as one component, 512 lanes): member 0 the bench's start, members 1 and 2 moved by
    1e-9-relative noise; all == sequential, member 0 the bench's number: 1578.9001138212975 after 726 evaluations"""
    pp = _sinusoid_from_the_committed_start()
    comps = (pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id)
    X = np.stack([pp.x0] + [pp.x0 * (1 + 1e-9 * np.random.default_rng(seed).standard_normal(pp.nvars)) for seed in range(2)])
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    (pr, rows), = run_steps(gctx, pp, X, [comps], {id(comps): population_plan(g, comps)}, pop)
    assert pr.fret[0, 0] == 1578.9001138212975 and int(pr.nfeval[0, 0]) == 726
    assert rows[0].tobytes() == pr.x[0].tobytes()


def test_bounds_and_rollback(gctx):
    """the two constructions of tests/test_gpu_multistart_nlp.py test_bounds_and_rollback as populations on the three subtrees.

    Bounds: the domains tightened around a point (half-widths 0.05 .. 1.5) so that the clamp is active in the line searches;
    members at that point, outside [lo, hi] (clamped at entry) and uniform inside.

    Roll-back: the 0.1 x^2 term of the second subtree's root made 0.1 x^0.5 and member 0 put at 0.01 there, so that its first
    bracketing step meets a NaN: that (member, component) comes back ROLLED_BACK, its row entries the clamped start -- although
    the row carried the trial points meanwhile -- and the neighbours, in the member and beside it, are none the wiser."""
    pp = P.make_high_dim_sinusoid()
    centre = np.random.default_rng(7).uniform(pp.lo, pp.hi, pp.nvars)
    rng = np.random.default_rng(31)
    w = rng.uniform(0.05, 1.5, pp.nvars)
    pp.lo[1:] = np.maximum(pp.lo, centre - w)[1:]
    pp.hi[1:] = np.minimum(pp.hi, centre + w)[1:]
    pp, g, root, sub = _root_and_subtrees(gctx, pp)
    fv = sub[1]
    outside = centre[fv] + 3.0 * (pp.hi[fv] - pp.lo[fv]) * np.where(np.arange(fv.shape[0]) % 2 == 0, 1.0, -1.0)
    assert np.all((outside > pp.hi[fv]) | (outside < pp.lo[fv]))
    X = np.stack([pp.x0] * 3)
    X[:, fv] = np.stack([centre[fv], outside, rng.uniform(pp.lo[fv], pp.hi[fv])])
    pop = capi.Population(g, x=X)
    (pr, rows), = run_steps(gctx, pp, X, [sub], {id(sub): population_plan(g, sub)}, pop)
    assert np.all(pr.x >= pp.lo[fv]) and np.all(pr.x <= pp.hi[fv]) and rows[:, fv].tobytes() == pr.x.tobytes()
    assert np.any((pr.x[0] == pp.lo[fv]) | (pr.x[0] == pp.hi[fv]))                   # the clamp was active
    assert np.all(pr.delta <= 0) and np.all(np.isfinite(pr.fret))
    g.close()

    pq = P.make_high_dim_sinusoid()
    r2 = 2                                                                            # (the second subtree's root)
    k = int(pq.rowptr[pq.nfac - pq.nvars + r2])                                       # (the squares are the last nvars factors)
    assert pq.vid[k] == r2 and pq.expo[k] == 2.0 and not pq.sine[k]
    pq.expo[k] = 0.5
    pq, g, root, sub = _root_and_subtrees(gctx, pq)
    fp, fv = sub[0], sub[1]
    assert int(fv[fp[1]]) == r2
    X = np.stack([pq.x0] * 2)
    X[:, fv] = _uniform_members(pq, n=2)[:, fv]
    X[0, r2], X[1, r2] = 0.01, 30.0
    pop = capi.Population(g, x=X)
    (pr, rows), = run_steps(gctx, pq, X, [sub], {id(sub): population_plan(g, sub)}, pop, maxiters=2)
    assert pr.status[0, 1] & capi.STATUS_ROLLED_BACK and pr.delta[0, 1] == 0
    second = fv[fp[1]:fp[2]]
    assert rows[0, second].tobytes() == X[0, second].tobytes() and pr.x[0, fp[1]:fp[2]].tobytes() == X[0, second].tobytes()
    assert not np.any(pr.status[:, [0, 2]] & capi.STATUS_ROLLED_BACK) and not (pr.status[1, 1] & capi.STATUS_ROLLED_BACK)
    assert np.all(pr.delta[:, [0, 2]] < 0) and pr.delta[1, 1] < 0
    assert rows[:, 0].tobytes() == X[:, 0].tobytes()


def _refused(call):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1 and len(str(e.value).split(":", 1)[1].strip()) > 0, e.value
    return str(e.value)


def test_state_afterwards_and_refusals(gctx):
    """without the option the solve is refused (the message names the kind and the option) and no member is written; with it the
    solve succeeds and leaves the problem's x and dir alone -- an ordinary solve on the same plan afterwards has the bytes of a
    sequential one; the two kinds of fetch do not serve each other; solve_starts on the plan still returns config 2's number;
    the option changes nothing for a bundle-adjustment plan (config 3's number)"""
    pp = _sinusoid_from_the_committed_start()
    comps = (pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id)
    X = np.stack([pp.x0, pp.x0 * (1 + 1e-9 * np.random.default_rng(0).standard_normal(pp.nvars))])
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    plan = capi.Plan(g)
    msg = _refused(lambda: plan.solve_population(pop, 25, 3e-8))
    assert "nonlinear-product" in msg and "population_plain" in msg, msg
    assert pop.get_x().tobytes() == X.tobytes()
    plan.set_option("population_plain", 1)
    plan.solve_population(pop, 25, 3e-8)
    pr = plan.fetch_population()
    assert pr.fret[0, 0] == 1578.9001138212975 and pop.get_x(0).tobytes() == pr.x[0].tobytes()
    assert g.get_x().tobytes() == pp.x0.tobytes()
    start = X[1]
    (want, x_want), = sequential(gctx, pp, start, [comps])
    plan.set_start(start)
    plan.solve(25, 3e-8)
    after = plan.fetch()
    for name in FIELDS + ("x",):
        assert getattr(after, name).tobytes() == getattr(want, name).tobytes(), name
        assert getattr(pr, name)[1].tobytes() == getattr(want, name).tobytes(), name
    assert g.get_x().tobytes() == x_want.tobytes()
    assert "fetch_population" in _refused(lambda: plan.fetch_starts())
    plan.solve_starts(pp.x0[None, :], 25, 3e-8)
    assert "fetch_starts" in _refused(lambda: plan.fetch_population())
    assert plan.fetch_starts().fret[0, 0] == 1578.9001138212975
    plan.set_option("population_plain", 0)
    assert "population_plain" in _refused(lambda: plan.solve_population(pop, 25, 3e-8))
    g.close()

    ba = P.load_bal(ncams=5, npts=30).single_component()
    g = capi.Problem(gctx, ba)
    plan = capi.Plan(g)
    plan.set_option("population_plain", 1)
    pop = capi.Population(g, x=np.stack([ba.x0] * 2))
    plan.solve_population(pop, 25, 3e-8)
    assert plan.info("components_lds") == 1 and plan.fetch_population().fret[1, 0] == 25.168503286225235
