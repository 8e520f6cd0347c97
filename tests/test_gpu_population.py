"""Population solves: S complete states on the device, one plan solved on all of them in one launch
(rdis_hip_population_*, rdis_hip_plan_solve_population / _fetch_population).

Every (member, component) of a population solve must be, bit for bit, what set_start(None) / solve / fetch returns on a
fresh Problem whose assigned x is that member's ("sequential" below: the path the other test files pin to the oracle with
==), and the member's x afterwards must be that problem's x.  Every comparison is == or byte equality.  No test here times
anything."""
import dataclasses
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval")


def sequential(gctx, pp, x, steps, maxiters, opts=None):
    """the parent's path: a fresh Problem with x assigned; per step (a decomposition) set_start(None), solve, fetch, get_x.
    Returns [(BatchResult, x after the step)] per step."""
    g = capi.Problem(gctx, pp)
    g.set_x(x)
    plans = {}
    out = []
    for comps in steps:
        key = id(comps)
        if key not in plans:
            plans[key] = capi.Plan(g, *comps)
            for k, v in (opts or {}).items():
                plans[key].set_option(k, v)
        plan = plans[key]
        plan.set_start(None)
        plan.solve(maxiters, 3e-8)
        out.append((plan.fetch(), g.get_x()))
    g.close()
    return out


def assert_step_equals(pr, pop, seq_rows, where=""):
    """pr: fetch_population() after a step; seq_rows[s] = (BatchResult, x) of the sequential run of member s at that step"""
    for s, (r, x_after) in enumerate(seq_rows):
        for name in FIELDS:
            a, b = getattr(pr, name)[s], getattr(r, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, s, name, a, b)
        assert pr.x[s].tobytes() == r.x.tobytes(), (where, s)
        assert pop.get_x(s).tobytes() == x_after.tobytes(), (where, s)


def set_options(plan, opts):
    for k, v in (opts or {}).items():
        plan.set_option(k, v)


def members_5_30(pp):
    rng = np.random.default_rng(7)
    return np.stack([pp.x0, pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)), pp.x0 * (1 + 1e-2 * rng.standard_normal(pp.nvars))])


def test_alternation_equals_sequential_and_the_oracle(gctx):
    """ladybug 5 / 30, three members that differ in ALL variables (so the constants differ by member), two rounds of camera plan
    then point plan: after each of the four solves every (member, component) row and every member's whole x == the sequential
    run; member 1's first camera step == the oracle with the member's constants assigned; the point step of members 0 and 1
    differs (the constants really are per member)."""
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    X = members_5_30(pp)
    steps = [cams, pts, cams, pts]
    seq = [sequential(gctx, pp, X[s], steps, 25) for s in range(3)]

    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    assert pop.nmembers == 3
    plan_c, plan_p = capi.Plan(g, *cams), capi.Plan(g, *pts)
    assert plan_c.info("components_lds") == plan_c.ncomp == 5 and plan_p.info("components_lds") == plan_p.ncomp == 30
    results = []
    for k, comps in enumerate(steps):
        plan = plan_c if comps is cams else plan_p
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert pr.best is None and pr.x.shape == (3, plan.nfree) and pr.fret.shape == (3, plan.ncomp)
        assert_step_equals(pr, pop, [seq[s][k] for s in range(3)], "step %d" % k)
        results.append(pr)
    assert np.all(results[1].fret[0] != results[1].fret[1])
    # the oracle: member 1's first camera step, its constants (the member's points) assigned
    fp, fv, cp, ci = cams
    pp1 = dataclasses.replace(pp, x0=X[1].copy())
    mf = int(np.diff(cp).max())
    threads = 64 if mf <= 64 else 128 if mf <= 128 else 256
    r = results[0]
    for c in (0, 3):
        v, f = fv[fp[c]:fp[c + 1]], ci[cp[c]:cp[c + 1]]
        want = O.OracleProblem.device_lds_default(pp1, free_vid=v, fac=f, threads=threads).cgd(free_vid=v, fac=f, x=X[1][v], maxiters=25)
        assert r.fret[1, c] == want.fret and r.delta[1, c] == want.delta and r.x[1, fp[c]:fp[c + 1]].tobytes() == want.x.tobytes(), (c, r.fret[1, c], want.fret)
        assert (int(r.iters[1, c]), int(r.status[1, c]), int(r.nfeval[1, c]), int(r.ngeval[1, c])) == (want.iters, want.status, want.nfeval, want.ngeval), c


def test_nothing_else_moves(gctx):
    """a population solve leaves the problem's x, the plan's ordinary outputs and its objective as a plain solve left them, and a
    plain solve on the same plan afterwards returns the sequential bits"""
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    X = members_5_30(pp)
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *cams)
    plan.set_start(pp.x0[cams[1]])
    plan.solve(25, 3e-8)
    before, x_before, obj_before = plan.fetch(), g.get_x(), plan.objective()
    pop = capi.Population(g, x=X)
    plan.solve_population(pop, 25, 3e-8)
    pr = plan.fetch_population()
    plan_p = capi.Plan(g, *pts)
    plan_p.solve_population(pop, 25, 3e-8)
    plan_p.fetch_population()
    assert g.get_x().tobytes() == x_before.tobytes()
    after = plan.fetch()
    for name in FIELDS + ("x",):
        assert getattr(after, name).tobytes() == getattr(before, name).tobytes(), name
    assert plan.objective() == obj_before
    (want, _), = sequential(gctx, pp, pp.x0, [cams], 25)
    plan.set_start(pp.x0[cams[1]])
    plan.solve(25, 3e-8)
    again = plan.fetch()
    for name in FIELDS + ("x",):
        assert getattr(again, name).tobytes() == getattr(want, name).tobytes(), name
        assert getattr(pr, name)[0].tobytes() == getattr(want, name).tobytes(), name     # (member 0 is x0)


def test_split_launches(gctx):
    """seven components, four members: a budget of three replicas gives two launches (3 + 1, the last one ragged), a budget of one
    byte four launches of one, the default budget one launch -- the same bytes every time, all == sequential"""
    pp = P.make_synthetic_ba(7, 3, 40)
    comps = (pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id)
    rng = np.random.default_rng(11)
    X = np.stack([pp.x0] + [pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)) for _ in range(3)])
    seq = [sequential(gctx, pp, X[s], [comps], 25)[0] for s in range(4)]
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    assert plan.info("components_lds") == 7
    # bytes of one replica of the per-solve workspace, from plan.device_bytes(): with a budget of one byte a launch holds one
    # replica whatever the number of members, so a second member adds its inputs and outputs only
    plan.set_option("starts_workspace_bytes", 1)
    grow = [plan.device_bytes()]
    for n in (1, 2):
        few = capi.Population(g, x=X[:n])
        plan.solve_population(few, 25, 3e-8)
        plan.fetch_population(want_x=False)
        grow.append(plan.device_bytes())
        few.close()
    rep = (grow[1] - grow[0]) - (grow[2] - grow[1])
    assert rep >= 8 * 5 * pp.nvars               # (at least the five vectors of the recurrence per free variable)

    def run(budget, per_launch, launches):
        pop = capi.Population(g, x=X)
        b0 = plan.device_bytes()
        plan.set_option("starts_workspace_bytes", budget)
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.info("starts_per_launch") == per_launch and plan.info("starts_launches") == launches
        assert plan.last_kernel_ms()[1] == launches
        assert plan.device_bytes() >= b0
        assert_step_equals(pr, pop, seq, "budget %d" % budget)
        pop.close()
        return pr

    one_byte = run(1, 1, 4)
    b1 = plan.device_bytes()
    split = run(3 * rep + rep // 2, 3, 2)
    assert plan.device_bytes() - b1 == 2 * rep       # two replicas more, the same inputs and outputs: plan_device_bytes counts them
    whole = run(1 << 30, 4, 1)
    for name in FIELDS + ("x",):
        assert getattr(one_byte, name).tobytes() == getattr(split, name).tobytes() == getattr(whole, name).tobytes(), name


def test_edges(gctx):
    """the inputs of test_bounds_and_rollback (tests/test_gpu_multistart.py): tight domains, a fifth of the variables not free --
    and one more variable that no factor reads, a component of its own.  Three members: inside the domains; free values outside
    [lo, hi], clamped at entry; an x that makes component 1's objective NaN -- returned restored with ROLLED_BACK while its
    neighbours are none the wiser.  The empty component ends EXIT_EMPTY with its variable untouched in every member; the
    variables that are not free are bytewise what was put in."""
    rng = np.random.default_rng(31)
    pp = P.make_synthetic_ba(7, 3, 40)
    nv = pp.nvars // 7
    w = np.where(np.arange(pp.nvars) % nv < 27, 0.02, 0.01)
    pp.lo = np.maximum(pp.lo, pp.x0 - w * rng.uniform(0.2, 1.0, pp.nvars) * np.maximum(np.abs(pp.x0), 1e-3))
    pp.hi = np.minimum(pp.hi, pp.x0 + w * rng.uniform(0.2, 1.0, pp.nvars) * np.maximum(np.abs(pp.x0), 1e-3))
    const = rng.random(pp.nvars) < 0.2
    v1, f1 = pp.component(1)
    cam, pt = int(pp.cam_vid0[f1[0]]), int(pp.pt_vid0[f1[0]])
    origin = np.r_[pt:pt + 3, cam + 3:cam + 6]
    const[origin] = False
    pp.lo[origin] = np.minimum(pp.lo[origin], -1.0)
    pp.hi[origin] = np.maximum(pp.hi[origin], 1.0)
    fp, fv, cp, ci = [0], [], [0], []
    for c in range(7):
        v, f = pp.component(c)
        v = v[~const[v]]
        fv.extend(v.tolist()); fp.append(len(fv)); ci.extend(f.tolist()); cp.append(len(ci))
    # the lonely variable: id N, read by no factor, component 7 with an empty factor list
    lonely = pp.nvars
    pp.x0, pp.lo, pp.hi = np.r_[pp.x0, 0.25], np.r_[pp.lo, -1.0], np.r_[pp.hi, 1.0]
    const = np.r_[const, False]
    fv.append(lonely); fp.append(len(fv)); cp.append(len(ci))
    comps = tuple(np.array(a, dtype=np.int64) for a in (fp, fv, cp, ci))
    fva = comps[1]
    solved = fva[:-1]
    inside = pp.x0.copy()
    outside = pp.x0.copy()
    outside[solved] += 3.0 * (pp.hi[solved] - pp.lo[solved]) * np.where(np.arange(solved.shape[0]) % 2 == 0, 1.0, -1.0)
    assert np.all((outside[solved] > pp.hi[solved]) | (outside[solved] < pp.lo[solved]))
    outside[lonely] = 7.0                                  # (outside its domain too: an empty component does not even clamp)
    nan_x = pp.x0.copy()
    nan_x[origin] = 0.0
    X = np.stack([inside, outside, nan_x])
    opts = {"coop_group_min_factors": 0, "coop_min_factors": 0}
    seq = [sequential(gctx, pp, X[s], [comps], 12, opts)[0] for s in range(3)]

    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    plan = capi.Plan(g, *comps)
    set_options(plan, opts)
    plan.solve_population(pop, 12, 3e-8)
    pr = plan.fetch_population()
    assert plan.info("components_lds") >= 7
    assert_step_equals(pr, pop, seq)
    xs = pr.x[:, :-1]
    assert np.all(xs >= pp.lo[solved]) and np.all(xs <= pp.hi[solved])
    assert np.any((xs[0] == pp.lo[solved]) | (xs[0] == pp.hi[solved]))                 # the clamp was active
    assert (pr.status[2, 1] & 0xFF) == 5 and (pr.status[2, 1] & capi.STATUS_ROLLED_BACK)
    assert np.array_equal(pr.x[2, fp[1]:fp[2]], nan_x[fva[fp[1]:fp[2]]])
    assert np.all(pr.delta[:2, :7] <= 0) and np.all(np.isfinite(pr.fret[0]))
    others = [c for c in range(7) if c != 1]
    assert pr.fret[2, others].tobytes() == pr.fret[0, others].tobytes()                # (member 2 differs from member 0 in component 1 only)
    assert np.all(pr.status[:, 7] == 6) and np.all(pr.fret[:, 7] == 0) and np.all(pr.iters[:, 7] == 0)
    after = pop.get_x()
    assert after.shape == X.shape
    assert after[:, lonely].tobytes() == X[:, lonely].tobytes() and pr.x[:, -1].tobytes() == X[:, lonely].tobytes()
    assert after[:, const].tobytes() == X[:, const].tobytes()
    assert g.get_x().tobytes() == pp.x0.tobytes()


def _sinusoid_from_the_committed_start():
    pp = P.make_high_dim_sinusoid()
    with open(os.path.join(os.path.dirname(__file__), "golden", "sinusoid_start.json")) as fh:
        pp.x0 = np.array(json.load(fh)["x0"])
    return pp


@pytest.mark.parametrize("case", ["ladybug", "the sinusoid"])
def test_population_eval(gctx, case):
    """f[s] == Problem.eval(fac) with member s's x assigned on a fresh problem: all factors, an explicit list of at most 512
    entries, a longer explicit list -- on full ladybug the long lists take the rotation-records branch (rebuilt from the member's
    x), the short one the per-factor branch.  The problem's own x is unchanged afterwards."""
    pp = P.load_bal() if case == "ladybug" else _sinusoid_from_the_committed_start()
    rng = np.random.default_rng(3)
    X = np.stack([pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)), pp.x0 * (1 + 1e-2 * rng.standard_normal(pp.nvars))])
    short = rng.choice(pp.nfac, size=150, replace=False).astype(np.int64)
    long_ = rng.permutation(pp.nfac)[:max(513, (3 * pp.nfac) // 4)].astype(np.int64) if pp.nfac > 600 else np.r_[np.arange(pp.nfac), np.arange(pp.nfac)].astype(np.int64)
    assert short.shape[0] <= 512 < long_.shape[0]
    if case == "ladybug":
        assert long_.shape[0] >= 4 * int(pp.meta["ncams"]) > short.shape[0]
    lists = [None, short, long_]
    want = []
    for s in range(2):
        h = capi.Problem(gctx, pp)
        h.set_x(X[s])
        want.append([h.eval(fac) for fac in lists])
        h.close()
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    f0 = g.eval()
    fd, _ = g.eval_grad_device()
    for k, fac in enumerate(lists):
        f = pop.eval(fac)
        assert f.shape == (2,) and f.dtype == np.float64
        assert f[0] == want[0][k] and f[1] == want[1][k], (k, f, want)
        assert want[0][k] != want[1][k]
    assert np.frombuffer(gctx.copy_to_host(fd, 8), dtype=np.float64)[0] == f0          # the problem's scalar as eval_grad_device left it
    assert g.get_x().tobytes() == pp.x0.tobytes() and g.eval() == f0
    assert pop.get_x().tobytes() == X.tobytes()


def test_set_get_assign(gctx):
    """set_x / get_x round trips with and without an id list over a member range; create(x=None) copies the assigned x;
    assign(s) makes member s the problem's x, from which set_start(None) + solve continues as sequential does"""
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    rng = np.random.default_rng(13)
    g = capi.Problem(gctx, pp)
    moved = pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars))
    g.set_x(moved)
    pop = capi.Population(g, 4)
    assert pop.get_x().tobytes() == np.stack([moved] * 4).tobytes()
    g.set_x(pp.x0)
    # whole rows over a range
    rows = rng.standard_normal((2, pp.nvars))
    pop.set_x(rows, first=1, count=2)
    got = pop.get_x()
    assert got[1:3].tobytes() == rows.tobytes() and got[0].tobytes() == moved.tobytes() and got[3].tobytes() == moved.tobytes()
    assert pop.get_x(first=1, count=2).tobytes() == rows.tobytes() and pop.get_x(2).tobytes() == rows[1].tobytes()
    # the first n variables (no id list), and an id list in no particular order
    head = rng.standard_normal((3, 7))
    pop.set_x(head, first=1)
    assert pop.get_x(first=1)[:, :7].tobytes() == head.tobytes() and pop.get_x(first=1, count=2)[:, 7:].tobytes() == rows[:, 7:].tobytes()
    vid = rng.permutation(pp.nvars)[:11].astype(np.int64)
    vals = rng.standard_normal((4, 11))
    pop.set_x(vals, vid=vid)
    assert pop.get_x(vid=vid).tobytes() == vals.tobytes()
    assert pop.get_x(3, vid=vid[::-1].copy()).tobytes() == vals[3, ::-1].tobytes()
    untouched = np.ones(pp.nvars, dtype=bool)
    untouched[vid] = False
    assert pop.get_x(0)[untouched].tobytes() == moved[untouched].tobytes()
    # out of range: refused, nothing written
    for call in (lambda: pop.set_x(vals, vid=vid, first=1, count=4), lambda: pop.get_x(first=3, count=2), lambda: pop.get_x(4),
                 lambda: pop.set_x(vals[:, :1], vid=np.array([pp.nvars])), lambda: pop.assign(4)):
        with pytest.raises(capi.RdisHipError) as e:
            call()
        assert e.value.code == -1
    assert g.get_x().tobytes() == pp.x0.tobytes()
    # assign, and continue from it
    X = members_5_30(pp)
    pop.set_x(X, count=3)
    pop.assign(2)
    assert g.get_x().tobytes() == pop.get_x(2).tobytes() == X[2].tobytes()
    plan = capi.Plan(g, *cams)
    plan.set_start(None)
    plan.solve(25, 3e-8)
    r = plan.fetch()
    (want, x_want), = sequential(gctx, pp, X[2], [cams], 25)
    for name in FIELDS + ("x",):
        assert getattr(r, name).tobytes() == getattr(want, name).tobytes(), name
    assert g.get_x().tobytes() == x_want.tobytes()
    assert pop.get_x(2).tobytes() == X[2].tobytes()


def _refused(call):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1 and len(str(e.value).split(":", 1)[1].strip()) > 0, e.value
    return str(e.value)


def test_refusals_leave_everything_usable(gctx):
    """what this version does not do is refused with EINVAL and a message that names the cause; afterwards a plain solve on the
    plan and a valid population solve both succeed"""
    def usable(plan, start):
        plan.set_start(start)
        plan.solve(2, 3e-8)
        assert np.all(np.isfinite(plan.fetch().fret))

    full = P.load_bal()
    cams, pts = P.ba_alternation_plans(full)
    g = capi.Problem(gctx, full)
    pop = capi.Population(g, 2)
    # the whole of ladybug as one component: a cooperative group
    fv, fc = np.arange(full.nvars, dtype=np.int64), np.arange(full.nfac, dtype=np.int64)
    plan = capi.Plan(g, np.array([0, full.nvars]), fv, np.array([0, full.nfac]), fc)
    msg = _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    assert "cooperative" in msg and "tiny" not in msg, msg
    usable(plan, full.x0)
    plan.close()
    # its point plan with default options: the tiny-component solver
    plan = capi.Plan(g, *pts)
    msg = _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    assert "tiny" in msg and "cooperative" not in msg, msg
    usable(plan, full.x0[pts[1]])
    # ... which a large row_min_components keeps on the LDS-resident solver: a valid population solve on the same plan
    plan.set_option("row_min_components", 1 << 40)
    assert plan.info("components_lds") == plan.ncomp
    plan.solve_population(pop, 2, 3e-8)
    assert np.all(np.isfinite(plan.fetch_population(want_x=False).fret))
    g.close()

    pp = P.load_bal(ncams=5, npts=30).single_component()
    g = capi.Problem(gctx, pp)
    other = capi.Problem(gctx, pp)
    pop, pop_other = capi.Population(g, 2), capi.Population(other, 2)
    plan = capi.Plan(g)

    def valid():
        usable(plan, pp.x0)
        fresh = capi.Population(g, x=np.stack([pp.x0] * 2))       # (not create(NULL): the plain solve above moved the assigned x)
        plan.solve_population(fresh, 25, 3e-8)
        assert plan.fetch_population().fret[1, 0] == 25.168503286225235          # (config 3's number, tests/test_gpu_multistart.py)
        fresh.close()

    assert "fetch" in _refused(lambda: plan.fetch_population())
    plan.set_option("factor_rounding", 1)
    assert "factor_rounding" in _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    plan.set_option("factor_rounding", -1)
    valid()
    plan.set_option("trace_records", 16)
    assert "trace_records" in _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    plan.set_option("trace_records", 0)
    valid()
    assert "another problem" in _refused(lambda: plan.solve_population(pop_other, 2, 3e-8))
    valid()
    assert "nmembers" in _refused(lambda: capi.Population(g, 0))
    valid()
    # the two kinds of fetch do not serve each other's solves
    assert "fetch_starts" in _refused(lambda: plan.fetch_starts())
    plan.solve_starts(pp.x0[None, :], 25, 3e-8)
    assert "fetch_population" in _refused(lambda: plan.fetch_population())
    assert plan.fetch_starts().fret[0, 0] == 25.168503286225235
    valid()
    assert pop.get_x().tobytes() == np.stack([pp.x0] * 2).tobytes()            # (no refused call wrote a member)
    g.close()
    other.close()

    # a nonlinear-product plan: the population itself works for that kind (test_population_eval), the solve is refused
    sn = _sinusoid_from_the_committed_start().single_component()
    g = capi.Problem(gctx, sn)
    pop = capi.Population(g, 2)
    plan = capi.Plan(g)
    assert "nonlinear-product" in _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    usable(plan, sn.x0)
    plan.solve_starts(sn.x0[None, :], 2, 3e-8)
    assert np.all(np.isfinite(plan.fetch_starts().fret))
