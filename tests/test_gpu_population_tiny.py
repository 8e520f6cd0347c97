"""Population solves on the tiny-component solver: rdis_hip_plan_solve_population with the plan option population_tiny = 1
(solver_quad_population.hpp: a few lanes per (component, member), persistent groups per member, rotation records per member).

Every (member, component) must be, bit for bit, what set_start(None) / solve / fetch returns on a fresh Problem whose assigned x
is that member's, with the SAME plan options ("sequential" below), and the member's x afterwards must be that problem's x.
Every comparison is == or byte equality.  No test here times anything."""
import dataclasses

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval")
LANES = {16: {"population_tiny": 1, "row_min_components": 1}, 4: {"population_tiny": 1, "quad_min_components": 1}}


def set_options(plan, opts):
    for k, v in (opts or {}).items():
        plan.set_option(k, v)


def sequential(gctx, pp, x, steps, maxiters):
    """a fresh Problem with x assigned; per step (a decomposition and its plan options) set_start(None), solve, fetch, get_x.
    steps: [(comps, opts)]; returns [(BatchResult, x after the step)] per step."""
    g = capi.Problem(gctx, pp)
    g.set_x(x)
    plans = {}
    out = []
    for comps, opts in steps:
        key = id(comps)
        if key not in plans:
            plans[key] = capi.Plan(g, *comps)
            set_options(plans[key], opts)
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


def same_bytes(a, b):
    return all(getattr(a, name).tobytes() == getattr(b, name).tobytes() for name in FIELDS + ("x",))


def members_5_30(pp):
    rng = np.random.default_rng(7)
    return np.stack([pp.x0, pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)), pp.x0 * (1 + 1e-2 * rng.standard_normal(pp.nvars))])


@pytest.mark.parametrize("lanes", [16, 4])
def test_alternation_equals_sequential_and_the_oracle(gctx, lanes):
    """ladybug 5 / 30, three members that differ in ALL variables, two rounds of camera plan (LDS-resident solver) then point plan
    (tiny-component solver, 16 or 4 lanes a point): after each of the four solves every field, every xout row and every member's
    whole x == the sequential run; the point step of members 0 and 1 differs; member 1's first point step == the oracle's run of
    that solver with the member's x at that moment assigned (its own cameras, as its camera step left them), on all seven fields"""
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    X = members_5_30(pp)
    steps = [(cams, None), (pts, LANES[lanes]), (cams, None), (pts, LANES[lanes])]
    seq = [sequential(gctx, pp, X[s], steps, 25) for s in range(3)]

    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    plan_c, plan_p = capi.Plan(g, *cams), capi.Plan(g, *pts)
    set_options(plan_p, LANES[lanes])
    assert plan_c.info("components_lds") == 5 and plan_p.info("components_tiny") == 30
    results = []
    for k, (comps, _) in enumerate(steps):
        plan = plan_c if comps is cams else plan_p
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert pr.best is None and pr.x.shape == (3, plan.nfree) and pr.fret.shape == (3, plan.ncomp)
        assert_step_equals(pr, pop, [seq[s][k] for s in range(3)], "step %d" % k)
        results.append(pr)
    assert np.all(results[1].fret[0] != results[1].fret[1])
    # the oracle: member 1's first point step; its constants are the member's cameras after its camera step
    fp, fv, cp, ci = pts
    x1 = seq[1][0][1]
    assert x1[:45].tobytes() != X[1][:45].tobytes() and x1[:45].tobytes() != seq[0][0][1][:45].tobytes()
    o = O.OracleProblem.device_group_default(dataclasses.replace(pp, x0=x1.copy()), lanes=lanes)
    r = results[1]
    for c in (0, 7, 16, 29):
        v, f = fv[fp[c]:fp[c + 1]], ci[cp[c]:cp[c + 1]]
        want = o.cgd(free_vid=v, fac=f, x=x1[v], maxiters=25)
        o.assign(v, x1[v])   # (the oracle leaves the component assigned at its end point: back to the start)
        assert r.fret[1, c] == want.fret and r.delta[1, c] == want.delta and r.x[1, fp[c]:fp[c + 1]].tobytes() == want.x.tobytes(), (c, r.fret[1, c], want.fret)
        assert (int(r.iters[1, c]), int(r.status[1, c]), int(r.nfeval[1, c]), int(r.ngeval[1, c])) == (want.iters, want.status, want.nfeval, want.ngeval), c


class Points12:
    """ladybug 12 / 300: its point plan (300 tiny components), four members whose cameras (and points) differ, and their
    sequential runs, computed once per group size and shared by the tests below (never modified)"""

    def __init__(self, gctx):
        self.gctx = gctx
        self.pp = P.load_bal(ncams=12, npts=300)
        self.pts = P.ba_alternation_plans(self.pp)[1]
        rng = np.random.default_rng(19)
        self.X = np.stack([self.pp.x0] + [self.pp.x0 * (1 + 1e-3 * rng.standard_normal(self.pp.nvars)) for _ in range(3)])
        assert len({self.X[s, :108].tobytes() for s in range(4)}) == 4
        self._seq = {}

    def seq(self, lanes):
        if lanes not in self._seq:
            self._seq[lanes] = [sequential(self.gctx, self.pp, self.X[s], [(self.pts, LANES[lanes])], 25)[0] for s in range(4)]
        return self._seq[lanes]


@pytest.fixture(scope="module")
def points12(gctx):
    return Points12(gctx)


@pytest.mark.parametrize("lanes", [4, 16])
def test_the_queue(gctx, points12, lanes):
    """300 points, 2 members, one block a member (tiny_max_blocks = 1): 64 groups of four lanes, or 4 groups of sixteen, walk the
    300 components of their member through the member's own queue counter -- the bytes of a launch with as many blocks as there
    are first components, and both == sequential"""
    pp, pts = points12.pp, points12.pts
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *pts)
    set_options(plan, LANES[lanes])
    out = {}
    for blocks in (1, 0):
        plan.set_option("tiny_max_blocks", blocks)
        pop = capi.Population(g, x=points12.X[:2])
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.info("components_tiny") == 300 and plan.last_kernel_ms()[1] == 1
        want_blocks = 1 if blocks else -(-300 // (64 if lanes == 4 else 4))
        assert plan.info("population_tiny_blocks") == want_blocks
        assert_step_equals(pr, pop, points12.seq(lanes)[:2], "tiny_max_blocks %d" % blocks)
        out[blocks] = pr
        pop.close()
    assert same_bytes(out[0], out[1])


def test_split_launches_and_stale_records(gctx, points12):
    """4 members whose cameras differ: a budget of one byte gives 4 launches on ONE replica of the rotation records (a replica
    that was not rebuilt for the launch's member holds the previous member's cameras), a budget of three replicas 3 + 1, the
    default 1 -- the same bytes every time, all == sequential.  One replica, measured through device_bytes(), is at least 8 N
    bytes: the records."""
    pp, pts, X = points12.pp, points12.pts, points12.X
    seq = points12.seq(16)
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *pts)
    set_options(plan, LANES[16])
    # with a budget of one byte a launch holds one replica whatever the number of members: a second member adds its inputs
    # and outputs only
    plan.set_option("starts_workspace_bytes", 1)
    grow = [plan.device_bytes()]
    for n in (1, 2):
        few = capi.Population(g, x=X[:n])
        plan.solve_population(few, 25, 3e-8)
        plan.fetch_population(want_x=False)
        grow.append(plan.device_bytes())
        few.close()
    rep = (grow[1] - grow[0]) - (grow[2] - grow[1])
    assert rep >= 8 * pp.nvars

    def run(budget, per_launch, launches):
        pop = capi.Population(g, x=X)
        plan.set_option("starts_workspace_bytes", budget)
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.info("starts_per_launch") == per_launch and plan.info("starts_launches") == launches
        assert plan.last_kernel_ms()[1] == launches
        assert_step_equals(pr, pop, seq, "budget %d" % budget)
        pop.close()
        return pr

    one_byte = run(1, 1, 4)
    split = run(3 * rep + rep // 2, 3, 2)
    whole = run(1 << 30, 4, 1)
    assert same_bytes(one_byte, split) and same_bytes(split, whole)


def test_records_off(gctx, points12):
    """camera_records = 0: no replica of the records, every factor forms its rotation from the member's row -- the bytes of
    camera_records = 1, for all members (and so the sequential run's)"""
    pp, pts, X = points12.pp, points12.pts, points12.X
    g = capi.Problem(gctx, pp)
    out = {}
    for rec in (1, 0):
        plan = capi.Plan(g, *pts)
        set_options(plan, LANES[16])
        plan.set_option("camera_records", rec)
        plan.set_option("starts_workspace_bytes", 1)     # (a replica of the records would be rebuilt four times)
        pop = capi.Population(g, x=X)
        plan.solve_population(pop, 25, 3e-8)
        out[rec] = (plan.fetch_population(), pop.get_x())
        assert plan.info("starts_launches") == (4 if rec else 1)     # (without records a replica holds nothing: one launch)
        pop.close()
        plan.close()
    assert same_bytes(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()
    for s, (r, x_after) in enumerate(points12.seq(16)):
        assert out[0][0].x[s].tobytes() == r.x.tobytes() and out[0][0].fret[s].tobytes() == r.fret.tobytes() and out[0][1][s].tobytes() == x_after.tobytes()


@pytest.mark.parametrize("lanes", [4, 16])
def test_partial_blocks_bounds_rollback_and_an_empty_component(gctx, lanes):
    """ladybug 49 / 300 with the tightened domains of test_quad_solver_partial_blocks_and_active_bounds: components of 1 .. 3 free
    coordinates of a point (the rest constants), one component without factors (a variable no factor reads), and four members:
    the start; a perturbed one; one whose free values lie outside [lo, hi] (clamped at entry); one that makes a component's
    objective NaN at its start (its point and one of its cameras' translation at the origin) -- returned restored, ROLLED_BACK.
    Everything == sequential; some results sit on a bound; the empty component reports EXIT_EMPTY, its variable untouched."""
    rng = np.random.default_rng(23)
    pp = P.load_bal(ncams=49, npts=300)
    pp.lo[441:] = pp.x0[441:] - rng.uniform(0.002, 0.05, pp.nvars - 441)
    pp.hi[441:] = pp.x0[441:] + rng.uniform(0.002, 0.05, pp.nvars - 441)
    lonely = pp.nvars                                     # read by no factor: a component with an empty factor list
    pp.x0, pp.lo, pp.hi = np.r_[pp.x0, 0.25], np.r_[pp.lo, -1.0], np.r_[pp.hi, 1.0]
    a = np.ones(pp.nvars, np.uint8)
    keep = rng.random(300) < 0.7
    for p in np.where(keep)[0]:                           # free 1 .. 3 coordinates of 70 % of the points
        k = rng.integers(1, 4)
        a[441 + 3 * p + rng.choice(3, size=k, replace=False)] = 0
    h = capi.Problem(gctx, pp)
    fp, fv, cp, ci = h.components(a)
    h.close()
    assert set(np.diff(fp)) == {1, 2, 3} and np.all(np.diff(cp) > 0)
    # the NaN member's component: one with all three coordinates free
    cn = int(np.where(np.diff(fp) == 3)[0][0])
    f0 = int(ci[cp[cn]])
    cam, pt = int(pp.cam_vid0[f0]), int(pp.pt_vid0[f0])
    assert sorted(fv[fp[cn]:fp[cn + 1]].tolist()) == [pt, pt + 1, pt + 2]
    pp.lo[pt:pt + 3] = np.minimum(pp.lo[pt:pt + 3], -1.0)
    pp.hi[pt:pt + 3] = np.maximum(pp.hi[pt:pt + 3], 1.0)
    ncomp = len(fp)                                       # (with the lonely one)
    comps = (np.r_[fp, fp[-1] + 1], np.r_[fv, lonely], np.r_[cp, cp[-1]], ci)
    fp, fv, cp, ci = comps
    solved = fv[:-1]
    inside = pp.x0.copy()
    moved = pp.x0.copy()
    moved[:441] *= 1 + 1e-3 * rng.standard_normal(441)
    outside = pp.x0.copy()
    outside[solved] += 3.0 * (pp.hi[solved] - pp.lo[solved]) * np.where(np.arange(solved.shape[0]) % 2 == 0, 1.0, -1.0)
    assert np.all((outside[solved] > pp.hi[solved]) | (outside[solved] < pp.lo[solved]))
    outside[lonely] = 7.0                                 # (outside its domain too: an empty component does not even clamp)
    nan_x = pp.x0.copy()
    nan_x[pt:pt + 3] = 0.0
    nan_x[cam + 3:cam + 6] = 0.0
    X = np.stack([inside, moved, outside, nan_x])
    seq = [sequential(gctx, pp, X[s], [(comps, LANES[lanes])], 25)[0] for s in range(4)]

    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    plan = capi.Plan(g, *comps)
    set_options(plan, LANES[lanes])
    plan.solve_population(pop, 25, 3e-8)
    pr = plan.fetch_population()
    assert plan.info("components_tiny") == ncomp == plan.ncomp and plan.last_kernel_ms()[1] == 1
    assert_step_equals(pr, pop, seq)
    xs = pr.x[:, :-1]
    assert np.all(xs >= pp.lo[solved]) and np.all(xs <= pp.hi[solved])
    for s in range(3):
        assert np.any((xs[s] == pp.lo[solved]) | (xs[s] == pp.hi[solved])), s          # some results sit on their bounds
    assert pr.status[3, cn] & capi.STATUS_ROLLED_BACK
    assert np.array_equal(pr.x[3, fp[cn]:fp[cn + 1]], nan_x[fv[fp[cn]:fp[cn + 1]]])
    assert np.all(pr.status[:, -1] == 6) and np.all(pr.fret[:, -1] == 0) and np.all(pr.iters[:, -1] == 0)      # EXIT_EMPTY
    after = pop.get_x()
    assert after[:, lonely].tobytes() == X[:, lonely].tobytes() and pr.x[:, -1].tobytes() == X[:, lonely].tobytes()
    assert after[:, a != 0].tobytes() == X[:, a != 0].tobytes()                        # what is not free is what was put in
    assert g.get_x().tobytes() == pp.x0.tobytes()


def test_mixed_plan(gctx):
    """six blocks of 3 cameras x 40 points: three stay whole components on the LDS-resident solver, three have their cameras
    fixed, so every point of theirs is a tiny component -- one plan, two solver launches per chunk of members (the group kernel
    on the tiny components, then the LDS-resident kernel on the rest of the batch list); 3 members == sequential, in one chunk
    and one member at a time"""
    pp = P.make_synthetic_ba(6, 3, 40)
    fp, fv, cp, ci = [0], [], [0], []
    for c in range(3):
        v, f = pp.component(c)
        fv.extend(v.tolist()); fp.append(len(fv)); ci.extend(f.tolist()); cp.append(len(ci))
    for c in range(3, 6):
        v, f = pp.component(c)
        for q in np.unique(pp.pt_vid0[f]):
            fq = f[pp.pt_vid0[f] == q]
            fv.extend([int(q), int(q) + 1, int(q) + 2]); fp.append(len(fv)); ci.extend(fq.tolist()); cp.append(len(ci))
    comps = tuple(np.array(t, dtype=np.int64) for t in (fp, fv, cp, ci))
    opts = dict(LANES[16], coop_min_factors=0, coop_group_min_factors=0)
    rng = np.random.default_rng(29)
    X = np.stack([pp.x0] + [pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)) for _ in range(2)])
    seq = [sequential(gctx, pp, X[s], [(comps, opts)], 25)[0] for s in range(3)]
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *comps)
    set_options(plan, opts)
    assert plan.info("components_tiny") == 120 and plan.info("components_lds") == 3
    out = []
    for budget, launches in ((1 << 30, 2), (1, 6)):
        plan.set_option("starts_workspace_bytes", budget)
        pop = capi.Population(g, x=X)
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.last_kernel_ms()[1] == launches and plan.info("starts_launches") == launches
        assert_step_equals(pr, pop, seq, "budget %d" % budget)
        out.append(pr)
        pop.close()
    assert same_bytes(out[0], out[1])


def _refused(call):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1 and len(str(e.value).split(":", 1)[1].strip()) > 0, e.value
    return str(e.value)


def test_refusals_and_nothing_else_moves(gctx, points12):
    """without the option the refusal of a plan with tiny components names it; with it a cooperative component and a trace are
    refused as before; after each refusal a plain solve and a valid population solve work.  A population solve leaves the
    problem's x, the plan's ordinary outputs and its objective alone, and an ordinary solve on the same plan afterwards has the
    sequential bytes (the problem's own rotation records and queue counter are intact)."""
    def usable(plan, start):
        plan.set_start(start)
        plan.solve(2, 3e-8)
        assert np.all(np.isfinite(plan.fetch().fret))

    full = P.load_bal()
    _, pts = P.ba_alternation_plans(full)
    g = capi.Problem(gctx, full)
    pop = capi.Population(g, 2)
    plan = capi.Plan(g, *pts)
    msg = _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    assert "population_tiny" in msg and "tiny" in msg and "cooperative" not in msg, msg
    usable(plan, full.x0[pts[1]])
    plan.set_option("population_tiny", 1)
    assert plan.info("components_tiny") == plan.ncomp
    plan.solve_population(pop, 2, 3e-8)
    assert np.all(np.isfinite(plan.fetch_population(want_x=False).fret))
    # the multi-start entry keeps refusing tiny components, option or not
    assert "tiny" in _refused(lambda: plan.solve_starts(full.x0[pts[1]][None, :], 2, 3e-8))
    plan.set_option("trace_records", 16)
    assert "trace_records" in _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    plan.set_option("trace_records", 0)
    usable(plan, full.x0[pts[1]])
    plan.solve_population(pop, 2, 3e-8)
    assert np.all(np.isfinite(plan.fetch_population(want_x=False).fret))
    plan.close()
    # the whole of ladybug as one component: a cooperative group, option or not
    fv, fc = np.arange(full.nvars, dtype=np.int64), np.arange(full.nfac, dtype=np.int64)
    plan = capi.Plan(g, np.array([0, full.nvars]), fv, np.array([0, full.nfac]), fc)
    plan.set_option("population_tiny", 1)
    msg = _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    assert "cooperative" in msg and "tiny" not in msg, msg
    usable(plan, full.x0)
    g.close()

    # nothing else moves
    pp, pts, X = points12.pp, points12.pts, points12.X
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *pts)
    set_options(plan, LANES[16])
    plan.set_start(X[1][pts[1]])
    plan.solve(25, 3e-8)
    before, x_before, obj_before = plan.fetch(), g.get_x(), plan.objective()
    pop = capi.Population(g, x=X[:2])
    plan.solve_population(pop, 25, 3e-8)
    pr = plan.fetch_population()
    assert g.get_x().tobytes() == x_before.tobytes()
    assert same_bytes(plan.fetch(), before) and plan.objective() == obj_before
    assert_step_equals(pr, pop, points12.seq(16)[:2])
    g.set_x(pp.x0)
    plan.set_start(None)
    plan.solve(25, 3e-8)
    want, x_want = points12.seq(16)[0]
    assert same_bytes(plan.fetch(), want) and g.get_x().tobytes() == x_want.tobytes()
