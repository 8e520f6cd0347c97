"""Population solves on the cooperative solver: rdis_hip_plan_solve_population_cooperative (Plan.solve_population(...,
cooperative=True); solver_coop_population.hpp: a cooperative group per (member, component), the groups of all members of a
launch side by side in one cooperative launch).

Every (member, component) must be, bit for bit, what a fresh Problem whose x is the member's row returns from set_start(None) /
solve / fetch / get_x on the same plan options ("sequential" below) -- with coop_pipeline = 0, the layout the population kernel
runs, AND with coop_pipeline = 1, the layout optimize() uses -- and the member's whole row afterwards must be that problem's x.
Every comparison is == or byte equality; no solve may end with an exchange that gave up (status & 0xFF == 7).  Every shape runs
once with factor_rounding at its default (the reference-rounding instantiation) and once at 0 (the fused one).  The shapes are
those tests/test_gpu_solver.py uses for the cooperative solver, at 6 - 10 iterations.  No test here times anything."""
import copy

import numpy as np
import pytest

from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval")
FTOL = 3e-8
ROUNDINGS = pytest.mark.parametrize("rounding", (None, 0), ids=("default rounding", "fused"))


def set_options(plan, opts):
    for k, v in (opts or {}).items():
        plan.set_option(k, v)


def with_rounding(opts, rounding):
    return dict(opts) if rounding is None else dict(opts, factor_rounding=rounding)


def whole(pp):
    """the decomposition with one component: everything"""
    return (np.array([0, pp.nvars], dtype=np.int64), np.arange(pp.nvars, dtype=np.int64),
            np.array([0, pp.nfac], dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))


def sequential(gctx, pp, comps, opts, x, iters):
    """a fresh Problem whose x is the member's row, the same plan options, set_start(None), solve, fetch, get_x"""
    g = capi.Problem(gctx, pp)
    g.set_x(x)
    plan = capi.Plan(g, *comps)
    set_options(plan, opts)
    plan.set_start(None)
    plan.solve(iters, FTOL)
    out = (plan.fetch(), g.get_x(), plan.info("components_cooperative"), plan.info("pipelined"))
    plan.close()
    g.close()
    return out


def sequential_both(gctx, pp, comps, opts, X, iters):
    """{coop_pipeline: [per member (BatchResult, x after, cooperative components, pipelined)]}"""
    return {pipe: [sequential(gctx, pp, comps, dict(opts, coop_pipeline=pipe), x, iters) for x in X] for pipe in (0, 1)}


def assert_rows(pr, rows, seq, where, members=None):
    """pr: fetch_population(); rows[i]: the population's row of fetch row i afterwards; seq: sequential_both's answer;
    members[i]: the member (index into seq's lists) fetch row i belongs to"""
    members = range(len(rows)) if members is None else members
    assert np.all((pr.status & 0xFF) != 7), where                    # no exchange gave up
    for pipe in (0, 1):
        for i, s in enumerate(members):
            r, x_after, ncoop, _ = seq[pipe][s]
            assert np.all((r.status & 0xFF) != 7), (where, pipe, s)
            for name in FIELDS:
                a, b = getattr(pr, name)[i], getattr(r, name)
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, "coop_pipeline", pipe, "member", s, name, a, b)
            assert pr.x[i].tobytes() == r.x.tobytes(), (where, "coop_pipeline", pipe, "member", s, "x of the components")
            assert rows[i].tobytes() == x_after.tobytes(), (where, "coop_pipeline", pipe, "member", s, "the whole row")


def population_solve(gctx, pp, comps, opts, X, iters, first=0, count=None, plan_opts_late=None):
    """the plan (coop_pipeline = 0) on a population of rows X through the cooperative entry:
    (fetch_population(), the rows of the solved range afterwards, every row afterwards, infos)"""
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    plan = capi.Plan(g, *comps)
    set_options(plan, dict(opts, coop_pipeline=0))
    set_options(plan, plan_opts_late)
    plan.solve_population(pop, iters, FTOL, first=first, count=count, cooperative=True)
    pr = plan.fetch_population()
    n = len(X) - first if count is None else count
    every = [pop.get_x(s) for s in range(len(X))]
    info = {k: plan.info(k) for k in ("starts_per_launch", "starts_launches", "population_cooperative_workgroups", "population_cooperative_cap",
                                      "components_cooperative", "components_lds", "components_tiny", "pipelined")}
    info["launches"] = plan.last_kernel_ms()[1]
    info["problem_x"] = g.get_x()
    plan.close(); pop.close(); g.close()
    return pr, every[first:first + n], every, info


def noisy(x0, n, seed, rel=1e-3):
    return x0 * (1 + rel * np.random.default_rng(seed).standard_normal((n, x0.shape[0])))


# ---- shape 1: one group ------------------------------------------------------------------------------------------------

ONE = {"coop_min_factors": 1000}


class OneGroup:
    """make_synthetic_ba(1, 3, 900, obs_per_pt=3) as one component (2700 factors: eleven workgroups), four members -- x0, x0 with
    1e-3 relative noise, the state after a previous solve, x0 with one NaN coordinate -- and their sequential runs per rounding,
    computed once and shared by the tests below (never modified)"""
    ITERS = 8

    def __init__(self, gctx):
        self.gctx = gctx
        self.pp = P.make_synthetic_ba(1, 3, 900, obs_per_pt=3)
        self.comps = whole(self.pp)
        x0 = self.pp.x0
        after = sequential(gctx, self.pp, self.comps, dict(ONE, coop_pipeline=0), x0, self.ITERS)[1]
        nan = x0.copy()
        nan[40] = np.nan                       # (a point's coordinate)
        self.X = np.vstack([x0[None, :], noisy(x0, 1, 21), after[None, :], nan[None, :]])
        self._seq = {}

    def seq(self, rounding):
        if rounding not in self._seq:
            self._seq[rounding] = sequential_both(self.gctx, self.pp, self.comps, with_rounding(ONE, rounding), self.X, self.ITERS)
        return self._seq[rounding]


@pytest.fixture(scope="module")
def one(gctx):
    return OneGroup(gctx)


@ROUNDINGS
def test_one_group_four_members(one, rounding):
    """x0, a perturbed start, the state after a solve and a start with a NaN: every member ends as its sequential solve ends --
    the NaN member too, and the others are untouched by it.  Refused before the entry existed."""
    seq = one.seq(rounding)
    pr, rows, _, info = population_solve(one.gctx, one.pp, one.comps, with_rounding(ONE, rounding), one.X, one.ITERS)
    print("one group:", info["population_cooperative_workgroups"], "workgroups a member, cap", info["population_cooperative_cap"], "members a launch",
          info["starts_per_launch"], "fret", pr.fret[:, 0])
    assert info["components_cooperative"] == 1 and info["pipelined"] == 0
    assert [s[2] for s in seq[0]] == [1] * 4 and [s[3] for s in seq[1]] == [1] * 4       # the sequential runs: cooperative too; pipelined with coop_pipeline = 1
    assert pr.best is None and pr.x.shape == (4, one.pp.nvars) and pr.fret.shape == (4, 1)
    assert_rows(pr, rows, seq, "one group")
    assert np.all(pr.delta[:3] < 0) and np.all(pr.nfeval[:3] > 20)                       # three real solves ...
    assert pr.fret[0, 0] != pr.fret[1, 0] and pr.fret[0, 0] != pr.fret[2, 0]
    # ... and one from a NaN (the clamp of the first point takes it onto a bound: another solve than x0's, the sequential one's bits)
    assert np.isnan(one.X[3, 40]) and pr.fret[3, 0] != pr.fret[0, 0]
    assert info["problem_x"].tobytes() == one.pp.x0.tobytes()
    assert info["starts_per_launch"] * info["population_cooperative_workgroups"] <= info["population_cooperative_cap"]


# ---- shape 2: a group of one workgroup -----------------------------------------------------------------------------------

@ROUNDINGS
def test_a_group_of_one_workgroup(gctx, rounding):
    pp = P.make_synthetic_ba(1, 3, 40, obs_per_pt=3)            # 120 factors, 147 variables: one workgroup of 256 lanes
    comps, opts, iters = whole(pp), with_rounding({"coop_min_factors": 1, "coop_group_min_factors": 0}, rounding), 10
    X = np.vstack([pp.x0[None, :], noisy(pp.x0, 2, 5)])
    seq = sequential_both(gctx, pp, comps, opts, X, iters)
    pr, rows, _, info = population_solve(gctx, pp, comps, opts, X, iters)
    assert info["components_cooperative"] == 1 and info["population_cooperative_workgroups"] == 1
    assert info["starts_per_launch"] == 3 and info["starts_launches"] == 1
    assert_rows(pr, rows, seq, "one workgroup")
    assert np.all(pr.delta < 0)


# ---- shape 3: five groups side by side --------------------------------------------------------------------------------------

FIVE = {"coop_min_factors": 1000}


class FiveGroups:
    """make_synthetic_ba(5, 3, 900, obs_per_pt=3), its five components five groups of one launch; the sequential runs of up to
    six members per rounding, computed once"""
    ITERS = 10

    def __init__(self, gctx):
        self.gctx = gctx
        self.pp = P.make_synthetic_ba(5, 3, 900, obs_per_pt=3)
        pp = self.pp
        self.comps = (pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id)
        self.X = np.vstack([pp.x0[None, :], noisy(pp.x0, 5, 31)])
        self._seq = {}

    def seq(self, rounding, n):
        have = self._seq.setdefault(rounding, {0: [], 1: []})
        for pipe in (0, 1):
            while len(have[pipe]) < n:
                have[pipe].append(sequential(self.gctx, self.pp, self.comps, dict(with_rounding(FIVE, rounding), coop_pipeline=pipe),
                                             self.X[len(have[pipe])], self.ITERS))
        return {pipe: have[pipe][:n] for pipe in (0, 1)}


@pytest.fixture(scope="module")
def five(gctx):
    return FiveGroups(gctx)


@ROUNDINGS
def test_five_groups_side_by_side(five, rounding):
    seq = five.seq(rounding, 3)
    pr, rows, _, info = population_solve(five.gctx, five.pp, five.comps, with_rounding(FIVE, rounding), five.X[:3], five.ITERS)
    assert info["components_cooperative"] == 5 and pr.fret.shape == (3, 5)
    assert info["launches"] == info["starts_launches"]
    assert_rows(pr, rows, seq, "five groups")
    assert np.all(pr.delta < 0) and len({float(f) for f in pr.fret.ravel()}) == 15


# ---- shape 4: odd lane maps --------------------------------------------------------------------------------------------------

@ROUNDINGS
@pytest.mark.parametrize("shape", ((2, 1500, 2), (2, 1153, 2), (3, 1067, 3)),
                         ids=("more variables than factors", "one factor beyond a full workgroup", "a mostly empty last workgroup"))
def test_odd_lane_maps(gctx, shape, rounding):
    c, q, o = shape
    pp = P.make_synthetic_ba(1, c, q, obs_per_pt=o)
    comps, opts, iters = whole(pp), with_rounding({"coop_min_factors": 1000}, rounding), 6
    X = np.vstack([pp.x0[None, :], noisy(pp.x0, 1, 7)])
    seq = sequential_both(gctx, pp, comps, opts, X, iters)
    pr, rows, _, info = population_solve(gctx, pp, comps, opts, X, iters)
    assert info["components_cooperative"] == 1
    assert_rows(pr, rows, seq, "%d x %d x %d" % shape)
    assert np.all(pr.delta < 0)


# ---- shape 5: constants among the slots, bounds that bite (ladybug 49 / 500) ------------------------------------------------------

@ROUNDINGS
@pytest.mark.parametrize("case", ("cameras constant", "active bounds"))
def test_constants_and_active_bounds(gctx, case, rounding):
    sub = P.load_bal(ncams=49, npts=500)
    if case == "cameras constant":
        # the first 441 variables (the cameras) held constant: only lane-owned variables, factor slots that read the member's row
        pp, iters = sub, 6
        comps = (np.array([0, sub.nvars - 441], dtype=np.int64), np.arange(441, sub.nvars, dtype=np.int64),
                 np.array([0, sub.nfac], dtype=np.int64), np.arange(sub.nfac, dtype=np.int64))
        opts = {"coop_min_factors": 1000, "coop_max_components": 4}
    else:
        # every seventh variable may move 1e-4 of its size up, every eleventh down: the clamp is part of a trial's arithmetic
        pp, iters = copy.deepcopy(sub), 8
        idx = np.arange(pp.nvars)
        pp.hi = np.where(idx % 7 == 0, pp.x0 + 1e-4 * np.abs(pp.x0) + 1e-9, pp.hi)
        pp.lo = np.where(idx % 11 == 0, pp.x0 - 1e-4 * np.abs(pp.x0) - 1e-9, pp.lo)
        comps, opts = whole(pp), {"coop_min_factors": 1000}
    opts = with_rounding(opts, rounding)
    # (the second member: the first one's constants moved, inside the tight domains)
    X = np.vstack([pp.x0[None, :], np.clip(noisy(pp.x0, 1, 3, rel=1e-5), pp.lo, pp.hi)])
    seq = sequential_both(gctx, pp, comps, opts, X, iters)
    pr, rows, _, info = population_solve(gctx, pp, comps, opts, X, iters)
    assert info["components_cooperative"] == 1
    assert_rows(pr, rows, seq, case)
    assert np.all(pr.delta <= 0) and pr.fret[0, 0] != pr.fret[1, 0]
    if case == "active bounds":
        assert np.sum(pr.x[0] == pp.hi) + np.sum(pr.x[0] == pp.lo) > 10               # ... and they do bite
    else:
        assert rows[1][:441].tobytes() == X[1][:441].tobytes()                         # the member's own constants, untouched


# ---- shape 6: a mixed plan ---------------------------------------------------------------------------------------------------

def mixed_plan(pp):
    """of make_synthetic_ba(3, 3, 900, obs_per_pt=3): all of its component 0 (cooperative), the cameras and the first 40 points of
    its component 1 (LDS-resident), and 200 points of its component 2 one by one against constant cameras (tiny)"""
    per_v, per_f = pp.nvars // 3, pp.nfac // 3
    fp, fv, cp, ci = [0], [], [0], []

    def add(vids, fids):
        fv.extend(vids); ci.extend(fids); fp.append(len(fv)); cp.append(len(ci))

    add(range(per_v), range(per_f))
    v1 = list(range(per_v, per_v + 27 + 3 * 40))
    add(v1, [f for f in range(per_f, 2 * per_f) if pp.pt_vid0[f] < per_v + 27 + 3 * 40])
    for q in range(200):
        v = 2 * per_v + 27 + 3 * q
        add(range(v, v + 3), [f for f in range(2 * per_f, 3 * per_f) if pp.pt_vid0[f] == v])
    return tuple(np.array(a, dtype=np.int64) for a in (fp, fv, cp, ci))


@ROUNDINGS
def test_a_mixed_plan(gctx, rounding):
    """one cooperative component beside an LDS-resident one and tiny ones (population_tiny = 1): three launch kinds in one call"""
    pp = P.make_synthetic_ba(3, 3, 900, obs_per_pt=3)
    comps = mixed_plan(pp)
    opts = with_rounding({"coop_min_factors": 1000, "coop_group_min_factors": 0, "row_min_components": 1, "quad_min_components": 1 << 30,
                          "population_tiny": 1}, rounding)
    iters = 8
    X = np.vstack([pp.x0[None, :], noisy(pp.x0, 2, 9)])
    seq = sequential_both(gctx, pp, comps, opts, X, iters)
    pr, rows, _, info = population_solve(gctx, pp, comps, opts, X, iters)
    assert (info["components_cooperative"], info["components_lds"], info["components_tiny"]) == (1, 1, 200)
    assert info["launches"] == info["starts_launches"] == 3 * -(-3 // info["starts_per_launch"])      # cooperative, tiny, LDS-resident per range
    assert_rows(pr, rows, seq, "mixed plan")
    assert np.all(pr.delta[:, :2] < 0)


# ---- 7: the split into launches changes no bit ----------------------------------------------------------------------------------

@ROUNDINGS
def test_one_member_a_launch_and_the_default_budget(one, rounding):
    seq = one.seq(rounding)
    opts = with_rounding(ONE, rounding)
    small = population_solve(one.gctx, one.pp, one.comps, opts, one.X, one.ITERS, plan_opts_late={"starts_workspace_bytes": 1})
    dflt = population_solve(one.gctx, one.pp, one.comps, opts, one.X, one.ITERS)
    assert small[3]["starts_per_launch"] == 1 and small[3]["starts_launches"] == 4 == small[3]["launches"]
    assert dflt[3]["starts_per_launch"] >= 1 and dflt[3]["launches"] == -(-4 // dflt[3]["starts_per_launch"])
    for pr, rows, _, _ in (small, dflt):
        assert_rows(pr, rows, seq, "split")


@ROUNDINGS
def test_a_member_range(one, rounding):
    """first = 1, count = 2 of the four members: row i of the fetch is member first + i, the members outside keep their bytes"""
    seq = one.seq(rounding)
    pr, rows, every, info = population_solve(one.gctx, one.pp, one.comps, with_rounding(ONE, rounding), one.X, one.ITERS, first=1, count=2)
    assert pr.fret.shape == (2, 1) and pr.x.shape == (2, one.pp.nvars)
    assert_rows(pr, rows, seq, "range", members=(1, 2))
    assert every[0].tobytes() == one.X[0].tobytes() and every[3].tobytes() == one.X[3].tobytes()
    assert every[1].tobytes() != one.X[1].tobytes()


@ROUNDINGS
def test_a_split_bound_by_residency(five, rounding):
    """five groups with enough members that the resident workgroups, not the budget, bound a launch (where the machine allows it:
    at most six members are tried); R times the workgroups a member stays within the cap"""
    opts = with_rounding(FIVE, rounding)
    probe = population_solve(five.gctx, five.pp, five.comps, opts, five.X[:1], 1)[3]
    wg, cap = probe["population_cooperative_workgroups"], probe["population_cooperative_cap"]
    print("five groups:", wg, "workgroups a member, cap", cap)
    assert wg >= 5 and cap >= wg
    n = cap // wg + 1
    if n > 6:
        pytest.skip("the device holds %d members of %d workgroups: more than this test solves" % (cap // wg, wg))
    seq = five.seq(rounding, n)
    pr, rows, _, info = population_solve(five.gctx, five.pp, five.comps, opts, five.X[:n], five.ITERS)
    assert info["starts_per_launch"] == cap // wg < n and info["starts_launches"] == 2
    assert info["starts_per_launch"] * info["population_cooperative_workgroups"] <= info["population_cooperative_cap"]
    assert_rows(pr, rows, seq, "residency")


# ---- 8: nothing else moves; the refusals ------------------------------------------------------------------------------------------

@ROUNDINGS
def test_nothing_else_moves_and_the_refusals_leave_everything_working(one, rounding):
    """(a transient plan, which the entry refuses too, exists only inside rdis_hip_cgd_batch: no caller can hand one over)"""
    gctx, pp, comps, X, iters = one.gctx, one.pp, one.comps, one.X[:2], one.ITERS
    seq = {pipe: rows[:2] for pipe, rows in one.seq(rounding).items()}
    g = capi.Problem(gctx, pp)
    plan, second = capi.Plan(g, *comps), capi.Plan(g, *comps)
    for p in (plan, second):
        set_options(p, dict(with_rounding(ONE, rounding), coop_pipeline=0))
    # the plan's ordinary outputs and a second plan's solve, before
    plan.set_start(None); plan.solve(iters, FTOL)
    before = plan.fetch()
    g.set_x(pp.x0)
    second.set_start(None); second.solve(iters, FTOL)
    second_before = second.fetch()
    g.set_x(pp.x0)
    pop = capi.Population(g, x=X)
    other = capi.Problem(gctx, pp)
    foreign = capi.Population(other, x=X)

    def refused(match, options=None, **kw):
        """the call with `options` set is refused with its message before any row is written; with the options put back the plan
        and the population work: the solve of both members has the sequential bits"""
        was = {"coop_pipeline": 0, "factor_rounding": -1 if rounding is None else rounding, "emulate_stale_cache": 0, "trace_records": 0, "dump_iters": 0,
               "force_stream": 0, "ptm_stream": 1}
        set_options(plan, options)
        with pytest.raises(capi.RdisHipError, match=match):
            plan.solve_population(kw.pop("pop", pop), iters, FTOL, cooperative=kw.pop("cooperative", True), **kw)
        assert pop.get_x().tobytes() == X.tobytes(), match          # before any row is written
        set_options(plan, {k: was[k] for k in (options or {})})
        plan.solve_population(pop, iters, FTOL, cooperative=True)
        pr = plan.fetch_population()
        assert_rows(pr, [pop.get_x(s) for s in range(2)], seq, "after the refusal " + match)
        pop.set_x(X)

    # each refusal of the entry, with its own message; the old entries' refusal of the same plan
    refused("every component of the plan must run on the LDS-resident solver.*1 to the cooperative solver.*rdis_hip_plan_solve_population_cooperative",
            cooperative=False)
    refused("every component of the plan must run on the LDS-resident solver.*1 to the cooperative solver", cooperative=False, first=0, count=1)
    with pytest.raises(capi.RdisHipError, match="cooperative solver"):
        plan.solve_starts(X, iters, FTOL)
    refused("belongs to another problem", pop=foreign)
    refused("members out of range", first=1, count=2)
    refused("plan_solve_population_cooperative: .*pipelined layout.*coop_pipeline = 0", {"coop_pipeline": 1})
    refused("factor_rounding = 1", {"factor_rounding": 1})
    refused("emulate_stale_cache", {"emulate_stale_cache": 1})
    refused("trace_records must be 0", {"trace_records": 16})
    refused("dump_iters must be 0", {"dump_iters": 2})
    # (ptm_stream 0: or the component would join the point-major solver as a wide group)
    refused("plan_solve_population_cooperative: 1 component\\(s\\) of the plan run on the grid solver", {"force_stream": 1, "ptm_stream": 0})

    # ... and once more at the end
    plan.solve_population(pop, iters, FTOL, cooperative=True)
    pr = plan.fetch_population()
    rows = [pop.get_x(s) for s in range(2)]
    assert_rows(pr, rows, seq, "after the refusals")
    # unchanged: the problem's x, the plan's ordinary outputs, a second plan of the same problem
    assert g.get_x().tobytes() == pp.x0.tobytes()
    after = plan.fetch()
    for name in FIELDS + ("x",):
        assert getattr(before, name).tobytes() == getattr(after, name).tobytes(), name
    second.set_start(None); second.solve(iters, FTOL)
    second_after = second.fetch()
    for name in FIELDS + ("x",):
        assert getattr(second_before, name).tobytes() == getattr(second_after, name).tobytes(), name
    assert second_after.x.tobytes() == seq[0][0][0].x.tobytes()
    for h in (plan, second, pop, foreign, g, other):
        h.close()
