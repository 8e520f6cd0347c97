"""Population solves on the point-major streaming solver: rdis_hip_plan_solve_population with the plan option
population_point_major = 1 (solver_ptm_population.hpp: one workgroup per (component, member), cameras in LDS, the member's
point blocks streamed from a replica of the plan's four per-solve arrays).

Every (member, component) must be, bit for bit, what set_x(X[s]) / set_start(None) / solve / fetch / get_x returns on the same
plan options ("sequential" below), and the member's whole row afterwards must be that problem's x.  Every comparison is == or
byte equality.  Small shapes reach the solver through ptm_stream = 2 (every component its tables fit) and ptm_group = 1 (one
workgroup a component: the only shape the entry takes).  No test here times anything."""
import dataclasses
import math

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval")
PTM = {"coop_min_factors": 0, "coop_group_min_factors": 0, "ptm_stream": 2, "ptm_group": 1, "population_point_major": 1}


def set_options(plan, opts):
    for k, v in (opts or {}).items():
        plan.set_option(k, v)


def sampling_intervals(pp):
    """optBA's sampling intervals: rotations in [-pi, pi], k1 / k2 within 1e-4 / 1e-6 and everything else within 100 of the
    initial value"""
    nc = int(pp.meta["ncams"])
    typ = np.concatenate([np.arange(9 * nc) % 9, 9 + np.arange(pp.nvars - 9 * nc) % 3])
    half = np.select([typ < 3, typ == 7, typ == 8], [math.pi, 1e-4, 1e-6], default=100.0)
    centre = np.where(typ < 3, 0.0, pp.x0)
    return centre - half, centre + half


def sampled(pp, n, seed):
    lo, hi = sampling_intervals(pp)
    return np.random.default_rng(seed).uniform(lo, hi, size=(n, pp.nvars))


def sequential(gctx, pp, x, steps, maxiters=25):
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


def whole(pp):
    """the decomposition with one component: everything"""
    return (np.array([0, pp.nvars], dtype=np.int64), np.arange(pp.nvars, dtype=np.int64),
            np.array([0, pp.nfac], dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))


def test_alternation_equals_sequential_and_the_oracle(gctx):
    """ladybug 5 / 30, four members drawn from the sampling intervals, two rounds of camera plan (free cameras, the member's
    points constants: rotation records that follow the trial point) then point plan (constant cameras, ROT_CAMFIX: each member's
    cameras are its own, as its camera step left them), all on the point-major solver: after each of the four solves every
    field, every xout row and every member's whole x == the sequential run; member 1's first camera step == the oracle's run of
    that solver (device_ptm_default) with the member's x assigned.  Refused before the option existed."""
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    X = sampled(pp, 4, 3)
    steps = [(cams, PTM), (pts, PTM), (cams, PTM), (pts, PTM)]
    seq = [sequential(gctx, pp, X[s], steps) for s in range(4)]

    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    plan_c, plan_p = capi.Plan(g, *cams), capi.Plan(g, *pts)
    set_options(plan_c, PTM)
    set_options(plan_p, PTM)
    results = []
    for k, (comps, _) in enumerate(steps):
        plan = plan_c if comps is cams else plan_p
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.info("components_point_major") == plan.ncomp and plan.info("population_point_major_threads") == 768
        assert plan.last_kernel_ms()[1] == 1 and plan.info("starts_launches") == 1 and plan.info("starts_per_launch") == 4
        assert pr.best is None and pr.x.shape == (4, plan.nfree) and pr.fret.shape == (4, plan.ncomp)
        assert_step_equals(pr, pop, [seq[s][k] for s in range(4)], "step %d" % k)
        results.append(pr)
    assert np.all(results[0].fret[0] != results[0].fret[1]) and np.all(results[1].fret[0] != results[1].fret[1])
    assert g.get_x().tobytes() == pp.x0.tobytes()
    # the oracle: member 1's first camera step, every camera a component whose constants are the member's points
    fp, fv, cp, ci = cams
    r = results[0]
    for c in range(5):
        v, f = fv[fp[c]:fp[c + 1]], ci[cp[c]:cp[c + 1]]
        o = O.OracleProblem.device_ptm_default(dataclasses.replace(pp, x0=X[1].copy()), fac=f)
        want = o.cgd(free_vid=v, fac=f, x=X[1][v], maxiters=25)
        print("camera", c, "device", float(r.fret[1, c]), "oracle", want.fret)
        assert r.fret[1, c] == want.fret and r.delta[1, c] == want.delta and r.x[1, fp[c]:fp[c + 1]].tobytes() == want.x.tobytes(), (c, r.fret[1, c], want.fret)
        assert (int(r.iters[1, c]), int(r.status[1, c]), int(r.nfeval[1, c]), int(r.ngeval[1, c])) == (want.iters, want.status, want.nfeval, want.ngeval), c


class Ragged:
    """ladybug 7 / 200 as ONE component (a last chunk of fewer than 64 blocks, chunks of unequal slot counts), five members --
    the start, two perturbed ones and two from the sampling intervals -- and their sequential runs per option set, computed
    once and shared by the tests below (never modified)"""

    def __init__(self, gctx):
        self.gctx = gctx
        self.pp = P.load_bal(ncams=7, npts=200).single_component()
        self.comps = whole(self.pp)
        rng = np.random.default_rng(11)
        x0 = self.pp.x0
        self.X = np.vstack([x0[None, :], x0 * (1 + 1e-3 * rng.standard_normal((2, self.pp.nvars))), sampled(self.pp, 2, 5)])
        self._seq = {}

    def seq(self, threads=0, slots=0):
        key = (threads, slots)
        if key not in self._seq:
            opts = dict(PTM, ptm_threads=threads, ptm_round_slots=slots)
            n = 5 if key == (0, 0) else 3      # (the default options serve the tests of five members)
            self._seq[key] = [sequential(self.gctx, self.pp, self.X[s], [(self.comps, opts)])[0] for s in range(n)]
        return self._seq[key]


@pytest.fixture(scope="module")
def ragged(gctx):
    return Ragged(gctx)


@pytest.mark.parametrize("threads, slots", [(256, 1), (256, 2), (512, 1), (512, 2), (768, 0)])
def test_one_ragged_component(gctx, ragged, threads, slots):
    """200 points are three full chunks and one of eight blocks, and the points are seen by different numbers of cameras: three
    members at every workgroup size, with the gradient's rounds staging one slot and two (256 and 512 lanes) == sequential"""
    pp = ragged.pp
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *ragged.comps)
    set_options(plan, dict(PTM, ptm_threads=threads, ptm_round_slots=slots))
    pop = capi.Population(g, x=ragged.X[:3])
    plan.solve_population(pop, 25, 3e-8)
    pr = plan.fetch_population()
    assert plan.info("components_point_major") == 1 and plan.info("population_point_major_threads") == threads
    assert plan.info("point_major_round_slots") == (slots if slots else 1)
    assert plan.last_kernel_ms()[1] == 1
    assert_step_equals(pr, pop, ragged.seq(threads, slots), "%d lanes, %d slots" % (threads, slots))
    g.close()


def replica_bytes(blocks, cptr_len):
    """population_grid.hpp: ptm_population_replica_bytes without the LDS-resident part (tests/test_population_ptm_cpu.py)"""
    return blocks * (6 + 6 + 6) * 8 + cptr_len * 32


def test_launch_splitting_and_the_replica_invariant(gctx, ragged):
    """five members that differ everywhere: a budget of two replicas and a half gives launches of 2 + 2 + 1, a budget of one byte
    five launches through ONE replica (which is never cleared: what the member before left there must not reach the next), the
    default one launch -- the same bytes every time, all == sequential.  A replica, measured through device_bytes(), is what the
    host function says for 200 point blocks and four wave-chunks (five entries of the chunk table); lowering the budget
    releases the replicas."""
    pp, X, seq = ragged.pp, ragged.X, ragged.seq()
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *ragged.comps)
    set_options(plan, PTM)
    rep = replica_bytes(200, 5)

    def run(budget, per_launch, launches):
        pop = capi.Population(g, x=X)
        plan.set_option("starts_workspace_bytes", budget)
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.info("starts_per_launch") == per_launch and plan.info("starts_launches") == launches
        assert plan.last_kernel_ms()[1] == launches
        assert_step_equals(pr, pop, seq, "budget %d" % budget)
        pop.close()
        return pr, plan.device_bytes()

    one_replica, b1 = run(1, 1, 5)                  # (builds the solver's tables and the members' inputs and outputs too)
    plan.set_option("starts_workspace_bytes", 1)    # the bound holds from now on: the replica goes
    b0 = plan.device_bytes()
    assert b1 - b0 == rep, (b1 - b0, rep)
    split, b2 = run(2 * rep + rep // 2, 2, 3)
    assert b2 - b0 == 2 * rep, (b2 - b0, rep)
    one_launch, b5 = run(1 << 30, 5, 1)
    assert b5 - b0 == 5 * rep, (b5 - b0, rep)
    assert same_bytes(split, one_replica) and same_bytes(one_replica, one_launch)
    g.close()


def test_bounds_a_start_outside_a_rollback_and_an_empty_component(gctx):
    """ladybug 7 / 200 with the tightened point domains of test_partial_blocks_bounds_rollback_and_an_empty_component
    (tests/test_gpu_population_tiny.py): one component of all cameras and 1 .. 3 free coordinates of 70 % of the points (the
    rest constants: blocks with no free variable too), one component without factors (a variable no factor reads), and four
    members: the start; a perturbed one; one whose free values lie outside [lo, hi] (clamped at entry); one that makes the
    objective NaN at its start (a point and its camera's translation at the origin) -- returned restored, ROLLED_BACK.
    Everything == sequential; some results sit on a bound; the empty component reports EXIT_EMPTY, its variable untouched."""
    rng = np.random.default_rng(23)
    pp = P.load_bal(ncams=7, npts=200)
    pp.lo[63:] = pp.x0[63:] - rng.uniform(0.002, 0.05, pp.nvars - 63)
    pp.hi[63:] = pp.x0[63:] + rng.uniform(0.002, 0.05, pp.nvars - 63)
    cam, pt = int(pp.cam_vid0[0]), int(pp.pt_vid0[0])
    origin = np.r_[pt:pt + 3, cam + 3:cam + 6]
    pp.lo[origin] = np.minimum(pp.lo[origin], -1.0)
    pp.hi[origin] = np.maximum(pp.hi[origin], 1.0)
    lonely = pp.nvars                                     # read by no factor: a component with an empty factor list
    pp.x0, pp.lo, pp.hi = np.r_[pp.x0, 0.25], np.r_[pp.lo, -1.0], np.r_[pp.hi, 1.0]
    free = np.zeros(pp.nvars, bool)
    free[:63] = True
    for q in np.where(rng.random(200) < 0.7)[0]:          # free 1 .. 3 coordinates of 70 % of the points
        free[63 + 3 * q + rng.choice(3, size=rng.integers(1, 4), replace=False)] = True
    free[pt:pt + 3] = True
    free[lonely] = False
    solved = np.where(free)[0].astype(np.int64)
    comps = (np.array([0, solved.shape[0], solved.shape[0] + 1], dtype=np.int64), np.r_[solved, lonely].astype(np.int64),
             np.array([0, pp.nfac, pp.nfac], dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))
    inside = pp.x0.copy()
    moved = pp.x0.copy()
    moved[:63] *= 1 + 1e-3 * rng.standard_normal(63)
    outside = pp.x0.copy()
    outside[solved] += 3.0 * (pp.hi[solved] - pp.lo[solved]) * np.where(np.arange(solved.shape[0]) % 2 == 0, 1.0, -1.0)
    assert np.all((outside[solved] > pp.hi[solved]) | (outside[solved] < pp.lo[solved]))
    outside[lonely] = 7.0                                 # (outside its domain too: an empty component does not even clamp)
    nan_x = pp.x0.copy()
    nan_x[origin] = 0.0
    X = np.stack([inside, moved, outside, nan_x])
    seq = [sequential(gctx, pp, X[s], [(comps, PTM)])[0] for s in range(4)]

    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    plan = capi.Plan(g, *comps)
    set_options(plan, PTM)
    plan.solve_population(pop, 25, 3e-8)
    pr = plan.fetch_population()
    assert plan.info("components_point_major") == 1 and plan.ncomp == 2 and plan.last_kernel_ms()[1] == 1
    assert_step_equals(pr, pop, seq)
    xs = pr.x[:, :-1]
    assert np.all(xs >= pp.lo[solved]) and np.all(xs <= pp.hi[solved])
    for s in range(3):
        assert np.any((xs[s] == pp.lo[solved]) | (xs[s] == pp.hi[solved])), s          # some results sit on their bounds
    assert pr.status[3, 0] & capi.STATUS_ROLLED_BACK
    assert np.array_equal(xs[3], nan_x[solved])
    assert not np.any(pr.status[:2, 0] & capi.STATUS_ROLLED_BACK)
    assert np.all(pr.status[:, -1] == 6) and np.all(pr.fret[:, -1] == 0) and np.all(pr.iters[:, -1] == 0)      # EXIT_EMPTY
    after = pop.get_x()
    assert after[:, lonely].tobytes() == X[:, lonely].tobytes() and pr.x[:, -1].tobytes() == X[:, lonely].tobytes()
    notfree = ~free
    assert after[:, notfree].tobytes() == X[:, notfree].tobytes()                      # what is not free is what was put in
    assert g.get_x().tobytes() == pp.x0.tobytes()
    g.close()


@pytest.mark.parametrize("with_tiny", [False, True])
def test_mixed_plan(gctx, with_tiny):
    """five blocks of 3 cameras x 1200 points: two stay whole components (3627 variables: too large for the LDS, so the
    point-major solver by default), two keep their cameras and their first 40 / 60 points (LDS-resident solver), and -- with_tiny
    -- the first 50 points of the fifth are components of their own against constant cameras (tiny-component solver,
    population_tiny = 1).  One plan; per chunk of members the tiny launch, the point-major launch, the LDS-resident launch, in
    that order.  3 members == sequential, in one chunk and one member at a time."""
    pp = P.make_synthetic_ba(5, 3, 1200)
    fp, fv, cp, ci = [0], [], [0], []

    def add(v, f):
        fv.extend(int(t) for t in v); fp.append(len(fv)); ci.extend(int(t) for t in f); cp.append(len(ci))

    for c in (0, 1):
        add(*pp.component(c))
    for c, keep in ((2, 40), (3, 60)):
        v, f = pp.component(c)
        q_end = v[0] + 27 + 3 * keep                     # the block's cameras and its first `keep` points
        add(v[v < q_end], f[pp.pt_vid0[f] < q_end])
    if with_tiny:
        v, f = pp.component(4)
        for q in v[27:27 + 3 * 50:3]:
            add([q, q + 1, q + 2], f[pp.pt_vid0[f] == q])
    comps = tuple(np.array(t, dtype=np.int64) for t in (fp, fv, cp, ci))
    opts = {"coop_min_factors": 0, "coop_group_min_factors": 0, "ptm_group": 1, "population_point_major": 1}
    if with_tiny:
        opts.update(population_tiny=1, row_min_components=1)
    rng = np.random.default_rng(29)
    X = np.stack([pp.x0] + [pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)) for _ in range(2)])
    seq = [sequential(gctx, pp, X[s], [(comps, opts)])[0] for s in range(3)]
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *comps)
    set_options(plan, opts)
    per_chunk = 3 if with_tiny else 2
    out = []
    for budget, launches in ((1 << 30, per_chunk), (1, 3 * per_chunk)):
        plan.set_option("starts_workspace_bytes", budget)
        pop = capi.Population(g, x=X)
        plan.solve_population(pop, 25, 3e-8)
        pr = plan.fetch_population()
        assert plan.info("components_point_major") == 2 and plan.info("components_lds") == 2
        assert plan.info("components_tiny") == (50 if with_tiny else 0) and plan.info("population_point_major_threads") == 768
        assert plan.last_kernel_ms()[1] == launches and plan.info("starts_launches") == launches
        assert_step_equals(pr, pop, seq, "budget %d" % budget)
        out.append(pr)
        pop.close()
    assert same_bytes(out[0], out[1])
    g.close()


def _refused(call):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1 and len(str(e.value).split(":", 1)[1].strip()) > 0, e.value
    return str(e.value)


def test_refusals_and_nothing_else_moves(gctx, ragged):
    """without the option a plan with point-major components is refused as before, and the message names the option; with it
    a plan whose ordinary solve shares a component among workgroups is refused naming ptm_group and the group size, and the
    parity option and a trace are refused with the messages they had; the multi-start entry refuses, option or not.  After each
    refusal the plan and the population work.  A population solve leaves the problem's x, the plan's ordinary outputs and its
    objective alone, and an ordinary solve on the same plan afterwards has the bytes of a fresh plan's (the plan's own point
    records are untouched).  (A transient plan is refused with its old message too, but no caller holds one: the only
    transient plan is the one inside rdis_hip_cgd_batch.)"""
    pp, X = ragged.pp, ragged.X

    def usable(plan, start):
        plan.set_start(start)
        plan.solve(2, 3e-8)
        assert np.all(np.isfinite(plan.fetch().fret))

    def works(plan, pop):
        plan.solve_population(pop, 2, 3e-8)
        assert np.all(np.isfinite(plan.fetch_population(want_x=False).fret))

    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X[:2])
    plan = capi.Plan(g, *ragged.comps)
    set_options(plan, dict(PTM, population_point_major=0))
    msg = _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    assert "every component of the plan must run on the LDS-resident solver" in msg and "1 to the point-major streaming solver" in msg, msg
    assert "population_point_major" in msg and "cooperative" not in msg and "tiny" not in msg, msg
    usable(plan, pp.x0)
    plan.set_option("population_point_major", 1)
    works(plan, pop)
    # the multi-start entry keeps refusing point-major components, option or not
    msg = _refused(lambda: plan.solve_starts(pp.x0[None, :], 2, 3e-8))
    assert "point-major streaming solver" in msg and "population_point_major" not in msg, msg
    plan.set_option("trace_records", 16)
    assert "trace_records must be 0" in _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    plan.set_option("trace_records", 0)
    plan.set_option("factor_rounding", 1)
    assert "the parity option (factor_rounding = 1) has no population entry" in _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    plan.set_option("factor_rounding", 0)
    usable(plan, pp.x0)
    works(plan, pop)
    plan.close()

    # nothing else moves
    plan = capi.Plan(g, *ragged.comps)
    set_options(plan, PTM)
    plan.set_start(X[1])
    plan.solve(25, 3e-8)
    before, x_before, obj_before = plan.fetch(), g.get_x(), plan.objective()
    pop2 = capi.Population(g, x=X[:2])
    plan.solve_population(pop2, 25, 3e-8)
    pr = plan.fetch_population()
    assert g.get_x().tobytes() == x_before.tobytes()
    assert same_bytes(plan.fetch(), before) and plan.objective() == obj_before
    assert_step_equals(pr, pop2, ragged.seq()[:2])
    g.set_x(X[0])
    plan.set_start(None)
    plan.solve(25, 3e-8)
    want, x_want = ragged.seq()[0]
    assert same_bytes(plan.fetch(), want) and g.get_x().tobytes() == x_want.tobytes()
    g.close()

    # groups: two components of 49 cameras x 3200 points, which the ordinary solve shares among workgroups
    big = P.make_synthetic_ba(2, 49, 3200, obs_per_pt=4)
    g = capi.Problem(gctx, big)
    plan = capi.Plan(g)
    set_options(plan, {"coop_min_factors": 0, "coop_group_min_factors": 0, "population_point_major": 1})
    usable(plan, big.x0)
    K = plan.info("point_major_group")
    assert plan.info("components_point_major") == 2 and K >= 2
    pop = capi.Population(g, 2)
    msg = _refused(lambda: plan.solve_population(pop, 2, 3e-8))
    assert "ptm_group" in msg and "groups of %d workgroups" % K in msg, msg
    usable(plan, big.x0)
    assert plan.info("point_major_group") == K
    plan.set_option("ptm_group", 1)
    works(plan, pop)
    assert plan.info("population_point_major_threads") == 768
    g.close()


def test_selection_on_the_device(gctx, ragged):
    """eval_device + assign_best after a point-major population solve leave the problem at the member the host route selects
    (eval on the host side, the lowest value, the lowest index on a tie, never a NaN)"""
    pp, X = ragged.pp, ragged.X
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *ragged.comps)
    set_options(plan, PTM)
    pop = capi.Population(g, x=X)
    plan.solve_population(pop, 25, 3e-8)
    f = pop.eval()
    assert np.any(np.isfinite(f))
    m = int(np.nanargmin(f))
    pop.eval_device()
    bm, bf = pop.best()
    assert (bm, bf) == (m, f[m]), (bm, bf, f)
    pop.assign_best()
    assert g.get_x().tobytes() == pop.get_x(m).tobytes() == ragged.seq()[m][1].tobytes()
    g.close()
