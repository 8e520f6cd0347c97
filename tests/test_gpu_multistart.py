"""Multi-start solves: one plan, many starting points, one launch (rdis_hip_plan_solve_starts / _fetch_starts).

Every start of a multi-start solve must be, bit for bit, what the existing set_start / solve / fetch returns from that
start on a fresh Problem ("sequential" below: the path the other test files pin to the oracle with ==) -- fret, delta,
the bytes of x, iterations, status, call counts.  What is left behind is what an RDIS node keeps of its restarts: per
component the start with the lowest value, as the plan's ordinary outputs and as the assignment of its variables.
No test here times anything."""
import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval")


def sequential(gctx, pp, comps, start, maxiters, opts=None):
    """the parent's path: a fresh Problem, one start, one solve"""
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *comps) if comps is not None else capi.Plan(g)
    for k, v in (opts or {}).items():
        plan.set_option(k, v)
    plan.set_start(start)
    plan.solve(maxiters, 3e-8)
    r = plan.fetch()
    x_after = g.get_x()
    g.close()
    return r, x_after


def assert_rows_equal_sequential(gctx, pp, comps, starts, ms, maxiters, opts=None):
    """every (start, component) of the multi-start result ms == the sequential solve from that row; returns the sequential results"""
    seq = []
    for s, row in enumerate(starts):
        r, _ = sequential(gctx, pp, comps, row, maxiters, opts)
        for name in FIELDS:
            a, b = getattr(ms, name)[s], getattr(r, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (s, name, a, b)
        assert ms.x[s].tobytes() == r.x.tobytes(), s
        seq.append(r)
    return seq


def config3_starts(pp):
    return np.stack([pp.x0] + [pp.x0 * (1 + 1e-12 * np.random.default_rng(seed).standard_normal(pp.nvars)) for seed in range(4)])


def test_config_3_all_free_equals_sequential_and_the_oracle(gctx):
    """BASELINE config 3 (ladybug 5 cameras / 30 points, one component, everything free) from x0 and four starts moved by
    1e-12-relative noise, one call: every row == the sequential solve and == the oracle with the device's arithmetic and the
    LDS-resident solver's sum trees.  Row 0 is the number smoke() prints: 25.168503286225235 after 540 evaluations."""
    pp = P.load_bal(ncams=5, npts=30).single_component()
    starts = config3_starts(pp)
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    assert plan.info("components_lds") == 1 and plan.info("starts_per_launch") == 5 and plan.info("starts_launches") == 1
    assert ms.x.shape == (5, pp.nvars) and ms.fret.shape == (5, 1) and ms.best.shape == (1,)
    assert_rows_equal_sequential(gctx, pp, None, starts, ms, 25)
    for s in range(5):
        want = O.OracleProblem.device_lds_default(pp).cgd(x=starts[s], maxiters=25)
        assert ms.fret[s, 0] == want.fret and ms.delta[s, 0] == want.delta and ms.x[s].tobytes() == want.x.tobytes(), (s, ms.fret[s, 0], want.fret)
        assert (int(ms.iters[s, 0]), int(ms.status[s, 0]), int(ms.nfeval[s, 0]), int(ms.ngeval[s, 0])) == (want.iters, want.status, want.nfeval, want.ngeval), s
    assert ms.fret[0, 0] == 25.168503286225235 and int(ms.nfeval[0, 0]) == 540


@pytest.mark.parametrize("which", ["cameras free, points constant", "points free, cameras constant"])
def test_constants_in_both_rotation_modes(gctx, which):
    """ladybug 5 / 30 with a separator assigned: the camera plan (5 components of nine free variables against constant points)
    and the point plan (30 components of three against constant cameras -- no camera variable free in the launch: the
    records-only rotation mode).  Three starts; the constants are shared by all of them and untouched afterwards."""
    pp = P.load_bal(ncams=5, npts=30)
    cams, pts = P.ba_alternation_plans(pp)
    comps = cams if which.startswith("cameras") else pts
    fv = comps[1]
    rng = np.random.default_rng(7)
    starts = np.stack([pp.x0[fv], pp.x0[fv] * (1 + 1e-3 * rng.standard_normal(fv.shape[0])), pp.x0[fv] * (1 + 1e-2 * rng.standard_normal(fv.shape[0]))])
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *comps)
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    ncomp = comps[0].shape[0] - 1
    assert plan.info("components_lds") == ncomp and ms.fret.shape == (3, ncomp)
    assert_rows_equal_sequential(gctx, pp, comps, starts, ms, 25)
    const = np.ones(pp.nvars, dtype=bool)
    const[fv] = False
    assert np.array_equal(g.get_x()[const], pp.x0[const])


def _device_bytes_per_replica(plan, starts):
    """bytes of one replica of the per-solve workspace, from plan.device_bytes(): with a budget of one byte a launch holds one
    replica whatever the number of starts, so a second start adds its inputs and outputs only"""
    plan.set_option("starts_workspace_bytes", 1)
    b0 = plan.device_bytes()
    plan.solve_starts(starts[:1], 25, 3e-8)
    plan.fetch_starts(want_x=False)
    b1 = plan.device_bytes()
    plan.solve_starts(starts[:2], 25, 3e-8)
    plan.fetch_starts(want_x=False)
    b2 = plan.device_bytes()
    assert plan.info("starts_per_launch") == 1 and plan.info("starts_launches") == 2
    io = b2 - b1
    return (b1 - b0) - io


def test_several_components_and_split_launches(gctx):
    """seven components, four starts, a budget that holds three replicas: two launches (3 + 1, the last one ragged), every one of
    the 28 solves == sequential; with the default budget one launch and the same bytes"""
    pp = P.make_synthetic_ba(7, 3, 40)
    rng = np.random.default_rng(11)
    starts = np.stack([pp.x0] + [pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)) for _ in range(3)])
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    assert plan.info("components_lds") == 7
    rep = _device_bytes_per_replica(plan, starts)
    assert rep >= 8 * 5 * pp.nvars     # (at least the five vectors of the recurrence per free variable)
    plan.set_option("starts_workspace_bytes", 3 * rep + rep // 2)
    plan.solve_starts(starts, 25, 3e-8)
    split = plan.fetch_starts()
    assert plan.info("starts_per_launch") == 3 and plan.info("starts_launches") == 2
    assert plan.last_kernel_ms()[1] == 2
    assert_rows_equal_sequential(gctx, pp, None, starts, split, 25)

    plan.set_option("starts_workspace_bytes", 1 << 30)
    plan.solve_starts(starts, 25, 3e-8)
    one = plan.fetch_starts()
    assert plan.info("starts_per_launch") == 4 and plan.info("starts_launches") == 1
    for name in FIELDS + ("x", "best"):
        assert getattr(one, name).tobytes() == getattr(split, name).tobytes(), name


def test_bounds_and_rollback(gctx):
    """the edges of CGDSubspaceOptimizer::optimize, start by start: the inputs of
    test_batch_solvers_with_active_bounds_partial_blocks_and_rollback on seven components of 3 cameras x 40 points -- domains
    tight enough that the clamp is active during the line searches, a fifth of the variables constant -- from the assigned x;
    a start outside [lo, hi], clamped at entry; and a start whose objective is NaN (a point and the camera that sees it at the
    origin: 0 / 0), returned restored with RDIS_HIP_STATUS_ROLLED_BACK while its neighbours are none the wiser."""
    rng = np.random.default_rng(31)
    pp = P.make_synthetic_ba(7, 3, 40)
    nv = pp.nvars // 7
    w = np.where(np.arange(pp.nvars) % nv < 27, 0.02, 0.01)
    pp.lo = np.maximum(pp.lo, pp.x0 - w * rng.uniform(0.2, 1.0, pp.nvars) * np.maximum(np.abs(pp.x0), 1e-3))
    pp.hi = np.minimum(pp.hi, pp.x0 + w * rng.uniform(0.2, 1.0, pp.nvars) * np.maximum(np.abs(pp.x0), 1e-3))
    const = rng.random(pp.nvars) < 0.2
    # the NaN start needs component 1's first point and its camera's translation free, with the origin inside their domains
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
    comps = tuple(np.array(a, dtype=np.int64) for a in (fp, fv, cp, ci))
    fva = comps[1]
    inside = pp.x0[fva]
    outside = inside + 3.0 * (pp.hi[fva] - pp.lo[fva]) * np.where(np.arange(fva.shape[0]) % 2 == 0, 1.0, -1.0)
    assert np.all((outside > pp.hi[fva]) | (outside < pp.lo[fva]))
    nan_start = inside.copy()
    nan_start[np.isin(fva, origin)] = 0.0
    starts = np.stack([inside, outside, nan_start])
    opts = {"coop_group_min_factors": 0, "coop_min_factors": 0}
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g, *comps)
    for k, v in opts.items():
        plan.set_option(k, v)
    plan.solve_starts(starts, 12, 3e-8)
    ms = plan.fetch_starts()
    assert plan.info("components_lds") == 7
    assert_rows_equal_sequential(gctx, pp, comps, starts, ms, 12, opts)
    assert np.all(ms.x >= pp.lo[fva]) and np.all(ms.x <= pp.hi[fva])
    assert np.any((ms.x[0] == pp.lo[fva]) | (ms.x[0] == pp.hi[fva]))                 # the clamp was active
    assert (ms.status[2, 1] & 0xFF) == 5 and (ms.status[2, 1] & capi.STATUS_ROLLED_BACK)
    assert np.array_equal(ms.x[2, fp[1]:fp[2]], nan_start[fp[1]:fp[2]])
    assert np.all(ms.delta[:2] <= 0) and np.all(np.isfinite(ms.fret[0]))
    assert np.all(ms.best[1] != 2)                                                   # a NaN is never the best
    after = g.get_x()
    assert np.array_equal(after[const], pp.x0[const])


def test_selection_and_state(gctx):
    """starts [a, b, a]: best is the argmin, the lower index on the tie; the problem's variables, plan.fetch() and
    plan.objective() hold the best rows; set_start(None) continues from them; a plain solve on the same plan afterwards is
    untouched; one start == the plain solve"""
    pp = P.make_synthetic_ba(7, 3, 40)
    fp = pp.comp_free_ptr
    rng = np.random.default_rng(5)
    a = pp.x0.copy()
    b = pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars))
    starts = np.stack([a, b, a])
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    assert ms.fret[0].tobytes() == ms.fret[2].tobytes() and ms.x[0].tobytes() == ms.x[2].tobytes()
    want_best = np.array([0 if ms.fret[0, c] <= ms.fret[1, c] else 1 for c in range(7)], dtype=np.int32)
    assert np.array_equal(ms.best, want_best) and ms.best.dtype == np.int32
    assert set(want_best.tolist()) == {0, 1}, want_best                               # (both starts win somewhere: the test selects)
    x_best = np.concatenate([ms.x[ms.best[c], fp[c]:fp[c + 1]] for c in range(7)])
    assert g.get_x(pp.comp_free_vid).tobytes() == x_best.tobytes()
    r = plan.fetch()
    assert r.x.tobytes() == x_best.tobytes()
    for name in FIELDS:
        rows = np.array([getattr(ms, name)[ms.best[c], c] for c in range(7)], dtype=getattr(r, name).dtype)
        assert getattr(r, name).tobytes() == rows.tobytes(), name
    # plan_objective_device adds the plan's fret like any solve's (eval_kernels.hpp: a lane per component, the wave's pairwise tree)
    f = r.fret
    total = plan.objective()
    assert total == ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + f[6])
    assert plan.allreduce_objective(None) == total
    plain, _ = sequential(gctx, pp, None, pp.x0, 25)
    # continue from the state left behind
    plan.set_start(None)
    plan.solve(25, 3e-8)
    cont = plan.fetch()
    want, _ = sequential(gctx, pp, None, x_best, 25)
    for name in FIELDS + ("x",):
        assert getattr(cont, name).tobytes() == getattr(want, name).tobytes(), name
    # a plain solve on the same plan afterwards, and a single start
    plan.set_start(pp.x0)
    plan.solve(25, 3e-8)
    again = plan.fetch()
    plan.solve_starts(pp.x0[None, :], 25, 3e-8)
    single = plan.fetch_starts()
    assert np.array_equal(single.best, np.zeros(7, dtype=np.int32))
    for name in FIELDS + ("x",):
        assert getattr(again, name).tobytes() == getattr(plain, name).tobytes(), name
        assert getattr(single, name)[0].tobytes() == getattr(plain, name).tobytes(), name


def test_plain_solve_after_multistart_keeps_config_3_bits(gctx):
    """a plain set_start(x0) + solve on a plan that has solved many starts returns config 3's bits"""
    pp = P.load_bal(ncams=5, npts=30).single_component()
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.solve_starts(config3_starts(pp)[::-1].copy(), 25, 3e-8)
    ms = plan.fetch_starts()
    assert ms.fret[4, 0] == 25.168503286225235
    plan.set_start(pp.x0)
    plan.solve(25, 3e-8)
    r = plan.fetch()
    assert r.fret[0] == 25.168503286225235 and int(r.nfeval[0]) == 540
    assert r.x.tobytes() == ms.x[4].tobytes()


def _refused(call):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1 and len(str(e.value).split(":", 1)[1].strip()) > 0, e.value
    return str(e.value)


def test_refusals_leave_the_plan_usable(gctx):
    """what the first version does not do is refused with EINVAL and a message that names the cause; the plan solves afterwards"""
    def usable(plan, start):
        plan.set_start(start)
        plan.solve(2, 3e-8)
        assert np.all(np.isfinite(plan.fetch().fret))

    full = P.load_bal()
    # the whole of ladybug as one component: a cooperative group
    full.single_component()
    g = capi.Problem(gctx, full)
    plan = capi.Plan(g)
    msg = _refused(lambda: plan.solve_starts(full.x0[None, :], 2, 3e-8))
    assert "cooperative" in msg and "tiny" not in msg, msg
    assert plan.info("components_cooperative") == 1
    usable(plan, full.x0)
    g.close()
    # its point plan at full size: the tiny-component solver
    cams, pts = P.ba_alternation_plans(full)
    g = capi.Problem(gctx, full)
    plan = capi.Plan(g, *pts)
    msg = _refused(lambda: plan.solve_starts(full.x0[pts[1]][None, :], 2, 3e-8))
    assert "tiny" in msg and "cooperative" not in msg, msg
    assert plan.info("components_tiny") > 0
    usable(plan, full.x0[pts[1]])
    g.close()
    # options of one solve, no starts, a fetch with nothing to fetch
    pp = P.load_bal(ncams=5, npts=30).single_component()
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    assert "fetch" in _refused(lambda: plan.fetch_starts())
    plan.set_option("factor_rounding", 1)
    assert "factor_rounding" in _refused(lambda: plan.solve_starts(pp.x0[None, :], 2, 3e-8))
    usable(plan, pp.x0)
    plan.set_option("factor_rounding", -1)
    plan.set_option("trace_records", 16)
    assert "trace_records" in _refused(lambda: plan.solve_starts(pp.x0[None, :], 2, 3e-8))
    usable(plan, pp.x0)
    plan.set_option("trace_records", 0)
    assert "nstarts" in _refused(lambda: plan.solve_starts(np.empty((0, pp.nvars)), 2, 3e-8))
    assert "fetch" in _refused(lambda: plan.fetch_starts())
    usable(plan, pp.x0)
    plan.solve_starts(pp.x0[None, :], 25, 3e-8)
    assert plan.fetch_starts().fret[0, 0] == 25.168503286225235
