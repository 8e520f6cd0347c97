"""Multi-start solves of nonlinear-product plans: rdis_hip_plan_solve_starts on the plain one-workgroup solver
(solver_wg_starts.hpp), one workgroup per (component, start) on a replica of the problem's x and dir.

Every start must be, bit for bit, what set_start / solve / fetch returns from that start on a fresh Problem ("sequential"
below, restated from test_gpu_multistart.py) and what the CPU oracle's restatement of that solver returns
(OracleProblem.device_wg_default: the device's sine / cosine, RO_SUM_TOPOLOGY_WG) -- fret, delta, the bytes of x, iterations,
status, call counts.  Everything is compared with == / .tobytes(); nothing is timed; maxiters 25, ftol 3e-8."""
import json
import os

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


def assert_row_equals_oracle(ms, s, c, want, x_row):
    assert ms.fret[s, c] == want.fret and ms.delta[s, c] == want.delta and x_row.tobytes() == want.x.tobytes(), (s, c, ms.fret[s, c], want.fret)
    assert (int(ms.iters[s, c]), int(ms.status[s, c]), int(ms.nfeval[s, c]), int(ms.ngeval[s, c])) == \
           (want.iters, want.status, want.nfeval, want.ngeval), (s, c)


def test_config_1_one_wave(gctx):
    """BASELINE config 1 (testpoly: two variables, seven factors; 64 lanes, one wave) from four starts that end in its three
    minima; rows 1 and 3 tie bit for bit in value while their x differ in the last digits: the lower index is kept"""
    pp = P.load_poly().single_component()
    starts = np.array([[3.0, 3.0], [-3.0, -3.0], [-3.0, 3.0], [0.0, 0.0]])
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    assert plan.info("components_plain") == 1 and plan.info("starts_per_launch") == 4 and plan.info("starts_launches") == 1
    assert ms.fret[:, 0].tolist() == [-132.5311627303028, -168.27208973577922, -150.40162623285318, -168.27208973577922]
    assert ms.x[1].tobytes() != ms.x[3].tobytes()
    assert_rows_equal_sequential(gctx, pp, None, starts, ms, 25)
    for s in range(4):
        assert_row_equals_oracle(ms, s, 0, O.OracleProblem.device_wg_default(pp).cgd(x=starts[s], maxiters=25), ms.x[s])
    assert ms.best.tolist() == [1]
    assert g.get_x().tobytes() == ms.x[1].tobytes() and plan.fetch().x.tobytes() == ms.x[1].tobytes()


def _sinusoid_from_the_committed_start():
    pp = P.make_high_dim_sinusoid()
    with open(os.path.join(os.path.dirname(__file__), "golden", "sinusoid_start.json")) as fh:
        pp.x0 = np.array(json.load(fh)["x0"])
    return pp.single_component()


def test_config_2_five_starts_in_one_launch(gctx):
    """BASELINE config 2 (the 121-variable sinusoid, one component, 512 lanes) from the bench's start and four copies moved by
    1e-9-relative noise, one call.  Row 0 is the bench's number: 1578.9001138212975 after 726 evaluations."""
    pp = _sinusoid_from_the_committed_start()
    starts = np.stack([pp.x0] + [pp.x0 * (1 + 1e-9 * np.random.default_rng(seed).standard_normal(pp.nvars)) for seed in range(4)])
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    assert plan.info("components_plain") == 1 and plan.info("starts_per_launch") == 5 and plan.info("starts_launches") == 1
    assert_rows_equal_sequential(gctx, pp, None, starts, ms, 25)
    for s in range(5):
        assert_row_equals_oracle(ms, s, 0, O.OracleProblem.device_wg_default(pp).cgd(x=starts[s], maxiters=25), ms.x[s])
    assert ms.fret[0, 0] == 1578.9001138212975 and int(ms.nfeval[0, 0]) == 726


def _three_subtrees(gctx, pp=None):
    """the sinusoid with its root held constant: three subtrees of 40 variables and 120 factors each (128 lanes)"""
    pp = P.make_high_dim_sinusoid() if pp is None else pp
    g = capi.Problem(gctx, pp)
    assigned = np.zeros(pp.nvars, np.uint8)
    assigned[0] = 1
    comps = g.components(assigned)
    plan = capi.Plan(g, *comps)
    assert plan.ncomp == 3 and plan.info("components_plain") == 3
    assert np.diff(comps[0]).tolist() == [40, 40, 40] and np.diff(comps[2]).tolist() == [120, 120, 120]
    return pp, g, plan, comps


def _uniform_starts(pp, fv, n=4, seed=7):
    return np.random.default_rng(seed).uniform(pp.lo, pp.hi, (n, pp.nvars))[:, fv]


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


def test_three_components_split_launches_and_replica_reuse(gctx):
    """three components, four uniform starts: with a budget for three replicas two launches (3 + 1), with a budget of one byte
    four launches on ONE replica -- whose x still holds what the start before left in the free entries: no refill is needed --
    and with the default budget one launch: the same bytes all three ways.  Every one of the 12 solves == sequential == the
    oracle; the selection is per component (start 2 wins the first subtree, start 0 the other two)."""
    pp, g, plan, comps = _three_subtrees(gctx)
    fp, fv, cp, ci = comps
    starts = _uniform_starts(pp, fv)
    rep = _device_bytes_per_replica(plan, starts)
    assert rep >= 8 * (2 * pp.nvars + 5 * fv.shape[0])    # (x and dir of the problem's size, the recurrence's five vectors)
    plan.set_option("starts_workspace_bytes", 3 * rep + rep // 2)
    plan.solve_starts(starts, 25, 3e-8)
    split = plan.fetch_starts()
    assert plan.info("starts_per_launch") == 3 and plan.info("starts_launches") == 2 and plan.last_kernel_ms()[1] == 2
    plan.set_option("starts_workspace_bytes", 1)
    plan.solve_starts(starts, 25, 3e-8)
    single = plan.fetch_starts()
    assert plan.info("starts_per_launch") == 1 and plan.info("starts_launches") == 4 and plan.last_kernel_ms()[1] == 4
    plan.set_option("starts_workspace_bytes", 1 << 30)
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    assert plan.info("starts_per_launch") == 4 and plan.info("starts_launches") == 1
    for name in FIELDS + ("x", "best"):
        assert getattr(ms, name).tobytes() == getattr(split, name).tobytes(), name
        assert getattr(ms, name).tobytes() == getattr(single, name).tobytes(), name

    assert_rows_equal_sequential(gctx, pp, comps, starts, ms, 25)
    for c in range(3):
        v, f = fv[fp[c]:fp[c + 1]], ci[cp[c]:cp[c + 1]]
        orc = O.OracleProblem.device_wg_default(pp, free_vid=v, fac=f)
        for s in range(4):
            want = orc.cgd(free_vid=v, fac=f, x=starts[s, fp[c]:fp[c + 1]], maxiters=25)
            assert_row_equals_oracle(ms, s, c, want, ms.x[s, fp[c]:fp[c + 1]])
    assert np.all(np.isfinite(ms.fret))
    assert np.array_equal(ms.best, np.argmin(ms.fret, axis=0)) and ms.best.dtype == np.int32
    assert ms.best.tolist() == [2, 0, 0]
    x_best = np.concatenate([ms.x[ms.best[c], fp[c]:fp[c + 1]] for c in range(3)])
    r = plan.fetch()
    assert r.x.tobytes() == x_best.tobytes() and g.get_x(fv).tobytes() == x_best.tobytes()
    for name in FIELDS:
        rows = np.array([getattr(ms, name)[ms.best[c], c] for c in range(3)], dtype=getattr(r, name).dtype)
        assert getattr(r, name).tobytes() == rows.tobytes(), name
    assert g.get_x([0])[0] == pp.x0[0]                     # the constant is untouched
    f = r.fret
    assert plan.objective() == (f[0] + f[1]) + f[2]


def test_state_afterwards(gctx):
    """set_start(None) continues from the best rows; a plain solve on the same plan afterwards has the bits of a sequential one
    (the problem's own x and dir were not disturbed); a single start == the plain solve"""
    pp, g, plan, comps = _three_subtrees(gctx)
    fp, fv = comps[0], comps[1]
    starts = _uniform_starts(pp, fv)
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    x_best = np.concatenate([ms.x[ms.best[c], fp[c]:fp[c + 1]] for c in range(3)])
    plan.set_start(None)
    plan.solve(25, 3e-8)
    cont = plan.fetch()
    want, _ = sequential(gctx, pp, comps, x_best, 25)
    for name in FIELDS + ("x",):
        assert getattr(cont, name).tobytes() == getattr(want, name).tobytes(), name
    x0 = starts[3]
    plain, _ = sequential(gctx, pp, comps, x0, 25)
    plan.set_start(x0)
    plan.solve(25, 3e-8)
    again = plan.fetch()
    plan.solve_starts(x0[None, :], 25, 3e-8)
    single = plan.fetch_starts()
    assert np.array_equal(single.best, np.zeros(3, dtype=np.int32))
    for name in FIELDS + ("x",):
        assert getattr(again, name).tobytes() == getattr(plain, name).tobytes(), name
        assert getattr(single, name)[0].tobytes() == getattr(plain, name).tobytes(), name


def test_bounds_and_rollback(gctx):
    """the edges of CGDSubspaceOptimizer::optimize, start by start, on the three subtrees.

    Bounds: the domains tightened around a start (half-widths 0.05 .. 1.5) so that the clamp is active in the line searches;
    from that start, from one outside [lo, hi] (clamped at entry) and from a uniform one inside.

    Roll-back (.cpp:66-80).  The issue asked for a start whose two-iteration solve ends above its initial value.  No such start
    exists for this function: a line minimisation brackets from f(0) and Brent keeps its best point, so the value never rises, and
    30000 two-iteration solves of these subtrees on the CPU oracle (uniform, outside and corner starts, open and tight domains)
    found none.  What does roll back on this solver is a solve that meets a NaN: here the 0.1 x^2 term of the second subtree's root
    is made 0.1 x^0.5 and its start put at 0.01, so the first bracketing step crosses zero.  The device returns the restored
    start with RDIS_HIP_STATUS_ROLLED_BACK while the neighbours and the other starts are none the wiser.  (pow is not part of the
    oracle's restatement: this case is compared with the sequential solve alone.)"""
    pp = P.make_high_dim_sinusoid()
    centre = np.random.default_rng(7).uniform(pp.lo, pp.hi, pp.nvars)
    rng = np.random.default_rng(31)
    w = rng.uniform(0.05, 1.5, pp.nvars)
    pp.lo[1:] = np.maximum(pp.lo, centre - w)[1:]
    pp.hi[1:] = np.minimum(pp.hi, centre + w)[1:]
    pp, g, plan, comps = _three_subtrees(gctx, pp)
    fv = comps[1]
    outside = centre[fv] + 3.0 * (pp.hi[fv] - pp.lo[fv]) * np.where(np.arange(fv.shape[0]) % 2 == 0, 1.0, -1.0)
    assert np.all((outside > pp.hi[fv]) | (outside < pp.lo[fv]))
    starts = np.stack([centre[fv], outside, rng.uniform(pp.lo[fv], pp.hi[fv])])
    plan.solve_starts(starts, 25, 3e-8)
    ms = plan.fetch_starts()
    assert_rows_equal_sequential(gctx, pp, comps, starts, ms, 25)
    assert np.all(ms.x >= pp.lo[fv]) and np.all(ms.x <= pp.hi[fv])
    assert np.any((ms.x[0] == pp.lo[fv]) | (ms.x[0] == pp.hi[fv]))                   # the clamp was active
    assert np.all(ms.delta <= 0) and np.all(np.isfinite(ms.fret))
    g.close()

    pq = P.make_high_dim_sinusoid()
    root = 2                                                                          # (the second subtree's)
    k = int(pq.rowptr[pq.nfac - pq.nvars + root])                                     # (the squares are the last nvars factors)
    assert pq.vid[k] == root and pq.expo[k] == 2.0 and not pq.sine[k]
    pq.expo[k] = 0.5
    pq, g, plan, comps = _three_subtrees(gctx, pq)
    fp, fv = comps[0], comps[1]
    assert int(fv[fp[1]]) == root
    starts = _uniform_starts(pq, fv, n=2)
    starts[0, fp[1]] = 0.01
    starts[1, fp[1]] = 30.0
    plan.solve_starts(starts, 2, 3e-8)
    ms = plan.fetch_starts()
    assert_rows_equal_sequential(gctx, pq, comps, starts, ms, 2)
    assert ms.status[0, 1] & capi.STATUS_ROLLED_BACK and ms.delta[0, 1] == 0
    assert np.array_equal(ms.x[0, fp[1]:fp[2]], starts[0, fp[1]:fp[2]])
    assert not np.any(ms.status[:, [0, 2]] & capi.STATUS_ROLLED_BACK) and not (ms.status[1, 1] & capi.STATUS_ROLLED_BACK)
    assert np.all(ms.delta[:, [0, 2]] < 0) and ms.delta[1, 1] < 0 and ms.best[1] == 1
    assert g.get_x(fv[fp[1]:fp[2]]).tobytes() == ms.x[1, fp[1]:fp[2]].tobytes()


def _refused(call):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1 and len(str(e.value).split(":", 1)[1].strip()) > 0, e.value
    return str(e.value)


def test_refusals_leave_the_plan_usable(gctx):
    """bundle adjustment on the plain solver (its rotation records are not replicated) and a trace are refused with EINVAL and a
    message that names the cause; the plan solves afterwards, and a valid multi-start solve succeeds"""
    def usable(plan, start):
        plan.set_start(start)
        plan.solve(2, 3e-8)
        assert np.all(np.isfinite(plan.fetch().fret))

    ba = P.make_synthetic_ba(2, 3, 40)
    g = capi.Problem(gctx, ba)
    plan = capi.Plan(g)
    forced = {"lds_resident": 0, "ptm_stream": 0, "coop_min_factors": 0, "coop_group_min_factors": 0}
    for k, v in forced.items():
        plan.set_option(k, v)
    assert plan.info("components_plain") == 2
    msg = _refused(lambda: plan.solve_starts(ba.x0[None, :], 2, 3e-8))
    assert "bundle-adjustment components on the plain batch solver" in msg and "rotation records" in msg, msg
    assert "cooperative" not in msg and "tiny" not in msg, msg
    usable(plan, ba.x0)
    plan.set_option("lds_resident", 1)
    plan.solve_starts(ba.x0[None, :], 2, 3e-8)
    assert plan.info("components_lds") == 2 and np.all(np.isfinite(plan.fetch_starts().fret))
    g.close()

    pp = _sinusoid_from_the_committed_start()
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.set_option("trace_records", 16)
    assert "trace_records" in _refused(lambda: plan.solve_starts(pp.x0[None, :], 2, 3e-8))
    usable(plan, pp.x0)
    plan.set_option("trace_records", 0)
    plan.solve_starts(pp.x0[None, :], 25, 3e-8)
    assert plan.fetch_starts().fret[0, 0] == 1578.9001138212975
