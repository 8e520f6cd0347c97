"""The wide class of the batched Levenberg-Marquardt entry (RDIS_HIP_LM_WIDE; capi: wide=True): components of 17 to 64 active
camera blocks, one workgroup each, the reduced system in the component's workspace slice and factorised in 16-column
panels on the matrix cores (rdis_amd/csrc/lm_batch.hip, class 3).  Every component is checked step by step against
oracle/lm_oracle.py (tests/lm_wide_shapes.py; tests/test_lm_wide_oracle_cpu.py pins that the oracle's own sensitivity on
these shapes is 100 times below the tolerances used here -- test_gpu_lm_batch._compare's, unchanged), against the
sequential entry rdis_hip_lm_optimize, for invariance under the batch's composition, for the state it leaves, for its
refusals, and through the plans and their population solves.  Without the option every one of these calls is refused
with RDIS_HIP_ERANGE."""
import numpy as np
import pytest

from rdis_amd import capi, problems as P

import lm_plan_members as M
import lm_wide_shapes as W
from test_gpu_lm_batch import _compare, _deviations, _same

pytestmark = pytest.mark.gpu

EINVAL, EOVERLAP, ERANGE = -1, -4, -5


def _batch(g, comps, **kw):
    return g.lm_batch(*W.csr(comps), **kw)


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", W.CASES)
def test_wide_steps_equal_dense_oracle(name, model, gctx):
    """one wide lm_batch call per shape, every component against its oracle run: 17 cameras (a partial last tile that holds the
    right-hand side too), two components of 33, the limit of 64 (the right-hand side in a tile row of its own), ladybug 21 / 120
    and 49 / 300 (three cameras without a listed point); rejected steps (re-damped solves) in every case"""
    pp, comps, iters, _, blocks, rejected = W.shape(name)
    ref = W.oracle_reference(name, model)
    rs = _batch(capi.Problem(gctx, pp), comps, maxiters=iters, model=model, wide=True)
    assert len(rs) == len(comps)
    assert any(not h[3] for r in rs for h in r.history) == rejected[model]
    worst = np.max([_deviations(r, ro) for r, ro in zip(rs, ref)], axis=0)
    print("LM wide %s, model %d, %d components against the oracle: history %.1e, x %.1e, fret %.1e" % ((name, model, len(comps)) + tuple(worst)))
    for r, ro in zip(rs, ref):
        _compare(r, ro)
        assert (r.camera_blocks, r.point_blocks) == blocks
        assert abs(r.delta - (r.fret - ro.finit)) <= 1e-12 * max(ro.finit, 1e-300)


# ---- 2. against the sequential entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2])
def test_wide_and_sequential_entry_agree(model, gctx):
    """rdis_hip_lm_optimize on ladybug 49 / 300 from the same start: equal accept / reject sequences, trial values within 1e-9
    (the criterion of test_gpu_lm_batch.test_batch_and_sequential_entry_agree)"""
    pp, comps, iters, _, _, _ = W.shape("ladybug-49-300-whole")
    r = _batch(capi.Problem(gctx, pp), comps, maxiters=iters, model=model, wide=True)[0]
    s = capi.Problem(gctx, pp).lm_optimize(maxiters=iters, model=model)
    assert len(r.history) == len(s.history) > 0 and np.array_equal(r.history[:, 3], s.history[:, 3])
    assert np.max(np.abs(r.history[:, 2] - s.history[:, 2]) / np.abs(s.history[:, 2])) <= 1e-9
    assert (r.iters, r.stop, r.nsolve, r.camera_blocks, r.point_blocks) == (s.iters, s.stop, s.nsolve, s.camera_blocks, s.point_blocks)
    assert abs(r.fret - s.fret) <= 1e-9 * abs(s.fret)


# ---- 3. all four classes in one call; invariance and determinism -----------------------------------------------------------------
def _four_classes():
    """five blocks of 20 cameras x 40 points: block 0 and block 4 whole (class 3: 20 cameras), 8 cameras of block 1 and its
    points (class 2), 3 cameras of block 2 and its points (class 1), the points of block 3 alone (class 0)"""
    pp = P.make_synthetic_ba(5, 20, 40, obs_per_pt=6, first_comp=13)
    nv, nf = pp.nvars // 5, pp.nfac // 5
    fac = [c * nf + np.arange(nf, dtype=np.int64) for c in range(5)]
    pts = 180 + np.arange(120)
    comps = [(np.arange(nv, dtype=np.int64), fac[0]),
             (nv + np.concatenate([np.arange(72), pts]).astype(np.int64), fac[1]),
             (2 * nv + np.concatenate([np.arange(27), pts]).astype(np.int64), fac[2]),
             (3 * nv + pts.astype(np.int64), fac[3]),
             (4 * nv + np.arange(nv, dtype=np.int64), fac[4])]
    return pp, comps


@pytest.mark.parametrize("model", [1, 2])
def test_one_call_with_all_four_classes(model, gctx):
    """the components of at most 16 cameras == a call without the option on them alone (every field, history and x); the wide
    ones == themselves solved alone, in reversed order, and in a second identical call on the same workspace"""
    pp, comps = _four_classes()

    def run(g, idx, wide):
        sub = [comps[i] for i in idx]
        return dict(zip(idx, _batch(g, sub, x=np.concatenate([pp.x0[f] for f, _ in sub]), maxiters=5, model=model, wide=wide)))

    g = capi.Problem(gctx, pp)
    a = run(g, [0, 1, 2, 3, 4], True)
    assert [a[i].camera_blocks for i in range(5)] == [20, 8, 3, 0, 20] and all(a[i].point_blocks == 40 for i in a)
    assert all(len(a[i].history) > 0 and a[i].delta < 0 for i in a)
    narrow = run(capi.Problem(gctx, pp), [1, 2, 3], False)
    assert all(_same(a[i], narrow[i]) for i in narrow)
    b = run(capi.Problem(gctx, pp), [4, 3, 2, 1, 0], True)
    c = run(capi.Problem(gctx, pp), [4], True)
    d = run(capi.Problem(gctx, pp), [0], True)
    e = run(g, [0, 1, 2, 3, 4], True)                                 # a second identical call, same problem and workspace
    assert all(_same(a[i], b[i]) for i in a) and _same(a[4], c[4]) and _same(a[0], d[0]) and all(_same(a[i], e[i]) for i in a)
    assert not _same(a[0], a[4])


# ---- 4. state ----------------------------------------------------------------------------------------------------------------
def test_wide_leaves_the_results_assigned_and_the_rest_untouched(gctx):
    """block 0 of synthetic 2 x (33, 90) with its last three cameras constant (30 active cameras, factors that read constants):
    the free variables end at the results, the three cameras and all of block 1 keep their bytes; x given and x = None"""
    pp, comps, iters, _, _, _ = W.shape("synthetic-2x33x90")
    free0, fac0 = comps[0]
    free = np.concatenate([free0[:9 * 30], free0[9 * 33:]])
    fp, fv, jp, fj = W.csr([(free, fac0)])
    g = capi.Problem(gctx, pp)
    before = g.get_x()
    rs = g.lm_batch(fp, fv, jp, fj, x=pp.x0[fv], maxiters=iters, model=2, wide=True)
    after = g.get_x()
    assert (rs[0].camera_blocks, rs[0].point_blocks) == (30, 90) and rs[0].delta < 0
    assert after[fv].tobytes() == rs[0].x.tobytes()
    rest = np.setdiff1d(np.arange(pp.nvars), fv)
    assert len(rest) == 27 + len(free0) and after[rest].tobytes() == before[rest].tobytes()
    assert abs(g.eval(fac0) - rs[0].fret) <= 1e-12 * rs[0].fret
    assert np.all(rs[0].x >= pp.lo[free]) and np.all(rs[0].x <= pp.hi[free])
    g2 = capi.Problem(gctx, pp)                                       # x = None starts at the assigned values
    rn = g2.lm_batch(fp, fv, jp, fj, maxiters=iters, model=2, wide=True)
    assert _all_same(rs, rn) and g2.get_x().tobytes() == after.tobytes()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _refused(g, comps, code, x=None, wide=False, words=()):
    before = g.get_x()
    with pytest.raises(capi.RdisHipError) as e:
        _batch(g, comps, x=x, maxiters=5, model=1, wide=wide)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    assert g.get_x().tobytes() == before.tobytes()                   # nothing was solved, nothing was written


def test_wide_refusals(gctx):
    pp = P.make_synthetic_ba(1, 65, 70, obs_per_pt=6)
    whole = [(np.arange(pp.nvars, dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))]
    g = capi.Problem(gctx, pp)
    _refused(g, whole, ERANGE, x=pp.x0 + 1e-3, wide=True, words=("component 0", "65", "64"))
    _refused(g, whole, ERANGE, wide=False, words=("component 0", "65", "16"))
    # 17 cameras without the option: today's text; also behind a valid component, with start values that differ
    pp = P.make_synthetic_ba(2, 17, 60, obs_per_pt=6)
    nv, nf = pp.nvars // 2, pp.nfac // 2
    free0 = np.concatenate([np.arange(27), 9 * 17 + np.arange(3 * 60)]).astype(np.int64)
    comps = [(free0, np.arange(nf, dtype=np.int64)), (nv + np.arange(nv, dtype=np.int64), nf + np.arange(nf, dtype=np.int64))]
    g = capi.Problem(gctx, pp)
    _refused(g, comps[1:], ERANGE, words=("component 0 has 17 active camera blocks, the limit is 16 (RDIS_HIP_LM_BATCH_MAX_CAMERAS)",))
    x = np.concatenate([pp.x0[f] for f, _ in comps]) + 1e-3
    _refused(g, comps, ERANGE, x=x, words=("component 1", "17", "16"))
    rs = _batch(g, comps, maxiters=3, model=2, wide=True)             # ... and with the option both are solved
    assert [(r.camera_blocks, r.point_blocks) for r in rs] == [(3, 60), (17, 60)] and all(r.delta < 0 for r in rs)


# ---- 6. plans ------------------------------------------------------------------------------------------------------------------
def _batch_from(gctx, pp, comps, x, iters, model):
    g = capi.Problem(gctx, pp)
    g.set_x(x)
    rs = g.lm_batch(*W.csr(comps), maxiters=iters, model=model, wide=True)
    return rs, g.get_x()


@pytest.mark.parametrize("model", [1, 2])
def test_wide_plan_solve_and_population_rows_equal_lm_batch(model, gctx):
    """LmPlan(wide=True) on synthetic 2 x (33, 90): solve + fetch == lm_batch; solve_population on three members that differ,
    each == lm_batch on a problem whose x is that member's; once more one member a launch: the split changes no bit; the same
    lists without the option are refused at create"""
    pp, comps, iters = W.shape("synthetic-2x33x90")[:3]
    lists = W.csr(comps)
    g = capi.Problem(gctx, pp)
    with pytest.raises(capi.RdisHipError) as e:
        capi.LmPlan(g, *lists, model=model)
    assert e.value.code == ERANGE and "lm_plan_create" in str(e.value) and "33" in str(e.value) and "16" in str(e.value)
    plan = capi.LmPlan(g, *lists, model=model, wide=True)
    ref, xref = _batch_from(gctx, pp, comps, pp.x0, iters, model)
    plan.solve(iters)
    assert _all_same(plan.fetch(), ref) and g.get_x().tobytes() == xref.tobytes()
    assert plan.info("launches") == 1 and plan.info("members_per_launch") == 1
    mb = plan.info("member_workspace_bytes")
    assert mb >= 2 * 8 * 19 * 20 // 2 * 256                           # two components' tiles: 19 tile rows at 297 unknowns
    X = M.members_of(pp, comps, 3)
    want = [_batch_from(gctx, pp, comps, X[s], iters, model) for s in range(3)]
    assert not _all_same(want[0][0], want[1][0]) and not _all_same(want[1][0], want[2][0])
    g.set_x(pp.x0)
    before = g.get_x()
    for budget, per, launches in ((1 << 30, 3, 1), (mb, 1, 3)):
        plan.set_option("workspace_bytes", budget)
        pop = capi.Population(g, x=X)
        plan.solve_population(pop, maxiters=iters)
        rows = plan.fetch_population()
        assert plan.info("members_per_launch") == per and plan.info("launches") == launches
        for s in range(3):
            assert _all_same(rows[s], want[s][0]), "member %d" % s
            assert pop.get_x(s).tobytes() == want[s][1].tobytes(), "member %d" % s
    assert g.get_x().tobytes() == before.tobytes()                   # the problem's own x is not touched
