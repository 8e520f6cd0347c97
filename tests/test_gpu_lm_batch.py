"""Levenberg-Marquardt for a batch of small components in one call (rdis_hip_lm_batch; rdis_amd/csrc/lm_batch.hip): one
workgroup per component, the whole iteration on the device.  Every component is checked step by step against
oracle/lm_oracle.py run component by component (tests/lm_batch_shapes.py; tests/test_lm_batch_oracle_cpu.py pins that
the oracle's own sensitivity on these shapes is 100 times below the tolerances used here), against the sequential
entry rdis_hip_lm_optimize, for the state it leaves, for invariance under the batch's composition and order, for its
refusals, and by properties at full size."""
import numpy as np
import pytest

from rdis_amd import capi, problems as P

import lm_batch_shapes as S
from lm_exit_cases import check_identities

pytestmark = pytest.mark.gpu

EINVAL, EOVERLAP, ERANGE = -1, -4, -5


def _compare(r, ro, tol_hist=1e-7, cap=64):
    # (tests/test_gpu_lm.py's)  Once a trial objective equals the current one to 1e-11 the solve has converged and accepting or
    # rejecting a step is decided by rounding: histories are compared up to that point, results always.
    n_cmp, fcur = len(ro.history), ro.finit
    for i, (_, _, ft, ok) in enumerate(ro.history):
        if abs(ft - fcur) <= 1e-11 * abs(fcur):
            n_cmp = i
            break
        if ok:
            fcur = ft
    # the loop's counter identities, whatever the exit (cap: the capacity the history was fetched with -- the default of Problem.lm_batch and LmPlan)
    check_identities(r, ro.finit, cap)
    if n_cmp == len(ro.history):
        assert (r.iters, r.stop, r.nsolve, r.nfev, r.njev) == (ro.iters, ro.stop, ro.nsolve, ro.nfev, ro.njev)
        assert len(r.history) == len(ro.history)
        assert abs(r.mu - ro.mu) <= 1e-6 * ro.mu
    else:
        # the oracle converged: the device ends as the oracle does, or -- where rounding decides the last steps -- with a small
        # step (2) or refused steps (5)
        assert r.stop in (2, 5, ro.stop)
        if ro.stop in (2, 5):
            assert r.stop in (2, 5)
    assert len(r.history) >= n_cmp
    for (mu, dp, ft, ok), (omu, odp, oft, ook) in list(zip(r.history, ro.history))[:n_cmp]:
        assert bool(ok) == bool(ook)                                    # same accept / reject decisions
        assert abs(mu - omu) <= tol_hist * omu and abs(dp - odp) <= tol_hist * odp and abs(ft - oft) <= tol_hist * abs(oft)
    assert abs(r.fret - ro.fret) <= 1e-8 * abs(ro.fret)
    assert np.max(np.abs(r.x - ro.x)) <= 1e-7 * (1.0 + np.max(np.abs(ro.x)))


def _deviations(r, ro):
    n = min(len(r.history), len(ro.history))
    dh = 0.0
    if n:
        h, oh = np.asarray(r.history, dtype=np.float64)[:n, :3], np.array(ro.history, dtype=np.float64)[:n, :3]
        dh = float(np.max(np.abs(h - oh) / np.abs(oh)))
    return (dh, float(np.max(np.abs(r.x - ro.x)) / (1.0 + np.max(np.abs(ro.x)))),
            abs(r.fret - ro.fret) / abs(ro.fret) if ro.fret != r.fret else 0.0)


def _same(a, b):
    """every field, the history and x of two results equal with =="""
    return ((a.fret, a.delta, a.iters, a.stop, a.nfev, a.njev, a.nsolve, a.mu, a.camera_blocks, a.point_blocks) ==
            (b.fret, b.delta, b.iters, b.stop, b.nfev, b.njev, b.nsolve, b.mu, b.camera_blocks, b.point_blocks) and
            a.history.tobytes() == b.history.tobytes() and a.x.tobytes() == b.x.tobytes())


def _batch(g, comps, **kw):
    return g.lm_batch(*S.csr(comps), **kw)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", S.CASES)
def test_batch_steps_equal_dense_oracle(name, model, gctx):
    """one lm_batch call per shape, every component against its oracle run: the classes no camera (points alone), few
    cameras (1, 2, 3, 5) and up to 16 (the limit itself), blocks with constant variables, constant cameras / points of
    listed factors, components of 0 to 463 factors, rejected steps (re-damped solves) in all but one case"""
    pp, comps, iters, _, blocks, _ = S.shape(name)
    ref = S.oracle_reference(name, model)
    rs = _batch(capi.Problem(gctx, pp), comps, maxiters=iters, model=model)
    assert len(rs) == len(comps)
    worst = np.max([_deviations(r, ro) for r, ro in zip(rs, ref)], axis=0)
    print("LM batch %s, model %d, %d components against the oracle: history %.1e, x %.1e, fret %.1e" % ((name, model, len(comps)) + tuple(worst)))
    for r, ro in zip(rs, ref):
        _compare(r, ro)
        assert (r.camera_blocks, r.point_blocks) == blocks
        assert abs(r.delta - (r.fret - ro.finit)) <= 1e-12 * max(ro.finit, 1e-300)
    if name == "ladybug-49-300-cameras":
        empty = [c for c, (_, fac) in enumerate(comps) if len(fac) == 0]
        assert len(empty) == 3
        for c in empty:
            free = comps[c][0]
            assert (rs[c].stop, rs[c].iters, rs[c].fret, len(rs[c].history)) == (6, 0, 0.0, 0)
            assert np.array_equal(rs[c].x, np.minimum(np.maximum(pp.x0[free], pp.lo[free]), pp.hi[free]))


# ---- 2. against the sequential entry -----------------------------------------------------------------------------------------
def _component_problem(pp, free, fac):
    """a component of a synthetic problem (a contiguous variable and factor range) as a problem of its own: the layout
    rdis_hip_lm_optimize requires, cameras first"""
    v0 = int(free[0])
    return P.PackedProblem(kind=pp.kind, x0=pp.x0[free].copy(), lo=pp.lo[free].copy(), hi=pp.hi[free].copy(),
                           cam_vid0=pp.cam_vid0[fac] - v0, pt_vid0=pp.pt_vid0[fac] - v0, obs=pp.obs[fac].copy())


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("name", ["ladybug-5-30-whole", "synthetic-6x3x40"])
def test_batch_and_sequential_entry_agree(name, model, gctx):
    """rdis_hip_lm_optimize component by component from the same start: equal accept / reject sequences, trial values
    within 1e-9 (the criterion of test_gpu_lm.test_sparse_and_dense_schur_products_agree)"""
    pp, comps, iters, _, _, _ = S.shape(name)
    rs = _batch(capi.Problem(gctx, pp), comps, maxiters=iters, model=model)
    for r, (free, fac) in zip(rs, comps):
        q = pp if len(comps) == 1 else _component_problem(pp, free, fac)
        s = capi.Problem(gctx, q).lm_optimize(maxiters=iters, model=model)
        assert len(r.history) == len(s.history) and np.array_equal(r.history[:, 3], s.history[:, 3])
        assert np.max(np.abs(r.history[:, 2] - s.history[:, 2]) / np.abs(s.history[:, 2])) <= 1e-9
        assert (r.iters, r.stop, r.nsolve, r.camera_blocks, r.point_blocks) == (s.iters, s.stop, s.nsolve, s.camera_blocks, s.point_blocks)
        assert abs(r.fret - s.fret) <= 1e-9 * abs(s.fret)


# ---- 3. state ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladybug-5-30-sub-block", "ladybug-5-30-points", "synthetic-6x3x40"])
def test_batch_leaves_the_results_assigned_and_the_rest_untouched(name, gctx):
    pp, comps, iters, _, _, _ = S.shape(name)
    fp, fv, jp, fj = S.csr(comps)
    g = capi.Problem(gctx, pp)
    before = g.get_x()
    rs = g.lm_batch(fp, fv, jp, fj, x=pp.x0[fv], maxiters=iters, model=2)
    after = g.get_x()
    assert after[fv].tobytes() == np.concatenate([r.x for r in rs]).tobytes()          # the variables are left assigned to the results
    rest = np.setdiff1d(np.arange(pp.nvars), fv)
    assert after[rest].tobytes() == before[rest].tobytes()                             # every other variable: the same bytes
    for r, (free, fac) in zip(rs, comps):
        assert abs(g.eval(fac) - r.fret) <= 1e-12 * r.fret
        assert np.all(r.x >= pp.lo[free]) and np.all(r.x <= pp.hi[free])
    # x = None starts at the assigned values
    g2 = capi.Problem(gctx, pp)
    rn = g2.lm_batch(fp, fv, jp, fj, maxiters=iters, model=2)
    assert all(_same(a, b) for a, b in zip(rs, rn)) and g2.get_x().tobytes() == after.tobytes()


# ---- 4. invariance and determinism ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2])
def test_a_components_bits_do_not_depend_on_the_batch(model, gctx):
    """the same components solved in order, in reversed order, two of them alone, and once more: every field, history and x
    of a component equal with =="""
    pp, comps, iters, _, _, _ = S.shape("synthetic-6x3x40")

    def run(g, idx):
        sub = [comps[i] for i in idx]
        return dict(zip(idx, _batch(g, sub, x=np.concatenate([pp.x0[f] for f, _ in sub]), maxiters=iters, model=model)))

    g = capi.Problem(gctx, pp)
    a = run(g, [0, 1, 2, 3, 4, 5])
    b = run(capi.Problem(gctx, pp), [5, 4, 3, 2, 1, 0])
    c = run(capi.Problem(gctx, pp), [4, 1])
    d = run(g, [0, 1, 2, 3, 4, 5])                                   # a second identical call, same problem and workspace
    assert all(len(a[i].history) > 0 for i in a)
    assert all(_same(a[i], b[i]) for i in a) and all(_same(a[i], c[i]) for i in c) and all(_same(a[i], d[i]) for i in a)


def test_the_camera_plans_bits_do_not_depend_on_the_order(gctx):
    pp, comps, iters, _, _, _ = S.shape("ladybug-49-300-cameras")
    a = _batch(capi.Problem(gctx, pp), comps, maxiters=iters, model=1)
    b = _batch(capi.Problem(gctx, pp), comps[::-1], maxiters=iters, model=1)[::-1]
    assert all(_same(x, y) for x, y in zip(a, b))


# ---- 5. the limit and the refusals -------------------------------------------------------------------------------------------
def _refused(g, comps, code, x=None, model=1, words=()):
    before = g.get_x()
    with pytest.raises(capi.RdisHipError) as e:
        _batch(g, comps, x=x, maxiters=5, model=model)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    assert g.get_x().tobytes() == before.tobytes()                   # nothing was solved, nothing was written
    return str(e.value)


def test_more_than_sixteen_cameras_are_refused(gctx):
    pp = P.make_synthetic_ba(1, 17, 60, obs_per_pt=6)
    whole = [(np.arange(pp.nvars, dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))]
    _refused(capi.Problem(gctx, pp), whole, ERANGE, words=("component 0", "17", "16"))
    # the same component last in a batch behind a valid one, with start values that differ from the assigned ones
    pp = P.make_synthetic_ba(2, 17, 60, obs_per_pt=6)
    nv, nf = pp.nvars // 2, pp.nfac // 2
    free0 = np.concatenate([np.arange(27), 9 * 17 + np.arange(3 * 60)]).astype(np.int64)      # 3 cameras and the points of block 0
    comps = [(free0, np.arange(nf, dtype=np.int64)), (nv + np.arange(nv, dtype=np.int64), nf + np.arange(nf, dtype=np.int64))]
    g = capi.Problem(gctx, pp)
    x = np.concatenate([pp.x0[f] for f, _ in comps]) + 1e-3
    _refused(g, comps, ERANGE, x=x, words=("component 1", "16"))
    rs = _batch(g, comps[:1], maxiters=3, model=2)                    # the valid one alone is solved
    assert rs[0].camera_blocks == 3 and rs[0].point_blocks == 60 and rs[0].delta < 0


def test_dependent_components_and_bad_arguments_are_refused(gctx):
    pp = P.load_bal(ncams=5, npts=30)
    g = capi.Problem(gctx, pp)
    pts = S.shape("ladybug-5-30-points")[1]
    shared = [pts[0], (np.concatenate([pts[1][0], pts[0][0][:1]]), pts[1][1])]
    _refused(g, shared, EOVERLAP)                                    # two components share a free variable
    reads = [pts[0], (pts[1][0], np.concatenate([pts[1][1], pts[0][1][:1]]))]
    _refused(g, [reads[1], (pts[0][0], pts[0][1][1:])], EOVERLAP)    # a factor of one reads a free variable of the other
    _refused(g, pts[:2], EINVAL, model=3)
    _refused(g, [(np.array([45, 46, pp.nvars], dtype=np.int64), pts[0][1])], EINVAL)          # variable id out of range
    q = P.load_poly()
    _refused(capi.Problem(gctx, q), [(np.array([0], dtype=np.int64), np.array([0], dtype=np.int64))], EINVAL)   # not bundle adjustment
    # two factors joining the same camera and point
    dup = P.PackedProblem(kind=pp.kind, x0=pp.x0.copy(), lo=pp.lo.copy(), hi=pp.hi.copy(), cam_vid0=np.concatenate([pp.cam_vid0, pp.cam_vid0[:1]]),
                          pt_vid0=np.concatenate([pp.pt_vid0, pp.pt_vid0[:1]]), obs=np.concatenate([pp.obs, pp.obs[:1] + 1.0]))
    gd = capi.Problem(gctx, dup)
    whole = [(np.arange(dup.nvars, dtype=np.int64), np.arange(dup.nfac, dtype=np.int64))]
    _refused(gd, whole, EINVAL, words=("same camera and point",))
    # ... which is fine where the camera (or the point) is constant: the pair forms no Z block
    p0 = int(dup.pt_vid0[0])
    rs = _batch(gd, [(p0 + np.arange(3, dtype=np.int64), np.where(dup.pt_vid0 == p0)[0].astype(np.int64))], maxiters=3, model=2)
    assert rs[0].point_blocks == 1 and rs[0].camera_blocks == 0 and rs[0].delta < 0


# ---- 6. full size, properties only -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", ["cameras", "points"])
def test_full_ladybug_plans_properties(fixed, gctx):
    """full ladybug with the cameras constant (7776 point components of 3 unknowns, one call) and with the points constant
    (49 camera components of 9 unknowns and 361 to 906 factors), components from rdis_hip_components, model 2, 5 iterations"""
    pp = P.load_bal()
    g = capi.Problem(gctx, pp)
    assigned = np.zeros(pp.nvars, dtype=np.uint8)
    if fixed == "cameras":
        assigned[:9 * 49] = 1
    else:
        assigned[9 * 49:] = 1
    fp, fv, jp, fj = g.components(assigned)
    ncomp = len(fp) - 1
    assert ncomp == (7776 if fixed == "cameras" else 49)
    f0 = g.eval()
    rs = g.lm_batch(fp, fv, jp, fj, maxiters=5, model=2, history=8)
    assert len(rs) == ncomp
    assert all(r.delta <= 0 for r in rs)
    assert all((r.camera_blocks, r.point_blocks) == ((0, 1) if fixed == "cameras" else (1, 0)) for r in rs)
    x = g.get_x()
    assert np.all(x >= pp.lo) and np.all(x <= pp.hi)
    assert x[fv].tobytes() == np.concatenate([r.x for r in rs]).tobytes()
    total, f1 = float(np.sum([r.fret for r in rs])), g.eval()
    print("LM batch, full ladybug, %s constant: %d components, %.6g -> %.6g" % (fixed, ncomp, f0, f1))
    assert abs(total - f1) <= 1e-12 * f1 and f1 < f0
