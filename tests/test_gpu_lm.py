"""The second subspace solver, Levenberg-Marquardt for bundle adjustment (rdis_hip_lm_optimize;
reference shape: LMSubspaceOptimizer + levmar).  levmar is not vendored by the reference, so parity
is UNPINNED; the device solver (block normal equations, Schur complement, fp64 matrix-core
contractions) is checked step by step against the dense numpy restatement in oracle/lm_oracle.py,
and by properties at full size."""
import numpy as np
import pytest

from oracle import lm_oracle as LM
from oracle import oracle as O
from rdis_amd import capi, problems as P

from lm_exit_cases import check_identities

pytestmark = pytest.mark.gpu


def _compare(r, ro, tol_hist=1e-7, cap=256):
    # Once a trial objective equals the current one to 1e-11 the solve has converged and accepting or
    # rejecting a step is decided by rounding: histories are compared up to that point, results always.
    n_cmp, fcur = len(ro.history), ro.finit
    for i, (_, _, ft, ok) in enumerate(ro.history):
        if abs(ft - fcur) <= 1e-11 * abs(fcur):
            n_cmp = i
            break
        if ok:
            fcur = ft
    # the loop's counter identities, whatever the exit (cap: the capacity the history was fetched with -- the default of Problem.lm_optimize)
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


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("nc,npt,iters", [(5, 30, 25), (49, 300, 12)])
def test_lm_steps_equal_dense_oracle(nc, npt, iters, model, gctx):
    """model 1: the reference's residual sqrt(2 E_j); model 2: the two pixel residuals per factor with
    trial points projected into the domains"""
    pp = P.load_bal(ncams=nc, npts=npt)
    r = capi.Problem(gctx, pp).lm_optimize(maxiters=iters, model=model)
    ro = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), maxiters=iters, model=model)
    _compare(r, ro)
    assert r.camera_blocks == nc and r.point_blocks == npt and r.delta < 0
    if model == 2 and nc == 5:
        assert r.fret < 25.09                       # below 25 CG iterations


def test_lm_sub_block_with_constants(gctx):
    """free: camera 0's rotation and translation (not its intrinsics), camera 3, points 0..9; only the
    factors of those points listed; everything else constant"""
    pp = P.load_bal(ncams=5, npts=30)
    free = np.concatenate([np.arange(0, 6), np.arange(27, 36), np.arange(45, 75)]).astype(np.int64)
    fac = np.where(pp.pt_vid0 < 75)[0].astype(np.int64)
    g = capi.Problem(gctx, pp)
    r = g.lm_optimize(free, fac, maxiters=15)
    ro = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), free, fac, maxiters=15)
    _compare(r, ro)
    x_all = g.get_x()
    rest = np.setdiff1d(np.arange(pp.nvars), free)
    assert np.array_equal(x_all[rest], pp.x0[rest]) and np.array_equal(x_all[free], r.x)   # constants untouched, block left assigned
    # cameras only (no free point: the reduced system is the whole system) and points only (no dense solve)
    for model in (1, 2):
        for fr in (np.arange(0, 45, dtype=np.int64), np.arange(45, 135, dtype=np.int64)):
            g.set_x(pp.x0)
            r = g.lm_optimize(fr, None, maxiters=8, model=model)
            ro = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), fr, None, maxiters=8, model=model)
            _compare(r, ro)


def test_lm_full_ladybug_properties(gctx):
    pp = P.load_bal()
    g = capi.Problem(gctx, pp)
    f0 = g.eval()
    r = g.lm_optimize(maxiters=10)
    assert r.camera_blocks == 49 and r.point_blocks == 7776 and r.iters == 10 and r.stop == 3
    assert abs((r.fret - r.delta) - f0) <= 1e-12 * f0 and r.fret < 0.6 * f0
    accepted = r.history[r.history[:, 3] == 1]
    assert len(accepted) == 10 and np.all(np.diff(accepted[:, 2]) < 0)     # every accepted step lowers the objective
    assert np.array_equal(g.get_x(), r.x) and abs(g.eval() - r.fret) <= 1e-12 * r.fret
    assert np.all(r.x >= pp.lo) and np.all(r.x <= pp.hi)
    o = O.OracleProblem(pp)
    o.assign(None, r.x)
    assert abs(o.eval() - r.fret) <= 1e-12 * r.fret                         # oracle's objective at the device's point
    # the first step solves the damped normal equations: check the residual of that linear system on the CPU
    # (domains removed: the final clamp -- 36 intrinsics here -- is not part of the linear step)
    pp = P.load_bal()
    pp.lo[:], pp.hi[:] = -np.inf, np.inf
    r1 = capi.Problem(gctx, pp).lm_optimize(maxiters=1)
    o = O.OracleProblem(pp, emulate_stale_cache=False)
    grad = o.gradient()
    dp = r1.x - pp.x0
    assert r1.history[-1, 3] == 1
    mu = r1.history[-1, 0]                                                   # the damping of the accepted solve
    E, G = o.eval_each(np.arange(pp.nfac)), o.grad_each_ba(np.arange(pp.nfac))
    Jd = np.zeros(pp.nvars)                                                  # (J^T J + mu I) dp + grad, matrix-free
    vids = np.concatenate([pp.cam_vid0[:, None] + np.arange(9), pp.pt_vid0[:, None] + np.arange(3)], axis=1)
    rows = G / np.sqrt(2.0 * E)[:, None]
    np.add.at(Jd, vids.reshape(-1), (rows * np.sum(rows * dp[vids], axis=1)[:, None]).reshape(-1))
    res = Jd + mu * dp + grad
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(grad)


def test_lm_pixel_residual_model_full_ladybug(gctx):
    """the usual bundle-adjustment model on the same machinery (pixel residuals, Marquardt scaling,
    projected trial points): 25 iterations take full ladybug from 8.5e5 to 1.5e4 -- 25 CG iterations end at
    8.3e4 (BASELINE config 4), the reference's whole RDIS run at 1.0e5 after 240 s"""
    pp = P.load_bal()
    g = capi.Problem(gctx, pp)
    r = g.lm_optimize(maxiters=25, model=2)
    assert r.iters == 25 and r.fret < 2.0e4 and r.delta < 0
    accepted = r.history[r.history[:, 3] == 1]
    assert np.all(np.diff(accepted[:, 2]) < 0)
    assert np.all(r.x >= pp.lo) and np.all(r.x <= pp.hi) and np.array_equal(g.get_x(), r.x)
    o = O.OracleProblem(pp)
    o.assign(None, r.x)
    assert abs(o.eval() - r.fret) <= 1e-12 * r.fret and abs(accepted[-1, 2] - r.fret) <= 1e-12 * r.fret


# ---- reduced systems beyond ladybug's: more than 512 unknowns --------------------------------------------------------
# ladybug has at most 49 cameras: a padded reduced system Mp of 64 or 448.  The tests below reach what lm_solver.hip
# does only for larger ones, on make_synthetic_ba blocks in which every point is seen by a cyclic window of K cameras
# (the reduced matrix couples different cameras: the off-block sums of k_trail, k_trsv and k_trsv_left multiply
# non-zeros).  Against the parent commit's run of this file (5 s on an MI355X host) they add 13 s, nearly all of it the
# CPU oracle: 3.5 s a case at 120 cameras, 1.3 s at 58 and 64, 0.4 s for the sub-block, 0.01 s for a boundary solve.
def _converged_at(ro):
    """index of the first history entry whose trial objective equals the current one to 1e-11 (where _compare stops
    comparing histories), or len(history)"""
    fcur = ro.finit
    for i, (_, _, ft, ok) in enumerate(ro.history):
        if abs(ft - fcur) <= 1e-11 * abs(fcur):
            return i
        if ok:
            fcur = ft
    return len(ro.history)


def _deviations(r, ro):
    n = min(len(r.history), len(ro.history))
    h, oh = np.asarray(r.history, dtype=np.float64)[:n, :3], np.array(ro.history, dtype=np.float64)[:n, :3]
    return (float(np.max(np.abs(h - oh) / np.abs(oh))), float(np.max(np.abs(r.x - ro.x)) / (1.0 + np.max(np.abs(ro.x)))),
            abs(r.fret - ro.fret) / abs(ro.fret))


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("nc,npt,k,iters", [(58, 400, 6, 8), (64, 400, 6, 8), (120, 700, 6, 4)])
def test_lm_steps_beyond_512_unknowns(nc, npt, k, iters, model, gctx):
    """Step by step against the dense oracle, dense (schur 1) and block-sparse (schur 2) Schur product, and the two
    against each other (the criteria of test_sparse_and_dense_schur_products_agree).
    58 cameras: M = 522, Mp = 576 -- 54 padding rows (unit diagonal from k_sfinish / k_sinit, the padding reset of k_rhs),
        and k_trsv's strided loop "more unknowns than threads" (Mp > TRSV_THREADS = 512) runs, one stride.
    64 cameras: M = Mp = 576 -- no padding at all (9 * 64 is a multiple of 64): no row takes the `else` of k_sfinish /
        k_sinit, and k_panel's right-hand-side row Mp directly follows the last real row.
    120 cameras: M = 1080, Mp = 1088 -- k_trsv's strided loop takes two strides (Mp >= 1088); 17 tiles: SK =
        2048 / 153 = 13 (ladybug's 49 cameras: 64), a k_syrk grid of 17 x 17 tile pairs by 13 slices.
    The comparison is of the whole history (the oracle never converges within the iteration limit) and includes
    re-damped solves (the oracle rejects at least one step); tests/test_lm_oracle_cpu.py pins that the oracle's
    own sensitivity to rounding is 100 times below _compare's tolerances on these problems.
    Observed on an MI355X, largest deviation from the oracle over both Schur paths (history, x, fret):
     58 cameras: model 1  8.8e-13, 1.2e-16, 7.7e-14;  model 2  2.1e-12, 3.1e-14, 2.8e-14
     64 cameras: model 1  1.3e-12, 3.4e-16, 2.1e-13;  model 2  3.7e-12, 2.9e-14, 9.4e-14
    120 cameras: model 1  1.0e-13, 2.0e-16, 1.1e-14;  model 2  8.0e-13, 3.7e-14, 7.8e-14
    With k_trsv's strided loop made to skip its second stride the two 120-camera cases fail and the others pass.
    Time: with the other tests of this section the file takes 18 s on an MI355X host where the parent commit's took 5 s."""
    pp = P.make_synthetic_ba(1, nc, npt, obs_per_pt=k, first_comp=7)
    ro = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), maxiters=iters, model=model)
    assert _converged_at(ro) == len(ro.history) and ro.stop == 3      # nothing truncated: _compare sees every solve
    assert any(not h[3] for h in ro.history)                           # a rejected step: the re-damped solve is compared
    res = {}
    for schur in (1, 2):
        r = res[schur] = capi.Problem(gctx, pp).lm_optimize(maxiters=iters, model=model, schur=schur)
        print("LM %d cameras (Mp %d), model %d, schur %d against the oracle: history %.1e, x %.1e, fret %.1e" % (
            (nc, (9 * nc + 63) // 64 * 64, model, schur) + _deviations(r, ro)))
        _compare(r, ro)
        assert r.camera_blocks == nc and r.point_blocks == npt
    a, b = res[1], res[2]
    assert len(a.history) == len(b.history) and np.array_equal(a.history[:, 3], b.history[:, 3])
    assert np.max(np.abs(a.history[:, 2] - b.history[:, 2]) / np.abs(a.history[:, 2])) <= 1e-9


@pytest.mark.parametrize("schur", [1, 2])
@pytest.mark.parametrize("nc", [455, 456])
def test_lm_linear_solve_at_the_trsv_boundary(nc, schur, gctx):
    """The first damped solve on 455 and 456 cameras x 700 points, 8 cameras a point (5600 factors): the residual of the
    damped normal equations (J^T J + mu I) dp + grad, formed without a matrix on the CPU as in
    test_lm_full_ladybug_properties, within that test's 1e-9 |grad|.
    455 cameras: M = 4095, Mp = 4096 = TRSV_MAX -- the last size k_trsv takes (`D.Mp <= TRSV_MAX`), zs[4096] full.
    456 cameras: M = 4104, Mp = 4160 -- the first size of k_trsv_left, which no other test runs.
    Both: 65 tiles, so SK = 2048 / 2145 = 0 clamped to 1 and k_syrk's grid is 4225 x 1; two or three of the
    cameras have 1 to 3 factors (the fewest: 1): k_cam with fewer rows than one MFMA step of four.
    Observed on an MI355X, |res| / |grad|: 455 cameras (mu 511.968) dense 2.02e-15, sparse 1.99e-15; 456 cameras
    (mu 286.447) dense 1.72e-15, sparse 1.72e-15.  With one row block left out of k_trsv_left's sums, or the second
    stride out of k_trsv's loop, the cases of that kernel fail."""
    pp = P.make_synthetic_ba(1, nc, 700, obs_per_pt=8, first_comp=11)
    pp.lo[:], pp.hi[:] = -np.inf, np.inf                          # (the final clamp is not part of the linear step)
    assert 1 <= np.min(np.bincount(pp.cam_vid0 // 9, minlength=nc)) < 4    # a camera of fewer rows than one MFMA step
    r1 = capi.Problem(gctx, pp).lm_optimize(maxiters=1, model=1, schur=schur)
    assert r1.camera_blocks == nc and r1.point_blocks == 700
    assert r1.history[-1, 3] == 1
    mu = r1.history[-1, 0]                                        # the damping of the accepted solve
    o = O.OracleProblem(pp, emulate_stale_cache=False)
    grad = o.gradient()
    dp = r1.x - pp.x0
    E, G = o.eval_each(np.arange(pp.nfac)), o.grad_each_ba(np.arange(pp.nfac))
    Jd = np.zeros(pp.nvars)
    vids = np.concatenate([pp.cam_vid0[:, None] + np.arange(9), pp.pt_vid0[:, None] + np.arange(3)], axis=1)
    rows = G / np.sqrt(2.0 * E)[:, None]
    np.add.at(Jd, vids.reshape(-1), (rows * np.sum(rows * dp[vids], axis=1)[:, None]).reshape(-1))
    res = Jd + mu * dp + grad
    print("LM %d cameras (Mp %d, %s), schur %d: mu %.6g, |res| / |grad| = %.2e" % (
        nc, (9 * nc + 63) // 64 * 64, "k_trsv" if nc == 455 else "k_trsv_left", schur, mu, np.linalg.norm(res) / np.linalg.norm(grad)))
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(grad)


@pytest.mark.parametrize("model", [1, 2])
def test_lm_sub_block_at_64_cameras(model, gctx):
    """test_lm_sub_block_with_constants beyond 512 unknowns: of 64 cameras x 400 points (6 cameras a point) all cameras
    but two and the first 200 points are free, the factors of those points listed, and of one free camera's listed
    factors all but one dropped.  62 active cameras: M = 558, Mp = 576 (k_trsv's strided loop, 18 padding rows), active
    blocks numbered differently from the problem's (cam_id / fci skip the constant cameras; the listed factors of the
    constant cameras have fci = -1, so k_z stops after T_j and k_back skips them), and k_cam on a camera of a single
    Jacobian row (model 1) or two (model 2).
    Observed on an MI355X, largest deviation from the oracle (history, x, fret):
    model 1  8.5e-11, 2.1e-13, 7.3e-11 (11 solves, 3 rejected);  model 2  4.4e-12, 5.8e-13, 4.5e-13 (10 solves, 2 rejected);
    the oracle's own sensitivity to one-ulp changes of the start here: 3.7e-11, 8.2e-14, 3.6e-11 and 9.4e-12, 5.1e-13, 2.8e-13."""
    nc, npt = 64, 400
    pp = P.make_synthetic_ba(1, nc, npt, obs_per_pt=6, first_comp=7)
    const_cams, lone = (5, 40), 17
    free = np.concatenate([np.setdiff1d(np.arange(9 * nc), np.concatenate([9 * c + np.arange(9) for c in const_cams])),
                           9 * nc + np.arange(3 * (npt // 2))]).astype(np.int64)
    fac = np.where(pp.pt_vid0 < 9 * nc + 3 * (npt // 2))[0].astype(np.int64)
    of_lone = fac[pp.cam_vid0[fac] == 9 * lone]
    assert len(of_lone) > 1
    fac = np.setdiff1d(fac, of_lone[1:])                          # camera `lone` keeps exactly one listed factor
    assert np.sum(pp.cam_vid0[fac] == 9 * lone) == 1
    g = capi.Problem(gctx, pp)
    r = g.lm_optimize(free, fac, maxiters=8, model=model)
    ro = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), free, fac, maxiters=8, model=model)
    print("LM sub-block of 64 cameras, model %d against the oracle: history %.1e, x %.1e, fret %.1e (%d of %d solves compared)" % (
        (model,) + _deviations(r, ro) + (_converged_at(ro), len(ro.history))))
    _compare(r, ro)
    assert r.camera_blocks == nc - 2 and r.point_blocks == npt // 2
    x_all = g.get_x()
    rest = np.setdiff1d(np.arange(pp.nvars), free)
    assert np.array_equal(x_all[rest], pp.x0[rest]) and np.array_equal(x_all[free], r.x)   # constants untouched, block left assigned


def test_lm_argument_errors(gctx):
    q = P.load_poly()
    with pytest.raises(capi.RdisHipError):
        capi.Problem(gctx, q).lm_optimize()
    pp = P.load_bal(ncams=5, npts=30)
    with pytest.raises(capi.RdisHipError):
        capi.Problem(gctx, pp).lm_optimize(np.array([0, 99999]), None)


@pytest.mark.parametrize("model", [1, 2])
def test_sparse_and_dense_schur_products_agree(model, gctx):
    """The Schur product Z Z^T formed two ways -- dense on the matrix cores (a rank-3P update that multiplies mostly
    zeros on a BAL problem) and block-sparse over the camera pairs that share a point -- against the dense oracle step
    by step, and against each other: same decisions, values to rounding.  On full ladybug the default (by fill) is
    the sparse one, and a damped solve is cheaper for it."""
    import time
    pp = P.load_bal(ncams=49, npts=300)
    ro = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), maxiters=10, model=model)
    res = {}
    for schur in (1, 2):
        res[schur] = capi.Problem(gctx, pp).lm_optimize(maxiters=10, model=model, schur=schur)
        _compare(res[schur], ro)
    a, b = res[1], res[2]
    assert len(a.history) == len(b.history) and np.array_equal(a.history[:, 3], b.history[:, 3])
    assert np.max(np.abs(a.history[:, 2] - b.history[:, 2]) / np.abs(a.history[:, 2])) <= 1e-9
    assert abs(a.fret - b.fret) <= 1e-9 * abs(a.fret) and np.max(np.abs(a.x - b.x)) <= 1e-8 * (1.0 + np.max(np.abs(a.x)))
    # a sub-block with constants, cameras only, both ways
    free = np.concatenate([np.arange(0, 6), np.arange(27, 36), np.arange(441, 471)]).astype(np.int64)
    fac = np.where(pp.pt_vid0 < 471)[0].astype(np.int64)
    rs = [capi.Problem(gctx, pp).lm_optimize(free, fac, maxiters=8, model=model, schur=s) for s in (1, 2)]
    assert abs(rs[0].fret - rs[1].fret) <= 1e-9 * abs(rs[0].fret) and np.array_equal(rs[0].history[:, 3], rs[1].history[:, 3])
    # full ladybug: time per call
    full = P.load_bal()
    g = capi.Problem(gctx, full)
    ms = {}
    for schur in (1, 2, 0):
        g.set_x(full.x0)
        g.lm_optimize(maxiters=3, model=model, schur=schur)
        best = float("inf")
        for _ in range(3):      # (best of three: a wall clock on a shared host; one slow call must not fail a correctness suite)
            g.set_x(full.x0)
            t = time.perf_counter()
            r = g.lm_optimize(maxiters=25, model=model, schur=schur)
            gctx.synchronize()
            best = min(best, (time.perf_counter() - t) * 1e3)
        ms[schur] = (best, r.fret, r.nsolve)
    print("LM model %d, full ladybug, 25 iterations: dense Schur %.1f ms, sparse %.1f ms, by fill %.1f ms (%d damped solves); end values %.8g / %.8g" % (
        model, ms[1][0], ms[2][0], ms[0][0], ms[0][2], ms[1][1], ms[2][1]))
    assert abs(ms[1][1] - ms[2][1]) <= 1e-6 * abs(ms[1][1]) and ms[0][1] == ms[2][1]      # by fill = sparse here, bit for bit
    assert ms[2][0] < 1.25 * ms[1][0]
