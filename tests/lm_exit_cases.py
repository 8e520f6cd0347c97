"""The exits of the Levenberg-Marquardt solvers other than the iteration limit, as cases shared by
tests/test_lm_exits_cpu.py (the oracle reaches the stated exit and keeps it under one-ulp changes of the start) and
tests/test_gpu_lm_exits.py (every device entry against the oracle).  A case: a problem, a list of independent components,
the complete start x, the iteration limit, ftol, the residual model, whether the wide class is asked for, what is compared
(kind) and the stop code its components must reach.

Shapes (the smallest of each class of rdis_amd/csrc/lm_batch.hpp; lm_batch_class: no camera 0, 1 to 6 cameras 1, 7 to 16
cameras 2, 17 to 64 with the option 3):
    points, cameras, sub-block, whole   ladybug 5 / 30 as tests/lm_batch_shapes.py cuts it: classes 0, 1, 1, 1
    whole-8                             ladybug 8 / 30 whole: 8 cameras are class 2 (ladybug 5 / 30 whole has 5: class 1)
    wide                                make_synthetic_ba(1, 17, 60, obs_per_pt=6) whole with wide=True: class 3
    two-wide                            make_synthetic_ba(2, 17, 60, obs_per_pt=6), each block a component: class 3 twice
    mixed                               make_synthetic_ba(4, 17, 60, obs_per_pt=6): block 0 whole (class 3), from block 1 its cameras
                                        0..7 (class 2), its camera 8 (class 1) and single points (class 0), and a second
                                        component of each of the classes 2, 1 and 3: block 2's cameras 0..7, its camera 8, block 3 whole
Every problem lays its cameras out first except `two-wide` and `mixed`, so every component of the others also fits
rdis_hip_lm_optimize.

Kinds:
    exact       the exit is decided far from rounding: stop, iterations and counters must equal the oracle's
                  small-error  stop 6 after k >= 1 accepted steps: ftol is the geometric mean of 2 f at two successive accepted
                               points of the oracle's own run whose ratio is at least 10; only components whose every accepted
                               2 f stays a factor sqrt(10) away from that ftol are kept
                  unread       stop 1 at iteration 0: the listed factors read no free variable of the component
                  idle         a free camera block no listed factor reads beside active ones: its values come back unchanged
    converged   stop 2 (small step; 5 where rounding refuses the last steps): maxiters is at least four times the oracle's
                iteration count, so the iteration limit cannot be a matter of rounding
    zero        one-observation points, ftol 0: the minimum is 0 and the oracle's own fret there (1e-25 to 1e-31, or exactly 0
                and then stop 6) is rounding -- no reference for fret, x or the stop code; properties only
    nonfinite   a start whose objective is not finite, beside healthy components of every class (the `mixed` batch)"""
import collections
import functools
import math

import numpy as np

from oracle import lm_oracle as LM
from oracle import oracle as O
from rdis_amd import problems as P

import lm_batch_shapes as S

Case = collections.namedtuple("Case", "name pp comps x maxiters ftol model wide kind stop")
# stop: {component index: the code it must reach} (exact, nonfinite); converged / zero: every component


def _i(a):
    return np.asarray(a, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def shape(key):
    """(problem, components, wide)"""
    if key in ("points", "cameras", "sub-block", "whole"):
        pp = P.load_bal(ncams=5, npts=30)
        return pp, {"points": S._each_point(pp, 5), "cameras": S._each_camera(pp, 5), "sub-block": S._sub_block(pp), "whole": S._whole(pp)}[key], False
    if key == "whole-8":
        pp = P.load_bal(ncams=8, npts=30)
        return pp, S._whole(pp), False
    if key == "wide":
        pp = P.make_synthetic_ba(1, 17, 60, obs_per_pt=6)
        return pp, S._whole(pp), True
    if key == "two-wide":
        pp = P.make_synthetic_ba(2, 17, 60, obs_per_pt=6)
        return pp, S._synthetic_components(pp, 2), True
    if key == "mixed":
        pp = P.make_synthetic_ba(4, 17, 60, obs_per_pt=6)
        nv, nf = pp.nvars // 4, pp.nfac // 4
        blk = np.arange(pp.nfac) // nf                                              # the block of a factor
        cam, pt = (pp.cam_vid0 - blk * nv) // 9, (pp.pt_vid0 - blk * nv - 153) // 3    # its camera / point inside the block

        def whole(b):
            return b * nv + np.arange(nv, dtype=np.int64), b * nf + np.arange(nf, dtype=np.int64)

        def cameras_0_to_7(b):      # their factors of points 0..29, those points constant
            return b * nv + np.arange(72, dtype=np.int64), _i(np.where((blk == b) & (cam < 8) & (pt < 30))[0])

        def camera_8(b):
            return b * nv + 72 + np.arange(9, dtype=np.int64), _i(np.where((blk == b) & (cam == 8) & (pt < 30))[0])

        comps = [whole(0), cameras_0_to_7(1), camera_8(1)]                          # 0, 1, 2: classes 3, 2, 1 -- the ones poisoned
        for p in range(30, 60):                                                     # 3 ..: block 1's points, their factors of cameras 9..16
            fac = _i(np.where((blk == 1) & (pt == p) & (cam >= 9))[0])
            if len(fac) >= 2:
                comps.append((nv + 153 + 3 * p + np.arange(3, dtype=np.int64), fac))
        comps += [cameras_0_to_7(2), camera_8(2), whole(3)]                         # a second component of classes 2, 1 and 3
        return pp, comps, True
    raise KeyError(key)


def oracle_runs(pp, comps, x, maxiters, ftol, model):
    """lm_oracle.lm_optimize component by component from the complete state x"""
    o = O.OracleProblem(pp, emulate_stale_cache=False)
    o.assign(None, x)
    return [LM.lm_optimize(o, free, fac, x=x[free], maxiters=maxiters, ftol=ftol, model=model) for free, fac in comps]


def accepted_2f(r):
    """2 f at the start and at every accepted point of an oracle run"""
    return [2.0 * r.finit] + [2.0 * ft for _, _, ft, ok in r.history if ok]


# ---- 1. small error after k >= 1 accepted steps ---------------------------------------------------------------------------------
SMALL_ERROR = [("points", 1), ("points", 2), ("cameras", 2), ("sub-block", 2), ("whole", 1), ("whole", 2), ("whole-8", 2), ("wide", 2)]


def _small_error(key, model):
    pp, comps, wide = shape(key)
    runs = oracle_runs(pp, comps, pp.x0, 10, 3e-8, model)
    ftol = None
    for r in runs:                      # the first component with a pair of ratio >= 10: its last such pair
        s = accepted_2f(r)
        pairs = [(a, b) for a, b in zip(s, s[1:]) if a >= 10.0 * b]
        if pairs:
            ftol = math.sqrt(pairs[-1][0] * pairs[-1][1])
            break
    assert ftol is not None
    far = math.sqrt(10.0)

    def crosses(s):                     # starts above ftol, falls below it after 1 to 9 accepted steps (the test at the head of
        return s[0] > ftol and 1 <= min([i for i, v in enumerate(s) if v < ftol], default=99) <= 9    # iteration 10 never runs)

    keep = [c for c, r in enumerate(runs) if all(v >= far * ftol or far * v <= ftol for v in accepted_2f(r)) and crosses(accepted_2f(r))]
    assert keep
    return Case("small-error/%s/m%d" % (key, model), pp, [comps[c] for c in keep], pp.x0, 10, ftol, model, wide, "exact", {i: 6 for i in range(len(keep))})


# ---- 2. small gradient at iteration 0; an idle block --------------------------------------------------------------------------------
def _unread(key, model):
    if key == "points":                 # class 0: free point 0 (2), listed the factors of point 1 (3)
        pp, pts, wide = shape("points")
        comps = [(pts[0][0], pts[1][1]), (pts[2][0], pts[3][1])]
    elif key == "camera":               # class 1: free camera 0, listed the factors of camera 1
        pp, cams, wide = shape("cameras")
        comps = [(cams[0][0], cams[1][1])]
    elif key == "sub-block":            # class 1: the sub-block's free variables, listed the factors of other cameras and points
        pp, sub, wide = shape("sub-block")
        comps = [(sub[0][0], _i(np.where((pp.pt_vid0 >= 75) & (pp.cam_vid0 != 0) & (pp.cam_vid0 != 27))[0]))]
    elif key == "cameras-7-of-8":       # class 2: free cameras 0..6 of ladybug 8 / 30, listed the factors of camera 7
        pp, _, wide = shape("whole-8")
        comps = [(np.arange(63, dtype=np.int64), _i(np.where(pp.cam_vid0 == 63)[0]))]
    else:                               # class 3: free block 0 of two synthetic blocks, listed block 1's factors
        pp, blocks, wide = shape("two-wide")
        comps = [(blocks[0][0], blocks[1][1])]
    assert all(len(fac) > 0 for _, fac in comps)
    return Case("unread/%s/m%d" % (key, model), pp, comps, pp.x0, 5, 3e-8, model, wide, "exact", {i: 1 for i in range(len(comps))})


def _idle(key, model):
    """-> the case and the idle block's variable ids"""
    if key == "cameras":                # class 1: cameras 0 and 1 free, listed camera 0's factors
        pp, cams, wide = shape("cameras")
        comps, idle = [(np.arange(18, dtype=np.int64), cams[0][1])], 9 + np.arange(9)
    elif key == "whole-8":              # class 2: everything free, camera 7's factors not listed
        pp, _, wide = shape("whole-8")
        comps, idle = [(np.arange(pp.nvars, dtype=np.int64), _i(np.where(pp.cam_vid0 != 63)[0]))], 63 + np.arange(9)
    else:                               # class 3: everything free, camera 16's factors not listed
        pp, _, wide = shape("wide")
        comps, idle = [(np.arange(pp.nvars, dtype=np.int64), _i(np.where(pp.cam_vid0 != 144)[0]))], 144 + np.arange(9)
    return Case("idle/%s/m%d" % (key, model), pp, comps, pp.x0, 6, 3e-8, model, wide, "exact", {}), _i(idle)


UNREAD = [(k, m) for k in ("points", "camera", "sub-block", "cameras-7-of-8", "wide-block") for m in (1, 2)]
IDLE = [(k, m) for k in ("cameras", "whole-8", "wide") for m in (1, 2)]


# ---- 3. small step: converged runs -----------------------------------------------------------------------------------------------------
CONVERGED = ["points", "restart-points", "restart-cameras", "restart-whole", "restart-whole-8", "restart-wide", "two-observations"]
MAXITERS = 200                          # no case runs longer


def _converged(key):
    """model 2.  maxiters: four times the oracle's largest iteration count; restarts: from the x at which the oracle stopped
    with code 2 (reached with as many iterations as that takes: the oracle is not a case), the components kept that stop again
    within MAXITERS / 4 iterations"""
    if key == "points":
        pp, comps, wide = shape("points")
        x, ftol = pp.x0, 3e-8
    elif key == "two-observations":
        pp, pts, wide = shape("points")
        comps, x, ftol = [(free, fac[:2]) for free, fac in pts], pp.x0, 0.0
    else:
        pp, comps, wide = shape(key[len("restart-"):])
        x, ftol = pp.x0.copy(), 3e-8
        for _ in range(2 if key == "restart-wide" else 1):     # (the wide shape's first restart takes 51 iterations, its second 49)
            first = oracle_runs(pp, comps, x, 1000, ftol, 2)
            assert all(r.stop == 2 for r in first)
            for (free, _), r in zip(comps, first):
                x[free] = r.x
    runs = oracle_runs(pp, comps, x, MAXITERS, ftol, 2)
    keep = [c for c, r in enumerate(runs) if r.stop == 2 and 4 * r.iters <= MAXITERS]
    assert keep
    # (at least 40: a restarted point stops after 1 to 3 iterations, after up to 6 once its start moves by an ulp)
    return Case("converged/" + key, pp, [comps[c] for c in keep], x, max(40, 4 * max(runs[c].iters for c in keep)), ftol, 2, wide, "converged", {})


def _zero(model=2):
    pp, pts, wide = shape("points")
    return Case("zero/one-observation", pp, [(free, fac[:1]) for free, fac in pts], pp.x0, 100, 0.0, model, wide, "zero", {})


# ---- 4. starts whose objective is not finite ---------------------------------------------------------------------------------------------
# (variant, the poisoned component of `mixed`): a NaN coordinate in a free point (class 0, and inside the wide component), in a free
# camera (classes 1, 2, 3), and a finite start on which the objective is not: a point in the plane of a camera
NONFINITE = [("nan-point", 3), ("nan-point", 0), ("nan-camera", 2), ("nan-camera", 1), ("nan-camera", 0),
             ("plane", 3), ("plane", 2), ("plane", 1), ("plane", 0)]


def poison(pp, comp, x, variant):
    """x with component comp = (free, fac) given a start whose objective is not finite.
    nan-point / nan-camera: the second coordinate of the component's first free point / its first free camera's translation.
    plane: the camera of the component's first listed factor gets the rotation 0 (first-order branch: P = X + t exactly) and
    t_z = -X_z, or the point z = -t_z where the camera is constant: P_z is an exact zero, the projection divides by it."""
    free, fac = comp
    x = np.array(x, dtype=np.float64)
    if variant == "nan-point":
        v = int(min(pp.pt_vid0[fac][np.isin(pp.pt_vid0[fac], free)]))
        x[v + 1] = np.nan
    elif variant == "nan-camera":
        v = int(min(pp.cam_vid0[fac][np.isin(pp.cam_vid0[fac], free)]))
        x[v + 4] = np.nan
    else:
        c, q = int(pp.cam_vid0[fac[0]]), int(pp.pt_vid0[fac[0]])
        x[c:c + 3] = 0.0
        if c + 5 in free:
            x[c + 5] = -x[q + 2]
        else:
            assert q + 2 in free
            x[q + 2] = -x[c + 5]
        assert np.all(x >= pp.lo) and np.all(x <= pp.hi)
    return x


def _nonfinite(variant, target, model):
    pp, comps, wide = shape("mixed")
    return Case("nonfinite/%s/component-%d/m%d" % (variant, target, model), pp, comps, poison(pp, comps[target], pp.x0, variant), 4, 3e-8, model, wide,
                "nonfinite", {target: 7})


# the same on ladybug 5 / 30, a component at a time, for rdis_hip_lm_optimize (cameras first): (shape, component, variant)
NONFINITE_SEQUENTIAL = [("points", 4, "nan-point"), ("whole", 0, "nan-point"), ("whole", 0, "nan-camera"), ("cameras", 1, "nan-camera"),
                        ("sub-block", 0, "nan-camera"), ("points", 4, "plane"), ("cameras", 1, "plane"), ("whole-8", 0, "plane")]


def _nonfinite_sequential(key, target, variant, model):
    pp, comps, wide = shape(key)
    return Case("nonfinite-sequential/%s-%d/%s/m%d" % (key, target, variant, model), pp, [comps[target]], poison(pp, comps[target], pp.x0, variant), 4, 3e-8,
                model, wide, "nonfinite", {0: 7})


@functools.lru_cache(maxsize=None)
def case(name):
    part = name.split("/")
    if part[0] == "small-error":
        return _small_error(part[1], int(part[2][1:]))
    if part[0] == "unread":
        return _unread(part[1], int(part[2][1:]))
    if part[0] == "idle":
        return _idle(part[1], int(part[2][1:]))[0]
    if part[0] == "converged":
        return _converged(part[1])
    if part[0] == "zero":
        return _zero()
    if part[0] == "nonfinite":
        return _nonfinite(part[1], int(part[2].split("-")[1]), int(part[3][1:]))
    if part[0] == "nonfinite-sequential":
        key, target = part[1].rsplit("-", 1)
        return _nonfinite_sequential(key, int(target), part[2], int(part[3][1:]))
    raise KeyError(name)


def idle_block(name):
    part = name.split("/")
    return _idle(part[1], int(part[2][1:]))[1]


SMALL_ERROR_NAMES = ["small-error/%s/m%d" % km for km in SMALL_ERROR]
UNREAD_NAMES = ["unread/%s/m%d" % km for km in UNREAD]
IDLE_NAMES = ["idle/%s/m%d" % km for km in IDLE]
EXACT_NAMES = SMALL_ERROR_NAMES + UNREAD_NAMES + IDLE_NAMES
CONVERGED_NAMES = ["converged/" + k for k in CONVERGED]
ZERO_NAMES = ["zero/one-observation"]
NONFINITE_NAMES = ["nonfinite/%s/component-%d/m%d" % (v, t, m) for v, t in NONFINITE for m in ((1, 2) if (v, t) in (("nan-point", 3), ("nan-camera", 1)) else (2,))]
NONFINITE_SEQUENTIAL_NAMES = ["nonfinite-sequential/%s-%d/%s/m%d" % (k, t, v, m) for k, t, v in NONFINITE_SEQUENTIAL
                              for m in ((1, 2) if k == "points" else (2,))]


@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    """the oracle's runs of a case (computed once, shared, not modified)"""
    c = case(name)
    return oracle_runs(c.pp, c.comps, c.x, c.maxiters, c.ftol, c.model)


def one_ulp(c, draw):
    """the case's start with every free coordinate moved by -1, 0 or +1 ulp (relative 2^-52, as
    test_sum_gradient_and_per_factor_parity draws them), draw 0..5"""
    rng = np.random.default_rng(100 + draw)
    x = np.array(c.x, dtype=np.float64)
    for free, _ in c.comps:
        x[free] = x[free] * (1.0 + rng.choice([-1.0, 0.0, 1.0], len(free)) * 2.0 ** -52)
    return x


DRAWS = 6


@functools.lru_cache(maxsize=None)
def perturbed_reference(name, draw):
    """the oracle's runs of a case from one_ulp(case, draw) (computed once, shared, not modified)"""
    c = case(name)
    return oracle_runs(c.pp, c.comps, one_ulp(c, draw), c.maxiters, c.ftol, c.model)


@functools.lru_cache(maxsize=None)
def stable_history(name):
    """Per component of a converged case: how many leading history records the oracle itself reproduces -- the same accept /
    reject decision and mu, |Dp|^2, f(trial) within 1e-9, a hundredth of the device comparison's 1e-7 -- in all DRAWS runs
    from one-ulp changes of the start, and never more than lm_batch_shapes.converged_at.  Near a converged point the gain ratio
    is a quotient of differences of nearly equal values, and mu and every later record inherit its rounding: a restart from a
    converged x loses the 1e-9 within its first records, long before a trial value equals the current one to 1e-11."""
    ref = oracle_reference(name)
    out = []
    for k, ro in enumerate(ref):
        n = S.converged_at(ro)
        for draw in range(DRAWS):
            m = 0
            for (mu, dp, ft, ok), (omu, odp, oft, ook) in zip(perturbed_reference(name, draw)[k].history, ro.history[:n]):
                if bool(ok) != bool(ook) or max(abs(mu - omu) / omu, abs(dp - odp) / odp, abs(ft - oft) / abs(oft)) > 1e-9:
                    break
                m += 1
            n = min(n, m)
        out.append(n)
    return out


# ---- the counter identities of the loop (oracle/lm_oracle.py, k_lm_batch, device_lm_ba) ---------------------------------------------
def check_identities(r, finit=None, cap=None):
    """r: an oracle LMResult, or a device LmResult with cap the capacity its history was fetched with.  Returns nfail, the
    solves whose factorisation was refused.  A stop 7 at the start (no solve: the start's objective is not finite) is told
    from a stop 7 at a trial point (one solve and one evaluation more than history records) by nsolve.
    A history of cap records may have been cut off there: the number of records written is then taken from nfev (so that
    identity is not a check), the accepted records present may be fewer than the iterations, and everything else holds."""
    hist = [tuple(h) for h in r.history]
    trial7 = r.stop == 7 and r.nsolve > 0
    cut = cap is not None and len(hist) >= cap
    assert cap is None or len(hist) <= cap
    nh = r.nfev - 1 - trial7 if cut else len(hist)
    assert r.njev == r.iters + (r.stop == 1), (r.njev, r.iters, r.stop)
    assert r.nfev == 1 + nh + trial7 and nh >= len(hist), (r.nfev, nh, r.stop)
    accepted = sum(1 for h in hist if h[3])
    want = r.iters - (r.stop in (2, 4, 5) or trial7)
    assert accepted <= want if cut else accepted == want, (accepted, r.iters, r.stop)
    nfail = r.nsolve - nh - (r.stop in (2, 4) or trial7)
    assert nfail >= 0, (r.nsolve, nh, r.stop)
    nu = 2
    for (mu, _, _, ok), (mu_next, _, _, _) in zip(hist, hist[1:]):
        if ok:
            if nfail == 0:              # (a refused factorisation in between would multiply it further)
                assert mu / 3.0 <= mu_next <= 2.0 * mu, (mu, mu_next)   # mu * max(1 - (2 rho - 1)^3, 0.3333333334), rho > 0
            nu = 2
        else:
            # rejected: mu times nu, and once more per refused factorisation in between, nu doubling each time: exact products
            # (with refused factorisations somewhere in the run, the nu at this entry may be any later power of two)
            match = []
            for n0 in ([nu] if nfail == 0 else [nu << s for s in range(31) if nu << s < 1 << 31]):
                m, n = mu, n0
                for _ in range(nfail + 1):
                    m, n = m * n, n * 2
                    if m == mu_next:
                        match.append(n)
            assert match, (mu, mu_next, nu)
            nu = match[0]
    delta = getattr(r, "delta", None)
    if finit is not None and delta is not None and math.isfinite(finit) and math.isfinite(r.fret):
        assert abs(delta - (r.fret - finit)) <= 1e-12 * max(abs(finit), 1e-300), (delta, r.fret, finit)
    return nfail
