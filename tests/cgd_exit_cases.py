"""The exits of the CGD minimiser (rdis_amd/csrc/minimizer.hpp: EXIT_*) as cases shared by tests/test_cgd_exits_cpu.py (the
reference-order oracle and every device-order restatement reach the stated exit) and tests/test_gpu_cgd_exits.py (every solver
kind and every many-solve entry against them).  A case: a problem, the free variables and the factor list of ONE component, its
start, the iteration limit, ftol, the exit code it must reach and whether the result is rolled back.

Every case is cut from make_synthetic_ba(1, 3, 8, obs_per_pt=3): 3 cameras, 8 points, 24 factors, 51 variables.

    name           how it is built                                                              exit
    flat           lo = hi = x0 for every free variable: every trial of every line returns      0, iters 0
                   the same value (Brent's fu <= fx branch every time, the Predictor's guess
                   "comes back worse" wrong every time)
    blocked        for every variable the bound on the side -gradient points to is closed       0, iters 0
                   (lo = x0 where g > 0, hi = x0 where g < 0): non-degenerate domains, the
                   first line still cannot leave the start
    exact          noise_px = 0, x0 = the truth: finit is exactly 0 in the reference's order    0, iters 0
                   (the device's arithmetic sees 3e-27 and descends a little first)
    one-factor     one point free, its first factor listed: three unknowns, two residuals       1
    three-factors  one point free, its three factors listed                                     0
    ordinary       the block as generated: the iteration limit in the LDS-resident solver's     0 or 3: the
                   order of sums, ftol after 6 to 11 iterations in the others -- no edge        restatement's
    maxiters-1     the same with maxiters = 1                                                   3, iters 0
    ftol-1         the same with ftol = 1.0                                                     0
    nan            a point and its camera's translation at the origin (0 / 0 in the             5, rolled back
                   projection): the start of test_batch_solvers_with_active_bounds_..._rollback
    empty          a point's variables, no factor                                               6
    gg-zero        ONE nonlinear-product factor 1e-170 x from x = 1e200 with ftol = -1: the     2, iters 0
                   gradient's square underflows to 0 while |x| keeps the gradient test at 1

(A coordinate of 1e200 is no NaN case: the reference-order oracle ends with code 5 on it, the device-order ones run to the
iteration limit -- an overflow that is an infinity in one association and a NaN in another.)

Exits without a bundle-adjustment case:
    2 (gg == 0)      unreachable for ftol >= 0 (test_cgd_exits_cpu.py::test_a_zero_gradient_start_leaves_by_ftol_not_by_gg): gg is the
                     sum of squares of the PREVIOUS gradient, zero only after a line along a zero direction; that line is flat and
                     the ftol test fires first.  For ftol < 0 the point has not moved either, and the gradient test comes first --
                     unless the squares underflow while max|g_j| max(|x_j|, 1) stays above 1e-8: the gg-zero case
    4 (Brent's 100)  unreached by the inputs tried: see CODE_4_SEARCH below and test_cgd_exits_cpu.py::test_code_4_search
    7 (exchange)     never provoked: the tests assert that it does not occur
ROLLED_BACK without a NaN: unreachable without the stale factor cache (with it fa is evaluated again and may differ from fp in
the last places, so the chain below has a gap of that size) -- every line search starts from fa = fp (the value
the previous line ended on, same point, same bits), mnbrak keeps fb <= fa through every swap and shift, Brent's x only ever
moves to a trial with fu <= fx, so fret = fx <= fp at every line's end and fret <= finit by induction; a NaN breaks the chain
(every comparison with it is false) and is caught by saw_nan instead."""
import collections
import functools

import numpy as np

from oracle import oracle as O
from rdis_amd import problems as P

from test_gpu_dispatch_fuzz import _concat

Case = collections.namedtuple("Case", "name pp free fac x maxiters ftol code rolled")
ROLLED_BACK = 0x100
NC, NP, K = 3, 8, 3               # cameras, points, observations per point of a block
NV, NF = 9 * NC + 3 * NP, NP * K


def _i(a):
    return np.asarray(a, dtype=np.int64)


def block(first_comp=0, noise_px=0.5):
    return P.make_synthetic_ba(1, NC, NP, obs_per_pt=K, first_comp=first_comp, noise_px=noise_px)


def clamp(pp, v, x):
    return np.minimum(np.maximum(np.asarray(x, dtype=np.float64), pp.lo[v]), pp.hi[v])


def _whole(pp):
    return np.arange(pp.nvars, dtype=np.int64), np.arange(pp.nfac, dtype=np.int64)


def _point(pp, q):
    """point q's three variables and its factors (cameras constant)"""
    v0 = 9 * NC + 3 * q
    return v0 + np.arange(3, dtype=np.int64), _i(np.nonzero(pp.pt_vid0 == v0)[0])


def flat(pp):
    pp.lo, pp.hi = pp.x0.copy(), pp.x0.copy()
    return pp


def blocked(pp):
    g = O.OracleProblem(pp, emulate_stale_cache=False).gradient()
    assert np.all(g != 0.0)
    pp.lo, pp.hi = np.where(g > 0, pp.x0, pp.lo), np.where(g < 0, pp.x0, pp.hi)
    return pp


def exact(first_comp=0):
    pp = block(first_comp, noise_px=0.0)
    pp.x0 = np.array(pp.meta["x_true"], dtype=np.float64)
    assert np.all(pp.x0 >= pp.lo) and np.all(pp.x0 <= pp.hi)
    return pp


def nan_start(pp, fac=None):
    """the first listed factor's point and its camera's translation at the origin, inside widened domains"""
    f0 = 0 if fac is None else int(fac[0])
    cam, pt = int(pp.cam_vid0[f0]), int(pp.pt_vid0[f0])
    for s in (slice(pt, pt + 3), slice(cam + 3, cam + 6)):
        pp.x0[s] = 0.0
        pp.lo[s], pp.hi[s] = np.minimum(pp.lo[s], -1.0), np.maximum(pp.hi[s], 1.0)
    return pp


NAMES = ["flat", "blocked", "exact", "one-factor", "three-factors", "ordinary", "maxiters-1", "ftol-1", "nan", "empty"]   # bundle adjustment
EXPECT = {"flat": (0, False), "blocked": (0, False), "exact": (0, False), "one-factor": (1, False), "three-factors": (0, False),
          "ordinary": (None, False), "gg-zero": (2, False), "maxiters-1": (3, False), "ftol-1": (0, False), "nan": (5, True), "empty": (6, False)}
ITERS = {"flat": 0, "blocked": 0, "exact": 0, "one-factor": 3, "three-factors": 5, "maxiters-1": 0, "ftol-1": 2, "gg-zero": 0}   # (every order of sums)


def gg_zero():
    return P._pack_nlp([(1e-170, [(0, 1.0, 0.0, 0)])], np.array([1e200]), np.array([-1e300]), np.array([1e300]), {})


def _cut(name, first_comp=0):
    """(block, free, fac) of a case"""
    if name == "exact":
        pp = exact(first_comp)
        return (pp,) + _whole(pp)
    pp = block(first_comp)
    if name == "flat":
        return (flat(pp),) + _whole(pp)
    if name == "blocked":
        return (blocked(pp),) + _whole(pp)
    if name == "one-factor":
        free, fac = _point(pp, 0)
        return pp, free, fac[:1]
    if name == "three-factors":
        return (pp,) + _point(pp, 0)
    if name == "nan":
        return (nan_start(pp),) + _whole(pp)
    if name == "room":
        x0 = pp.x0.copy()
        nan_start(pp).x0[:] = x0
        return (pp,) + _whole(pp)
    if name == "empty":
        return pp, _point(pp, 0)[0], np.zeros(0, np.int64)
    if name == "gg-zero":
        pp = gg_zero()
        return (pp,) + _whole(pp)
    return (pp,) + _whole(pp)


@functools.lru_cache(maxsize=None)
def case(name):
    pp, free, fac = _cut(name)
    code, rolled = EXPECT[name]
    ftol = {"ftol-1": 1.0, "gg-zero": -1.0}.get(name, 3e-8)
    return Case(name, pp, free, fac, pp.x0[free].copy(), 1 if name == "maxiters-1" else 25, ftol, code, rolled)


# ---- every case side by side in one problem -------------------------------------------------------------------------------------
# (maxiters and ftol belong to a solve, not to a component: the combined plan is solved three times, and `ordinary` stands for
# maxiters-1 and ftol-1 in the second and the third)
COMBINED = ["ordinary", "flat", "blocked", "exact", "one-factor", "three-factors", "ordinary", "nan", "empty"]
ORDINARY = (0, 6)                 # the two ordinary components (blocks of first_comp 0 and 6)
SOLVES = [(25, 3e-8), (1, 3e-8), (25, 1.0)]

Combined = collections.namedtuple("Combined", "pp comps names csr x_true")   # x_true: the blocks' truths, complete


def _csr(comps):
    fp = np.cumsum([0] + [len(v) for v, _ in comps]).astype(np.int64)
    cp = np.cumsum([0] + [len(f) for _, f in comps]).astype(np.int64)
    return fp, _i(np.concatenate([v for v, _ in comps])), cp, _i(np.concatenate([f for _, f in comps]))


@functools.lru_cache(maxsize=None)
def combined(spec=tuple((n, i) for i, n in enumerate(COMBINED))):
    """the cases (name, first_comp of its block) as independent components of ONE problem"""
    cuts = [_cut(n, first_comp=i) for n, i in spec]
    pp, voff, foff = _concat([c[0] for c in cuts])
    comps = [(voff[i] + c[1], foff[i] + c[2]) for i, c in enumerate(cuts)]
    return Combined(pp, comps, [n for n, _ in spec], _csr(comps), np.concatenate([c[0].meta["x_true"] for c in cuts]))


def without_empty():
    """(the LDS-resident solver's two options take no plan with a component for the plain solver, which an empty one is)"""
    return combined(tuple((n, i) for i, n in enumerate(COMBINED) if n != "empty"))


def plain_pair():
    """the two ordinary components alone: the bits they must also return beside the edge cases"""
    return combined(tuple(("ordinary", i) for i in ORDINARY))


def expected(name, maxiters, ftol):
    """(code, rolled back) of a component of the combined problem in the solve (maxiters, ftol); code None: whatever the
    solver's own restatement reaches (the == comparison carries it)"""
    if (maxiters, ftol) == SOLVES[0]:
        return EXPECT[name]
    if name == "ordinary":
        return (3 if maxiters == 1 else 0), False
    if name in ("one-factor", "three-factors"):
        return None, False
    return EXPECT[name]


@functools.lru_cache(maxsize=None)
def tiny():
    """every point of a block against its constant cameras (three free variables each: the tiny-component solver's shape).  Point 3
    sits in the plane of camera 0 -- that camera gets the rotation 0 (first-order branch: P = X + t exactly), the point z = -t_z,
    so P_z is an exact zero: the value is an infinity, the gradient is not a number (code 5) -- and lists that one factor; the
    others list their factors of cameras 1 and 2, but point 1, which keeps a single factor (code 1), and point 2 has
    lo = hi = x0 (flat)"""
    pp = block(20)
    comps, names = [], []
    for q in range(NP):
        free, fac = _point(pp, q)
        cam0 = pp.cam_vid0[fac] == 0
        name = {1: "one-factor", 2: "flat", 3: "nan"}.get(q, "two-factors")
        fac = fac[cam0] if q == 3 else fac[~cam0][:1] if q == 1 else fac[~cam0]
        if q == 2:
            pp.lo[free], pp.hi[free] = pp.x0[free].copy(), pp.x0[free].copy()
        if q == 3:
            pp.x0[0:3] = 0.0
            pp.x0[free[2]] = -pp.x0[5]
            pp.hi[free[2]] = max(pp.hi[free[2]], pp.x0[free[2]] + 1.0)
        comps.append((free, fac)); names.append(name)
    return Combined(pp, comps, names, _csr(comps), np.array(pp.meta["x_true"]))


TINY_EXPECT = {"one-factor": (1, False), "flat": (0, False), "nan": (5, True), "two-factors": (0, False)}


# ---- the many-solve entries: rows (starts, members) of one plan -------------------------------------------------------------------
MANY = ["ordinary", "flat", "blocked", "room", "three-factors", "room", "ordinary", "empty"]


def many():
    """-> (the combined problem, rows [3, nvars], the index of the NaN row).  Rows: the ordinary start, the truth, and a NaN
    start -- x0 with, in every `room` component (an ordinary block whose domains also hold the origin for point 0 and its
    camera's translation), that point and translation at the origin.  The flat and blocked domains hold for every row: a
    row's start is clamped into them."""
    cb = combined(tuple((n, i) for i, n in enumerate(MANY)))
    rows = np.stack([cb.pp.x0, cb.x_true, cb.pp.x0])
    const = np.setdiff1d(np.arange(cb.pp.nvars), cb.csr[1])
    rows[:, const] = cb.pp.x0[const]     # (solve_starts reads the constants from the problem's x: the same in every row)
    for (v, f), n in zip(cb.comps, cb.names):
        if n == "room":
            cam, pt = int(cb.pp.cam_vid0[f[0]]), int(cb.pp.pt_vid0[f[0]])
            rows[2, pt:pt + 3] = 0.0
            rows[2, cam + 3:cam + 6] = 0.0
    return cb, rows, 2


# ---- the contract of CGDSubspaceOptimizer::optimize -------------------------------------------------------------------------------
class Problems(list):
    """assertions gathered over the components of a solve, so that one run names every case that fails"""

    def check(self, ok, *what):
        if not ok:
            self.append(what)


def value_floor(pp, f):
    """The least error two correct fp64 evaluations of the listed factors can differ by where the values themselves vanish: a
    factor's value is r_x^2 + r_y^2, r = projection - observation, and the projection (some thirty operations on numbers of the
    observation's size) carries at least delta = 32 eps max(|o_x|, |o_y|, 1): the value an error of delta^2 per residual.  Only a
    component whose start AND end values are rounding noise (the `exact` case: 1e-27, where the reference-order and the
    device-order oracle themselves part by 3e-27) is below it, and check_contract applies it to that case alone: every other
    component keeps 1e-12 of the sum of the values."""
    if pp.kind != P.KIND_BA:
        return 0.0
    d = 32.0 * np.finfo(np.float64).eps * np.maximum(np.abs(pp.obs[f]).max(axis=1), 1.0)
    return float(2.0 * np.sum(d * d))


def check_contract(pp, comps, r, x_after, names=None, x_start=None):
    """r: a BatchResult over comps (x in the components' order); x_after: the problem's complete x after the solve; x_start: the
    complete x the solve started from (None: pp.x0).  -> Problems"""
    bad = Problems()
    x_start = np.asarray(pp.x0 if x_start is None else x_start, dtype=np.float64)
    fv = np.concatenate([v for v, _ in comps])
    const = np.setdiff1d(np.arange(pp.nvars), fv)
    bad.check(not np.any((r.status & 0xFF) == 7), "an exchange gave up", r.status)
    bad.check(np.all(r.delta <= 0.0), "delta <= 0", r.delta)
    bad.check(np.all(r.x >= pp.lo[fv]) and np.all(r.x <= pp.hi[fv]), "x inside the domains")
    bad.check(np.array_equal(x_after[fv], r.x, equal_nan=True), "the variables are left assigned to r.x")
    bad.check(x_after[const].tobytes() == x_start[const].tobytes(), "constants untouched")
    o = O.OracleProblem(pp, emulate_stale_cache=False)
    o.assign(None, x_start)
    e0 = o.eval_each()
    o.assign(None, np.ascontiguousarray(x_after))
    e1 = o.eval_each()
    off = 0
    for c, (v, f) in enumerate(comps):
        xc = r.x[off:off + len(v)]
        off += len(v)
        name = None if names is None else names[c]
        start = clamp(pp, v, x_start[v])
        code, rolled = int(r.status[c]) & 0xFF, bool(int(r.status[c]) & ROLLED_BACK)
        if rolled:
            bad.check(xc.tobytes() == start.tobytes() and r.delta[c] == 0.0, c, name, "restored: the clamped start, delta 0", r.delta[c])
        if len(f) == 0:
            bad.check(code == 6 and r.fret[c] == 0.0 and r.delta[c] == 0.0 and xc.tobytes() == start.tobytes(), c, name, "empty", code)
            continue
        bad.check(code != 6, c, name, "code 6 with factors")
        if name in ("flat", "blocked"):
            bad.check(xc.tobytes() == start.tobytes() and int(r.iters[c]) == 0 and not rolled and code == 0, c, name, "stays at the clamped start", code, int(r.iters[c]))
        if code == 5:
            bad.check(rolled, c, name, "code 5 without the roll-back")
            continue                                # (the value of a start that is not a number: nothing to compare)
        scale = float(np.sum(np.abs(e0[f]) + np.abs(e1[f])))
        tol = max(1e-12 * scale, value_floor(pp, f)) if name == "exact" else 1e-12 * scale
        f1, f0 = float(np.sum(e1[f])), float(np.sum(e0[f]))
        bad.check(abs(r.fret[c] - f1) <= tol, c, name, "fret is the oracle's objective at the returned point", r.fret[c], f1, tol)
        bad.check(abs(r.delta[c] - (f1 - f0)) <= tol, c, name, "delta is the descent from the start", r.delta[c], f1 - f0, tol)
    return bad


# ---- the search for exit 4 (Brent's own iteration limit, nrc :403) -----------------------------------------------------------------
# f, df, start: what oracle.frprmn was run on (ftol 3e-8 and 0.0, 200 iterations).  Brent halves its bracket at least every other
# trial, so a line needs a bracket 2^50 times its tolerance 3e-8 |x| + 2e-19 and a slope that never lets a secant step be taken.
CODE_4_SEARCH = [
    ("x^4 from 1", lambda x: x[0] ** 4, lambda x: [4 * x[0] ** 3], [1.0]),
    ("x^6 from 1", lambda x: x[0] ** 6, lambda x: [6 * x[0] ** 5], [1.0]),
    ("x^4 + y^4 from (1, 2)", lambda x: x[0] ** 4 + x[1] ** 4, lambda x: [4 * x[0] ** 3, 4 * x[1] ** 3], [1.0, 2.0]),
    ("(xy)^4 from (1, 2)", lambda x: (x[0] * x[1]) ** 4, lambda x: [4 * x[0] ** 3 * x[1] ** 4, 4 * x[0] ** 4 * x[1] ** 3], [1.0, 2.0]),
    ("|x| from 1e-3", lambda x: abs(x[0]), lambda x: [np.sign(x[0])], [1e-3]),
    ("|x| from 1e8", lambda x: abs(x[0]), lambda x: [np.sign(x[0])], [1e8]),
    ("|x|^1.5 from 1", lambda x: abs(x[0]) ** 1.5, lambda x: [1.5 * np.sign(x[0]) * abs(x[0]) ** 0.5], [1.0]),
    ("|x| + |y| from (1, 1e-9)", lambda x: abs(x[0]) + abs(x[1]), lambda x: [np.sign(x[0]), np.sign(x[1])], [1.0, 1e-9]),
    ("a step at 1e-9: f = x^2 + [x > 1e-9]", lambda x: x[0] ** 2 + (x[0] > 1e-9), lambda x: [2 * x[0]], [1.0]),
    ("value and slope that disagree: f = x^2, df = -1", lambda x: x[0] ** 2, lambda x: [-1.0], [1.0]),
    ("slope of the wrong sign: f = x^2, df = -2x", lambda x: x[0] ** 2, lambda x: [-2 * x[0]], [1.0]),
    ("exp(-x) from 0", lambda x: float(np.exp(-x[0])), lambda x: [-float(np.exp(-x[0]))], [0.0]),
    ("1e-300 x^2 from 1e150", lambda x: 1e-300 * x[0] ** 2, lambda x: [2e-300 * x[0]], [1e150]),
]
