"""Every exit of the CGD minimiser on the CPU: the reference-order oracle and each device-order restatement (the constructors
tests/test_gpu_parity.py compares the solvers with) reach the exit tests/cgd_exit_cases.py states for every case they can take.
Until now the restatements were pinned at one exit, the iteration limit (test_gpu_parity.py: `want.iters == 24 and
want.status == 3`)."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import problems as P

import cgd_exit_cases as X

# a restatement and the cases it cannot take (the tiny-component solver: at most four free variables; the others' topologies
# are built from a non-empty factor list)
MAKERS = {
    "reference order": (lambda pp, v, f: O.OracleProblem(pp, emulate_stale_cache=False), lambda c: True),
    "reference order, stale cache": (lambda pp, v, f: O.OracleProblem(pp), lambda c: True),
    "device_parity": (lambda pp, v, f: O.OracleProblem.device_parity(pp), lambda c: True),
    "device_parity, no cache": (lambda pp, v, f: O.OracleProblem.device_parity(pp, emulate_stale_cache=False), lambda c: True),
    "device_default": (lambda pp, v, f: O.OracleProblem.device_default(pp, v, f), lambda c: len(c.fac) > 0),
    "device_lds_default": (lambda pp, v, f: O.OracleProblem.device_lds_default(pp, v, f), lambda c: len(c.fac) > 0),
    "device_ptm_default": (lambda pp, v, f: O.OracleProblem.device_ptm_default(pp, fac=f), lambda c: len(c.fac) > 0),
    "device_ptm_default, group of 2": (lambda pp, v, f: O.OracleProblem.device_ptm_default(pp, fac=f, threads=256, group=2), lambda c: len(c.fac) > 0),
    "device_group_default, 4 lanes": (lambda pp, v, f: O.OracleProblem.device_group_default(pp, 4), lambda c: len(c.free) <= 4),
    "device_group_default, 16 lanes": (lambda pp, v, f: O.OracleProblem.device_group_default(pp, 16), lambda c: len(c.free) <= 4),
    "device_wg_default": (lambda pp, v, f: O.OracleProblem.device_wg_default(pp, v, f), lambda c: True),
    "device_wg_default, grid of 1": (lambda pp, v, f: O.OracleProblem.device_wg_default(pp, v, f, grid_workgroups=1), lambda c: len(c.fac) > 0),
}


def _run(make, c):
    return make(c.pp, c.free, c.fac).cgd(c.free, c.fac, x=c.x, maxiters=c.maxiters, ftol=c.ftol)


# the ordinary block has no edge: where it ends depends on the order of the sums, and is that order's own -- (code, iters)
ORDINARY = {"device_lds_default": (3, 24), "device_ptm_default": (0, 11), "device_ptm_default, group of 2": (0, 11),
            "device_wg_default": (0, 6), "device_wg_default, grid of 1": (0, 6)}      # every other restatement: (0, 8)
TAKEN = [(name, maker) for name in X.NAMES for maker in MAKERS if MAKERS[maker][1](X.case(name))]


@pytest.mark.parametrize("name, maker", TAKEN)
def test_every_restatement_reaches_the_stated_exit(name, maker):
    c = X.case(name)
    make = MAKERS[maker][0]
    r = _run(make, c)
    code, rolled = r.status & 0xFF, bool(r.status & X.ROLLED_BACK)
    if c.code is not None:
        assert (code, rolled) == (c.code, c.rolled), (code, rolled, r.iters)
    else:
        assert (code, r.iters) == ORDINARY.get(maker, (0, 8)) and not rolled
    if name in X.ITERS:
        assert r.iters == X.ITERS[name]
    start = X.clamp(c.pp, c.free, c.x)
    assert np.all(r.x >= c.pp.lo[c.free]) and np.all(r.x <= c.pp.hi[c.free])
    if rolled or name in ("flat", "blocked", "empty"):
        assert r.x.tobytes() == start.tobytes() and r.delta == 0.0
    if name in ("flat", "blocked"):
        # 30 f / 26 df calls: f(x0), Frprmn's own, the bracket's three, Brent's first and its 24 equal-valued trials (every one
        # taken, fu <= fx, until the bracket closes on the tolerance); df: Frprmn's, Brent's first and one per trial
        assert (r.nfeval, r.ngeval) == (30, 26) and r.fret == r.finit
    if name == "exact" and maker.startswith("reference order"):
        assert r.finit == 0.0 and r.fret == 0.0
    if name == "nan":
        assert math.isnan(r.fret) and math.isnan(r.finit)
    elif name != "empty":
        assert r.delta <= 0.0 and r.delta == r.fret - r.finit


def test_the_nonlinear_product_restatement_on_a_flat_line():
    """load_poly() with lo = hi = x0 on the plain solver's restatement: the same 30 / 26 as bundle adjustment"""
    pp = P.load_poly()
    pp.lo, pp.hi = pp.x0.copy(), pp.x0.copy()
    for o in (O.OracleProblem(pp, emulate_stale_cache=False), O.OracleProblem.device_wg_default(pp)):
        r = o.cgd(x=pp.x0, maxiters=25)
        assert (r.status, r.iters, r.nfeval, r.ngeval, r.delta) == (0, 0, 30, 26, 0.0) and r.x.tobytes() == pp.x0.tobytes()


def test_a_zero_gradient_start_leaves_by_ftol_not_by_gg():
    """Exit 2 (gg == 0).  gg is the sum of squares of the PREVIOUS gradient (oracle/rdis_oracle.c frprmn_ex: gg += g[j] * g[j];
    minimizer.hpp S_REDUCED takes it from the same reduction, after the ftol test of line_done() and the gradient test).  It is
    zero only after a line along a zero direction; every trial of that line is the same point, so the line is flat and the ftol
    test 2 |fx - fp| <= ftol (|fx| + |fp| + 1e-18) fires for every ftol >= 0.  For ftol < 0 the point still has not moved: the new
    gradient is the old one, zero, and test < GTOL comes first.  What is left is underflow: a gradient whose squares vanish while
    max |g_j| max(|x_j|, 1) / max(|f|, 1) stays above GTOL -- cgd_exit_cases.gg_zero, ftol < 0 only."""
    z = P._pack_nlp([(1.0, [(0, 2.0, 0.0, 0)])], np.array([0.0]), np.array([-5.0]), np.array([5.0]), {})     # x^2 from 0
    for make in (lambda q: O.OracleProblem(q, emulate_stale_cache=False), O.OracleProblem.device_wg_default):
        for ftol, code in ((3e-8, 0), (0.0, 0), (-1.0, 1)):
            r = make(z).cgd(x=z.x0, maxiters=25, ftol=ftol)
            assert (r.status, r.iters, r.fret, r.delta) == (code, 0, 0.0, 0.0), (ftol, r)
        c = X.case("gg-zero")
        for ftol, code in ((3e-8, 0), (0.0, 0), (-1.0, 2)):
            r = make(c.pp).cgd(x=c.x, maxiters=25, ftol=ftol)
            assert (r.status, r.iters, r.fret, r.delta) == (code, 0, 1e30, 0.0) and r.x[0] == 1e200, (ftol, r)
    rc, _, _, it = O.frprmn(lambda x: 0.0, lambda x: [0.0, 0.0], [1.0, 2.0])                                   # ... and on callbacks
    assert (rc, it) == (0, 0)


def test_code_4_search():
    """Exit 4 (Brent's own limit of 100 trials, nrc :403): unreached by the inputs tried -- cgd_exit_cases.CODE_4_SEARCH, each
    with ftol 3e-8 and 0 -- and by every case of this file.  (A NaN start does run Brent to its limit, every comparison false;
    the code it is reported with is 5.)  This records the search: every input ends with another code."""
    for name, f, df, x0 in X.CODE_4_SEARCH:
        for ftol in (3e-8, 0.0):
            rc, x, fret, it = O.frprmn(f, df, x0, maxiters=200, ftol=ftol)
            assert rc in (0, 1, 3), (name, ftol, rc, it)
    pp = P.load_poly()
    for x0 in ([0.0, 0.0], [8.0, -9.0], [1e-9, 1e9]):
        r = O.OracleProblem(pp, emulate_stale_cache=False).cgd(x=np.array(x0), maxiters=200, ftol=0.0)
        assert (r.status & 0xFF) in (0, 1, 3), (x0, r.status)


def test_the_tiny_components():
    """the tiny-component solver's cases (cgd_exit_cases.tiny) on its restatement, 4 and 16 lanes, and on the LDS-resident one"""
    t = X.tiny()
    for make in (lambda v, f: O.OracleProblem.device_group_default(t.pp, 4), lambda v, f: O.OracleProblem.device_group_default(t.pp, 16),
                 lambda v, f: O.OracleProblem.device_lds_default(t.pp, v, f)):
        for (v, f), name in zip(t.comps, t.names):
            r = make(v, f).cgd(v, f, x=t.pp.x0[v], maxiters=25)
            code, rolled = X.TINY_EXPECT[name]
            assert bool(r.status & X.ROLLED_BACK) == rolled and (r.status & 0xFF) == (code if code is not None else r.status & 0xFF), (name, r)
            assert (r.status & 0xFF) in (0, 1, 3, 5)
            if name in ("flat", "nan"):
                assert r.x.tobytes() == t.pp.x0[v].tobytes() and r.delta == 0.0
