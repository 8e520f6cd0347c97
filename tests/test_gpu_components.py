"""Connected components of the residual factor graph on the device (rdis_hip_components, the
step before the solver: Component::createChildren) against the CPU oracle.  Index work: exact."""
import numpy as np
import pytest

import component_graphs as G
from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu


def _same(dev, orc):
    return all(np.array_equal(a, b) for a, b in zip(dev, orc))


@pytest.mark.parametrize("case", ["cameras_fixed", "points_fixed", "46_cameras", "random20", "random60", "random95", "none", "all"])
def test_ladybug_components_equal_oracle(case, gctx):
    pp = P.load_bal()
    rng = np.random.default_rng(17)
    a = np.zeros(pp.nvars, np.uint8)
    if case == "cameras_fixed": a[:441] = 1
    elif case == "points_fixed": a[441:] = 1
    elif case == "46_cameras": a[:9 * 46] = 1            # the separator PaToH found
    elif case.startswith("random"): a[rng.random(pp.nvars) < int(case[6:]) / 100.0] = 1
    elif case == "all": a[:] = 1
    dev = capi.Problem(gctx, pp).components(a)
    orc = O.OracleProblem(pp).components(a)
    assert _same(dev, orc)
    cams, pts = P.ba_alternation_plans(pp)
    if case == "cameras_fixed": assert _same(dev, pts)   # the classic alternation: 7776 point components
    if case == "points_fixed": assert _same(dev, cams)
    if case == "none": assert len(dev[0]) == 2 and dev[0][1] == pp.nvars and dev[2][1] == pp.nfac
    if case == "all": assert len(dev[0]) == 1 and len(dev[1]) == 0 and len(dev[3]) == 0
    if case == "46_cameras":
        # three cameras and every point they see form one component; all other points are alone
        sizes = np.diff(dev[0])
        assert sizes[-1] > 27 and np.all(sizes[:-1] == 3) and (sizes[-1] - 27) % 3 == 0


def test_synthetic_decomposition_is_recovered(gctx):
    pp = P.make_synthetic_ba(300, 3, 40)
    g = capi.Problem(gctx, pp)
    dev = g.components(np.zeros(pp.nvars, np.uint8))
    assert _same(dev, O.OracleProblem(pp).components(np.zeros(pp.nvars, np.uint8)))
    assert len(dev[0]) - 1 == 300 and np.all(np.diff(dev[0]) == 147)
    # the generator's own decomposition, component by component (equal sizes: ordered by smallest id)
    assert np.array_equal(dev[1], pp.comp_free_vid) and np.array_equal(dev[3], pp.comp_fac_id)


def test_nonlinear_products_and_isolated_variables(gctx):
    rng = np.random.default_rng(3)
    pp = P.make_high_dim_sinusoid()
    for frac in (0.0, 0.3, 0.8):
        a = (rng.random(pp.nvars) < frac).astype(np.uint8)
        assert _same(capi.Problem(gctx, pp).components(a), O.OracleProblem(pp).components(a))
    terms = [(2.0, [(0, 1.0, 0.0, 0), (1, 1.0, 0.0, 0)]), (1.0, [(3, 2.0, 0.0, 0)]), (-7.0, [])]
    q = P._pack_nlp(terms, np.zeros(4), np.full(4, -5.0), np.full(4, 5.0), {})
    dev = capi.Problem(gctx, q).components(np.zeros(4, np.uint8))
    assert list(dev[0]) == [0, 1, 2, 4] and list(dev[1]) == [2, 3, 0, 1] and list(dev[2]) == [0, 0, 1, 2] and list(dev[3]) == [1, 0]


def test_components_feed_the_solver(gctx):
    """labelling -> plan -> one launch: the same result as the hand-built alternation plan, bit for bit"""
    pp = P.load_bal(ncams=49, npts=500)
    g = capi.Problem(gctx, pp)
    a = np.zeros(pp.nvars, np.uint8); a[:441] = 1
    comps = g.components(a)
    r1 = _solve(g, pp, comps)
    r2 = _solve(g, pp, P.ba_alternation_plans(pp)[1])
    assert np.array_equal(r1.fret, r2.fret) and np.array_equal(r1.x, r2.x) and np.array_equal(r1.iters, r2.iters)
    # a mixed separator: components of very different sizes in one plan (isolated-variable components included)
    rng = np.random.default_rng(1)
    a = (rng.random(pp.nvars) < 0.5).astype(np.uint8)
    comps = g.components(a)
    r = _solve(g, pp, comps)
    assert np.all(r.delta <= 0) and np.all((r.status & 0xFF) != 5)
    empty = np.diff(comps[2]) == 0
    assert np.all((r.status[empty] & 0xFF) == 6) and np.all(r.fret[empty] == 0.0)   # empty factor list => 0 (.cpp:26-29)


def _solve(g, pp, comps):
    g.set_x(pp.x0)
    plan = capi.Plan(g, *comps)
    plan.set_start(None)
    plan.solve(25, 3e-8)
    return plan.fetch()


# ---------------------------------------------------------------------------------------------------
# Graphs and sizes the problems above never form (tests/component_graphs.py): the answer is known from
# the construction, and tests/test_components_cpu.py pins it against the oracle without a device.
#
# components.hip caps every launch at 4096 blocks of 256 lanes, 1 048 576 work items, and strides beyond:
# ladybug has 23 769 variables.  The large cases are the smallest that make each loop take a second pass
# (1 048 833 = the cap + 257, no multiple of 256) in each orientation -- variables, factors, components --
# and the sorts and copies that go with them.
# ---------------------------------------------------------------------------------------------------

SMALL, LARGE = G.small_cases(), G.large_cases()
_uploaded = {}


def _problem(gctx, pp):
    """cases that share a problem follow each other in LARGE: one upload serves them (and the labelling's workspace
    and result are reused across their masks, as a level driver reuses them)"""
    if "pp" not in _uploaded or not G.same_problem(_uploaded["pp"], pp):
        _uploaded.clear()
        _uploaded.update(pp=pp, prob=capi.Problem(gctx, pp))
    return _uploaded["prob"]


@pytest.mark.parametrize("name", list(SMALL))
def test_constructed_graphs_small(name, gctx):
    pp, a, exp = SMALL[name]()
    dev = capi.Problem(gctx, pp).components(a)
    G.check_lists(pp, a, dev)
    assert G.same(dev, exp)
    assert G.same(dev, O.OracleProblem(pp).components(a))


@pytest.mark.parametrize("name", list(LARGE))
def test_constructed_graphs_past_the_capped_grid(name, gctx):
    """N, F, max(N, F) in both orientations and the number of components beyond one pass of the grid-stride loops; a star
    whose hub every union meets and a merge tree 18 levels deep at a size that fills the device.  (expected == oracle at
    these sizes: test_components_cpu.py)"""
    pp, a, exp = LARGE[name]()
    dev = _problem(gctx, pp).components(a)
    G.check_lists(pp, a, dev)
    assert G.same(dev, exp)


@pytest.mark.parametrize("name", ["star300000-last", "merge18"])
def test_labelling_does_not_depend_on_the_schedule(name, gctx):
    """the promise of the lock-free union-find -- smallest id is the root whatever lane wins -- on the two graphs where
    every union contends: three labellings of one problem, the same four arrays each time"""
    pp, a, exp = LARGE[name]()
    g = _problem(gctx, pp)
    for _ in range(3):
        assert G.same(g.components(a), exp)


@pytest.mark.parametrize("name", ["chain4097-s0", "rows-edge-s0", "grid64x48-s0", "ba7x500x3-none"])
def test_mask_sequence_on_one_problem(name, gctx):
    """the workspace and the last result live in the problem: all assigned (the early return without components) ->
    none -> a random half -> all assigned -> the random half again"""
    pp, _, _ = SMALL[name]()
    g, orc = capi.Problem(gctx, pp), O.OracleProblem(pp)
    rng = np.random.default_rng(23)
    every, none = np.ones(pp.nvars, np.uint8), np.zeros(pp.nvars, np.uint8)
    half = (rng.random(pp.nvars) < 0.5).astype(np.uint8)
    seen = []
    for a in (every, none, half, every, half):
        dev = g.components(a)
        G.check_lists(pp, a, dev)
        assert G.same(dev, orc.components(a))
        seen.append(dev)
    assert len(seen[0][0]) == 1 and len(seen[0][1]) == 0 and len(seen[0][3]) == 0 and G.same(seen[0], seen[3])
    assert G.same(seen[2], seen[4])
    if name == "chain4097-s0":
        assert G.same(seen[1], G.chain(4097, 0, 0)[2])


def test_fetch_before_compute_and_null_mask_are_refused(gctx):
    pp, a, exp = SMALL["chain4097-cut64-s0"]()
    g = capi.Problem(gctx, pp)
    lib = gctx.lib
    out = [np.full(pp.nvars + 1, -7, np.int64) for _ in range(4)]
    ptrs = [o.ctypes.data_as(capi.C.c_void_p) for o in out]
    assert lib.rdis_hip_components_fetch(g.h, *ptrs) == -1                 # RDIS_HIP_EINVAL: nothing computed yet
    assert all(np.all(o == -7) for o in out)
    sizes = np.full(3, -7, np.int64)
    sp = [capi.C.c_void_p(sizes.ctypes.data + 8 * i) for i in range(3)]
    assert lib.rdis_hip_components(g.h, None, *sp) == -1                   # RDIS_HIP_EINVAL: assigned is null
    assert np.all(sizes == -7)
    assert lib.rdis_hip_components_fetch(g.h, *ptrs) == -1                 # ... and the refusal computed nothing
    assert G.same(g.components(a), exp)                                    # the problem is none the worse for it
    assert lib.rdis_hip_components(g.h, None, *sp) == -1
    assert G.same(g.components(a), exp)


def test_variables_without_any_factor(gctx):
    """N > 0, F = 0: N singleton components in id order, every factor list empty"""
    pp, a, exp = G.rows(dict(nvars=777), 6)
    assert pp.nfac == 0
    dev = capi.Problem(gctx, pp).components(a)
    assert np.array_equal(dev[0], np.arange(778)) and np.array_equal(dev[1], np.arange(777))
    assert np.array_equal(dev[2], np.zeros(778, np.int64)) and len(dev[3]) == 0 and G.same(dev, exp)


def test_constructed_lists_feed_the_solver(gctx):
    """a labelling that is not bundle adjustment -> plan -> solve: the device's lists and the lists known from the
    sinusoid's tree give the same plan, bit for bit"""
    pp = P.make_high_dim_sinusoid()
    rng = np.random.default_rng(29)
    pp.x0 = rng.uniform(-3.0, 3.0, pp.nvars)
    a = (rng.random(pp.nvars) < 0.35).astype(np.uint8)
    exp = G.sinusoid_expected(pp, a)
    g = capi.Problem(gctx, pp)
    dev = g.components(a)
    G.check_lists(pp, a, dev)
    assert G.same(dev, exp) and G.same(dev, O.OracleProblem(pp).components(a)) and len(dev[0]) - 1 > 10
    r1, r2 = _solve5(g, pp, dev), _solve5(g, pp, exp)
    for f in ("x", "fret", "delta", "iters", "status", "nfeval", "ngeval"):
        assert np.array_equal(getattr(r1, f), getattr(r2, f)), f
    assert np.all(r1.delta <= 0) and np.any(r1.delta < 0)


def _solve5(g, pp, comps):
    g.set_x(pp.x0)
    plan = capi.Plan(g, *comps)
    plan.set_start(None)
    plan.solve(5, 3e-8)
    return plan.fetch()
