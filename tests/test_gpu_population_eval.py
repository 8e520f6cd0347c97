"""The population's evaluation with the member as a grid dimension, and the selection of the best member on the device
(rdis_hip_population_eval / _eval_device / _best / _assign_best / _set_option / _get_info).

f[s] must be, bit for bit, what Problem.eval(fac) returns on a fresh Problem whose assigned x is member s's row, whatever the
branch (rotation records / per factor / two-pass) and however the members are split into launches; best() must be the
sequential scan of select_best_start_kernel restated in numpy; assign_best() must leave the problem as assign(best) does.
Every value is compared with ==, every x with .tobytes().  Nothing is timed."""
import dataclasses
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval", "x")


def members_5_30(pp):
    rng = np.random.default_rng(7)
    return np.stack([pp.x0, pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)), pp.x0 * (1 + 1e-2 * rng.standard_normal(pp.nvars))])


def scan(f):
    """select_best_start_kernel's rule as its sequential scan"""
    b = 0
    for s in range(1, len(f)):
        if f[s] < f[b] or (f[b] != f[b] and f[s] == f[s]):
            b = s
    return b


def fresh_evals(gctx, pp, X, lists):
    """want[s][k] = Problem.eval(lists[k]) on a fresh problem with X[s] assigned"""
    want = []
    for x in X:
        h = capi.Problem(gctx, pp)
        h.set_x(x)
        want.append([h.eval(fac) for fac in lists])
        h.close()
    return want


def same_value(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.fixture(scope="module")
def small():
    return P.load_bal(ncams=5, npts=30)


@pytest.fixture(scope="module")
def full():
    return P.load_bal()


def _sinusoid_from_the_committed_start():
    pp = P.make_high_dim_sinusoid()
    with open(os.path.join(os.path.dirname(__file__), "golden", "sinusoid_start.json")) as fh:
        pp.x0 = np.array(json.load(fh)["x0"])
    return pp


def test_5_30_every_branch(gctx, small):
    """three members of ladybug 5 / 30: all factors (records branch), 12 listed factors (per factor: 12 < 4 x 5), 40 with
    duplicates (records branch) -- == Problem.eval on a fresh problem, == the oracle's restatement for member 1, and the same bytes
    member by member (eval_batched = 0)"""
    pp = small
    rng = np.random.default_rng(17)
    X = members_5_30(pp)
    twelve = rng.choice(pp.nfac, size=12, replace=False).astype(np.int64)
    forty = rng.integers(0, pp.nfac, size=40).astype(np.int64)
    forty[1] = forty[0]
    assert pp.nfac >= 4 * 5 and len(np.unique(forty)) < 40
    lists = [None, twelve, forty]
    want = fresh_evals(gctx, pp, X, lists)
    g = capi.Problem(gctx, pp)
    x_before, f_before = g.get_x(), g.eval()
    pop = capi.Population(g, x=X)
    o = O.OracleProblem.device_eval(dataclasses.replace(pp, x0=X[1].copy()))
    o.assign(None, X[1])
    for k, fac in enumerate(lists):
        pop.set_option("eval_batched", 1)
        f = pop.eval(fac)
        assert f.shape == (3,) and f.dtype == np.float64
        print("list", k, "batched", f.tolist(), "fresh", [want[s][k] for s in range(3)])
        for s in range(3):
            assert f[s] == want[s][k], (k, s, f[s], want[s][k])
        assert f[1] == o.eval_device(fac), (k, f[1], o.eval_device(fac))
        assert pop.info("eval_members_per_launch") == 3
        assert pop.info("eval_launches") == (2 if k == 1 else 3)      # (rotation records), chunk sums, final sums
        pop.set_option("eval_batched", 0)
        assert pop.eval(fac).tobytes() == f.tobytes(), k
        assert pop.info("eval_launches") == 3 * (2 if k == 1 else 3)
    assert f[0] != f[1] != f[2]
    assert g.get_x().tobytes() == x_before.tobytes() and g.eval() == f_before
    assert pop.get_x().tobytes() == X.tobytes()


def test_full_ladybug_ragged_chunks(gctx, full):
    """four members of full ladybug: all 31843 factors (62 chunks and a ragged one of 99), a permuted list of 1300 (three chunks,
    the last ragged), a list of 150 (one chunk, per-factor branch: 150 < 4 x 49) -- each == Problem.eval"""
    pp = full
    assert pp.nfac == 62 * 512 + 99
    rng = np.random.default_rng(23)
    X = np.stack([pp.x0 * (1 + e * rng.standard_normal(pp.nvars)) for e in (1e-3, 1e-2, 1e-3, 1e-2)])
    perm = rng.permutation(pp.nfac).astype(np.int64)
    lists = [None, perm[:1300].copy(), perm[2000:2150].copy()]
    want = fresh_evals(gctx, pp, X, lists)
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    for k, fac in enumerate(lists):
        f = pop.eval(fac)
        print("list", k, f.tolist())
        for s in range(4):
            assert f[s] == want[s][k], (k, s, f[s], want[s][k])
        assert len(set(f.tolist())) == 4, f
        assert pop.info("eval_launches") == (2 if k == 2 else 3) and pop.info("eval_members_per_launch") == 4


@pytest.mark.parametrize("case", ["the sinusoid", "testpoly"])
def test_nonlinear_products(gctx, case):
    """the two-pass form, three members: all factors and an explicit list with duplicates == Problem.eval, and for the sinusoid
    == the oracle's grid sum"""
    pp = _sinusoid_from_the_committed_start() if case == "the sinusoid" else P.load_poly()
    rng = np.random.default_rng(29)
    X = np.stack([pp.x0] + [np.minimum(np.maximum(pp.x0 + e * rng.standard_normal(pp.nvars), pp.lo), pp.hi) for e in (0.05, 0.37)])
    dup = rng.integers(0, pp.nfac, size=max(7, (3 * pp.nfac) // 2)).astype(np.int64)
    dup[1] = dup[0]
    lists = [None, dup]
    want = fresh_evals(gctx, pp, X, lists)
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    oracles = []
    if case == "the sinusoid":
        for s in range(3):
            oracles.append(O.OracleProblem.device_wg_default(pp.single_component()))
            oracles[s].assign(None, X[s])
    for k, fac in enumerate(lists):
        f = pop.eval(fac)
        print(case, "list", k, f.tolist())
        for s in range(3):
            assert f[s] == want[s][k], (k, s, f[s], want[s][k])
            if oracles:
                assert f[s] == oracles[s].eval_device_grid(fac), (k, s, f[s], oracles[s].eval_device_grid(fac))
        assert pop.info("eval_launches") == 2 and pop.info("eval_members_per_launch") == 3
        pop.set_option("eval_batched", 0)
        assert pop.eval(fac).tobytes() == f.tobytes()
        pop.set_option("eval_batched", 1)
    assert pop.get_x().tobytes() == X.tobytes()


def test_split_launches(gctx, full):
    """full ladybug, five members whose cameras differ: a budget of two members' scratch gives launches of 2 + 2 + 1, a budget of
    one byte five launches of one -- the rotation records rebuilt before every launch --, the bytes of f those of one launch"""
    pp = full
    rng = np.random.default_rng(31)
    ncam = int(pp.meta["ncams"])
    X = np.stack([pp.x0] * 5)
    X[:, :9 * ncam] *= 1 + 1e-3 * rng.standard_normal((5, 9 * ncam))
    per = 8 * (63 + pp.nvars)                       # 63 chunk sums and the records' replica, per member of a launch
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    whole = pop.eval()
    assert pop.info("eval_members_per_launch") == 5 and pop.info("eval_launches") == 3
    assert len(set(whole.tolist())) == 5
    for budget, R in ((2 * per + per // 2, 2), (per - 1, 1), (1, 1), (1 << 30, 5)):
        pop.set_option("eval_workspace_bytes", budget)
        f = pop.eval()
        assert pop.info("eval_members_per_launch") == R
        assert pop.info("eval_launches") == -(-5 // R) * 3
        assert f.tobytes() == whole.tobytes(), (budget, f, whole)
    # ... and a sub-list on the per-factor branch: no records in the count
    short = np.arange(150, dtype=np.int64)
    one = pop.eval(short)
    pop.set_option("eval_workspace_bytes", 2 * 8)
    assert pop.eval(short).tobytes() == one.tobytes()
    assert pop.info("eval_members_per_launch") == 2 and pop.info("eval_launches") == 3 * 2


def test_one_launch_not_one_per_member(gctx, small):
    """64 members of 5 / 30: three kernels for the whole population; member by member at least one each"""
    pp = small
    X = pp.x0 * (1 + 1e-3 * np.random.default_rng(37).standard_normal((64, pp.nvars)))
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    f = pop.eval()
    assert pop.info("eval_launches") <= 3 and pop.info("eval_members_per_launch") == 64
    pop.set_option("eval_batched", 0)
    assert pop.eval().tobytes() == f.tobytes()
    assert pop.info("eval_launches") >= 64


def test_selection(gctx, small):
    """1000 members, the minimum's row at 63, 64, 255, 256 and 700, NaN rows at 0 and 999: best() == the scan restated, member 63;
    three NaN members: (0, NaN); one member; an empty list (all +0.0: member 0); best() after a sub-list refers to it"""
    pp = small
    rng = np.random.default_rng(41)
    X = pp.x0 * (1 + 1e-3 * rng.standard_normal((1000, pp.nvars)))
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    f = pop.eval()
    m = int(np.argmin(f))
    row = X[m].copy()
    if m < 63:
        X[m] = X[int(np.argmax(f))]                 # (the minimum must not also stand below 63)
    for s in (63, 64, 255, 256, 700):
        X[s] = row
    X[0] = np.nan
    X[999] = np.nan
    pop.set_x(X)
    f = pop.eval()
    assert np.isnan(f[0]) and np.isnan(f[999]) and np.sum(np.isnan(f)) == 2
    assert f[63] == f[64] == f[255] == f[256] == f[700] == np.nanmin(f)
    b, fb = pop.best()
    print("best", b, fb, "scan", scan(f))
    assert b == scan(f) == 63 and same_value(fb, f[63])
    assert pop.best() == (b, fb)                    # (asked twice: the same)
    # a sub-list: other values, and best() refers to them
    sub = rng.choice(pp.nfac, size=25, replace=False).astype(np.int64)
    fd = pop.eval_device(sub)
    b2, fb2 = pop.best()
    fs = np.frombuffer(gctx.copy_to_host(fd, 8 * 1000), dtype=np.float64)
    assert fs.tobytes() == pop.eval(sub).tobytes() and fs.tobytes() != f.tobytes()
    assert b2 == scan(fs) and same_value(fb2, fs[b2])
    # an empty list: every value +0.0, a tie that the lowest index wins
    assert pop.eval(np.zeros(0, dtype=np.int64)).tobytes() == np.zeros(1000).tobytes()
    assert pop.best() == (0, 0.0)
    pop.close()
    # every value a NaN: member 0
    nan3 = capi.Population(g, x=np.full((3, pp.nvars), np.nan))
    assert np.all(np.isnan(nan3.eval()))
    b, fb = nan3.best()
    assert b == 0 and fb != fb
    nan3.close()
    # a NaN first, then numbers with a tie
    tie = capi.Population(g, x=np.stack([np.full(pp.nvars, np.nan), X[5], X[63], X[63], X[5]]))
    ft = tie.eval()
    assert tie.best() == (scan(ft), ft[scan(ft)]) and scan(ft) in (1, 2)
    tie.close()
    # a population of one
    one = capi.Population(g, x=X[63:64])
    f1 = one.eval()
    assert one.best() == (0, f1[0]) and f1[0] == f[63]


def test_assign_best(gctx, small):
    """assign_best(): the problem's x is the best member's, its value f[best], X untouched; set_start(None) + solve from there
    has the bytes of the sequential continuation"""
    pp = small
    cams, pts = P.ba_alternation_plans(pp)
    X = members_5_30(pp)[::-1].copy()
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    f = pop.eval()
    pop.assign_best()
    b, fb = pop.best()
    assert b == scan(f) and same_value(fb, f[b])
    assert g.get_x().tobytes() == pop.get_x(b).tobytes() == X[b].tobytes()
    assert g.eval() == f[b]
    assert pop.get_x().tobytes() == X.tobytes()
    plan = capi.Plan(g, *cams)
    plan.set_start(None)
    plan.solve(25, 3e-8)
    r = plan.fetch()
    h = capi.Problem(gctx, pp)
    h.set_x(X[b])
    seq = capi.Plan(h, *cams)
    seq.set_start(None)
    seq.solve(25, 3e-8)
    want = seq.fetch()
    for name in FIELDS:
        assert getattr(r, name).tobytes() == getattr(want, name).tobytes(), name
    assert g.get_x().tobytes() == h.get_x().tobytes()
    assert pop.get_x().tobytes() == X.tobytes()


def test_asynchronous_chain(gctx, small):
    """two rounds of (camera plan, point plan), eval_device, assign_best with nothing read in between: member, value and the
    problem's x == the route through eval() + the scan on the host + assign()"""
    pp = small
    cams, pts = P.ba_alternation_plans(pp)
    X = members_5_30(pp)

    def loop(device):
        g = capi.Problem(gctx, pp)
        pop = capi.Population(g, x=X)
        plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
        chosen = None
        for _ in range(2):
            for plan in plans:
                plan.solve_population(pop, 25, 3e-8)
            if device:
                pop.eval_device()
                pop.assign_best()
            else:
                f = pop.eval()
                chosen = (scan(f), float(f[scan(f)]))
                pop.assign(chosen[0])
        if device:
            chosen = pop.best()
        return chosen, g.get_x(), pop.get_x(), g.eval()

    (b, fb), x, rows, fx = loop(True)
    (wb, wfb), wx, wrows, wfx = loop(False)
    assert b == wb and same_value(fb, wfb), (b, fb, wb, wfb)
    assert x.tobytes() == wx.tobytes() == rows[b].tobytes() and rows.tobytes() == wrows.tobytes()
    assert fx == wfx == fb


def _refused(call, word):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), e.value


def test_staleness_and_refusals(gctx, small):
    """best / assign_best before any evaluation, after set_x and after solve_population: EINVAL, "evaluate first"; unknown option
    and info names: EINVAL; get_x, assign and evaluations do not invalidate; afterwards everything works and the problem's x
    is untouched"""
    pp = small
    cams, pts = P.ba_alternation_plans(pp)
    X = members_5_30(pp)
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    assert pop.info("eval_valid") == 0
    _refused(pop.best, "evaluate first")
    _refused(pop.assign_best, "evaluate first")
    f = pop.eval()
    assert pop.info("eval_valid") == 1
    b = pop.best()
    pop.get_x()
    pop.eval_device()
    assert pop.info("eval_valid") == 1 and pop.best() == b
    pop.set_x(X[1:2], first=1, count=1)
    assert pop.info("eval_valid") == 0
    _refused(pop.best, "evaluate first")
    _refused(pop.assign_best, "evaluate first")
    assert pop.eval().tobytes() == f.tobytes() and pop.best() == b
    plan = capi.Plan(g, *cams)
    plan.solve_population(pop, 25, 3e-8)
    assert pop.info("eval_valid") == 0
    _refused(pop.best, "evaluate first")
    _refused(pop.assign_best, "evaluate first")
    _refused(lambda: pop.set_option("eval_everything", 1), "unknown")
    _refused(lambda: pop.info("eval_everything"), "unknown")
    _refused(lambda: pop.set_option("eval_workspace_bytes", -1), "eval_workspace_bytes")
    assert g.get_x().tobytes() == pp.x0.tobytes()              # no refused call, and no evaluation, wrote the problem's x
    f2 = pop.eval()
    assert pop.info("eval_valid") == 1
    b2, fb2 = pop.best()
    assert b2 == scan(f2) and same_value(fb2, f2[b2]) and f2.tobytes() != f.tobytes()
    assert g.get_x().tobytes() == pp.x0.tobytes()
    pop.assign(0)                                   # (does not invalidate)
    assert pop.best() == (b2, fb2)
    pop.assign_best()
    assert g.get_x().tobytes() == pop.get_x(b2).tobytes()
