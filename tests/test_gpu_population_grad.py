"""The members' values and gradients with the member as a grid dimension (rdis_hip_population_eval_grad / _eval_grad_device /
_grad_max, the option grad_workspace_bytes, the info names grad_members_per_launch / grad_launches / grad_branch).

Row k of (f, g) must be, bit for bit, what Problem.eval_grad(fac) returns on a FRESH Problem whose assigned x is member
first + k's row, whatever the branch (fused / short / two-pass) and however the members are split into rounds; a gradient call
writes neither the population's X and values nor the problem.  Everything is compared with == / .tobytes().  Nothing is timed."""
import dataclasses
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FUSED, SHORT, TWO_PASS = 1, 2, 3


def members_5_30(pp):
    """(tests/test_gpu_population_eval.py: members_5_30, restated)"""
    rng = np.random.default_rng(7)
    return np.stack([pp.x0, pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)), pp.x0 * (1 + 1e-2 * rng.standard_normal(pp.nvars))])


def scan(f):
    """select_best_start_kernel's rule as its sequential scan"""
    b = 0
    for s in range(1, len(f)):
        if f[s] < f[b] or (f[b] != f[b] and f[s] == f[s]):
            b = s
    return b


def fresh_grads(gctx, pp, X, lists):
    """want[s][k] = Problem.eval_grad(lists[k]) on a fresh problem with X[s] assigned"""
    want = []
    for x in X:
        h = capi.Problem(gctx, pp)
        h.set_x(x)
        want.append([h.eval_grad(fac) for fac in lists])
        h.close()
    return want


def check_rows(f, g, want, k, first=0):
    """rows of (f, g) against want[first + row][k]: the value ==, the gradient the same bytes"""
    assert f.dtype == np.float64 and g.dtype == np.float64 and g.shape[0] == f.shape[0]
    for r in range(f.shape[0]):
        wf, wg = want[first + r][k]
        assert f[r] == wf, (k, first + r, f[r], wf)
        assert g[r].tobytes() == wg.tobytes(), (k, first + r, float(np.max(np.abs(g[r] - wg))))


@pytest.fixture(scope="module")
def small():
    return P.load_bal(ncams=5, npts=30)


@pytest.fixture(scope="module")
def full():
    return P.load_bal()


def small_lists(pp):
    rng = np.random.default_rng(17)
    twelve = rng.choice(pp.nfac, size=12, replace=False).astype(np.int64)
    forty = rng.integers(0, pp.nfac, size=40).astype(np.int64)
    forty[1] = forty[0]
    assert len(np.unique(twelve)) == 12 and len(np.unique(forty)) < 40 and pp.nfac <= 512
    return [None, twelve, forty]


@pytest.fixture(scope="module")
def small5(gctx, small):
    """ladybug 5 / 30 grown to five members, the lists of case 1 and the fresh problems' (f, g) of every (member, list): computed
    once, read only"""
    pp = small
    rng = np.random.default_rng(43)
    X = np.concatenate([members_5_30(pp), pp.x0 * (1 + 3e-3 * rng.standard_normal((2, pp.nvars)))])
    lists = small_lists(pp)
    return X, lists, fresh_grads(gctx, pp, X, lists)


def _sinusoid_from_the_committed_start():
    pp = P.make_high_dim_sinusoid()
    with open(os.path.join(os.path.dirname(__file__), "golden", "sinusoid_start.json")) as fh:
        pp.x0 = np.array(json.load(fh)["x0"])
    return pp


def test_5_30_every_branch(gctx, small, small5):
    """three members of ladybug 5 / 30: all factors (fused, one ragged chunk), 12 distinct listed factors and 40 with a duplicate
    (short) -- == Problem.eval_grad on fresh problems, == the oracle's restatement for member 1, exact zeros where the fresh
    gradient has them; the problem's x and own eval_grad keep their bytes; best() after eval() + eval_grad() still answers"""
    pp = small
    X5, lists, want = small5
    X = X5[:3]
    g = capi.Problem(gctx, pp)
    x_before = g.get_x()
    own_before = [g.eval_grad(fac) for fac in lists]
    pop = capi.Population(g, x=X)
    o = O.OracleProblem.device_eval(dataclasses.replace(pp, x0=X[1].copy()))
    o.assign(None, X[1])
    # all factors stand in one ragged chunk and one tile, so no block is staged: the combine kernel has items only where a
    # variable is read by no factor (its entry is set to zero there)
    read = np.zeros(pp.nvars, dtype=bool)
    read[(pp.cam_vid0[:, None] + np.arange(9)[None, :]).ravel()] = True
    read[(pp.pt_vid0[:, None] + np.arange(3)[None, :]).ravel()] = True
    assert 0 < pp.nfac < 512
    for k, fac in enumerate(lists):
        f, gr = pop.eval_grad(fac)
        assert f.shape == (3,) and gr.shape == (3, pp.nvars)
        print("list", k, "batched", f.tolist(), "fresh", [want[s][k][0] for s in range(3)])
        check_rows(f, gr, want, k)
        fo, go = o.eval_grad_device(fac)
        assert f[1] == fo and (gr[1].tobytes() == go.tobytes() or np.array_equal(gr[1], go)), (k, f[1], fo)
        for s in range(3):
            zero = want[s][k][1] == 0.0
            assert np.all(gr[s][zero] == 0.0) and (k == 0 or zero.any())
        assert pop.info("grad_branch") == (FUSED, SHORT, SHORT)[k]
        assert pop.info("grad_members_per_launch") == 3
        if k == 0:
            assert pop.info("grad_launches") == (3 if read.all() else 4)   # records, fused pass, (combine when it has items), final sums
            assert len({f[0], f[1], f[2]}) == 3
        else:
            assert pop.info("grad_launches") == 4           # partials, gather, the one chunk's value, final sums
    assert g.get_x().tobytes() == x_before.tobytes()
    for (bf, bg), fac in zip(own_before, lists):
        af, ag = g.eval_grad(fac)
        assert af == bf and ag.tobytes() == bg.tobytes()
    assert pop.get_x().tobytes() == X.tobytes()
    # the gradient call leaves the evaluation and its best member alone
    fe = pop.eval()
    pop.eval_grad(lists[1])
    assert pop.info("eval_valid") == 1
    b, fb = pop.best()
    assert b == scan(fe) and fb == fe[b]


def test_full_ladybug(gctx, full):
    """four members of full ladybug: all 31843 factors (62 chunks and a ragged one of 99), a permuted 1300 (staged blocks: the
    combine kernel runs), camera-major order, arange(513), 512 scattered (short), one factor -- each == the fresh problems"""
    pp = full
    assert pp.nfac == 62 * 512 + 99
    rng = np.random.default_rng(23)
    X = np.stack([pp.x0 * (1 + e * rng.standard_normal(pp.nvars)) for e in (1e-3, 1e-2, 1e-3, 1e-2)])
    X = np.minimum(np.maximum(X, pp.lo), pp.hi)
    perm = rng.permutation(pp.nfac).astype(np.int64)
    lists = [None, perm[:1300].copy(), np.argsort(pp.cam_vid0, kind="stable").astype(np.int64), np.arange(513, dtype=np.int64),
             perm[3000:3512].copy(), np.array([31842], dtype=np.int64)]
    want = fresh_grads(gctx, pp, X, lists)
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    for k, fac in enumerate(lists):
        f, gr = pop.eval_grad(fac)
        print("list", k, f.tolist(), "launches", pop.info("grad_launches"))
        check_rows(f, gr, want, k)
        assert len(set(f.tolist())) == 4, f
        for a in range(4):
            for b in range(a + 1, 4):
                assert gr[a].tobytes() != gr[b].tobytes()
        assert pop.info("grad_branch") == (SHORT if k >= 4 else FUSED) and pop.info("grad_members_per_launch") == 4
        assert pop.info("grad_launches") == 4               # (fused: blocks are staged across chunks and tiles, the combine kernel runs)
    assert pop.get_x().tobytes() == X.tobytes()


def test_more_cameras_than_a_chunk_holds(gctx):
    """96 cameras in a camera-scattered order, two members: every chunk meets more than 56 distinct cameras (the cur.extra path of
    the fused kernel); the whole list and its first 5000 == the fresh problems"""
    pp = P.make_synthetic_ba(1, 96, 6000, obs_per_pt=4)
    rng = np.random.default_rng(17)
    scattered = rng.permutation(pp.nfac).astype(np.int64)
    assert len(np.unique(pp.cam_vid0[scattered[:512]])) > 56
    X = np.stack([pp.x0, np.minimum(np.maximum(pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)), pp.lo), pp.hi)])
    lists = [scattered, scattered[:5000].copy()]
    want = fresh_grads(gctx, pp, X, lists)
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    for k, fac in enumerate(lists):
        f, gr = pop.eval_grad(fac)
        check_rows(f, gr, want, k)
        assert pop.info("grad_branch") == FUSED and f[0] != f[1]


def nonlinear_case(case):
    """(tests/test_gpu_population_eval.py: test_nonlinear_products' members and lists, restated)"""
    pp = _sinusoid_from_the_committed_start() if case == "the sinusoid" else P.load_poly()
    rng = np.random.default_rng(29)
    X = np.stack([pp.x0] + [np.minimum(np.maximum(pp.x0 + e * rng.standard_normal(pp.nvars), pp.lo), pp.hi) for e in (0.05, 0.37)])
    dup = rng.integers(0, pp.nfac, size=max(7, (3 * pp.nfac) // 2)).astype(np.int64)
    dup[1] = dup[0]
    return pp, X, [None, dup]


@pytest.mark.parametrize("case", ["the sinusoid", "testpoly"])
def test_nonlinear_products(gctx, case):
    """the two-pass form, three members: all factors and an explicit list with duplicates == the fresh problems; all factors of
    member 1 == the oracle's gradient with the device's arithmetic; grad_max == the maximum taken on the host"""
    pp, X, lists = nonlinear_case(case)
    want = fresh_grads(gctx, pp, X, lists)
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    for k, fac in enumerate(lists):
        f, gr = pop.eval_grad(fac)
        print(case, "list", k, f.tolist())
        check_rows(f, gr, want, k)
        assert pop.info("grad_branch") == TWO_PASS and pop.info("grad_launches") == 3 and pop.info("grad_members_per_launch") == 3
        assert pop.grad_max().tobytes() == np.max(np.abs(gr), axis=1).tobytes()
        if fac is None:
            o = O.OracleProblem.device_wg_default(pp.single_component())
            o.assign(None, X[1])
            assert np.array_equal(gr[1], o.gradient()), float(np.max(np.abs(gr[1] - o.gradient())))
    assert pop.get_x().tobytes() == X.tobytes()


def test_splitting_and_ranges(gctx, small, small5):
    """five members of 5 / 30: a budget of two and a half members' bytes gives rounds of 2 + 2 + 1, one byte one replica for all
    five in turn (the camera records rebuilt before every round) -- the bytes of the unsplit call; a member range gives the
    whole call's rows; count = 0 gives empty arrays; ranges outside the population are refused"""
    pp = small
    X, lists, want = small5
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    for k, fac in enumerate(lists):
        whole_f, whole_g = pop.eval_grad(fac)
        assert pop.info("grad_members_per_launch") == 5
        per_round = pop.info("grad_launches")
        check_rows(whole_f, whole_g, want, k)
        # a member's bytes by the rule of population_grid.hpp: no staged block on the one chunk of 5 / 30; twelve partials a factor
        per = 8 * (14 * 5 + 9 + 3 + 1) if fac is None else 8 * (12 * pp.nfac + 1)
        for budget, R in ((2 * per + per // 2, 2), (1, 1), (per - 1, 1), (1 << 30, 5)):
            pop.set_option("grad_workspace_bytes", budget)
            f, gr = pop.eval_grad(fac)
            assert pop.info("grad_members_per_launch") == R, (k, budget)
            assert pop.info("grad_launches") == -(-5 // R) * per_round
            assert f.tobytes() == whole_f.tobytes() and gr.tobytes() == whole_g.tobytes(), (k, budget)
        f, gr = pop.eval_grad(fac, first=1, count=2)
        assert f.tobytes() == whole_f[1:3].tobytes() and gr.tobytes() == whole_g[1:3].tobytes()
        assert pop.grad_max().tobytes() == np.max(np.abs(whole_g[1:3]), axis=1).tobytes()
        f, gr = pop.eval_grad(fac, first=4)
        assert f.tobytes() == whole_f[4:].tobytes() and gr.tobytes() == whole_g[4:].tobytes()
    f, gr = pop.eval_grad(first=2, count=0)
    assert f.shape == (0,) and gr.shape == (0, pp.nvars)
    assert pop.grad_max().shape == (1,)                    # (count = 0 did nothing: still the call before it)
    for first, count in ((0, 6), (5, 1), (-1, 2), (3, -1), (6, 0)):
        with pytest.raises(capi.RdisHipError, match="out of range") as e:
            pop.eval_grad(first=first, count=count)
        assert e.value.code == -1
    assert pop.get_x().tobytes() == X.tobytes()


def test_the_device_form(gctx, small, small5):
    """eval_grad_device's buffers hold the host form's bytes; a chain solve -> eval_grad_device -> eval_device -> assign_best with
    nothing waited for gives the bytes of the same steps with a synchronisation after each"""
    pp = small
    X5, lists, want = small5
    X = X5[:3]
    cams, pts = P.ba_alternation_plans(pp)
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    for fac in lists:
        f, gr = pop.eval_grad(fac)
        fd, gd = pop.eval_grad_device(fac)
        assert gctx.copy_to_host(fd, 8 * 3) == f.tobytes() and gctx.copy_to_host(gd, 8 * 3 * pp.nvars) == gr.tobytes()

    def chain(waits):
        h = capi.Problem(gctx, pp)
        p2 = capi.Population(h, x=X)
        plan = capi.Plan(h, *cams)
        if waits:
            plan.solve_population(p2, 25, 3e-8)
            plan.fetch_population()
            f, gr = p2.eval_grad()
            fe = p2.eval()
            p2.assign_best()
            h.get_x()
        else:
            p2.eval_grad_device()                          # (the list's tables are built at its first use: not part of the chain)
            plan.solve_population(p2, 25, 3e-8)
            fd, gd = p2.eval_grad_device()
            ed = p2.eval_device()
            p2.assign_best()
            f = np.frombuffer(gctx.copy_to_host(fd, 8 * 3), dtype=np.float64)
            gr = np.frombuffer(gctx.copy_to_host(gd, 8 * 3 * pp.nvars), dtype=np.float64).reshape(3, -1)
            fe = np.frombuffer(gctx.copy_to_host(ed, 8 * 3), dtype=np.float64)
        return f.tobytes(), gr.tobytes(), fe.tobytes(), h.get_x().tobytes(), p2.get_x().tobytes(), p2.best()

    a, b = chain(False), chain(True)
    assert a == b
    assert a[0] == a[2]                                    # (all factors: the gradient call's value is the evaluation's)


def test_grad_max(gctx, small, small5):
    """grad_max == max |g| per row; a member with a NaN variable that a listed factor reads has a NaN maximum, the other rows keep
    theirs; a later set_x does not change it; before any gradient call it is refused"""
    pp = small
    X5, lists, want = small5
    X = X5[:3].copy()
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    with pytest.raises(capi.RdisHipError, match="evaluate the gradient first") as e:
        pop.grad_max()
    assert e.value.code == -1
    for fac in lists:
        f, gr = pop.eval_grad(fac)
        m = pop.grad_max()
        assert m.shape == (3,) and m.tobytes() == np.max(np.abs(gr), axis=1).tobytes()
    twelve = lists[1]
    Xn = X.copy()
    Xn[1, pp.pt_vid0[twelve[0]] + 1] = np.nan              # a point coordinate that the list's first factor reads
    pop.set_x(Xn)
    assert m.tobytes() == pop.grad_max().tobytes()         # (the rows of the last gradient call, not of X as it is now)
    for fac in (None, twelve):
        f, gr = pop.eval_grad(fac)
        m = pop.grad_max()
        assert np.isnan(m[1]) and np.isnan(gr[1]).any() and not np.isnan(gr[[0, 2]]).any()
        assert m[[0, 2]].tobytes() == np.max(np.abs(gr[[0, 2]]), axis=1).tobytes()


def test_refusals_and_the_empty_list(gctx, small):
    """a list with an exponential factor is refused with eval_grad's message, a clean sub-list accepted and == the fresh problem;
    an empty list gives zeros without a kernel; unknown option / info names are refused and the message names the new ones"""
    s = _sinusoid_from_the_committed_start()
    rng = np.random.default_rng(3)
    flags = (rng.random(s.nfac) < 0.4).astype(np.uint8)
    X = np.stack([s.x0, np.minimum(np.maximum(s.x0 + 0.05 * rng.standard_normal(s.nvars), s.lo), s.hi)])
    g = capi.Problem(gctx, s)
    g.set_exponential(flags)
    pop = capi.Population(g, x=X)
    with pytest.raises(capi.RdisHipError, match="eval_grad: factor .* is exponential") as e:
        pop.eval_grad()
    assert e.value.code == -1
    with pytest.raises(capi.RdisHipError, match="exponential"):
        g.eval_grad()
    clean = np.flatnonzero(flags == 0).astype(np.int64)
    f, gr = pop.eval_grad(clean)
    for r in range(2):
        h = capi.Problem(gctx, s)
        h.set_exponential(flags)
        h.set_x(X[r])
        wf, wg = h.eval_grad(clean)
        assert f[r] == wf and gr[r].tobytes() == wg.tobytes()
        h.close()
    f, gr = pop.eval_grad(np.zeros(0, dtype=np.int64))
    assert f.tobytes() == np.zeros(2).tobytes() and gr.tobytes() == np.zeros((2, s.nvars)).tobytes()
    assert pop.info("grad_branch") == 0 and pop.info("grad_launches") == 0
    assert pop.grad_max().tobytes() == np.zeros(2).tobytes()
    with pytest.raises(capi.RdisHipError, match="requires nf == factor count"):
        pop.ctx.check(pop.ctx.lib.rdis_hip_population_eval_grad(pop.h, 0, 2, 3, None, capi._ptr(f), capi._ptr(gr)))
    with pytest.raises(capi.RdisHipError, match="unknown option.*grad_workspace_bytes"):
        pop.set_option("grad_everything", 1)
    with pytest.raises(capi.RdisHipError, match="unknown name.*grad_members_per_launch.*grad_launches.*grad_branch"):
        pop.info("grad_everything")
    with pytest.raises(capi.RdisHipError, match="grad_workspace_bytes must not be negative"):
        pop.set_option("grad_workspace_bytes", -1)
    # existing names and defaults as before
    assert pop.info("eval_valid") == 0
    pop.set_option("eval_workspace_bytes", 1 << 30)
    pop.set_option("eval_batched", 1)
