"""A restart loop on the device: members drawn (rdis_hip_population_set_sampling / _sample), ranked and reordered
(rdis_hip_population_sort) and a member range solved (rdis_hip_plan_solve_population_range).

A drawn value must be oracle.levels.splitmix_restart_value(seed, stream, member, variable, ...) bit for bit, whatever the
range's cut into calls; the order must be sorted() under best()'s rule restated (numbers ascending, ties by index, NaNs last)
and the rows must move with it; a range solve must leave, for its members, the bytes the whole-population entry leaves (the
parent's path is the reference) and nothing else.  Every comparison is == / .tobytes(); nothing is timed."""
import numpy as np
import pytest

from oracle.levels import splitmix_restart_value
from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("fret", "delta", "iters", "status", "nfeval", "ngeval", "x")
SEED = 0x5D15
OPTIONS = {"row_min_components": 1 << 40, "coop_min_factors": 0, "coop_group_min_factors": 0}   # (examples/ba_population.py)


def sampling_intervals(pp):
    """examples/ba_multistart.py: rotations in [-pi, pi], k1 / k2 within 1e-4 / 1e-6 and everything else within 100 of x0"""
    nc = int(pp.meta["ncams"])
    typ = np.concatenate([np.arange(9 * nc) % 9, 9 + np.arange(pp.nvars - 9 * nc) % 3])
    half = np.select([typ < 3, typ == 7, typ == 8], [np.pi, 1e-4, 1e-6], default=100.0)
    centre = np.where(typ < 3, 0.0, pp.x0)
    return centre - half, centre + half


def rule_order(f):
    return sorted(range(len(f)), key=lambda s: (f[s] != f[s], 0.0 if f[s] != f[s] else f[s], s))


def draws(pp, slo, shi, stream, members, vid=None):
    vid = range(pp.nvars) if vid is None else vid
    return np.array([[splitmix_restart_value(SEED, stream, s, int(v), slo[v], shi[v], pp.lo[v], pp.hi[v]) for v in vid] for s in members])


def set_options(plan, opts):
    for k, v in opts.items():
        plan.set_option(k, v)


def _refused(call, word, code=-1):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == code and word in str(e.value), e.value
    return str(e.value)


@pytest.fixture(scope="module")
def small():
    return P.load_bal(ncams=5, npts=30)


# ---------------------------------------------------------------------------------------------------------------- sample

def test_sample(gctx, small):
    pp = small
    slo, shi = sampling_intervals(pp)
    X0 = pp.x0 * (1 + 1e-3 * np.random.default_rng(3).standard_normal((8, pp.nvars)))
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X0)
    pop.set_sampling(slo, shi)
    pop.eval()
    assert pop.info("eval_valid") == 1
    pop.sample(SEED, 3, first=2, count=5)
    assert pop.info("eval_valid") == 0                       # marks the evaluation stale, as set_x does
    _refused(pop.best, "evaluate first")
    X = pop.get_x()
    want = draws(pp, slo, shi, 3, range(2, 7))
    assert X[2:7].tobytes() == want.tobytes(), np.argwhere(X[2:7] != want)[:5]
    for s in (0, 1, 7):
        assert X[s].tobytes() == X0[s].tobytes(), s
    assert np.all(X[2:7] >= pp.lo) and np.all(X[2:7] <= pp.hi) and len(np.unique(X[2:7])) > 5 * pp.nvars - 5
    # the same rows in two calls: the same bytes
    cut = capi.Population(g, x=X0)
    cut.set_sampling(slo, shi)
    cut.sample(SEED, 3, first=2, count=2)
    cut.sample(SEED, 3, first=4, count=3)
    assert cut.get_x().tobytes() == X.tobytes()
    # another stream: other values
    cut.sample(SEED, 4, first=2, count=5)
    other = cut.get_x()
    assert other[2:7].tobytes() == draws(pp, slo, shi, 4, range(2, 7)).tobytes() and not np.any(other[2:7] == X[2:7])
    cut.close()
    # seven variables listed, unsorted: those and nothing else
    vid = np.array([133, 4, 77, 0, 9, 50, 12], dtype=np.int64)
    lst = capi.Population(g, x=X0)
    lst.set_sampling(slo, shi)
    lst.sample(SEED, 3, first=1, count=3, vid=vid)
    got = lst.get_x()
    wantl = X0.copy()
    wantl[1:4, vid] = draws(pp, slo, shi, 3, range(1, 4), vid)
    assert got.tobytes() == wantl.tobytes()
    # before set_sampling: the problem's domains
    lst.set_sampling(None, None)
    lst.sample(SEED, 3, first=0, count=1)
    assert lst.get_x(0).tobytes() == draws(pp, pp.lo, pp.hi, 3, [0])[0].tobytes()
    lst.close()
    # stream out of range, members out of range
    _refused(lambda: pop.sample(SEED, -1), "stream")
    _refused(lambda: pop.sample(SEED, (1 << 31) - 1), "stream")
    _refused(lambda: pop.sample(SEED, 0, first=7, count=2), "out of range")
    pop.sample(SEED, (1 << 31) - 2, first=7, count=1)
    assert pop.get_x(7).tobytes() == draws(pp, slo, shi, (1 << 31) - 2, [7])[0].tobytes()


def test_sample_clamps_and_refusals(gctx, small):
    """three variables whose interval lies outside the domain come back at lo / hi, a zero-width interval at its bound;
    set_sampling with lo > hi, a NaN or one array alone is refused and changes nothing"""
    pp = small
    slo, shi = sampling_intervals(pp)
    a, b, c, z = 7, 60, 101, 30
    slo[a], shi[a] = pp.hi[a] + 1.0, pp.hi[a] + 2.0         # above the domain
    slo[b], shi[b] = pp.lo[b] - 2.0, pp.lo[b] - 1.0         # below it
    slo[c], shi[c] = pp.hi[c] + 5.0, pp.hi[c] + 5.0         # zero width, above
    slo[z], shi[z] = pp.x0[z], pp.x0[z]                     # zero width, inside
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, nmembers=8)
    pop.set_sampling(slo, shi)
    pop.sample(SEED, 3)
    X = pop.get_x()
    assert X.tobytes() == draws(pp, slo, shi, 3, range(8)).tobytes()
    assert np.all(X[:, a] == pp.hi[a]) and np.all(X[:, b] == pp.lo[b]) and np.all(X[:, c] == pp.hi[c]) and np.all(X[:, z] == pp.x0[z])
    bad = slo.copy()
    bad[17] = shi[17] + 1.0
    assert "17" in _refused(lambda: pop.set_sampling(bad, shi), "variable")
    bad = shi.copy()
    bad[5] = np.nan
    assert "5" in _refused(lambda: pop.set_sampling(slo, bad), "variable")
    bad[5] = np.inf
    _refused(lambda: pop.set_sampling(slo, bad), "variable")
    _refused(lambda: pop.set_sampling(slo, None), "together")
    pop.sample(SEED, 5)                                      # the intervals are the ones set before the refusals
    assert pop.get_x().tobytes() == draws(pp, slo, shi, 5, range(8)).tobytes()


# ------------------------------------------------------------------------------------------------------------------ sort

@pytest.fixture(scope="module")
def thousand(gctx, small):
    """test_gpu_population_eval.py's argmin members: the minimum's row at 63, 64, 255, 256 and 700, NaN rows at 0 and 999"""
    pp = small
    X = pp.x0 * (1 + 1e-3 * np.random.default_rng(41).standard_normal((1000, pp.nvars)))
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    f = pop.eval()
    m = int(np.argmin(f))
    row = X[m].copy()
    if m < 63:
        X[m] = X[int(np.argmax(f))]
    for s in (63, 64, 255, 256, 700):
        X[s] = row
    X[0] = np.nan
    X[999] = np.nan
    pop.close()
    g.close()
    return X


def test_sort_thousand(gctx, small, thousand):
    pp, X = small, thousand
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    f = pop.eval()
    assert np.sum(np.isnan(f)) == 2 and f[63] == f[64] == f[255] == f[256] == f[700] == np.nanmin(f)
    fd = pop.eval_device()
    order = pop.sort()
    want = rule_order(f)
    assert order.dtype == np.int64 and order.tolist() == want
    # (the minimum's own row is a sixth copy, wherever it stands: equal values come by index)
    assert [s for s in want[:6] if s in (63, 64, 255, 256, 700)] == [63, 64, 255, 256, 700] and want[-2:] == [0, 999]
    assert want[:6] == sorted(want[:6]) and len(set(f[want[:6]].tolist())) == 1
    assert pop.get_x().tobytes() == X[order].tobytes()
    assert pop.info("eval_valid") == 1
    assert pop.best() == (0, f[order[0]])
    assert np.frombuffer(gctx.copy_to_host(fd, 8 * 1000), dtype=np.float64).tobytes() == f[order].tobytes()
    assert pop.eval().tobytes() == f[order].tobytes()
    assert pop.sort().tolist() == list(range(1000))          # sorted already: the identity
    assert pop.get_x().tobytes() == X[order].tobytes()
    # all values +0.0 (an explicit empty list): every pair a tie, the identity
    assert pop.eval(np.zeros(0, dtype=np.int64)).tobytes() == np.zeros(1000).tobytes()
    assert pop.sort().tolist() == list(range(1000)) and pop.get_x().tobytes() == X[order].tobytes()
    # stale values: refused, and nothing moves
    pop.set_x(X[5:6], first=5, count=1)
    before = pop.get_x()
    _refused(pop.sort, "evaluate first")
    _refused(lambda: pop.sort(want_order=False), "evaluate first")
    assert pop.get_x().tobytes() == before.tobytes() and pop.info("eval_valid") == 0


@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_sort_small_populations(gctx, small, thousand, n):
    """one member; three all-NaN members (the identity); 64 and 65 members (a wave, a wave and one)"""
    pp = small
    X = np.full((3, pp.nvars), np.nan) if n == 3 else thousand[700 - n + 2:702][::-1].copy()
    assert X.shape[0] == n
    g = capi.Problem(gctx, pp)
    fresh = capi.Population(g, x=X)
    _refused(fresh.sort, "evaluate first")                   # before any evaluation
    f = fresh.eval()
    order = fresh.sort()
    assert order.tolist() == rule_order(f)
    if n == 3:
        assert np.all(np.isnan(f)) and order.tolist() == [0, 1, 2]
    assert fresh.get_x().tobytes() == X[order].tobytes() and fresh.eval().tobytes() == f[order].tobytes()


def test_sort_then_assign_best_without_a_wait(gctx, small, thousand):
    pp, X = small, thousand[600:720]
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, x=X)
    f = pop.eval()
    b = rule_order(f)[0]
    assert b != 0 and f[b] == f[100]                         # (row 700 of the thousand is one of the minimum's copies)
    assert pop.sort(want_order=False) is None
    pop.assign_best()
    assert g.get_x().tobytes() == X[b].tobytes() == pop.get_x(0).tobytes()
    assert pop.best() == (0, f[b])


def test_sort_refuses_more_than_2_18_members(gctx):
    pp = P.PackedProblem(kind=P.KIND_NLP, x0=np.array([0.5]), lo=np.array([-1.0]), hi=np.array([1.0]), coeff=np.array([1.0]),
                         rowptr=np.array([0, 1], dtype=np.int64), vid=np.array([0], dtype=np.int64), expo=np.array([2.0]),
                         cons=np.array([0.0]), sine=np.array([0], dtype=np.uint8))
    g = capi.Problem(gctx, pp)
    pop = capi.Population(g, nmembers=(1 << 18) + 1)
    assert "2^18" in _refused(pop.sort, "population_sort", code=-5)
    _refused(lambda: pop.sort(want_order=False), "population_sort", code=-5)
    ok = capi.Population(g, nmembers=4)
    ok.eval()
    assert ok.sort().tolist() == [0, 1, 2, 3]


# ----------------------------------------------------------------------------------------------------------------- range

def assert_range_equals_whole(plan, twin_plan, pop, twin, X, first, count):
    """pop: solved on [first, first + count) by `plan`; twin: the same members solved whole by `twin_plan` (the parent's path)"""
    pr, wr = plan.fetch_population(), twin_plan.fetch_population()
    n = X.shape[0]
    assert pr.fret.shape == (count, plan.ncomp) and pr.x.shape == (count, plan.nfree) and wr.fret.shape == (n, plan.ncomp)
    for name in FIELDS:
        a, b = getattr(pr, name), getattr(wr, name)[first:first + count]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    rows, wrows = pop.get_x(), twin.get_x()
    assert rows[first:first + count].tobytes() == wrows[first:first + count].tobytes()
    for s in list(range(first)) + list(range(first + count, n)):
        assert rows[s].tobytes() == X[s].tobytes(), s
    assert wrows[first:first + count].tobytes() != X[first:first + count].tobytes()


@pytest.mark.parametrize("budget", [1 << 30, 1])
def test_range_mixed_plan(gctx, budget):
    """test_gpu_population_ptm.py::test_mixed_plan's plan with tiny components: the tiny-component, the point-major and the
    LDS-resident kernel in one solve; 5 members, range (1, 3), in one launch set and member by member"""
    pp = P.make_synthetic_ba(5, 3, 1200)
    fp, fv, cp, ci = [0], [], [0], []

    def add(v, f):
        fv.extend(int(t) for t in v); fp.append(len(fv)); ci.extend(int(t) for t in f); cp.append(len(ci))

    for c in (0, 1):
        add(*pp.component(c))
    for c, keep in ((2, 40), (3, 60)):
        v, f = pp.component(c)
        q_end = v[0] + 27 + 3 * keep
        add(v[v < q_end], f[pp.pt_vid0[f] < q_end])
    v, f = pp.component(4)
    for q in v[27:27 + 3 * 50:3]:
        add([q, q + 1, q + 2], f[pp.pt_vid0[f] == q])
    comps = tuple(np.array(t, dtype=np.int64) for t in (fp, fv, cp, ci))
    opts = {"coop_min_factors": 0, "coop_group_min_factors": 0, "ptm_group": 1, "population_point_major": 1, "population_tiny": 1,
            "row_min_components": 1}
    rng = np.random.default_rng(29)
    X = np.stack([pp.x0] + [pp.x0 * (1 + 1e-3 * rng.standard_normal(pp.nvars)) for _ in range(4)])
    g = capi.Problem(gctx, pp)
    plan, twin_plan = capi.Plan(g, *comps), capi.Plan(g, *comps)
    for q in (plan, twin_plan):
        set_options(q, opts)
        q.set_option("starts_workspace_bytes", budget)
    assert plan.info("components_point_major") == 2 and plan.info("components_lds") == 2 and plan.info("components_tiny") == 50
    pop, twin = capi.Population(g, x=X), capi.Population(g, x=X)
    twin_plan.solve_population(twin, 25, 3e-8)
    plan.solve_population(pop, 25, 3e-8, first=1, count=3)
    launches = 3 if budget > 1 else 9                        # what three members give: tiny, point-major, LDS-resident per launch set
    assert plan.info("starts_launches") == launches and plan.last_kernel_ms()[1] == launches
    assert plan.info("starts_per_launch") == (3 if budget > 1 else 1)
    assert_range_equals_whole(plan, twin_plan, pop, twin, X, 1, 3)


def test_range_plain_solver(gctx):
    """the sinusoid's three subtrees on the plain batch solver (population_plain = 1): 6 members, range (4, 2)"""
    pp = P.make_high_dim_sinusoid()
    g = capi.Problem(gctx, pp)
    assigned = np.zeros(pp.nvars, np.uint8)
    assigned[0] = 1
    sub = g.components(assigned)
    assert np.diff(sub[0]).tolist() == [40, 40, 40]
    X = np.random.default_rng(7).uniform(pp.lo, pp.hi, (6, pp.nvars))
    plan, twin_plan = capi.Plan(g, *sub), capi.Plan(g, *sub)
    for q in (plan, twin_plan):
        q.set_option("population_plain", 1)
        assert q.info("components_plain") == q.ncomp
    pop, twin = capi.Population(g, x=X), capi.Population(g, x=X)
    twin_plan.solve_population(twin, 25, 3e-8)
    plan.solve_population(pop, 25, 3e-8, first=4, count=2)
    assert plan.info("starts_launches") == 1 and plan.info("starts_per_launch") == 2
    assert_range_equals_whole(plan, twin_plan, pop, twin, X, 4, 2)


def test_range_whole_and_refusals(gctx, small):
    """range (0, nmembers) == the whole-population entry; count = 0, a range beyond the population and another problem's
    population are refused, and the plan and the population stay usable"""
    pp = small
    cams, pts = P.ba_alternation_plans(pp)
    slo, shi = sampling_intervals(pp)
    X = np.random.default_rng(3).uniform(slo, shi, size=(6, pp.nvars))
    g, h = capi.Problem(gctx, pp), capi.Problem(gctx, pp)
    plan, twin_plan = capi.Plan(g, *cams), capi.Plan(g, *cams)
    for q in (plan, twin_plan):
        set_options(q, OPTIONS)
    pop, twin, foreign = capi.Population(g, x=X), capi.Population(g, x=X), capi.Population(h, x=X)
    _refused(lambda: plan.solve_population(pop, 25, 3e-8, first=2, count=0), "out of range")
    _refused(lambda: plan.solve_population(pop, 25, 3e-8, first=4, count=3), "out of range")
    _refused(lambda: plan.solve_population(pop, 25, 3e-8, first=-1, count=2), "out of range")
    _refused(lambda: plan.solve_population(pop, 25, 3e-8, first=6), "out of range")
    _refused(lambda: plan.solve_population(foreign, 25, 3e-8, first=1, count=2), "another problem")
    _refused(lambda: plan.solve_population(pop, 0, 3e-8, first=1, count=2), "maxiters")
    assert pop.get_x().tobytes() == X.tobytes()
    twin_plan.solve_population(twin, 25, 3e-8)
    plan.solve_population(pop, 25, 3e-8, first=0, count=6)
    pr, wr = plan.fetch_population(), twin_plan.fetch_population()
    for name in FIELDS:
        assert getattr(pr, name).tobytes() == getattr(wr, name).tobytes(), name
    assert pop.get_x().tobytes() == twin.get_x().tobytes() != X.tobytes()
    assert pop.info("eval_valid") == 0


# ------------------------------------------------------------------------------------------------------------------ loop

def test_halving_loop_equals_the_host_route(gctx, small):
    """16 members of ladybug 5 / 30 drawn on the device, two rounds of (camera plan, point plan on members 0 .. k-1, evaluate,
    sort, k //= 2) through the new entries alone == the same loop on the host: eval, sorted() by the rule, the rows moved with
    get_x / set_x, the survivors solved by the whole-population entry on a population of their own"""
    pp = small
    cams, pts = P.ba_alternation_plans(pp)
    slo, shi = sampling_intervals(pp)
    g = capi.Problem(gctx, pp)
    plans = [capi.Plan(g, *cams), capi.Plan(g, *pts)]
    for plan in plans:
        set_options(plan, OPTIONS)
        assert plan.info("components_lds") == plan.ncomp
    # the device's loop: nothing read but the orders (kept for the comparison)
    pop = capi.Population(g, nmembers=16)
    pop.set_sampling(slo, shi)
    pop.sample(SEED, 0)
    X0 = pop.get_x()
    assert X0.tobytes() == draws(pp, slo, shi, 0, range(16)).tobytes()
    k, orders = 16, []
    for _ in range(2):
        for plan in plans:
            plan.solve_population(pop, 25, 3e-8, first=0, count=k)
        pop.eval_device()
        orders.append(pop.sort())
        k //= 2
    pop.assign_best()
    final = pop.get_x()
    # the host's
    rows, k, want_orders = X0.copy(), 16, []
    for _ in range(2):
        part = capi.Population(g, x=rows[:k])
        for plan in plans:
            plan.solve_population(part, 25, 3e-8)
        rows[:k] = part.get_x()
        part.close()
        whole = capi.Population(g, x=rows)
        f = whole.eval()
        whole.close()
        order = rule_order(f)
        want_orders.append(order)
        rows = rows[order]
        k //= 2
    for a, b in zip(orders, want_orders):
        assert a.tolist() == b
    assert sorted(orders[0].tolist()) == list(range(16)) and orders[0].tolist() != list(range(16))
    assert final.tobytes() == rows.tobytes()
    assert g.get_x().tobytes() == rows[0].tobytes()
