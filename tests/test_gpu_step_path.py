"""What rdis_hip_plan_set_start / _solve / _fetch put on the stream around the solver, for a resident plan that is solved again
and again: the results block lands in pinned memory, and a plan whose one launch is the single-group pipelined solver gets its
objective from that kernel (no objective_sum_kernel).  Neither may change a bit of a result, whatever the order of solves, fetches,
plans and options -- every comparison here is ==.

Shapes: A one small component on the pipelined solver (a few workgroups: the one-launch case); B five groups side by side in one
pipelined launch (the objective kernel stays); C the same five with six small components of the same plan in a batch launch
beside them."""
import numpy as np
import pytest

from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

EXIT_SYNC_TIMEOUT = 7
ITERS, FTOL = 8, 3e-8


def _with_small_components(big, small):
    """one problem: `big`'s components, then `small`'s behind them (variables and factors renumbered)"""
    nv, nf = big.nvars, big.nfac
    cat = np.concatenate
    return P.PackedProblem(
        kind=big.kind, x0=cat([big.x0, small.x0]), lo=cat([big.lo, small.lo]), hi=cat([big.hi, small.hi]),
        cam_vid0=cat([big.cam_vid0, small.cam_vid0 + nv]), pt_vid0=cat([big.pt_vid0, small.pt_vid0 + nv]),
        obs=np.ascontiguousarray(cat([big.obs, small.obs])),
        comp_free_ptr=cat([big.comp_free_ptr, small.comp_free_ptr[1:] + nv]), comp_free_vid=cat([big.comp_free_vid, small.comp_free_vid + nv]),
        comp_fac_ptr=cat([big.comp_fac_ptr, small.comp_fac_ptr[1:] + nf]), comp_fac_id=cat([big.comp_fac_id, small.comp_fac_id + nf]))


def _build(name):
    if name == "A":
        return P.make_synthetic_ba(1, 3, 100, obs_per_pt=3).single_component(), {"coop_min_factors": 256}
    big = P.make_synthetic_ba(5, 3, 900, obs_per_pt=3)
    if name == "B":
        return big, {"coop_min_factors": 1000}
    return _with_small_components(big, P.make_synthetic_ba(6, 3, 40, first_comp=5)), {"coop_min_factors": 1000}


class _Shape:
    def __init__(self, gctx, name):
        self.name = name
        self.pp, self.opts = _build(name)
        self.comps = (self.pp.comp_free_ptr, self.pp.comp_free_vid, self.pp.comp_fac_ptr, self.pp.comp_fac_id)
        self.x0 = np.ascontiguousarray(self.pp.x0[self.pp.comp_free_vid])
        self.g = capi.Problem(gctx, self.pp)
        self._fresh = {}

    def plan(self, **more):
        plan = capi.Plan(self.g, *self.comps)
        for k, v in {**self.opts, **more}.items():
            plan.set_option(k, v)
        return plan

    def solve(self, plan):
        plan.set_start(self.x0)
        plan.solve(ITERS, FTOL)

    def round(self, plan, out=None, want_x=True):
        self.solve(plan)
        return _copy(plan.fetch(want_x=want_x, out=out))

    def fresh(self, pipeline=1):
        """a fresh plan's result and objective under coop_pipeline = pipeline: computed once, never written again"""
        if pipeline not in self._fresh:
            plan = self.plan(coop_pipeline=pipeline)
            r = self.round(plan)
            assert plan.info("pipelined") == pipeline and np.all((r.status & 0xFF) != EXIT_SYNC_TIMEOUT), (self.name, pipeline)
            assert np.all(r.delta < 0) and np.all(r.nfeval > 10), (self.name, pipeline)      # (the solve did something)
            self._fresh[pipeline] = (r, plan.objective())
            plan.close()
        return self._fresh[pipeline]


def _copy(r):
    return capi.BatchResult(*(None if a is None else np.array(a, copy=True) for a in (r.x, r.fret, r.delta, r.iters, r.status, r.nfeval, r.ngeval)))


def _same(want, got, what, x=True):
    assert np.all((got.status & 0xFF) != EXIT_SYNC_TIMEOUT), what
    assert np.array_equal(want.fret, got.fret) and np.array_equal(want.delta, got.delta), what
    assert not x or np.array_equal(want.x, got.x), what
    assert np.array_equal(want.iters, got.iters) and np.array_equal(want.status, got.status), what
    assert np.array_equal(want.nfeval, got.nfeval) and np.array_equal(want.ngeval, got.ngeval), what


@pytest.fixture(scope="module")
def shapes(gctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Shape(gctx, name)
        return made[name]
    return get


def test_the_shapes_are_what_they_are_meant_to_be(shapes):
    a, b, c = shapes("A"), shapes("B"), shapes("C")
    for s in (a, b, c):
        plan = s.plan()
        s.round(plan)
        launches = plan.last_kernel_ms()[1]
        assert plan.info("pipelined") == 1 and (launches == 1 if s is not c else launches >= 2), (s.name, launches)
        plan.close()
    assert a.pp.ncomp == 1 and b.pp.ncomp == 5 and c.pp.ncomp == 11


@pytest.mark.parametrize("name", ["A", "B"])
def test_three_rounds_on_one_plan_equal_the_first_and_a_fresh_plans(shapes, name):
    s = shapes(name)
    want, _ = s.fresh()
    plan = s.plan()
    keep, rounds = None, []
    for i in range(3):
        s.solve(plan)
        keep = plan.fetch(out=keep)          # (into the caller's own arrays from the second round on, as the benchmark's step does)
        rounds.append(_copy(keep))
    for i, r in enumerate(rounds):
        _same(rounds[0], r, (name, "round", i))
        _same(want, r, (name, "fresh plan against round", i))
    plan.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_two_solves_with_no_fetch_between_them(shapes, name):
    s = shapes(name)
    want, _ = s.fresh()
    plan = s.plan()
    _same(want, s.round(plan), (name, "first"))
    s.solve(plan)                                      # (its results and its objective are never read)
    _same(want, s.round(plan), (name, "solve, solve, fetch"))
    _same(want, s.round(plan), (name, "and once more after a fetch"))
    plan.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_rounds_fetched_without_x(shapes, name):
    s = shapes(name)
    want, _ = s.fresh()
    plan = s.plan()
    for i in range(3):
        r = s.round(plan, want_x=False)
        assert r.x is None
        _same(want, r, (name, "without x, round", i), x=False)
    _same(want, s.round(plan), (name, "with x after rounds without"))
    plan.close()


def test_two_plans_of_one_problem_solved_alternately(shapes):
    s = shapes("A")
    want, _ = s.fresh()
    one, two = s.plan(), s.plan()
    for i, plan in enumerate((one, two, one, two, two, one)):
        _same(want, s.round(plan), ("A", "alternating plans, solve", i))
    one.close()
    _same(want, s.round(two), ("A", "the other plan closed"))
    two.close()


def test_pipeline_switched_off_and_on_again_between_solves(shapes):
    s = shapes("A")
    plan = s.plan()
    for i, pipeline in enumerate((1, 0, 1, 1, 0, 0, 1)):
        plan.set_option("coop_pipeline", pipeline)
        r = s.round(plan)
        assert plan.info("pipelined") == pipeline
        _same(s.fresh(pipeline)[0], r, ("A", "coop_pipeline", pipeline, "solve", i))
        assert plan.objective() == s.fresh(pipeline)[1] == r.fret[0]
    plan.close()


def _comm(gctx):
    try:
        return capi.Comm(gctx, 1, 0, capi.Comm.unique_id())
    except capi.RdisHipError as exc:
        pytest.skip("RCCL does not come up: %s" % exc)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_objective_is_what_the_sum_kernel_returns(shapes, name):
    s = shapes(name)
    want, _ = s.fresh()
    # A: the kernel's sum of one component is that component's fret (0.0 + fret and further zeros).  B, C: the objective of a second
    # plan with coop_pipeline = 0 -- objective_sum_kernel behind the cooperative solver, whose groups of this size return the
    # pipelined solver's bits (tests/test_gpu_pipe_poll_ring.py: "five groups") -- is what these plans returned before
    want_obj = want.fret[0] if name == "A" else s.fresh(0)[1]
    if name != "A":
        _same(s.fresh(0)[0], want, (name, "coop_pipeline 0 against 1"))
    plan = s.plan()
    where = plan.objective_device_ptr()
    for i in range(3):
        r = s.round(plan)
        _same(want, r, (name, "round", i))
        first, second = plan.objective(), plan.objective()
        assert first == second == want_obj, (name, i, first, second, want_obj)
        assert plan.objective_device_ptr() == where      # (callers keep the address across solves)
    assert s.fresh()[1] == want_obj
    plan.close()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_one_rank_allreduce_returns_the_objective_again(gctx, shapes, name):
    comm = _comm(gctx)
    s = shapes(name)
    want_obj = s.fresh()[0].fret[0] if name == "A" else s.fresh(0)[1]
    plan = s.plan()
    for i in range(2):
        s.round(plan)
        assert plan.allreduce_objective(None) == want_obj, (name, i)
        assert plan.allreduce_objective(comm) == want_obj, (name, i)      # in place on the device
        assert plan.objective() == want_obj, (name, i)
        s.solve(plan)
        plan.allreduce_objective(comm, fetch=False)                       # behind the solve on its stream, as the benchmark's step does
        plan.fetch()
        assert plan.objective() == want_obj, (name, i)
    plan.close()
    comm.close()
