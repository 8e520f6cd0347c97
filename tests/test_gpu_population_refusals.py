"""Every refusal the population entries share a rule for (rdis_amd/csrc/population_rules.hpp), through the library: the return
code and the context's last error, the whole message (tests/test_population_rules_cpu.py holds the same literals), and after
each refusal the population as it was -- get_x of all rows == the rows before, eval_valid as before.  Every case is refused on
the host before anything is launched.  Then one sort and one permute with the inverse order: X and f return bit for bit."""
import numpy as np
import pytest

from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -5
NO_VALUES = ("%s: the population has no current values (evaluate first: rdis_hip_population_eval or _eval_device after the last "
             "population_set_x / plan_solve_population)")
NO_VALUES_SORT = ("population_sort: the population has no current values (evaluate first: rdis_hip_population_eval or _eval_device after the last "
                  "population_set_x / population_sample / plan_solve_population)")


@pytest.fixture(scope="module")
def setup(gctx):
    pp = P.load_bal(ncams=5, npts=30)
    X0 = pp.x0 * (1 + 1e-3 * np.random.default_rng(11).standard_normal((4, pp.nvars)))
    prob = capi.Problem(gctx, pp)
    return pp, prob, X0


def _refused(gctx, pop, call, code, message):
    """the call is refused with that code and that whole message, and the population is as it was"""
    rows, valid = pop.get_x(), pop.info("eval_valid")
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == code, e.value
    assert gctx.lib.rdis_hip_last_error(gctx.h).decode() == message
    assert pop.get_x().tobytes() == rows.tobytes() and pop.info("eval_valid") == valid


def _raw(gctx, rc):
    gctx.check(rc)


def test_range_refusals(gctx, setup):
    pp, prob, X0 = setup
    pop = capi.Population(prob, x=X0)
    pop.eval()                                                       # (eval_valid set: a refusal must leave it set)
    N, lib, h = pp.nvars, gctx.lib, pop.h
    val, out = np.zeros((8, N + 1)), np.zeros((8, N + 1))
    big = np.zeros(1)                                                # (never read: refused before)
    entries = {
        "population_set_x": lambda first, count, n: _raw(gctx, lib.rdis_hip_population_set_x(h, first, count, n, None, capi._ptr(val))),
        "population_get_x": lambda first, count, n: _raw(gctx, lib.rdis_hip_population_get_x(h, first, count, n, None, capi._ptr(out))),
        "population_sample": lambda first, count, n: _raw(gctx, lib.rdis_hip_population_sample(h, first, count, n, None, 7, 0)),
    }
    for who, call in entries.items():
        for first, count in ((4, 1), (5, 0), (-1, 1), (0, -1), (3, 2), (1, 2 ** 63 - 1)):
            _refused(gctx, pop, lambda: call(first, count, N), EINVAL, who + ": members out of range")
        _refused(gctx, pop, lambda: call(0, 4, N + 1), EINVAL, who + ": n > nvars")
        call(4, 0, N)                                                # first == nmembers with count == 0 passes, and nothing happens
        assert pop.info("eval_valid") == 1
    # eval_grad's range is of whole rows: n is nvars
    for first, count in ((4, 1), (5, 0), (-1, 1), (0, -1), (3, 2), (1, 2 ** 63 - 1)):
        _refused(gctx, pop, lambda: _raw(gctx, lib.rdis_hip_population_eval_grad(h, first, count, prob.nfac, None, capi._ptr(big), capi._ptr(big))),
                 EINVAL, "population_eval_grad: members out of range")
    f, g = pop.eval_grad(first=4, count=0)
    assert f.shape == (0,) and g.shape == (0, N)
    # too many values: a list (the ids are not looked at before the bound) on a population whose range allows the count
    vid = np.zeros(1, np.int64)
    for who, rc in (("population_set_x", lambda: lib.rdis_hip_population_set_x(h, 0, 4, 3 * 10 ** 15, capi._ptr(vid), capi._ptr(val))),
                    ("population_get_x", lambda: lib.rdis_hip_population_get_x(h, 0, 4, 3 * 10 ** 15, capi._ptr(vid), capi._ptr(out))),
                    ("population_sample", lambda: lib.rdis_hip_population_sample(h, 0, 4, 3 * 10 ** 15, capi._ptr(vid), 7, 0))):
        _refused(gctx, pop, lambda: _raw(gctx, rc()), ERANGE, who + ": too many values")


def test_permute_and_sampling_refusals(gctx, setup):
    pp, prob, X0 = setup
    pop = capi.Population(prob, x=X0)
    pop.eval()
    _refused(gctx, pop, lambda: pop.permute([0, 4, 1, 2]), EINVAL, "population_permute: order[1] = 4 is out of range (the population has 4 members)")
    _refused(gctx, pop, lambda: pop.permute([-1, 0, 1, 2]), EINVAL, "population_permute: order[0] = -1 is out of range (the population has 4 members)")
    _refused(gctx, pop, lambda: pop.permute([2, 0, 2, 1]), EINVAL, "population_permute: member 2 is named twice (order[2]): not a permutation")
    _refused(gctx, pop, lambda: pop.permute(None), EINVAL, "population_permute: order is NULL (order[r]: the row that becomes row r)")
    lo, hi = pp.lo.copy(), pp.hi.copy()
    lo[~np.isfinite(lo)], hi[~np.isfinite(hi)] = -1e3, 1e3
    together = "population_set_sampling: lo and hi are given together (both NULL: the problem's domains)"
    _refused(gctx, pop, lambda: pop.set_sampling(lo, None), EINVAL, together)
    _refused(gctx, pop, lambda: pop.set_sampling(None, hi), EINVAL, together)
    bad = lo.copy()
    bad[7] = hi[7] + 1.0
    bad[9] = np.nan
    _refused(gctx, pop, lambda: pop.set_sampling(bad, hi), EINVAL, "population_set_sampling: variable 7: the sampling interval must be finite with lo <= hi")
    bad = hi.copy()
    bad[pp.nvars - 1] = np.inf
    _refused(gctx, pop, lambda: pop.set_sampling(lo, bad), EINVAL,
             "population_set_sampling: variable %d: the sampling interval must be finite with lo <= hi" % (pp.nvars - 1))
    pop.set_sampling(lo, hi)                                         # (and what is an interval is taken)
    pop.set_sampling(None, None)


def test_readers_without_values_and_unknown_names(gctx, setup):
    pp, prob, X0 = setup
    pop = capi.Population(prob, x=X0)

    def readers():
        _refused(gctx, pop, pop.best, EINVAL, NO_VALUES % "population_best")
        _refused(gctx, pop, pop.assign_best, EINVAL, NO_VALUES % "population_assign_best")
        _refused(gctx, pop, pop.sort, EINVAL, NO_VALUES_SORT)

    x_assigned = prob.get_x()
    readers()                                                        # before any evaluation
    pop.eval()
    assert pop.info("eval_valid") == 1 and pop.best()[0] in range(4)
    pop.set_x(X0[1], first=2, count=1)
    assert pop.info("eval_valid") == 0
    readers()                                                        # after a set_x
    assert prob.get_x().tobytes() == x_assigned.tobytes()            # (a refused assign_best assigned nothing)
    _refused(gctx, pop, pop.grad_max, EINVAL,
             "population_grad_max: evaluate the gradient first (rdis_hip_population_eval_grad or _eval_grad_device)")
    _refused(gctx, pop, lambda: pop.set_option("eval_workspace", 1), EINVAL,
             "population_set_option: unknown option 'eval_workspace' (eval_workspace_bytes, eval_batched, grad_workspace_bytes)")
    _refused(gctx, pop, lambda: pop.info("launches"), EINVAL,
             "population_get_info: unknown name 'launches' (eval_members_per_launch, eval_launches, eval_valid, grad_members_per_launch, "
             "grad_launches, grad_branch, nmembers, problem_handle)")


def test_sort_then_the_inverse_permute_returns_x_and_f(gctx, setup):
    pp, prob, X0 = setup
    X = X0[[2, 0, 3, 1]]
    pop = capi.Population(prob, x=X)
    fd = pop.eval_device()                                           # f's address: it holds through both reorders
    f0 = np.frombuffer(gctx.copy_to_host(fd, 32))
    assert f0.tobytes() == pop.eval().tobytes() and len(set(f0.tolist())) == 4   # (four values: the sort has something to move)
    order = pop.sort()
    assert sorted(order.tolist()) == [0, 1, 2, 3] and order.tolist() != [0, 1, 2, 3]
    assert gctx.copy_to_host(fd, 32) == f0[order].tobytes() and pop.get_x().tobytes() == X[order].tobytes()
    pop.permute(np.argsort(order))                                   # (row order[r] went to r: the inverse order takes it back)
    assert pop.info("eval_valid") == 1                               # a valid evaluation is permuted with the rows
    assert pop.get_x().tobytes() == X.tobytes() and gctx.copy_to_host(fd, 32) == f0.tobytes()
    assert pop.best() == (int(np.argmin(f0)), float(f0.min()))
