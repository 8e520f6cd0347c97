"""The dense Levenberg-Marquardt oracle alone (oracle/lm_oracle.py) on the exit cases of tests/lm_exit_cases.py.  No device
code runs here: what is pinned is that the oracle reaches the exit every case states, that the exits decided far from rounding
keep their (stop, iterations) under one-ulp changes of the start, that the converged cases stay converged well inside their
iteration limit under the same changes, and that the loop's counter identities (lm_exit_cases.check_identities) hold for every
oracle run -- so that tests/test_gpu_lm_exits.py compares the device with a reference that is one."""
import math

import numpy as np
import pytest

import lm_batch_shapes as S
import lm_exit_cases as E

DRAWS = E.DRAWS


def _perturbed(c, draw):
    return E.perturbed_reference(c.name, draw)


@pytest.mark.parametrize("name", E.EXACT_NAMES)
def test_exact_exits_are_reached_and_kept_under_one_ulp_changes(name):
    """cases 1 and 2: the stated stop code (6 after at least one accepted step; 1 at iteration 0 with nothing solved), and the
    same (stop, iterations) in every component for six draws of one-ulp changes of the start"""
    c = E.case(name)
    ref = E.oracle_reference(name)
    for k, r in enumerate(ref):
        E.check_identities(r)
        if k in c.stop:
            assert r.stop == c.stop[k]
            if r.stop == 6:
                assert r.iters >= 1 and sum(1 for h in r.history if h[3]) == r.iters
            if r.stop == 1:
                free = c.comps[k][0]
                assert (r.iters, r.njev, r.nsolve, r.nfev, len(r.history)) == (0, 1, 0, 1, 0)
                assert abs(r.fret - r.finit) <= 1e-15 * r.finit       # (the oracle sums finit from the residuals, fret from the factors)
                assert r.x.tobytes() == np.minimum(np.maximum(c.x[free], c.pp.lo[free]), c.pp.hi[free]).tobytes()
    if name.startswith("idle/"):
        idle = E.idle_block(name)
        free = c.comps[0][0]
        assert ref[0].x[np.isin(free, idle)].tobytes() == c.x[idle].tobytes() and ref[0].iters == c.maxiters
    for draw in range(DRAWS):
        for r, rp in zip(ref, _perturbed(c, draw)):
            E.check_identities(rp)
            assert (rp.stop, rp.iters) == (r.stop, r.iters)
    print("LM exits, oracle, %s: %d components, exits %s" % (name, len(ref), sorted(set((r.stop, r.iters) for r in ref))))


@pytest.mark.parametrize("name", E.CONVERGED_NAMES)
def test_converged_cases_stay_converged_under_one_ulp_changes(name):
    """case 3: stop 2 within a quarter of the iteration limit; under six draws of one-ulp changes the iteration count stays below
    half the limit and the code in {2, 5}; fret and x of the perturbed runs lie within 1e-10 and 1e-8 of the unperturbed ones (the
    device is held to 1e-8 and 1e-7).  The history is another matter: measured, the oracle's own records before the convergence
    point move by up to 2e-8 (points from the start), 2e-7 (two-observation points) and 7e-5 to 2e-3 (the restarts) under these
    changes, so the device's history is compared over the records lm_exit_cases.stable_history counts, printed here"""
    c = E.case(name)
    ref = E.oracle_reference(name)
    assert c.maxiters <= E.MAXITERS
    for r in ref:
        E.check_identities(r)
        assert r.stop == 2 and 4 * r.iters <= c.maxiters
    dev_f = dev_x = 0.0
    worst = 0
    for draw in range(DRAWS):
        for r, rp in zip(ref, _perturbed(c, draw)):
            E.check_identities(rp)
            assert rp.stop in (2, 5) and 2 * rp.iters < c.maxiters
            worst = max(worst, rp.iters)
            dev_f = max(dev_f, abs(rp.fret - r.fret) / abs(r.fret))
            dev_x = max(dev_x, float(np.max(np.abs(rp.x - r.x)) / (1.0 + np.max(np.abs(r.x)))))
    assert dev_f <= 1e-10 and dev_x <= 1e-8                      # (a hundredth and a tenth of what the device is held to)
    stable, conv = E.stable_history(name), [S.converged_at(r) for r in ref]
    print("LM exits, oracle, %s: %d components, maxiters %d, iterations %d to %d (perturbed: up to %d); one-ulp changes move fret %.1e, x %.1e; "
          "history records the oracle reproduces to 1e-9: %d of the %d before convergence (of %d in all)" % (
              name, len(ref), c.maxiters, min(r.iters for r in ref), max(r.iters for r in ref), worst, dev_f, dev_x, sum(stable), sum(conv),
              sum(len(r.history) for r in ref)))


def test_one_observation_points_have_no_reference():
    """A point with one listed observation and ftol 0: two residuals, three unknowns, minimum 0.  The oracle ends with code 2 at a
    fret of rounding size, or at exactly 0 and then with code 6 -- which of the two is decided by rounding, so the case is
    compared by properties only on the device (tests/test_gpu_lm_exits.py)"""
    name = E.ZERO_NAMES[0]
    c = E.case(name)
    ref = E.oracle_reference(name)
    stops = set()
    for draw in range(-1, DRAWS):
        for r in (ref if draw < 0 else _perturbed(c, draw)):
            E.check_identities(r)
            stops.add(r.stop)
            assert r.stop in (2, 5, 6) and 2 * r.iters < c.maxiters and r.fret <= 1e-20 * r.finit
    print("LM exits, oracle, %s: stops %s" % (name, sorted(stops)))


@pytest.mark.parametrize("name", E.NONFINITE_NAMES + E.NONFINITE_SEQUENTIAL_NAMES)
def test_a_start_without_a_finite_objective_ends_with_code_7_before_any_linearisation(name):
    """case 4 in the oracle: the start is finite or holds one NaN, its objective is not finite; code 7, nothing linearised or
    solved, a NaN coordinate comes back NaN and a finite one clamped; the neighbours' runs do not see it"""
    c = E.case(name)
    ref = E.oracle_reference(name)
    (k, stop), = c.stop.items()
    free = c.comps[k][0]
    r = ref[k]
    E.check_identities(r)
    assert (r.stop, r.iters, r.njev, r.nsolve, r.nfev, len(r.history)) == (stop, 0, 0, 0, 1, 0)
    assert not math.isfinite(r.finit) and not math.isfinite(r.fret)
    start = c.x[free]
    assert int(np.sum(np.isnan(start))) == (0 if "/plane/" in name else 1)
    want = np.minimum(np.maximum(start, c.pp.lo[free]), c.pp.hi[free])
    assert np.array_equal(np.isnan(r.x), np.isnan(start)) and r.x[~np.isnan(start)].tobytes() == want[~np.isnan(start)].tobytes()
    for j, rj in enumerate(ref):
        if j != k:
            E.check_identities(rj)
            assert rj.stop in (2, 3) and math.isfinite(rj.fret)


def test_identities_hold_on_the_existing_shapes():
    """the counter identities on every oracle run the other Levenberg-Marquardt tests compare the device with: the batch shapes,
    the wide shapes and the population members (cached references: computed once for all the files that use them); no run
    has a refused factorisation"""
    import lm_plan_members as M
    import lm_wide_shapes as W
    runs = [r for name, model in S.CASES for r in S.oracle_reference(name, model)]
    runs += [r for name, model in W.CASES for r in W.oracle_reference(name, model)]
    runs += [r for name, model in M.ORACLE_CASES for s in range(M.NMEMBERS) for r in M.oracle_member_reference(name, model, s)]
    for r in runs:
        assert E.check_identities(r) == 0
    print("LM exits, oracle: identities on %d runs of the older shapes" % len(runs))
