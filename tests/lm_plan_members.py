"""The members the Levenberg-Marquardt plan's population solves are checked on, shared by tests/test_lm_plan_cpu.py (the
oracle's own sensitivity at these starts) and tests/test_gpu_lm_plan.py (the device): four complete states of a shape of
tests/lm_batch_shapes.py.  Member 0 is the problem's start; members 1 to 3 move every free variable of every component by
about 1e-3 of its size, each with its own generator, so that no two rows are alike and a wrong stride shows."""
import functools

import numpy as np

import lm_batch_shapes as S

NMEMBERS = 4

# the shapes of the population tests, and the one (shape, model) whose oracle runs at the perturbed starts are too
# sensitive to rounding to serve as a reference (tests/test_lm_plan_cpu.py measures it)
NAMES = ["ladybug-5-30-whole", "ladybug-5-30-points", "ladybug-5-30-cameras", "ladybug-5-30-sub-block", "synthetic-6x3x40",
         "synthetic-2x16x60"]
TOO_SENSITIVE = ("synthetic-6x3x40", 1)
ORACLE_CASES = [(n, m) for n in NAMES for m in (1, 2) if (n, m) != TOO_SENSITIVE]


def members_of(pp, comps, n=NMEMBERS):
    """X [n, nvars]: X[0] = x0; X[s], s >= 1: component by component the free variables moved by
    1e-3 (1 + |x0|) N(0, 1) drawn from default_rng(1000 + s); then every row clipped into the domains"""
    X = np.tile(pp.x0, (n, 1))
    for s in range(1, n):
        rng = np.random.default_rng(1000 + s)
        for free, _ in comps:
            X[s, free] = pp.x0[free] + 1e-3 * (1.0 + np.abs(pp.x0[free])) * rng.standard_normal(len(free))
    return np.clip(X, pp.lo, pp.hi)


@functools.lru_cache(maxsize=None)
def members(name):
    pp, comps = S.shape(name)[:2]
    X = members_of(pp, comps)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def oracle_member_reference(name, model, s):
    """lm_oracle.lm_optimize on every component of the shape from member s's x (computed once, shared, not modified)"""
    pp, comps, iters = S.shape(name)[:3]
    return S.oracle_runs(pp, comps, iters, model, x=np.array(members(name)[s]))
