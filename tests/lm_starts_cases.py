"""What the tests of the Levenberg-Marquardt plan's multi-start solve share (tests/test_lm_starts_cpu.py: the inputs
discriminate; tests/test_gpu_lm_starts.py: the device): the starts of a shape of tests/lm_batch_shapes.py -- the six rows of
lm_plan_members.members_of, of which a start is the plan's free variables -- and the select rule written with numpy."""
import functools

import numpy as np

import lm_batch_shapes as S
import lm_plan_members as M

NSTARTS = 6

# the shapes whose winners are compared with the oracle's (model 1): tests/test_lm_starts_cpu.py pins that they discriminate
ORACLE_NAMES = ["ladybug-5-30-points", "ladybug-5-30-cameras", "synthetic-6x3x40", "synthetic-2x16x60"]


@functools.lru_cache(maxsize=None)
def rows(name, n=NSTARTS):
    """X [n, nvars]: complete states (row 0 the problem's start), read-only; the starts are X[:, free_vid]"""
    pp, comps = S.shape(name)[:2]
    X = M.members_of(pp, comps, n)
    X.setflags(write=False)
    return X


def select(fret):
    """best[ncomp] of fret[nstarts, ncomp]: the lowest value, the lowest index on a tie (-0.0 against +0.0 is one), a NaN never
    unless the whole column is NaN: then 0"""
    fret = np.asarray(fret, dtype=np.float64)
    best = np.zeros(fret.shape[1], dtype=np.int32)
    for c, col in enumerate(fret.T):
        numbers = np.flatnonzero(~np.isnan(col))
        if len(numbers):
            best[c] = numbers[np.argmin(col[numbers])]      # (argmin: the first of equal values)
    return best


@functools.lru_cache(maxsize=None)
def oracle_frets(name, model):
    """fret [NSTARTS, ncomp] of lm_oracle.lm_optimize from every start (computed once, shared)"""
    pp, comps, iters = S.shape(name)[:3]
    X = rows(name)
    f = np.array([[r.fret for r in S.oracle_runs(pp, comps, iters, model, x=np.array(X[s]))] for s in range(NSTARTS)])
    f.setflags(write=False)
    return f


def smallest_gap(fret):
    """the smallest relative distance between the best and the second value of a column"""
    f = np.sort(np.asarray(fret), axis=0)
    return float(np.min((f[1] - f[0]) / np.abs(f[0])))
