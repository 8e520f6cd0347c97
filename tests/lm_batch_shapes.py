"""The component shapes the batched Levenberg-Marquardt entry (rdis_hip_lm_batch) is checked on, shared by
tests/test_lm_batch_oracle_cpu.py (the oracle's own sensitivity on them) and tests/test_gpu_lm_batch.py (the device
against the oracle).  A shape: a problem, a list of independent components (free variable ids, factor ids), the
iteration limit, the residual models it is used with, the active camera / point blocks of each of its components, and
for each model whether the oracle's runs hold a rejected step."""
import functools

import numpy as np

from oracle import lm_oracle as LM
from oracle import oracle as O
from rdis_amd import problems as P


def _i(a):
    return np.asarray(a, dtype=np.int64)


def _whole(pp):
    return [(np.arange(pp.nvars, dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))]


def _each_point(pp, ncams):
    npts = (pp.nvars - 9 * ncams) // 3
    return [(9 * ncams + 3 * p + np.arange(3, dtype=np.int64), _i(np.where(pp.pt_vid0 == 9 * ncams + 3 * p)[0])) for p in range(npts)]


def _each_camera(pp, ncams):
    return [(9 * c + np.arange(9, dtype=np.int64), _i(np.where(pp.cam_vid0 == 9 * c)[0])) for c in range(ncams)]


def _synthetic_components(pp, ncomp):
    nv, nf = pp.nvars // ncomp, pp.nfac // ncomp
    return [(c * nv + np.arange(nv, dtype=np.int64), c * nf + np.arange(nf, dtype=np.int64)) for c in range(ncomp)]


def _sub_block(pp):
    free = np.concatenate([np.arange(0, 6), np.arange(27, 36), np.arange(45, 75)]).astype(np.int64)
    return [(free, _i(np.where(pp.pt_vid0 < 75)[0]))]


# name: (problem, components, iterations, models, (camera blocks, point blocks) of a component, {model: a rejected step})
@functools.lru_cache(maxsize=None)
def shape(name):
    if name == "ladybug-5-30-whole":
        pp = P.load_bal(ncams=5, npts=30)
        return pp, _whole(pp), 25, (1, 2), (5, 30), {1: True, 2: True}
    if name == "ladybug-5-30-points":
        pp = P.load_bal(ncams=5, npts=30)
        return pp, _each_point(pp, 5), 3, (1, 2), (0, 1), {1: True, 2: False}
    if name == "ladybug-5-30-cameras":
        pp = P.load_bal(ncams=5, npts=30)
        return pp, _each_camera(pp, 5), 8, (1, 2), (1, 0), {1: True, 2: True}
    if name == "ladybug-5-30-sub-block":
        pp = P.load_bal(ncams=5, npts=30)
        return pp, _sub_block(pp), 15, (1, 2), (2, 10), {1: True, 2: True}
    if name == "synthetic-6x3x40":
        pp = P.make_synthetic_ba(6, 3, 40, first_comp=7)
        return pp, _synthetic_components(pp, 6), 5, (1, 2), (3, 40), {1: True, 2: True}
    if name == "synthetic-2x16x60":
        pp = P.make_synthetic_ba(2, 16, 60, obs_per_pt=6, first_comp=3)
        return pp, _synthetic_components(pp, 2), 6, (1, 2), (16, 60), {1: True, 2: True}
    if name == "ladybug-16-60-whole":
        pp = P.load_bal(ncams=16, npts=60)
        return pp, _whole(pp), 10, (1, 2), (16, 60), {1: True, 2: True}
    if name == "ladybug-49-300-cameras":
        pp = P.load_bal(ncams=49, npts=300)
        return pp, _each_camera(pp, 49), 4, (1,), (1, 0), {1: True}
    raise KeyError(name)


NAMES = ["ladybug-5-30-whole", "ladybug-5-30-points", "ladybug-5-30-cameras", "ladybug-5-30-sub-block", "synthetic-6x3x40",
         "synthetic-2x16x60", "ladybug-16-60-whole", "ladybug-49-300-cameras"]
CASES = [(n, m) for n in NAMES for m in ((1, 2) if n != "ladybug-49-300-cameras" else (1,))]


def csr(comps):
    """(free_ptr, free_vid, fac_ptr, fac_id) of a list of (free, fac)"""
    fp = np.concatenate([[0], np.cumsum([len(f) for f, _ in comps])]).astype(np.int64)
    jp = np.concatenate([[0], np.cumsum([len(j) for _, j in comps])]).astype(np.int64)
    fv = np.concatenate([f for f, _ in comps]).astype(np.int64) if comps else np.zeros(0, np.int64)
    fj = np.concatenate([j for _, j in comps]).astype(np.int64) if comps else np.zeros(0, np.int64)
    return fp, fv, jp, fj


def oracle_runs(pp, comps, iters, model, x=None):
    """the reference of every comparison: lm_oracle.lm_optimize component by component (the components are independent:
    one oracle problem serves them all), from x (all variables; default the problem's start)"""
    x = pp.x0 if x is None else x
    o = O.OracleProblem(pp, emulate_stale_cache=False)
    o.assign(None, x)
    return [LM.lm_optimize(o, free, fac, x=x[free], maxiters=iters, model=model) for free, fac in comps]


@functools.lru_cache(maxsize=None)
def oracle_reference(name, model):
    pp, comps, iters, _, _, _ = shape(name)
    return oracle_runs(pp, comps, iters, model)


def converged_at(ro):
    """index of the first history entry whose trial objective equals the current one to 1e-11 (where _compare stops
    comparing histories), or len(history)"""
    fcur = ro.finit
    for i, (_, _, ft, ok) in enumerate(ro.history):
        if abs(ft - fcur) <= 1e-11 * abs(fcur):
            return i
        if ok:
            fcur = ft
    return len(ro.history)
