"""The problems tests/test_lm_levels_cpu.py and tests/test_gpu_lm_levels.py run the Levenberg-Marquardt level driver on, and
what their level trees hand a subspace optimiser: per launch of a sweep the (camera blocks, point blocks, factors) of every
component and the class of rdis_amd/csrc/lm_batch.hpp it falls into (0: points only, 1: up to 6 cameras, 2: up to 16, 3: the
wide class, up to 64; 4 here: beyond every plan -- a call of its own)."""
import functools

import numpy as np

from oracle import levels as LV
from oracle import oracle as O
from rdis_amd import problems as P

WIDE_MAX_CAMERAS = 64
BEYOND = 4

# name -> (problem, AVblkpct, sepPiecePct)
CASES = {
    "ladybug-5-30": (("bal", 5, 30), 0.2, 0.0),
    "ladybug-8-30": (("bal", 8, 30), 0.2, 0.0),
    "ladybug-8-300": (("bal", 8, 300), 0.2, 0.0),
    "ladybug-20-120": (("bal", 20, 120), 0.2, 0.0),
    "ladybug-20-120-pieces": (("bal", 20, 120), 0.2, 0.5),
    "ladybug-49-300": (("bal", 49, 300), 0.2, 0.0),
    "synthetic-160-400": (("synthetic", 160, 400), 0.2, 0.0),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    kind, nc, npnt = CASES[name][0]
    return P.load_bal(ncams=nc, npts=npnt) if kind == "bal" else P.make_synthetic_ba(ncomp=1, ncams=nc, npts=npnt)


@functools.lru_cache(maxsize=None)
def plans(name):
    """the launches of a sweep as oracle/levels.py states them: (depth, kind, node indices, free_ptr, free_vid, fac_ptr, fac_id)"""
    pp = problem(name)
    _, pct, seppct = CASES[name]
    return LV.level_plans(LV.build_tree(pp, O.OracleProblem(pp), blkpct=pct, seppct=seppct))


def lm_class(ncameras):
    return 0 if ncameras == 0 else 1 if ncameras <= 6 else 2 if ncameras <= 16 else 3 if ncameras <= WIDE_MAX_CAMERAS else BEYOND


def shapes(name):
    """per launch: (depth, kind, [(camera blocks, point blocks, factors, class) per component])"""
    pp = problem(name)
    ncam_vars = int(pp.pt_vid0.min())
    out = []
    for d, k, _idx, fp, fv, cp, _ci in plans(name):
        comps = []
        for c in range(len(fp) - 1):
            v = fv[fp[c]:fp[c + 1]]
            cams = len(np.unique(v[v < ncam_vars] // 9))
            pts = len(np.unique((v[v >= ncam_vars] - ncam_vars) // 3))
            comps.append((cams, pts, int(cp[c + 1] - cp[c]), lm_class(cams)))
        out.append((d, k, comps))
    return out
