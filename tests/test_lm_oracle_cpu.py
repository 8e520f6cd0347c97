"""The dense Levenberg-Marquardt oracle alone (oracle/lm_oracle.py), on the synthetic problems that
tests/test_gpu_lm.py uses for reduced systems of more than 512 unknowns.  No device code runs here: what is
pinned is that those problems are well enough conditioned for the device comparison's tolerances
(test_gpu_lm._compare: histories 1e-7, x 1e-7, fret 1e-8) to separate a kernel error from the oracle's
own sensitivity to rounding."""
import numpy as np
import pytest

from oracle import lm_oracle as LM
from oracle import oracle as O
from rdis_amd import problems as P

# (cameras, points, cameras per point, iterations): the shapes of test_gpu_lm.test_lm_steps_beyond_512_unknowns
SHAPES = [(58, 400, 6, 8), (64, 400, 6, 8), (120, 700, 6, 4)]


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("nc,npt,k,iters", SHAPES)
def test_lm_oracle_insensitive_to_one_ulp_changes_of_the_start(nc, npt, k, iters, model):
    """The oracle from x0 and from x0 with random one-ulp changes: the same accept / reject decisions, and
    histories, x and fret that differ by at least 100 times less than the device comparison allows
    (measured: history <= 8e-12, x <= 1e-13, fret <= 6e-13).  Also what the device tests state as their
    condition: the run ends at the iteration limit with no converged entry (so the whole history is
    compared) and holds a rejected step (so a re-damped solve is compared)."""
    pp = P.make_synthetic_ba(1, nc, npt, obs_per_pt=k, first_comp=7)
    a = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), maxiters=iters, model=model)
    rng = np.random.default_rng(nc + model)
    x1 = pp.x0 * (1.0 + rng.choice([-1.0, 0.0, 1.0], pp.nvars) * 2.0 ** -52)
    b = LM.lm_optimize(O.OracleProblem(pp, emulate_stale_cache=False), x=x1, maxiters=iters, model=model)
    assert a.stop == 3 and a.iters == iters
    fcur = a.finit
    for _, _, ft, ok in a.history:
        assert abs(ft - fcur) > 1e-11 * abs(fcur)
        if ok:
            fcur = ft
    assert any(not h[3] for h in a.history)
    assert len(a.history) == len(b.history) and [bool(h[3]) for h in a.history] == [bool(h[3]) for h in b.history]
    ha, hb = np.array(a.history, dtype=np.float64)[:, :3], np.array(b.history, dtype=np.float64)[:, :3]
    dev_hist = float(np.max(np.abs(ha - hb) / np.abs(ha)))
    dev_x = float(np.max(np.abs(a.x - b.x)) / (1.0 + np.max(np.abs(a.x))))
    dev_fret = abs(a.fret - b.fret) / abs(a.fret)
    print("LM oracle, %d cameras, model %d, one-ulp changes of x0: history %.1e, x %.1e, fret %.1e; %d rejections" % (
        nc, model, dev_hist, dev_x, dev_fret, sum(not h[3] for h in a.history)))
    assert dev_hist <= 1e-9 and dev_x <= 1e-9 and dev_fret <= 1e-10
