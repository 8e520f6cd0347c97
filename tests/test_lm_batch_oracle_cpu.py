"""The dense Levenberg-Marquardt oracle alone (oracle/lm_oracle.py) on the component shapes of
tests/test_gpu_lm_batch.py (tests/lm_batch_shapes.py), component by component.  No device code runs here: what is
pinned is that those shapes are well enough conditioned for the device comparison's tolerances (_compare: histories
1e-7, x 1e-7, fret 1e-8) to separate a kernel error from the oracle's own sensitivity to rounding -- and that the
library exports the batch entry at all."""
import numpy as np
import pytest

from rdis_amd import capi

import lm_batch_shapes as S


@pytest.mark.parametrize("name,model", S.CASES)
def test_lm_oracle_on_batch_shapes_insensitive_to_one_ulp_changes_of_the_start(name, model):
    """The oracle from x0 and from x0 with random one-ulp changes of the free start: the same accept / reject decisions
    in every component, and histories, x and fret that differ at least 100 times less than the device comparison allows.
    No history is truncated by convergence (the device comparison sees every solve), and where the shape says so the
    runs hold a rejected step (a re-damped solve is compared).
    Measured (history / x / fret; rejected steps), model 1 and model 2:
      ladybug 5/30 whole (25 iterations)            5.8e-11 / 2.8e-16 / 2.3e-13; 3      1.6e-11 / 5.1e-15 / 2.6e-14; 2
      ... each point alone (30 components; 3)       7.5e-11 / 2.5e-15 / 3.2e-12; 84     5.7e-11 / 1.8e-14 / 1.8e-13; 0
      ... each camera alone (5; 8)                  2.9e-12 / 2.8e-16 / 4.9e-13; 19     1.2e-10 / 4.2e-16 / 6.0e-14; 16
      ... the sub-block with constants (1; 15)      3.4e-11 / 2.8e-16 / 1.2e-12; 6      2.7e-11 / 1.1e-16 / 9.0e-15; 1
      synthetic 6 x (3, 40) (6; 5)                  1.4e-11 / 7.6e-15 / 1.4e-11; 17     2.1e-12 / 3.6e-15 / 2.8e-13; 17
      synthetic 2 x (16, 60), the size limit (2; 6) 3.6e-12 / 1.4e-15 / 3.6e-12; 4      2.5e-12 / 1.1e-14 / 7.2e-14; 4
      ladybug 16/60 whole, 463 factors (1; 10)      9.1e-13 / 2.8e-16 / 8.4e-13; 2      1.5e-12 / 4.4e-15 / 2.0e-14; 3
      ladybug 49/300, each camera alone (49; 4)     1.7e-10 / 2.9e-16 / 6.3e-12; 127    not used (too sensitive: 3.6e-9)"""
    pp, comps, iters, _, _, rejected = S.shape(name)
    a = S.oracle_reference(name, model)
    rng = np.random.default_rng(len(comps) + model)
    x1 = pp.x0.copy()
    for free, _ in comps:
        x1[free] = pp.x0[free] * (1.0 + rng.choice([-1.0, 0.0, 1.0], len(free)) * 2.0 ** -52)
    b = S.oracle_runs(pp, comps, iters, model, x=x1)
    dev_hist = dev_x = dev_fret = 0.0
    nrej = 0
    for ra, rb in zip(a, b):
        assert S.converged_at(ra) == len(ra.history)                           # nothing truncated by convergence
        assert (ra.stop, ra.iters) == (rb.stop, rb.iters)
        assert [bool(h[3]) for h in ra.history] == [bool(h[3]) for h in rb.history]
        nrej += sum(not h[3] for h in ra.history)
        if ra.history:
            ha, hb = np.array(ra.history, dtype=np.float64)[:, :3], np.array(rb.history, dtype=np.float64)[:, :3]
            dev_hist = max(dev_hist, float(np.max(np.abs(ha - hb) / np.abs(ha))))
        dev_x = max(dev_x, float(np.max(np.abs(ra.x - rb.x)) / (1.0 + np.max(np.abs(ra.x)))))
        if ra.fret != rb.fret:
            dev_fret = max(dev_fret, abs(ra.fret - rb.fret) / abs(ra.fret))
    print("LM oracle, %s, model %d, one-ulp changes of the start: history %.1e, x %.1e, fret %.1e; %d rejections" % (
        name, model, dev_hist, dev_x, dev_fret, nrej))
    assert dev_hist <= 1e-9 and dev_x <= 1e-9 and dev_fret <= 1e-10
    assert (nrej > 0) == rejected[model]


def test_empty_components_of_the_camera_plan_end_with_stop_6():
    """of ladybug 49 / 300's cameras three see none of the 300 points: components with an empty factor list, which the
    oracle ends with stop 6, no iteration, fret 0 and x = clamp(start)"""
    pp, comps, _, _, _, _ = S.shape("ladybug-49-300-cameras")
    runs = S.oracle_reference("ladybug-49-300-cameras", 1)
    empty = [c for c, (_, fac) in enumerate(comps) if len(fac) == 0]
    assert len(empty) == 3 and max(len(fac) for _, fac in comps) == 300
    for c in empty:
        r, free = runs[c], comps[c][0]
        assert (r.stop, r.iters, r.fret, len(r.history)) == (6, 0, 0.0, 0)
        assert np.array_equal(r.x, np.minimum(np.maximum(pp.x0[free], pp.lo[free]), pp.hi[free]))


def test_host_tables_of_the_batch_entry(tmp_path):
    """rdis_amd/csrc/lm_batch.hpp without a device -- the classes and their LDS, the workspace slice, and lm_batch_prepare's
    tables, order and refusals on problems written out by hand (tests/cpp/lm_batch_prepare_test.cpp)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lm_batch_prepare_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "lm_batch_prepare_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_library_exports_the_batch_entry():
    assert "rdis_hip_lm_batch" in capi.SYMBOLS
    lib = capi.load_library()
    assert getattr(lib, "rdis_hip_lm_batch") is not None
    assert lib.rdis_hip_lm_batch(None, 0, None, None, None, None, None, 1, 1e-8, 1, None, None, None, None, 0, None) == -1
