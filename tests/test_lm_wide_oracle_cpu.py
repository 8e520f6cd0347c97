"""The wide class of the batched Levenberg-Marquardt entry without a device: the dense oracle alone (oracle/lm_oracle.py)
on the shapes of tests/test_gpu_lm_wide.py (tests/lm_wide_shapes.py), the host tables of class 3
(tests/cpp/lm_wide_prepare_test.cpp) and the option's constants in the binding.  What the first pins is that the shapes
are well enough conditioned for the device comparison's tolerances (test_gpu_lm_batch._compare: histories 1e-7, x 1e-7,
fret 1e-8) to separate a kernel error from the oracle's own sensitivity to rounding."""
import os
import re
import subprocess

import numpy as np
import pytest

from rdis_amd import capi

import lm_wide_shapes as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,model", W.CASES)
def test_lm_oracle_on_wide_shapes_insensitive_to_one_ulp_changes_of_the_start(name, model):
    """The oracle from x0 and from x0 with random one-ulp changes of the free start: the same accept / reject decisions
    in every component, histories, x and fret that differ at least 100 times less than the device comparison allows,
    no history truncated by convergence, and a rejected step (a re-damped solve) in every case.
    Measured (history / x / fret; rejected steps), model 1 and model 2:
      synthetic 1 x (17, 60), 6 iterations      3.3e-12 / 5.4e-16 / 3.1e-12; 4      1.2e-12 / 2.3e-14 / 2.4e-14; 2
      synthetic 2 x (33, 90), 5                 2.2e-12 / 5.7e-16 / 4.8e-13; 6      2.6e-12 / 8.2e-14 / 8.0e-13; 4
      synthetic 1 x (64, 120), 4                6.2e-13 / 1.2e-15 / 2.8e-13; 1      1.2e-12 / 6.2e-14 / 4.3e-14; 2
      ladybug 21/120 whole, 8                   2.1e-13 / 2.8e-16 / 1.9e-15; 4      2.2e-12 / 1.1e-14 / 2.7e-14; 2
      ladybug 49/300 whole, 6                   2.8e-13 / 2.8e-16 / 3.7e-14; 4      1.1e-11 / 1.1e-12 / 1.1e-13; 2"""
    pp, comps, iters, _, _, rejected = W.shape(name)
    a = W.oracle_reference(name, model)
    rng = np.random.default_rng(len(comps) + model)
    x1 = pp.x0.copy()
    for free, _ in comps:
        x1[free] = pp.x0[free] * (1.0 + rng.choice([-1.0, 0.0, 1.0], len(free)) * 2.0 ** -52)
    b = W.oracle_runs(pp, comps, iters, model, x=x1)
    dev_hist = dev_x = dev_fret = 0.0
    nrej = 0
    for ra, rb in zip(a, b):
        assert W.converged_at(ra) == len(ra.history)                           # nothing truncated by convergence
        assert (ra.stop, ra.iters) == (rb.stop, rb.iters)
        assert [bool(h[3]) for h in ra.history] == [bool(h[3]) for h in rb.history]
        nrej += sum(not h[3] for h in ra.history)
        ha, hb = np.array(ra.history, dtype=np.float64)[:, :3], np.array(rb.history, dtype=np.float64)[:, :3]
        dev_hist = max(dev_hist, float(np.max(np.abs(ha - hb) / np.abs(ha))))
        dev_x = max(dev_x, float(np.max(np.abs(ra.x - rb.x)) / (1.0 + np.max(np.abs(ra.x)))))
        if ra.fret != rb.fret:
            dev_fret = max(dev_fret, abs(ra.fret - rb.fret) / abs(ra.fret))
    print("LM oracle, %s, model %d, one-ulp changes of the start: history %.1e, x %.1e, fret %.1e; %d rejections" % (
        name, model, dev_hist, dev_x, dev_fret, nrej))
    assert dev_hist <= 1e-9 and dev_x <= 1e-9 and dev_fret <= 1e-10
    assert (nrej > 0) == rejected[model]


def test_host_tables_of_the_wide_class(tmp_path):
    """rdis_amd/csrc/lm_batch.hpp without a device -- class 3's limits, its tiles appended to the slice, the LDS bound, the
    tables and order of a 17- and a 64-camera component written out by hand, the refusals at 65 with the option and at 17
    without, and a 16-camera component's pair order equal to what the call without the option builds
    (tests/cpp/lm_wide_prepare_test.cpp)"""
    exe = str(tmp_path / "lm_wide_prepare_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lm_wide_prepare_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_the_binding_exports_the_options_constants():
    """capi.LM_WIDE and capi.LM_WIDE_MAX_CAMERAS are include/rdis_hip.h's, and the bit lies outside the model's and
    rdis_hip_lm_optimize's Schur bits"""
    with open(os.path.join(ROOT, "include", "rdis_hip.h")) as f:
        header = f.read()
    defines = {k: int(v, 0) for k, v in re.findall(r"^#define (RDIS_HIP_LM_\w+) (\w+)$", header, flags=re.M)}
    assert capi.LM_WIDE == defines["RDIS_HIP_LM_WIDE"] == 0x100
    assert capi.LM_WIDE_MAX_CAMERAS == defines["RDIS_HIP_LM_WIDE_MAX_CAMERAS"] == 64
    assert defines["RDIS_HIP_LM_BATCH_MAX_CAMERAS"] == 16
    assert capi.LM_WIDE & 0x3f == 0
