"""The pipelined solver's stepper (rdis_amd/csrc/solver_pipe.hpp) takes Brent's trials in two parts: CgdMachine::hot_pre, the
part of the step that does not read the reply (formed while the sums travel), and CgdMachine::hot_post.  Together they must be
CgdMachine::hot() bit for bit -- decision, next trial step, new state, counters -- on the host and on the device
(tests/cpp/hot_split_test.hip).  And on the GPU, speculation and trace records must not move a bit of the pipelined solve, on
one group (cgd_pipe_single_kernel) and on several (cgd_pipe_kernel)."""
import os
import re
import subprocess

import numpy as np
import pytest

from rdis_amd import capi, problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "hot_split_test.hip")


def _build(tmp_path):
    exe = str(tmp_path / "hot_split_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, SRC],
                          stderr=subprocess.DEVNULL)
    return exe


def _run(exe, where, n, seed):
    out = subprocess.run([exe, where, str(n), str(seed)], capture_output=True, text=True, timeout=600)
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", out.stdout)}
    assert out.returncode == 0 and counts.get("bad") == 0, (out.returncode, out.stdout, out.stderr)
    assert counts["cases"] == n
    # every branch of the step is exercised: both classes of reply, both updates of the worse one, NaN replies, and each way
    # hot() declines (convergence, the iteration limit, a minimal step that went uphill), secant steps taken
    for k in ("taken", "le", "c1", "c2", "nan", "conv", "itmax", "tiny", "accept"):
        assert counts[k] > n // 1000, (k, counts)
    return counts


def test_split_step_is_hot_bit_for_bit_on_the_host(tmp_path):
    exe = _build(tmp_path)
    _run(exe, "host", 1_000_000, 1)
    _run(exe, "host", 1_000_000, 0x5EED)


@pytest.mark.gpu
def test_split_step_is_hot_bit_for_bit_on_the_device(tmp_path):
    exe = _build(tmp_path)
    _run(exe, "device", 4_000_000, 3)


def _whole(pp):
    return (np.array([0, pp.nvars]), np.arange(pp.nvars, dtype=np.int64), np.array([0, pp.nfac]), np.arange(pp.nfac, dtype=np.int64))


@pytest.mark.gpu
def test_pipelined_solve_is_the_same_with_and_without_guesses_and_trace(gctx):
    """coop_speculate 0 / 1 x trace_records on / off: the same fret, x, iterations, status, call counts, and (where recorded) the
    same trace -- full ladybug as one group, and five components on a multi-group launch"""
    lb = P.load_bal().single_component()
    syn = P.make_synthetic_ba(5, 3, 900, obs_per_pt=3)
    cases = (("ladybug", lb, _whole(lb), {}, 25),
             ("five groups", syn, (syn.comp_free_ptr, syn.comp_free_vid, syn.comp_fac_ptr, syn.comp_fac_id), {"coop_min_factors": 1000}, 10))
    for name, pp, comps, opts, iters in cases:
        g = capi.Problem(gctx, pp)
        ncomp = len(comps[0]) - 1
        runs = {}
        for spec in (1, 0):
            for traced in (True, False):
                g.set_x(pp.x0)
                plan = capi.Plan(g, *comps)
                for k, v in {**opts, "coop_speculate": spec}.items():
                    plan.set_option(k, v)
                if traced:
                    plan.set_option("trace_records", 4096)
                plan.set_start(None)
                plan.solve(iters, 3e-8)
                r = plan.fetch()
                assert plan.info("pipelined") == 1, name
                assert np.all((r.status & 0xFF) != 7), (name, spec, traced)      # no exchange gave up
                tr = [plan.get_trace(c, 4096) for c in range(ncomp)] if traced else None
                runs[(spec, traced)] = (r, g.get_x(), tr)
                plan.close()
        ra, xa, ta = runs[(1, True)]
        assert np.all(ra.delta < 0) and np.all(ra.nfeval > 20), name
        for key, (rb, xb, tb) in runs.items():
            assert np.array_equal(ra.fret, rb.fret) and np.array_equal(ra.x, rb.x) and np.array_equal(xa, xb), (name, key)
            assert np.array_equal(ra.iters, rb.iters) and np.array_equal(ra.status, rb.status), (name, key)
            assert np.array_equal(ra.nfeval, rb.nfeval) and np.array_equal(ra.ngeval, rb.ngeval), (name, key)
            if tb is not None:
                for (tra, ca), (trb, cb) in zip(ta, tb):
                    assert ca == cb > 0 and np.array_equal(tra[:min(ca, 4096)], trb[:min(cb, 4096)]), (name, key)
