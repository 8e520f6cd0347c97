"""Levenberg-Marquardt plans (rdis_hip_lm_plan; include/rdis_hip.h) without a GPU: the library exports the entries, the
two buffers of a solve are laid out as rdis_amd/csrc/replica_layout.hpp's lm_plan_layout says (tests/cpp/lm_plan_layout_test.cpp),
and the dense oracle (oracle/lm_oracle.py) is insensitive enough to rounding at the perturbed starts of
tests/lm_plan_members.py to serve as the reference of tests/test_gpu_lm_plan.py's comparison."""
import os
import subprocess

import numpy as np
import pytest

from rdis_amd import capi

import lm_batch_shapes as S
import lm_plan_members as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["rdis_hip_lm_plan_create", "rdis_hip_lm_plan_destroy", "rdis_hip_lm_plan_solve", "rdis_hip_lm_plan_fetch",
           "rdis_hip_lm_plan_solve_population", "rdis_hip_lm_plan_fetch_population", "rdis_hip_lm_plan_set_option",
           "rdis_hip_lm_plan_get_info"]


def test_library_exports_the_plan_entries():
    lib = capi.load_library()
    for name in ENTRIES:
        assert name in capi.SYMBOLS
        assert getattr(lib, name) is not None
    assert lib.rdis_hip_lm_plan_create(None, 0, None, None, None, None, 1, 0, None) == -1
    assert lib.rdis_hip_lm_plan_solve(None, 5, 1e-8) == -1
    assert lib.rdis_hip_lm_plan_fetch(None, None, None, None, None, None, None) == -1
    assert lib.rdis_hip_lm_plan_solve_population(None, None, 0, 1, 5, 1e-8) == -1
    assert lib.rdis_hip_lm_plan_fetch_population(None, None, None, None, None, None, None) == -1
    assert lib.rdis_hip_lm_plan_set_option(None, b"workspace_bytes", 0) == -1
    assert lib.rdis_hip_lm_plan_get_info(None, b"launches", None) == -1
    lib.rdis_hip_lm_plan_destroy(None)
    assert hasattr(capi, "LmPlan")


def test_layout_of_a_plans_buffers(tmp_path):
    """the program's own checks (order, no overlap, 8-byte alignment, total = parts, members_per_launch at budgets of
    nothing, one member and count members), and every figure it prints against the same arithmetic written out here"""
    exe = str(tmp_path / "lm_plan_layout_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lm_plan_layout_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    rows = out.stdout.splitlines()
    assert rows[-1] == "ok" and len(rows) == 7
    for row in rows[:-1]:
        w = row.split()
        assert w[0] == "lmplan"
        nc, rd, cap, nfr, ws, n, r, member, total, o_res, o_hist, o_x, s_res, s_hist, s_x, work_total, s_ws = (int(v) for v in w[1:])
        assert rd == 12
        assert member == nc * 12 * 8 + nc * cap * 4 * 8 + nfr * 8            # a member's result rows, history and x
        assert total == n * member                                           # ... for every member of the solve
        assert (o_res, o_hist, o_x) == (0, n * nc * 12 * 8, n * nc * (12 + 4 * cap) * 8)   # [n][ncomp][12], [n][ncomp][cap][4], [n][nfree]
        assert (s_res, s_hist, s_x) == (nc * 12, nc * cap * 4, nfr)          # the member strides the kernel is handed, in doubles
        assert (work_total, s_ws) == (r * ws * 8, ws)                        # workspace: the members of one launch only


@pytest.mark.parametrize("name,model", M.ORACLE_CASES)
def test_lm_oracle_at_the_perturbed_starts_insensitive_to_one_ulp_changes(name, model):
    """tests/test_lm_batch_oracle_cpu.py's criterion at members 1 to 3 of tests/lm_plan_members.py: the oracle from X[s] and from
    X[s] with random one-ulp changes of the free start takes the same accept / reject decisions in every component, histories and
    x differ by at most 1e-9 and fret by at most 1e-10 (100 times below what the device comparison allows), and no history is
    truncated by convergence.
    synthetic-6x3x40 with model 1 is left out (lm_plan_members.TOO_SENSITIVE): from the perturbed starts its fret moves by up to
    7.6e-10 under one-ulp changes, beyond the 1e-10 this criterion asks, so it is no reference for the device comparison either.
    Worst of the rest, with that test's generator for the one-ulp changes: history 6.2e-10 (ladybug 5/30 whole, model 1),
    x 2.8e-14, fret 1.2e-11."""
    pp, comps, iters = S.shape(name)[:3]
    X = M.members(name)
    worst = np.zeros(3)
    for s in range(1, M.NMEMBERS):
        a = M.oracle_member_reference(name, model, s)
        rng = np.random.default_rng(len(comps) + model)                      # (that test's generator, for every member)
        x1 = np.array(X[s])
        for free, _ in comps:
            x1[free] = X[s, free] * (1.0 + rng.choice([-1.0, 0.0, 1.0], len(free)) * 2.0 ** -52)
        b = S.oracle_runs(pp, comps, iters, model, x=x1)
        for ra, rb in zip(a, b):
            assert S.converged_at(ra) == len(ra.history)                       # nothing truncated by convergence
            assert (ra.stop, ra.iters) == (rb.stop, rb.iters)
            assert [bool(h[3]) for h in ra.history] == [bool(h[3]) for h in rb.history]
            if ra.history:
                ha, hb = np.array(ra.history, dtype=np.float64)[:, :3], np.array(rb.history, dtype=np.float64)[:, :3]
                worst[0] = max(worst[0], float(np.max(np.abs(ha - hb) / np.abs(ha))))
            worst[1] = max(worst[1], float(np.max(np.abs(ra.x - rb.x)) / (1.0 + np.max(np.abs(ra.x)))))
            if ra.fret != rb.fret:
                worst[2] = max(worst[2], abs(ra.fret - rb.fret) / abs(ra.fret))
    print("LM oracle, %s, model %d, members 1-3, one-ulp changes of the start: history %.1e, x %.1e, fret %.1e" % ((name, model) + tuple(worst)))
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9 and worst[2] <= 1e-10


def test_members_differ_and_lie_inside_the_domains():
    for name in M.NAMES:
        pp, comps = S.shape(name)[:2]
        X = M.members(name)
        assert X.shape == (M.NMEMBERS, pp.nvars) and X[0].tobytes() == np.clip(pp.x0, pp.lo, pp.hi).tobytes()
        assert np.all(X >= pp.lo) and np.all(X <= pp.hi)
        free = np.concatenate([f for f, _ in comps])
        rest = np.setdiff1d(np.arange(pp.nvars), free)
        for s in range(1, M.NMEMBERS):
            assert X[s, rest].tobytes() == X[0, rest].tobytes()
            for t in range(s):
                assert np.count_nonzero(X[s, free] != X[t, free]) > 0.9 * len(free)
