"""rdis_amd/csrc/plan_tables.hpp -- the host functions that build every index table a plan's solvers read -- without a GPU:
tests/cpp/plan_tables_test.hip runs them on small components and checks the tables' structure; here its output is compared
with the independent restatements of the same rules in oracle/oracle.py."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("plan_tables") / "plan_tables_test")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "plan_tables_test.hip")], stderr=subprocess.DEVNULL)
    return out


def _run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr          # (the program's own structural checks)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok"
    return {ln.split()[0]: np.array(ln.split()[1:], dtype=np.int64) for ln in lines[:-1]}


@pytest.mark.parametrize("how", ["spread", "wide"])
def test_point_major_order_of_a_small_component(exe, how):
    """6 cameras, 200 points of 2 .. 4 observations (three full wave-chunks and a partial one, several runs of equal slot
    count): exactly oracle.ptm_point_order, dealt round robin and as for a wide group"""
    t = _run(exe, "order", 6, 200, 2, 4, how, 0)
    assert t["fits"][0] == 1
    cams, pts = O.ptm_point_order(t["factor_cam"], t["factor_pt"], wide=(how == "wide"))
    assert len(pts) == 200 and len(np.unique(np.bincount(np.unique(t["factor_pt"], return_inverse=True)[1]))) > 1
    assert np.array_equal(t["cams"], cams)
    assert np.array_equal(t["pts"], pts)


def test_point_major_order_of_a_local_group(exe):
    """30 cameras, 26 500 points of 2 observations, 32 compute units: 415 chunks, 17 workgroups -- the order and the
    workgroups' chunk ranges are oracle.ptm_point_order(..., local_cus=32)'s; 300 chunks are too few for a local group"""
    t = _run(exe, "order", 30, 26500, 2, 2, "local", 32)
    assert t["fits"][0] == 1 and t["local_K"][0] == 17
    cams, pts, wg_chunk0 = O.ptm_point_order(t["factor_cam"], t["factor_pt"], local_cus=32)
    assert np.array_equal(t["cams"], cams)
    assert np.array_equal(t["pts"], pts)
    assert np.array_equal(t["wg_chunk0"], wg_chunk0)
    assert _run(exe, "order", 30, 19200, 2, 2, "local", 32)["fits"][0] == 0


def test_wave_owners_of_a_cooperative_group(exe, monkeypatch):
    """one free camera under 200 factors and a free point: the nine camera variables (more than COOP_LONG_LIST = 48 partials
    each) are wave-owned, longest first and ties in list order, every other variable lane-owned -- the variables
    oracle.OracleProblem.set_cooperative_topology picks; with fewer waves than long lists the first of them"""
    t = _run(exe, "owners")
    assert t["long_list"][0] == 48
    fv, fcam, fpt = t["free_vid"], t["factor_cam"], t["factor_pt"]
    # the oracle's rule, run on this component; what it would hand to its C library is caught
    got = {}

    class Lib:
        @staticmethod
        def ro_set_sum_topology(h, mode, count, ptr):
            got["wave"] = np.ctypeslib.as_array((O.C.c_int64 * count).from_address(ptr.value)).copy() if count else np.zeros(0, np.int64)

    monkeypatch.setattr(O, "lib", lambda: Lib)
    pp = types.SimpleNamespace(nvars=int(max(fcam.max() + 9, fpt.max() + 3)), nfac=len(fcam), cam_vid0=fcam, pt_vid0=fpt)
    O.OracleProblem.set_cooperative_topology(types.SimpleNamespace(pp=pp, h=None), free_vid=fv, lanes_per_workgroup=128)
    wave = t["wave_var_640"]
    assert len(wave) == 10 and np.array_equal(fv[wave[:9]], got["wave"]) and np.all(wave[9:] == -1)
    assert np.array_equal(wave[:9], np.arange(9))                     # equal lengths: list order
    lane = t["lane_var_640"]
    assert np.array_equal(lane[:12], [-1] * 9 + [9, 10, 11]) and np.all(lane[12:] == -1)
    assert np.array_equal(t["wave_var_128"], [0, 1])
    assert np.array_equal(t["lane_var_128"][:12], [-1, -1] + list(range(2, 12))) and np.all(t["lane_var_128"][12:] == -1)
    # the local free index of every factor slot
    where = {int(v): i for i, v in enumerate(fv)}
    want = np.array([[where.get(int(c) + k, -1) for k in range(9)] + [where.get(int(q) + k, -1) for k in range(3)] for c, q in zip(fcam, fpt)]).ravel()
    assert np.array_equal(t["slot_li"], want)
