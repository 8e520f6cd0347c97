"""The batched population evaluation and the selection on the device, without a GPU: the entry points are exported, bound and
refuse NULL handles; rdis_amd/csrc/population_grid.hpp's members-per-launch rule holds its properties over a grid of arguments
(tests/cpp/population_eval_members_test.cpp: at least 1; never above the members or 65535; monotone in the budget; a budget
below one member's bytes gives 1; the rotation records are counted only on the records branch) and the cases the program
prints are compared with the rule restated."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from rdis_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rdis_hip_population_eval_device", "rdis_hip_population_best", "rdis_hip_population_assign_best",
       "rdis_hip_population_set_option", "rdis_hip_population_get_info")


def test_symbols_and_null_handles():
    for name in NEW + ("rdis_hip_population_eval",):
        assert name in capi.SYMBOLS, name
    with open(os.path.join(ROOT, "include", "rdis_hip.h")) as fh:
        header = fh.read()
    for name in NEW:
        assert "int %s(" % name in header, name
    for method in ("eval", "eval_device", "best", "assign_best", "set_option", "info"):
        assert callable(getattr(capi.Population, method)), method
    lib = capi.load_library()                       # (binds every symbol of SYMBOLS: AttributeError if one is not exported)
    fd, member, f, v = C.c_void_p(), C.c_int64(), C.c_double(), C.c_int64()
    assert lib.rdis_hip_population_eval_device(None, 0, None, C.byref(fd)) == -1
    assert lib.rdis_hip_population_best(None, C.byref(member), C.byref(f)) == -1
    assert lib.rdis_hip_population_assign_best(None) == -1
    assert lib.rdis_hip_population_set_option(None, b"eval_batched", 1) == -1
    assert lib.rdis_hip_population_get_info(None, b"eval_launches", C.byref(v)) == -1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("population_eval") / "population_eval_members_test")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "population_eval_members_test.cpp")],
                          stderr=subprocess.DEVNULL)
    return out


def test_members_per_launch(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr          # (the program's own checks of the properties)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok"
    cases = [tuple(int(t) for t in ln.split()[1:]) for ln in lines[:-1]]
    assert len(cases) >= 10
    for members, budget, partials, nvars, records, got in cases:
        per = 8 * (partials + (nvars if records else 0))
        want = min(members, 65535, max(1, budget // per))
        assert got == want >= 1, (members, budget, partials, nvars, records, got, want)
    # full ladybug, all factors (63 chunks, 23769 variables, the records branch): a budget of two members' bytes holds two, one
    # byte less holds one; 256 members of ladybug 5 / 30 go in one launch by default
    per = 8 * (63 + 23769)
    assert (5, 2 * per, 63, 23769, 1, 2) in cases and (5, 2 * per - 1, 63, 23769, 1, 1) in cases
    assert (256, 1 << 30, 1, 135, 1, 256) in cases
    assert (1000000, 1 << 30, 1, 135, 0, 65535) in cases
