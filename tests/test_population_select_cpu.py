"""Drawing, ranking and solving a member range of a population, without a GPU: the four entry points are exported, bound,
declared and refuse NULL handles, the Python methods exist; rdis_amd/csrc/population_select.hpp's draw equals
oracle.levels.splitmix_restart_value bit for bit over a grid (tests/cpp/population_select_test.cpp prints it), better() is a
strict total order (the program's own checks) and rank by counting with it is the permutation sorted() gives under the rule
restated."""
import ctypes as C
import inspect
import os
import shutil
import struct
import subprocess

import pytest

from oracle.levels import splitmix_restart_value
from rdis_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rdis_hip_population_set_sampling", "rdis_hip_population_sample", "rdis_hip_population_sort",
       "rdis_hip_plan_solve_population_range")


def test_symbols_and_null_handles():
    for name in NEW:
        assert name in capi.SYMBOLS, name
    with open(os.path.join(ROOT, "include", "rdis_hip.h")) as fh:
        header = fh.read()
    for name in NEW:
        assert "int %s(" % name in header, name
    for method in ("set_sampling", "sample", "sort"):
        assert callable(getattr(capi.Population, method)), method
    params = inspect.signature(capi.Plan.solve_population).parameters
    assert "first" in params and "count" in params and params["first"].default == 0 and params["count"].default is None
    lib = capi.load_library()                       # (binds every symbol of SYMBOLS: AttributeError if one is not exported)
    lo = (C.c_double * 1)(0.0)
    order = (C.c_int64 * 1)()
    assert lib.rdis_hip_population_set_sampling(None, lo, lo) == -1
    assert lib.rdis_hip_population_set_sampling(None, None, None) == -1
    assert lib.rdis_hip_population_sample(None, 0, 1, 1, None, 0x5D15, 0) == -1
    assert lib.rdis_hip_population_sort(None, order) == -1
    assert lib.rdis_hip_population_sort(None, None) == -1
    assert lib.rdis_hip_plan_solve_population_range(None, None, 0, 1, 10, 3e-8) == -1


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("population_select") / "population_select_test")
    # (for the host alone: the header's kernels are the HIP compiler's business, its two rules are plain C++)
    subprocess.check_call([hipcc, "-x", "c++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "population_select_test.cpp")],
                          stderr=subprocess.DEVNULL)
    run = subprocess.run([out], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr      # (the program's own checks: the draw's range, the total order, the permutation)
    got = run.stdout.splitlines()
    assert got[-1] == "ok"
    return got[:-1]


def _d(hexbits):
    return struct.unpack("<d", struct.pack("<Q", int(hexbits, 16)))[0]


def test_draw_is_restart_value(lines):
    draws = [ln.split()[1:] for ln in lines if ln.startswith("draw ")]
    assert len(draws) == 4 * 3 * 5 * 5 * 9
    streams, zero_width, clamped = set(), 0, 0
    for seed, stream, member, var, slo, shi, lo, hi, val in draws:
        seed, stream, member, var = int(seed), int(stream), int(member), int(var)
        slo, shi, lo, hi = _d(slo), _d(shi), _d(lo), _d(hi)
        want = splitmix_restart_value(seed, stream, member, var, slo, shi, lo, hi)
        assert struct.pack("<d", want) == struct.pack("<Q", int(val, 16)), (seed, stream, member, var, slo, shi, lo, hi, _d(val), want)
        streams.add(stream)
        zero_width += slo == shi
        clamped += (slo < lo or shi > hi) and _d(val) in (lo, hi)
    assert (1 << 31) - 2 in streams and zero_width > 0 and clamped > 0


def test_rank_by_counting_is_the_sort(lines):
    sets = [i for i, ln in enumerate(lines) if ln.startswith("set ")]
    assert len(sets) == 5
    sizes = []
    for i in sets:
        n = int(lines[i].split()[1])
        f = [_d(t) for t in lines[i + 1].split()[1:]]
        order = [int(t) for t in lines[i + 2].split()[1:]]
        assert len(f) == n and len(order) == n
        assert order == sorted(range(n), key=lambda s: (f[s] != f[s], 0.0 if f[s] != f[s] else f[s], s)), (n, order)
        sizes.append(n)
    assert max(sizes) > 512 and 1 in sizes
