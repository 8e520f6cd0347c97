"""rdis_amd/csrc/population_grid.hpp -- the blocks per member of the tiny-component solver's population launch
(solver_quad_population.hpp) -- without a GPU: tests/cpp/population_tiny_grid_test.cpp checks the function's properties over a
grid of arguments (at least one block; never more than ceil(ntiny / groups_per_block); the cap; the device filled when there
is enough work; not increasing in the members; ntiny = 1, 65535 members, nothing resident); here the cases it prints are
compared with the rule restated."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("population_tiny") / "population_tiny_grid_test")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "population_tiny_grid_test.cpp")],
                          stderr=subprocess.DEVNULL)
    return out


def test_blocks_per_member(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr          # (the program's own checks of the properties)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok"
    cases = [tuple(int(t) for t in ln.split()[1:]) for ln in lines[:-1]]
    assert len(cases) >= 10
    for ntiny, gpb, res, members, cap, got in cases:
        want = min(-(-ntiny // gpb), max(1, -(-max(res, 1) // members)))
        if cap > 0:
            want = min(want, cap)
        assert got == want >= 1, (ntiny, gpb, res, members, cap, got, want)
    # full ladybug's points, sixteen lanes each, 64 members on a device that holds 4096 such blocks: 64 blocks a member
    assert (7776, 4, 4096, 64, 0, 64) in cases
