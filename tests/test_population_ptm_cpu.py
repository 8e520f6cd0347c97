"""rdis_amd/csrc/population_grid.hpp -- the bytes of one replica of a population launch with point-major components
(solver_ptm_population.hpp) and the members of a launch under the budget starts_workspace_bytes -- without a GPU:
tests/cpp/population_ptm_replica_test.cpp checks the functions' properties over a grid of arguments (the point-major part alone;
with the LDS-resident part; zero blocks; at least one member a launch, never beyond the budget with more than one, never one
fewer than fits, the grid's 65535); here the cases it prints are compared with the rules restated."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("population_ptm") / "population_ptm_replica_test")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "population_ptm_replica_test.cpp")],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr          # (the program's own checks of the properties)
    rows = out.stdout.splitlines()
    assert rows[-1] == "ok"
    return rows[:-1]


def test_replica_bytes(lines):
    cases = [tuple(int(t) for t in ln.split()[1:]) for ln in lines if ln.startswith("replica ")]
    assert len(cases) >= 6
    for blocks, cptr_len, lds, nfree, ngfac, got in cases:
        want = (blocks * 18 * 8 + cptr_len * 32 if blocks else 0) + (8 * (5 * nfree + ngfac) if lds else 0)
        assert got == want, (blocks, cptr_len, lds, nfree, ngfac, got, want)
    # ladybug 7 / 200 as one component: 200 point blocks in four wave-chunks
    assert (200, 5, 0, 0, 0, 28960) in cases
    # full ladybug as one component: 7776 point blocks in 122 wave-chunks, 1.1 MB a member
    assert (7776, 123, 0, 0, 0, 7776 * 144 + 123 * 32) in cases
    # zero blocks: the LDS-resident part alone, or nothing
    assert (0, 0, 1, 45, 384, 8 * (5 * 45 + 384)) in cases and (0, 0, 0, 45, 384, 0) in cases


def test_members_per_launch(lines):
    cases = [tuple(int(t) for t in ln.split()[1:]) for ln in lines if ln.startswith("members ")]
    assert len(cases) >= 8
    for members, budget, rep, got in cases:
        want = min(members, 65535, max(1, budget // rep) if rep else members)
        assert got == want >= 1, (members, budget, rep, got, want)
    # five members of ladybug 7 / 200 under two replicas and a half: 2 + 2 + 1; under one byte: at least one
    assert (5, 72400, 28960, 2) in cases and (5, 1, 28960, 1) in cases and (3, 0, 28960, 1) in cases
    # 256 members of full ladybug fit the default budget of 2^30 bytes, a quarter of it holds 238
    assert (256, 1 << 30, 1123680, 256) in cases and (256, 1 << 28, 1123680, (1 << 28) // 1123680) in cases
