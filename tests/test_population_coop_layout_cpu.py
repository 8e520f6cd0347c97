"""Population solves on the cooperative solver, what needs no GPU: the replicas of a member of a launch
(rdis_amd/csrc/replica_layout.hpp: population_coop_layout), the members of a launch under the budget and the resident workgroups
(coop_members_per_launch), the entry's refusal messages (population_rules.hpp) -- tests/cpp/population_coop_layout_test.cpp
answers, every figure is restated here -- and the entry itself in the library: exported, bound, RDIS_HIP_EINVAL on NULL handles."""
import os
import shutil
import subprocess

import pytest

from rdis_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = 4 * (512 * 8) * 4 * 8 + 64      # sizeof CoopState: COOP_NBUF buffers of COOP_MAX_WG * COOP_MAX_WAVES entries of COOP_KP granules, the abort word's line


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("population_coop_layout") / "population_coop_layout_test")
    # (for the host alone, as tests/test_plan_options_cpu.py builds its program)
    subprocess.check_call([hipcc, "-x", "c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "population_coop_layout_test.cpp")],
                          stderr=subprocess.DEVNULL)

    def ask(commands):
        run = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr
        got = run.stdout.splitlines()
        assert got[-1] == "ok" and len(got) == len(commands) + 1
        return got[:-1]
    return ask


def pad32(doubles):
    return (8 * doubles + 31) // 32 * 32


def test_three_parts_in_order_states_on_32_bytes(ask):
    """[R][gfac] [R][xi] [R][groups states]: the two parts of doubles padded to whole 32 bytes a member, so that every state lies
    on 32 bytes (sizeof CoopState is a multiple of 32) whatever R is; a member's stride is the padded part"""
    assert STATE % 32 == 0
    cases = [(ngfac, xi, groups, R) for ngfac in (0, 1, 4, 10803, 285228) for xi in (1, 9, 414, 23769) for groups in (1, 5, 49) for R in (1, 2, 3, 65535)]
    got = ask(["layout %d %d %d %d %d" % (ngfac, xi, groups, STATE, R) for ngfac, xi, groups, R in cases])
    for (ngfac, xi, groups, R), line in zip(cases, got):
        member, total, off_gfac, off_xi, off_state, stride_gfac, stride_xi = (int(t) for t in line.split())
        assert member == pad32(ngfac) + pad32(xi) + groups * STATE
        assert total == R * member
        assert (off_gfac, off_xi, off_state) == (0, R * pad32(ngfac), R * (pad32(ngfac) + pad32(xi)))
        assert (stride_gfac, stride_xi) == (pad32(ngfac) // 8, pad32(xi) // 8)
        assert stride_gfac >= ngfac and stride_xi >= xi and stride_gfac - ngfac < 4 and stride_xi - xi < 4
        assert off_state % 32 == 0 and off_xi % 32 == 0


def test_a_plan_without_cooperative_components_has_no_such_part(ask):
    assert ask(["layout 1000 500 0 %d 7" % STATE]) == ["0 0 0 0 0 0 0"]


def test_members_of_a_launch(ask):
    """members_per_launch's answer, further bounded by cap / launch workgroups, at least 1"""
    GIB = 1 << 30
    cases = [
        ((8, 0, 1000, 256, 10), 1),                 # budget 0: one member a launch
        ((8, GIB, 1000, 9, 10), 1),                 # the cap below one member's workgroups: one (the entry refuses such a plan before it asks)
        ((8, GIB, 1000, 0, 10), 1),
        ((8, GIB, 1000, 30, 10), 3),                # cap = k x workgroups: k
        ((8, GIB, 1000, 39, 10), 3),
        ((8, GIB, 1000, 40, 10), 4),
        ((8, GIB, 1000, 80, 10), 8),
        ((3, GIB, 1000, 256, 10), 3),               # count below the fit
        ((8, 2500, 1000, 256, 10), 2),              # the budget below the cap
        ((8, 2500, 1000, 10, 10), 1),               # the cap below the budget
        ((100000, 1 << 62, 8, 1 << 40, 1), 65535),  # the grid's second dimension
        ((100000, 1 << 62, 0, 1 << 40, 1), 65535),  # (a replica of nothing bounds nothing)
        ((8, GIB, 1000, 0, 0), 8),                  # no cooperative launch: the cap bounds nothing
        ((8, 2500, 1000, 5, 0), 2),
        ((1, 0, 1 << 40, 1, 512), 1),
    ]
    got = ask(["members %d %d %d %d %d" % c for c, _ in cases])
    assert [int(g) for g in got] == [want for _, want in cases]


def test_refusal_messages(ask):
    pipelined, grid, hint, residency = ask(["refusal pipelined plan_solve_population_cooperative 0", "refusal grid plan_solve_population_cooperative 2",
                                            "refusal hint - 0", "refusal residency plan_solve_population_cooperative 300"])
    assert residency == ("plan_solve_population_cooperative: a cooperative launch of the plan has 300 workgroups a member, and the population kernel "
                         "can have 150 resident: not one member fits a launch (set the plan option coop_workgroups to at most that)")
    assert pipelined == ("plan_solve_population_cooperative: cooperative components are solved on a population in the plain cooperative layout, and "
                         "this plan's ordinary solve runs them in the pipelined layout (other lane tables; the same bits): set the plan option "
                         "coop_pipeline = 0")
    assert grid == ("plan_solve_population_cooperative: 2 component(s) of the plan run on the grid solver, which has no population entry (too large "
                    "for a cooperative group of resident workgroups)")
    assert hint == (" (cooperative components are solved on a population by rdis_hip_plan_solve_population_cooperative, a group per member: "
                    "solver_coop_population.hpp)")


def test_the_entry_is_exported_and_rejects_null_handles():
    assert "rdis_hip_plan_solve_population_cooperative" in capi.SYMBOLS
    lib = capi.load_library()
    assert getattr(lib, "rdis_hip_plan_solve_population_cooperative") is not None
    assert lib.rdis_hip_plan_solve_population_cooperative(None, None, 0, 1, 10, 3e-8) == -1      # RDIS_HIP_EINVAL
