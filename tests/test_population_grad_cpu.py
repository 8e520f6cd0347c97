"""rdis_amd/csrc/population_grid.hpp -- the bytes of one member's scratch in a launch of the population's value + gradient
(rdis_hip_population_eval_grad: by branch) and the members of a launch under the budget grad_workspace_bytes -- without a GPU:
tests/cpp/population_grad_members_test.cpp checks the functions' properties over a grid of arguments (at least one member a
launch, never beyond the budget with more than one, never one fewer than fits, the grid's 65535, zero slots counted as one);
here the cases it prints are compared with the rules restated."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED, SHORT, TWO_PASS = 1, 2, 3


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("population_grad") / "population_grad_members_test")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "population_grad_members_test.cpp")],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr          # (the program's own checks of the properties)
    rows = out.stdout.splitlines()
    assert rows[-1] == "ok"
    return rows[:-1]


def test_member_bytes(lines):
    cases = [tuple(int(t) for t in ln.split()[1:]) for ln in lines if ln.startswith("bytes ")]
    assert len(cases) >= 6
    for branch, ncb, cs, ps, nch, nslots, blocks, got in cases:
        want = {FUSED: 8 * (14 * ncb + 9 * max(cs, 1) + 3 * max(ps, 1) + max(nch, 1)),
                SHORT: 8 * (nslots + 1),
                TWO_PASS: 8 * (nslots + max(blocks, 1))}.get(branch, 0)
        assert got == want, (branch, ncb, cs, ps, nch, nslots, blocks, got, want)
    # the pinned case: 49 camera blocks, 10 camera slots, 20 point slots, 63 chunks
    assert (FUSED, 49, 10, 20, 63, 0, 0, 8 * (686 + 90 + 60 + 63)) in cases and 8 * (686 + 90 + 60 + 63) == 7192
    # ladybug 5 / 30 on one ragged chunk: no staged block, each array one slot
    assert (FUSED, 5, 0, 0, 1, 0, 0, 8 * (70 + 9 + 3 + 1)) in cases
    # full ladybug on the two-pass form: twelve partials a factor and 125 block sums
    assert (TWO_PASS, 0, 0, 0, 0, 382116, 125, 8 * 382241) in cases


def test_members_per_launch(lines):
    cases = [tuple(int(t) for t in ln.split()[1:]) for ln in lines if ln.startswith("members ")]
    assert len(cases) >= 8
    for count, budget, per, got in cases:
        want = min(count, 65535, max(1, budget // per))
        assert got == want >= 1, (count, budget, per, got, want)
    # five members under two and a half members' bytes: 2 + 2 + 1; under one byte and under none: one replica for all
    assert (5, 17980, 7192, 2) in cases and (5, 1, 7192, 1) in cases and (3, 0, 7192, 1) in cases
    # the grid's second dimension
    assert (100000, 1 << 30, 8, 65535) in cases and (70000, 1 << 40, 7192, 65535) in cases
    # 256 members with full ladybug's per-factor partials (3 MB each) fit the default budget, 1000 do not
    assert (256, 1 << 30, 3056936, 256) in cases and (1000, 1 << 30, 3056936, (1 << 30) // 3056936) in cases
