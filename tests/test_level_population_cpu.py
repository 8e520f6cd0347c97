"""The level driver on a population without a GPU: the bookkeeping of a population run (rdis_amd/host/level_members.h, pure host
functions: tests/cpp/level_members_test.cpp) -- the stop rule of one member, the stable partition of the rows into running and
stopped members as the order of rdis_hip_population_permute, the row-to-member map and the permutation that restores the original
numbering -- and that the library, the header and the binding name the three new entries."""
import os
import subprocess

import pytest

from rdis_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("level_members") / "level_members_test")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", path, os.path.join(ROOT, "tests", "cpp", "level_members_test.cpp")])
    return path


def _run(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return out.stdout


def test_stop_rule(exe):
    """!(before - objective > steptol), the driver's own expression"""
    tol = 1e-4
    rows = [
        (10.0, 9.0, tol, 0),                       # a gain beyond steptol goes on
        (1.0, 1.0 - tol, tol, int(not (1.0 - (1.0 - tol) > tol))),   # (whatever the rounding of this difference makes of it)
        (0.5, 0.25, 0.25, 1),                      # a gain EQUAL to steptol, exactly representable: stops
        (0.5, 0.25, 0.2499999, 0),
        (10.0, 10.0, tol, 1),                      # no gain
        (10.0, 11.0, tol, 1),                      # a loss
        (10.0, float("nan"), tol, 1),              # an objective that is not a number stops
        (float("nan"), 1.0, tol, 1),
        (10.0, float("-inf"), tol, 0),             # -inf goes on
        (10.0, float("inf"), tol, 1),
        (float("inf"), float("inf"), tol, 1),      # inf - inf is not a number
    ]
    got = [int(v) for v in _run(exe, "stop", "".join("%r %r %r\n" % r[:3] for r in rows)).split()]
    assert got == [r[3] for r in rows]


PATTERNS = {
    "none": lambda a: [0] * a,
    "all": lambda a: [1] * a,
    "one stopped": lambda a: [1 if r == a // 2 else 0 for r in range(a)],
    "one left": lambda a: [0 if r == a // 2 else 1 for r in range(a)],
    "alternating": lambda a: [r % 2 for r in range(a)],
    "alternating from 1": lambda a: [(r + 1) % 2 for r in range(a)],
}
SEQUENCES = [(k, k, k) for k in PATTERNS] + [("alternating", "one stopped", "one left"), ("one stopped", "alternating from 1", "all"),
                                              ("none", "one left", "none")]


def _parse(line):
    head, order, rows = line.split("|")
    return [int(v) for v in head.split()], [int(v) for v in order.split()], [int(v) for v in rows.split()]


@pytest.mark.parametrize("n", [1, 2, 5, 64])
@pytest.mark.parametrize("seq", SEQUENCES, ids=["-".join(s).replace(" ", "_") for s in SEQUENCES])
def test_stable_partition_map_and_restore(exe, n, seq):
    # the flags of every round depend on how many rows are still active: simulate here, feed the program the same flags
    active, rounds = n, []
    for name in seq:
        flags = PATTERNS[name](active)
        rounds.append(flags)
        active -= sum(flags)
    text = "%d %d\n" % (n, len(seq)) + "".join(" ".join(map(str, f)) + "\n" for f in rounds)
    lines = _run(exe, "partition", text).strip().split("\n")
    assert len(lines) == len(seq) + 1
    member_of_row, active = list(range(n)), n                        # the population as the permutes leave it
    stopped_at = {}
    for k, (flags, line) in enumerate(zip(rounds, lines)):
        (moved, got_active), order, rows = _parse(line)
        assert sorted(order) == list(range(n))                       # a permutation
        running = [r for r in range(active) if not flags[r]]
        stopped = [r for r in range(active) if flags[r]]
        # the active rows first in their old order, the rows stopped now behind them in theirs, the rows stopped earlier in place
        assert order == running + stopped + list(range(active, n))
        assert moved == int(order != list(range(n)))
        for r in stopped:
            stopped_at[member_of_row[r]] = k
        member_of_row = [member_of_row[o] for o in order]            # X_new[r] = X_old[order[r]]
        active = len(running)
        assert got_active == active and rows == member_of_row        # the map names the member every row holds
        assert all(m not in stopped_at for m in member_of_row[:active]) and all(m in stopped_at for m in member_of_row[active:])
    (moved,), order, rows = _parse(lines[-1])
    assert sorted(order) == list(range(n)) and moved == int(order != list(range(n)))
    member_of_row = [member_of_row[o] for o in order]
    assert member_of_row == list(range(n)) == rows                   # the partitions composed with the last permutation: the identity


ENTRIES = ["rdis_hip_lm_plan_summary_population", "rdis_hip_lm_plan_summary_population_device", "rdis_hip_population_permute"]


def test_library_header_and_binding_name_the_new_entries():
    lib = capi.load_library()
    with open(os.path.join(ROOT, "include", "rdis_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None and "int %s(" % name in header
    assert lib.rdis_hip_lm_plan_summary_population(None, None) == -1 and lib.rdis_hip_lm_plan_summary_population_device(None, None) == -1
    assert lib.rdis_hip_population_permute(None, None) == -1
    assert hasattr(capi.LmPlan, "summary_population") and hasattr(capi.Population, "permute")
    with open(os.path.join(ROOT, "include", "rdis_optba.h")) as fh:
        assert '#include "rdis_optba_samples.h"\n' in fh.read()
    with open(os.path.join(ROOT, "include", "rdis_optba_samples.h")) as fh:
        optba = fh.read()
    assert "int rdis_optba_run_samples(" in optba and "#define RDIS_OPTBA_MEMBER_COLS 8\n" in optba
    # the host library exports the entry (built here if need be, as tests/test_capi_cpu.py builds it) and refuses bad calls
    import ctypes as C
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rdis_amd", "host")], stdout=subprocess.DEVNULL)
    run = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so")).rdis_optba_run_samples
    run.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p,
                    C.c_void_p]
    out, mem = (C.c_double * 10)(), (C.c_double * 16)()
    assert run(None, 0, 0, 0, None, None, 0, 2, 1, 1, out, mem, None) == -3               # no file name
    assert run(b"x", 0, 0, 0, None, None, 0, 0, 1, 1, out, mem, None) == -3               # no member
    assert run(b"x", 0, 0, 0, None, None, 0, 2, 1, 0, out, mem, None) == -3               # the file's state is one member
    assert run(b"/nonexistent/problem.txt", 0, 0, 0, None, None, 0, 2, 1, 1, out, mem, None) == -1   # cannot be loaded
