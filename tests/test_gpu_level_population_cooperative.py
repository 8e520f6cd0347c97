"""The level driver on a population with the level option populationCooperative = 1, on full ladybug with CGD (optBA's default
configuration, whose tree has components on the cooperative solver: the separator as one large group, the camera level as groups
side by side): HipRDISLevelOptimizer::optimizePopulation against optimize() run alone from every member's start -- with ==, rows,
start and final values, sweep counts and every trace record --; without the option the same call is refused with the population
entry's message, which names the cooperative solver; the C entry rdis_optba_run_samples with the option.
The C++ side is tests/cpp/harness_level_population_cooperative.cpp, built by this file's fixture."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from rdis_amd import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXIT, SWEEPS = 3, 2            # SSmaxit, maxSweeps
TRACE_COLS, TRACE_CAP = 12, 64
COMPARED = [0, 1, 2, 3, 6, 7, 9, 10, 11]   # sweep, depth, kind, ncomp, iters, objective, fevals, invalid, nonfinite
v = lambda a: a.ctypes.data_as(C.c_void_p)
LL = C.c_longlong

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rdis_amd", "host")], stdout=subprocess.DEVNULL)
    out = os.path.join(ROOT, "tests", "cpp", "libharness_level_population_cooperative.so")
    src = os.path.join(ROOT, "tests", "cpp", "harness_level_population_cooperative.cpp")
    deps = [src, os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so")]
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", out, src, "-L" + os.path.join(ROOT, "rdis_amd", "lib"),
                               "-lrdis_host", "-lrdis_hip", "-Wl,-rpath,$ORIGIN/../../rdis_amd/lib"])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def bal_path(tmp_path_factory):
    dst = tmp_path_factory.mktemp("bal") / "ladybug.txt"
    with gzip.open(P.LADYBUG_PATH, "rb") as src, open(dst, "wb") as out:
        shutil.copyfileobj(src, out)
    return str(dst).encode()


def single(h, path, sweeps, x):
    """optimize() alone from x: (out, trace, x afterwards)"""
    out, tr, xo = np.zeros(5), np.zeros((TRACE_CAP, TRACE_COLS)), np.zeros(len(x))
    x = np.ascontiguousarray(x, dtype=np.float64)
    rc = h.harness_coop_single(path, MAXIT, sweeps, v(x), v(out), v(tr), LL(TRACE_CAP), v(xo))
    assert rc == 0, rc
    assert out[4] <= TRACE_CAP
    return out, tr[:int(out[4])].copy(), xo


class PopRun:
    pass


def pop_run(h, path, cooperative, starts):
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    S, N = starts.shape
    r = PopRun()
    r.out, r.members, traces, ntr = np.zeros(4), np.zeros((S, 4)), np.zeros((S, TRACE_CAP, TRACE_COLS)), np.zeros(S, dtype=np.int64)
    r.rows, r.x_before, r.x_problem = np.zeros((S, N)), np.zeros(N), np.zeros(N)
    msg = C.create_string_buffer(4096)
    r.rc = h.harness_coop_run(path, MAXIT, SWEEPS, cooperative, LL(S), v(starts), v(r.out), v(r.members), v(traces), LL(TRACE_CAP), v(ntr), v(r.rows),
                              v(r.x_before), v(r.x_problem), msg, LL(len(msg)))
    assert r.rc in (0, 1), r.rc
    r.msg = msg.value.decode()
    assert np.all(ntr <= TRACE_CAP)
    r.traces = [traces[s, :int(ntr[s])].copy() for s in range(S)]
    return r


@pytest.fixture(scope="module")
def members_and_singles(harness, bal_path):
    """three members -- x0, the single run's state after one sweep, x0 with noise -- and optimize() alone from each"""
    x0 = P.load_bal().x0.copy()
    after1 = single(harness, bal_path, 1, x0)[2]
    rng = np.random.default_rng(5)
    members = np.stack([x0, after1, x0 * (1.0 + 1e-3 * rng.standard_normal(len(x0)))])
    return members, [single(harness, bal_path, SWEEPS, m) for m in members]


def test_population_run_equals_the_single_runs_on_full_ladybug(harness, bal_path, members_and_singles):
    members, singles = members_and_singles
    run = pop_run(harness, bal_path, 1, members)
    assert run.rc == 0, run.msg
    nplans = int(run.out[2])
    print("full ladybug, CGD, populationCooperative: %d launches a sweep; values %s -> %s, sweeps %s" %
          (nplans, run.members[:, 0].tolist(), run.members[:, 1].tolist(), run.members[:, 3].tolist()))
    for s, (out, tr, x) in enumerate(singles):
        assert run.rows[s].tobytes() == x.tobytes(), s
        m = run.members[s]
        assert np.array([m[0], m[1], m[3]]).tobytes() == np.array([out[1], out[0], out[2]]).tobytes(), (s, m, out)
        got = run.traces[s]
        assert len(got) == len(tr) == int(out[2]) * nplans == int(out[2]) * int(out[3]), (s, len(got), len(tr))
        assert got[:, COMPARED].tobytes() == tr[:, COMPARED].tobytes(), (s, got[:, COMPARED], tr[:, COMPARED])
        assert m[2].tobytes() == tr[-1, 7].tobytes()                  # the running objective
    best = int(np.argmin(run.members[:, 1]))
    assert int(run.out[1]) == best and run.out[0].tobytes() == run.members[best, 1].tobytes()
    assert run.x_problem.tobytes() == run.rows[best].tobytes()
    assert np.all(run.members[:, 1] < run.members[:, 0])


def test_without_the_option_the_same_call_is_refused(harness, bal_path, members_and_singles):
    """... with the population entry's message, which names the cooperative solver: the test above ran the new path"""
    members, _ = members_and_singles
    run = pop_run(harness, bal_path, 0, members)
    print("refused: " + run.msg)
    assert run.rc == 1, "the call went through"
    assert "plan_solve_population_range" in run.msg and "cooperative solver" in run.msg and "rdis_hip_plan_solve_population_cooperative" in run.msg
    assert run.rows.tobytes() == members.tobytes() and run.x_problem.tobytes() == run.x_before.tobytes()


def test_optba_run_samples_on_full_ladybug(bal_path):
    """rdis_optba_run_samples, useCGD 1 on the whole file: 0 with populationCooperative 1, -2 (refused) without"""
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run_samples.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int32, C.c_int64,
                                           C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(opts, nsamples=2):
        names, vals = [k.encode() for k in opts], list(opts.values())
        out, mem = np.zeros(10), np.zeros((nsamples, 8))
        rc = lib.rdis_optba_run_samples(bal_path, 0, 0, len(names), (C.c_char_p * len(names))(*names), (C.c_double * len(vals))(*vals), 0, nsamples, 7, 1,
                                        v(out), v(mem), None)
        return rc, out, mem
    base = {"SSmaxit": float(MAXIT), "maxSweeps": float(SWEEPS), "useCGD": 1.0}
    rc, out, mem = run(dict(base, populationCooperative=1.0))
    print("rdis_optba_run_samples: starts %s -> %s, sweeps %s" % (mem[:, 0].tolist(), mem[:, 1].tolist(), mem[:, 2].tolist()))
    assert rc == 0
    finite = mem[:, 1][~np.isnan(mem[:, 1])]
    assert len(finite) > 0 and out[0] == finite.min() and np.all(mem[:, 2] >= 1)
    assert run(base)[0] == -2
