"""The level driver on a population (optBA's sample loop as one run) on the device: the member summaries of a Levenberg-Marquardt
plan (rdis_hip_lm_plan_summary_population) against a numpy restatement of the stated order and against the single-state summary;
rdis_hip_population_permute; HipRDISLevelOptimizer::optimizePopulation against optimize() run alone from every member's start --
with ==, rows, values, sweep counts and every trace record --; its refusals; the C entry rdis_optba_run_samples.
The C++ side is tests/cpp/harness_level_population.cpp, built by this file's fixture."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from rdis_amd import capi, problems as P

import lm_levels_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTOL, STEPTOL = 3e-8, 1e-4      # SubspaceOptimizer's and the level driver's defaults
TRACE_COLS, TRACE_CAP = 12, 64
COMPARED = [0, 1, 2, 3, 6, 7, 9, 10, 11]   # sweep, depth, kind, ncomp, iters, objective, fevals, invalid, nonfinite
v = lambda a: a.ctypes.data_as(C.c_void_p)
LL, D = C.c_longlong, C.c_double


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rdis_amd", "host")], stdout=subprocess.DEVNULL)
    out = os.path.join(ROOT, "tests", "cpp", "libharness_level_population.so")
    src = os.path.join(ROOT, "tests", "cpp", "harness_level_population.cpp")
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


# ---- 1. member summaries ----------------------------------------------------------------------------------------------------
def _device_sum(a):
    """the stated order (tests/test_gpu_lm_levels.py): 256 lanes, a lane's stride over the components in component order, a
    butterfly over each wave of 64, then the four waves in wave order"""
    a = np.asarray(a, dtype=np.float64)
    acc = np.zeros(256)
    for c0 in range(0, len(a), 256):
        part = a[c0:c0 + 256]
        acc[:len(part)] = acc[:len(part)] + part
    w = acc.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    s = 0.0
    for k in range(4):
        s = s + w[k, 0]
    return s


def _summary_of(rows):
    fret = np.array([r.fret for r in rows])
    want = np.zeros(16)
    want[0] = _device_sum(fret)
    want[1] = _device_sum([r.delta for r in rows])
    for k, name in ((2, "iters"), (3, "nfev"), (4, "njev"), (5, "nsolve")):
        want[k] = _device_sum([getattr(r, name) for r in rows])
    for code in range(1, 8):
        want[5 + code] = _device_sum([1.0 if r.stop == code else 0.0 for r in rows])
    want[13] = _device_sum([0.0 if np.isfinite(f) else 1.0 for f in fret])
    return want


def _fetch_bytes(members):
    return b"".join(r.x.tobytes() + np.array([r.fret, r.delta, r.iters, r.stop, r.nfev, r.njev, r.nsolve, r.mu]).tobytes() + r.history.tobytes()
                    for rows in members for r in rows)


def _refused(call):
    with pytest.raises(capi.RdisHipError) as e:
        call()
    assert e.value.code == -1
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", [("ladybug-5-30", "points"), ("ladybug-20-120", "leaves")])
@pytest.mark.parametrize("model", [1, 2])
def test_member_summaries_are_the_single_state_summaries(name, which, model, gctx):
    pp = K.problem(name)
    g = capi.Problem(gctx, pp)
    if which == "points":
        assigned = np.zeros(pp.nvars, np.uint8)
        assigned[:int(pp.pt_vid0.min())] = 1                         # every point on its own, the cameras held
        lists = g.components(assigned)
    else:
        lists = K.plans(name)[1][3:]
    plan = capi.LmPlan(g, *lists, model=model, history=1, wide=True)
    assert plan.ncomp == {"ladybug-5-30": 30, "ladybug-20-120": 89}[name]
    _refused(plan.summary_population)                               # before any solve
    rng = np.random.default_rng(11)
    members = np.stack([pp.x0, pp.x0 * (1.0 + 1e-3 * rng.standard_normal(pp.nvars)), pp.x0 + 1e-3 * rng.standard_normal(pp.nvars)])
    pop = capi.Population(g, x=members)
    plan.solve_population(pop, 0, 3, 5, FTOL)
    fetched = plan.fetch_population()
    before = _fetch_bytes(fetched)
    S = plan.summary_population()
    assert S.shape == (3, 16)
    for m in range(3):
        want = _summary_of(fetched[m])
        assert S[m].tobytes() == want.tobytes(), (m, S[m], want)
        assert S[m, 6:13].sum() == plan.ncomp and S[m, 14] == 0 and S[m, 15] == 0 and S[m, 1] < 0 and S[m, 2] > 0
    _refused(plan.summary)                                          # the single-state entries keep refusing after a population solve
    _refused(plan.objective)
    assert plan.summary_population().tobytes() == S.tobytes()
    assert _fetch_bytes(plan.fetch_population()) == before          # nothing a fetch returns was written
    # the same bytes with one member per launch, and for a range that does not start at member 0
    classes = plan.info("launches")
    assert plan.info("member_workspace_bytes") > 0
    plan.set_option("workspace_bytes", 0)
    pop1 = capi.Population(g, x=members)
    plan.solve_population(pop1, 0, 3, 5, FTOL)
    assert plan.info("members_per_launch") == 1 and plan.info("launches") == 3 * classes
    assert plan.summary_population().tobytes() == S.tobytes()
    plan.set_option("workspace_bytes", 1 << 30)
    pop2 = capi.Population(g, x=members)
    plan.solve_population(pop2, 1, 2, 5, FTOL)
    R = plan.summary_population()
    assert R.shape == (2, 16) and R.tobytes() == S[1:].tobytes()
    assert pop2.get_x(0).tobytes() == members[0].tobytes()
    # row m is what the single-state summary returns on a problem whose x is member m's; after such a solve: refused
    for m in range(3):
        g.set_x(members[m])
        plan.solve(5, FTOL)
        assert plan.summary().tobytes() == S[m].tobytes(), m
        _refused(plan.summary_population)
    g.set_x(pp.x0)
    plan.solve_starts(members[:2, plan.free_vid], 5, FTOL)
    _refused(plan.summary_population)                               # after a multi-start solve


# ---- 2. permute -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_permute_moves_rows_and_values(gctx):
    pp = K.problem("ladybug-5-30")
    g = capi.Problem(gctx, pp)
    rng = np.random.default_rng(3)
    X = np.stack([pp.x0 * (1.0 + 1e-3 * (k + 1) * rng.standard_normal(pp.nvars)) for k in range(5)])
    pop = capi.Population(g, x=X)
    order = np.array([3, 0, 4, 1, 2], dtype=np.int64)
    pop.permute(order)                                              # stale values: the rows move, best() still refuses
    assert pop.get_x().tobytes() == X[order].tobytes()
    assert "evaluate first" in _refused(pop.best) and pop.info("eval_valid") == 0
    pop.set_x(X)
    f = pop.eval()
    assert len(set(f.tolist())) == 5
    pop.permute(order)
    assert pop.get_x().tobytes() == X[order].tobytes() and pop.info("eval_valid") == 1
    fd = np.frombuffer(gctx.copy_to_host(pop.eval_device(), 8 * 5), dtype=np.float64)
    assert fd.tobytes() == f[order].tobytes() == pop.eval().tobytes()
    pop.set_x(X[order])                                             # (marks the values stale) ... evaluate, permute, ask for the best
    f2 = pop.eval()
    pop.permute(order)
    m, fb = pop.best()
    assert fb == f2.min() and m == int(np.argmin(f2[order])) and pop.get_x(m).tobytes() == X[order][order][m].tobytes()
    pop.assign_best()
    assert g.get_x().tobytes() == X[order][order][m].tobytes()
    now = pop.get_x().copy()
    pop.permute(np.arange(5))                                       # the identity leaves every byte
    assert pop.get_x().tobytes() == now.tobytes() and pop.best() == (m, fb)
    for bad, word in ((np.array([0, 1, 2, 3, 3]), "twice"), (np.array([0, 1, 2, 3, 5]), "out of range"), (np.array([0, -1, 2, 3, 4]), "out of range"),
                      (None, "NULL")):
        assert word in _refused(lambda: pop.permute(bad))
        assert pop.get_x().tobytes() == now.tobytes() and pop.best() == (m, fb)


# ---- 3. and 4. the driver ---------------------------------------------------------------------------------------------------
def _single(h, path, case, use_cgd, maxit, sweeps, model, x):
    """optimize() alone from x"""
    (_, nc, npnt), pct, seppct = K.CASES[case]
    out, tr, xo = np.zeros(5), np.zeros((TRACE_CAP, TRACE_COLS)), np.zeros(len(x))
    x = np.ascontiguousarray(x, dtype=np.float64)
    rc = h.harness_pop_single(path, LL(nc), LL(npnt), use_cgd, maxit, sweeps, D(pct), D(seppct), model, v(x), v(out), v(tr), LL(TRACE_CAP), v(xo))
    assert rc == 0, rc
    assert out[4] <= TRACE_CAP
    return out, tr[:int(out[4])].copy(), xo


class _PopRun:
    pass


def _pop_run(h, path, key, use_cgd, maxit, sweeps, model, starts, batch=1, mode=0):
    """key: a name of K.CASES, or ((nc, npnt), pct, seppct) for a file of its own"""
    (_, nc, npnt), pct, seppct = K.CASES[key] if isinstance(key, str) else key
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    S, N = starts.shape
    r = _PopRun()
    r.out, r.members, traces, ntr = np.zeros(4), np.zeros((S, 9)), np.zeros((S, TRACE_CAP, TRACE_COLS)), np.zeros(S, dtype=np.int64)
    r.rows, r.x_before, r.x_problem, r.x_mirror = np.zeros((S, N)), np.zeros(N), np.zeros(N), np.zeros(N)
    msg = C.create_string_buffer(2048)
    r.rc = h.harness_pop_run(path, LL(nc), LL(npnt), use_cgd, maxit, sweeps, D(pct), D(seppct), model, batch, mode, LL(S), v(starts), v(r.out),
                             v(r.members), v(traces), LL(TRACE_CAP), v(ntr), v(r.rows), v(r.x_before), v(r.x_problem), v(r.x_mirror), msg, LL(len(msg)))
    assert r.rc in (0, 1), r.rc
    r.msg = msg.value.decode()
    assert np.all(ntr <= TRACE_CAP)
    r.traces = [traces[s, :int(ntr[s])].copy() for s in range(S)]
    return r


def _best_by_rule(f):
    """population_best: the lowest value, the lowest index on a tie, a NaN never unless every value is one"""
    ok = [i for i in range(len(f)) if not np.isnan(f[i])]
    return min(ok, key=lambda i: (f[i], i)) if ok else 0


_RUNS = {}


def _members_and_single_runs(h, path, case, use_cgd, maxit, model, with_nan):
    """the members of a case and optimize() run alone from each of them: computed once, shared by the tests of the case"""
    key = (case, use_cgd, maxit, model, with_nan)
    if key in _RUNS:
        return _RUNS[key]
    pp = K.problem(case)
    x0 = pp.x0.copy()
    after1 = _single(h, path, case, use_cgd, maxit, 1, model, x0)[2]      # the single run from x0 is a prefix of itself
    after2 = _single(h, path, case, use_cgd, maxit, 2, model, x0)[2]
    full = _single(h, path, case, use_cgd, maxit, 8, model, x0)
    rng = np.random.default_rng(5)
    members = [x0, after1, after2, full[2].copy(), x0 * (1.0 + 1e-3 * rng.standard_normal(len(x0)))]
    if with_nan:
        bad = x0.copy()
        bad[int(pp.pt_vid0.max()) + 1] = np.nan                       # one coordinate of the last point
        members.append(bad)
        members.append(_three_sweeps_before_the_end(h, path, case, use_cgd, maxit, model, x0))
    singles = [full] + [_single(h, path, case, use_cgd, maxit, 8, model, m) for m in members[1:]]
    _RUNS[key] = np.stack(members), singles
    return _RUNS[key]


def _three_sweeps_before_the_end(h, path, case, use_cgd, maxit, model, x0, chunk=256):
    """The state of the single run from x0 three sweeps before that run stops by its own rule (no maxSweeps in its way): the
    members "after 1 sweep" and "after 2 sweeps" taken from the far end of the same run.  The run is continued in chunks of
    `chunk` sweeps, each from the state the one before left -- the same solves, so the same states --, until a chunk stops early;
    then the last chunks are run again three sweeps short.  How many sweeps this member needs is read from ITS single run."""
    (_, nc, npnt), pct, seppct = K.CASES[case]

    def go(x, sweeps):
        out, xo = np.zeros(5), np.zeros(len(x))
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert h.harness_pop_single(path, LL(nc), LL(npnt), use_cgd, maxit, sweeps, D(pct), D(seppct), model, v(x), v(out), None, LL(0), v(xo)) == 0
        return int(out[2]), xo
    states = [x0]
    for _ in range(64):
        done, x = go(states[-1], chunk)
        if done < chunk:
            break
        states.append(x)
    else:
        raise AssertionError("the single run has not stopped after %d sweeps" % (64 * chunk))
    total = (len(states) - 1) * chunk + done                          # sweeps of the whole run
    assert total > 3, total
    start, left = divmod(total - 3, chunk)                            # states[k]: after k * chunk sweeps
    x = states[start]
    if left > 0:
        done, x = go(x, left)
        assert done == left, (done, left)
    return x


def _expected_permutes(sweeps, max_sweeps=8):
    """the permutes a run makes when member s stops after sweeps[s] sweeps: the stable partition after every sweep but the last
    possible one (nothing is solved after it, so the rows stay) in which some but not all active members stop, where it moves a row,
    and the one that restores the numbering, likewise.  A member with max_sweeps sweeps -- stopped by the rule there or cut off --
    is never moved for it."""
    rows, active, n = list(range(len(sweeps))), len(sweeps), 0
    for k in range(1, min(max(sweeps), max_sweeps - 1) + 1):
        order = [r for r in range(active) if sweeps[rows[r]] > k] + [r for r in range(active) if sweeps[rows[r]] == k] + list(range(active, len(rows)))
        n += order != list(range(len(rows)))
        rows = [rows[o] for o in order]
        active = sum(1 for s in sweeps if s > k)
    return n + (rows != list(range(len(rows))))


def _check_run_against_single_runs(run, singles, members):
    nplans = int(run.out[2])
    assert run.rc == 0, run.msg
    for s, (out, tr, x) in enumerate(singles):
        assert run.rows[s].tobytes() == x.tobytes(), s                # the row's bytes, NaN included: row s is member s
        m = run.members[s]
        assert np.array([m[0], m[1], m[3]]).tobytes() == np.array([out[1], out[0], out[2]]).tobytes(), (s, m, out)
        got = run.traces[s]
        assert len(got) == len(tr) == int(out[2]) * nplans == int(out[2]) * int(out[3]), (s, len(got), len(tr))
        assert got[:, COMPARED].tobytes() == tr[:, COMPARED].tobytes(), (s, got[:, COMPARED], tr[:, COMPARED])
        assert (m[4], m[5], m[6], m[7], m[8]) == (tr[:, 3].sum(), tr[:, 6].sum(), tr[:, 9].sum(), tr[:, 10].sum(), tr[:, 11].sum())
        assert m[2].tobytes() == tr[-1, 7].tobytes()                  # the running objective
        assert np.all(got[:, 8] == 0)                                 # no component by a call of its own
    best = _best_by_rule(run.members[:, 1])
    assert int(run.out[1]) == best and run.out[0].tobytes() == run.members[best, 1].tobytes() and not np.isnan(run.out[0])
    assert run.x_problem.tobytes() == run.rows[best].tobytes() == run.x_mirror.tobytes()
    assert run.members[best, 1] <= run.members[0, 0]
    assert run.out[3] == _expected_permutes([int(o[2]) for o, _, _ in singles])


LM_CASES = [("ladybug-5-30", 2), ("ladybug-8-30", 2), ("ladybug-20-120", 2), ("ladybug-20-120-pieces", 2), ("ladybug-5-30", 1), ("ladybug-20-120", 1)]
LM_MAXIT = 3


@pytest.mark.gpu
@pytest.mark.parametrize("case,model", LM_CASES)
def test_population_run_equals_the_single_runs_levenberg_marquardt(case, model, harness, bal_path):
    """seven members -- x0, the single run's states after 1, 2 and all of its 8 sweeps, x0 with noise, x0 with a NaN, and that run's
    state three sweeps before it stops by itself -- against optimize() alone from each (LMsingleMinFactors 0): rows, values, sweeps
    and every trace record with ==.  That the members stop at different times is the next test's to assert."""
    members, singles = _members_and_single_runs(harness, bal_path, case, 0, LM_MAXIT, model, with_nan=True)
    sweeps = [int(o[2]) for o, _, _ in singles]
    print("%s, model %d: sweeps of the single runs %s, values %s" % (case, model, sweeps, [float(o[0]) for o, _, _ in singles]))
    assert sweeps[5] == 1 and sweeps[0] >= 2                         # the NaN member stops by the stop rule; x0 goes on
    assert np.isnan(singles[5][0][1]) and np.isnan(singles[5][1][-1, 7])
    run = _pop_run(harness, bal_path, case, 0, LM_MAXIT, 8, model, members)
    print("    population run: best member %d, %d permute(s)" % (run.out[1], run.out[3]))
    _check_run_against_single_runs(run, singles, members)
    assert int(run.out[1]) != 5                                      # never the NaN member
    assert run.members[5, 7] >= 1 and run.members[5, 8] >= 1          # its components are counted, not thrown


@pytest.mark.gpu
@pytest.mark.parametrize("case,model", LM_CASES)
def test_the_members_stop_after_three_distinct_sweep_counts(case, model, harness, bal_path):
    """The condition under which the test above exercises the partition more than once, asserted from the single runs (not from
    the code under test): at least three distinct sweep counts among the members, the NaN member after exactly one sweep, x0 after
    at least two.
    Measured (SSmaxit 3, maxSweeps 8, default steptol), the six members x0, after 1 sweep, after 2, final, noise, NaN alone give
        model 1: ladybug-5-30 [8, 8, 7, 1, 8, 1], ladybug-20-120 [8, 8, 8, 7, 8, 1] -- three counts;
        model 2: all four cases [8, 8, 8, 8, 8, 1] -- two counts, and the same with SSmaxit 2 and 1: with the two pixel residuals
        the alternation gains more than steptol a sweep far beyond maxSweeps (it stops by itself after 150, 132, 1538 and 1771
        sweeps), so no state from the first sweeps of the run from x0 stops between the second and the seventh sweep.
    The seventh member is such a state from the far end of the same run: three sweeps before the run's own stop (measured: it
    needs 3 sweeps in all six cases).  The condition itself is as stated, over all seven."""
    _, singles = _members_and_single_runs(harness, bal_path, case, 0, LM_MAXIT, model, with_nan=True)
    sweeps = [int(o[2]) for o, _, _ in singles]
    assert sweeps[5] == 1 and sweeps[0] >= 2
    assert len(set(sweeps)) >= 3, sweeps


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ladybug-5-30", "ladybug-8-30"])
def test_population_run_equals_the_single_runs_cgd(case, harness, bal_path):
    members, singles = _members_and_single_runs(harness, bal_path, case, 1, 3, 1, with_nan=False)
    sweeps = [int(o[2]) for o, _, _ in singles]
    print("%s, CGD: sweeps of the single runs %s, values %s" % (case, sweeps, [float(o[0]) for o, _, _ in singles]))
    assert len(set(sweeps)) >= 2 and sweeps[0] >= 2                  # the condition, from the single runs
    run = _pop_run(harness, bal_path, case, 1, 3, 8, 1, members)
    print("    population run: best member %d, %d permute(s)" % (run.out[1], run.out[3]))
    _check_run_against_single_runs(run, singles, members)
    assert run.out[3] >= 1 and np.all(run.members[:, 6:] == 0)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def _check_refused(run, starts, *words):
    assert run.rc == 1, "the call went through"
    for w in words:
        assert w in run.msg, run.msg
    assert run.rows.tobytes() == starts.tobytes() and run.x_problem.tobytes() == run.x_before.tobytes()


@pytest.mark.gpu
def test_refusals_come_before_any_row_is_written(harness, bal_path, tmp_path):
    pp = K.problem("synthetic-160-400")
    path = str(tmp_path / "synthetic_160_400.txt")
    P.save_bal(pp, path)
    starts = np.stack([pp.x0, pp.x0 * 1.001])
    run = _pop_run(harness, path.encode(), ((None, 0, 0), 0.2, 0.0), 0, 3, 1, 1, starts)
    _check_refused(run, starts, "node 0", "89 cameras")               # the separator of the top component
    lb = K.problem("ladybug-5-30")
    starts = np.stack([lb.x0, lb.x0 * 1.001])
    for use_cgd in (0, 1):
        _check_refused(_pop_run(harness, bal_path, "ladybug-5-30", use_cgd, 3, 1, 1, starts, batch=0), starts, "batch = 0")
        _check_refused(_pop_run(harness, bal_path, "ladybug-5-30", use_cgd, 3, 1, 1, starts, mode=1), starts, "another problem")


@pytest.mark.gpu
def test_a_cgd_tree_the_population_entry_refuses(harness, bal_path):
    pp = K.problem("ladybug-49-300")
    starts = np.stack([pp.x0, pp.x0 * 1.001])
    run = _pop_run(harness, bal_path, "ladybug-49-300", 1, 3, 1, 1, starts)
    if run.rc == 0:
        print("ladybug 49 / 300: every plan of the CGD tree is taken by the population entry on this machine")
        pytest.skip("the population entry takes ladybug 49 / 300's separator on this machine: nothing to refuse")
    print("refused: " + run.msg)
    _check_refused(run, starts, "plan_solve_population")              # the entry's own message


# ---- 6. the C entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("use_cgd", [1, 0])
def test_optba_run_samples(use_cgd, harness, bal_path, gctx):
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run_samples.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int32, C.c_int64,
                                           C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rdis_optba_run.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                   C.c_int32, C.c_void_p, C.c_void_p]
    pp = K.problem("ladybug-5-30")
    N, seed = pp.nvars, 20240611

    def args(opts):
        names, vals = [k.encode() for k in opts], list(opts.values())
        return len(names), (C.c_char_p * len(names))(*names), (C.c_double * len(vals))(*vals)

    def run(opts, nsamples, randinit=1):
        out, mem, x = np.zeros(10), np.zeros((max(nsamples, 1), 8)), np.zeros(N)
        rc = lib.rdis_optba_run_samples(bal_path, 5, 30, *args(opts), 0, nsamples, seed, randinit, v(out), v(mem), v(x))
        return rc, out, mem, x
    opts = {"SSmaxit": 3.0, "maxSweeps": 3.0, "useCGD": float(use_cgd)}
    if not use_cgd:
        opts.update({"LMmodel": 2.0, "LMsingleMinFactors": 1024.0, "lmStepDetail": 1.0})   # (the last two: accepted, ignored)
    rc4, out4, mem4, x4 = run(opts, 4)
    rc2, out2, mem2, _ = run(opts, 2)
    assert rc4 == rc2 == 0
    print("useCGD %d: starts %s -> %s, sweeps %s" % (use_cgd, mem4[:, 0].tolist(), mem4[:, 1].tolist(), mem4[:, 2].tolist()))
    assert mem4[:2].tobytes() == mem2.tobytes()                       # a member does not depend on nsamples
    finite = mem4[:, 1][~np.isnan(mem4[:, 1])]
    assert len(finite) > 0 and out4[0] == finite.min()
    best = _best_by_rule(mem4[:, 1])
    assert out4[1] == mem4[best, 0] and out4[2] == mem4[:, 3].sum() and out4[3] == mem4[:, 4].sum() and out4[9] == mem4[:, 2].max()
    assert out4[8] == (0 if use_cgd else mem4[:, 5].sum()) and out4[4] == 2 * mem4[best, 2]
    g = capi.Problem(gctx, pp)
    every = np.arange(pp.nfac, dtype=np.int64)
    g.set_x(x4)
    assert g.eval(every) == out4[0]
    # the drawn starts: restartValue(seed, 0, s, v, dom) for every variable, and their values are the members' start values
    dev, host = np.zeros((4, N)), np.zeros((4, N))
    assert harness.harness_pop_drawn_starts(bal_path, LL(5), LL(30), LL(4), C.c_ulonglong(seed), v(dev), v(host)) == 0
    assert dev.tobytes() == host.tobytes() and len(np.unique(dev[:, 0])) == 4
    for s in range(4):
        g.set_x(dev[s])
        assert g.eval(every) == mem4[s, 0], s
    # randinit 0: the file's state, one member -- rdis_optba_run's run (Levenberg-Marquardt: with LMsingleMinFactors 0)
    rc, out1, mem1, x1 = run(opts, 1, randinit=0)
    ref_opts = dict(opts)
    if not use_cgd:
        ref_opts["LMsingleMinFactors"] = 0.0
    ref_out, ref_x = np.zeros(10), np.zeros(N)
    assert lib.rdis_optba_run(bal_path, 5, 30, 0, *args(ref_opts), 0, v(ref_out), v(ref_x)) == 0
    assert rc == 0 and x1.tobytes() == ref_x.tobytes() and out1[0] == ref_out[0] and out1[1] == ref_out[1] == mem1[0, 0]
    assert (out1[2], out1[3], out1[4], out1[7], out1[8], out1[9]) == (ref_out[2], ref_out[3], ref_out[4], ref_out[7], ref_out[8], ref_out[9])
    # bad arguments
    assert run(opts, 0)[0] == -3 and run(opts, 2, randinit=0)[0] == -3 and run(opts, 2, randinit=2)[0] == -3
    for name in ("nRRperLvl", "nRRatTop", "minRR", "maxNAtoRR", "noAssignLimitAtTop", "restartSeed", "maxCalls"):
        assert run(dict(opts, **{name: 2.0}), 2)[0] == -3, name
    assert run(dict(opts, useCGD=0.5), 2)[0] == -3 and run(dict(opts, bogus=1.0), 2)[0] == -3


@pytest.mark.gpu
def test_optba_run_samples_returns_minus_two_and_stays_usable(harness, bal_path):
    """the refusals of the population run through the C entry: -2, the population released before its problem, and the next call
    of the same process gives the run it gave before"""
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run_samples.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int32, C.c_int64,
                                           C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(nc, npnt, opts, nsamples=2):
        names, vals = [k.encode() for k in opts], list(opts.values())
        out, mem = np.zeros(10), np.zeros((nsamples, 8))
        rc = lib.rdis_optba_run_samples(bal_path, nc, npnt, len(names), (C.c_char_p * len(names))(*names), (C.c_double * len(vals))(*vals), 0, nsamples, 7, 1,
                                        v(out), v(mem), None)
        return rc, out, mem
    base = {"SSmaxit": 3.0, "maxSweeps": 2.0}
    rc, out, mem = run(5, 30, dict(base, useCGD=0.0, LMmodel=2.0))
    assert rc == 0
    for use_cgd in (1.0, 0.0):
        assert run(5, 30, dict(base, useCGD=use_cgd, batch=0.0))[0] == -2          # batch = 0 has no population form
    rc49 = run(49, 300, dict(base, useCGD=1.0))[0]                                   # a CGD tree the population entry refuses
    starts = np.stack([K.problem("ladybug-49-300").x0] * 2)
    refused = _pop_run(harness, bal_path, "ladybug-49-300", 1, 3, 1, 1, starts).rc == 1
    print("ladybug 49 / 300 with useCGD 1: rdis_optba_run_samples returned %d (the driver %s the tree)" % (rc49, "refuses" if refused else "takes"))
    assert rc49 == (-2 if refused else 0)
    rc, out2, mem2 = run(5, 30, dict(base, useCGD=0.0, LMmodel=2.0))
    assert rc == 0 and mem2.tobytes() == mem.tobytes() and out2[[0, 1, 2, 3, 4, 7, 8, 9]].tobytes() == out[[0, 1, 2, 3, 4, 7, 8, 9]].tobytes()
