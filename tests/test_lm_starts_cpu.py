"""Multi-start solves of Levenberg-Marquardt plans (rdis_hip_lm_plan_solve_starts; include/rdis_hip.h) without a GPU: the
library exports the entries; the buffers are laid out as rdis_amd/csrc/replica_layout.hpp's lm_starts_layout says and the two
int32 tables and the select scan of rdis_amd/csrc/lm_starts.hpp do what the kernels rely on (tests/cpp/lm_starts_layout_test.cpp);
and the starts tests/test_gpu_lm_starts.py uses discriminate: the oracle's winners differ between components and no winner is
close to the second."""
import os
import struct
import subprocess

import numpy as np
import pytest

from rdis_amd import capi

import lm_batch_shapes as S
import lm_starts_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["rdis_hip_lm_plan_solve_starts", "rdis_hip_lm_plan_solve_starts_population", "rdis_hip_lm_plan_fetch_starts",
           "rdis_hip_lm_plan_objective_device"]


def test_library_exports_the_starts_entries():
    lib = capi.load_library()
    with open(os.path.join(ROOT, "include", "rdis_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None and "int %s(" % name in header
    assert lib.rdis_hip_lm_plan_solve_starts(None, 1, None, 5, 1e-8) == -1
    assert lib.rdis_hip_lm_plan_solve_starts_population(None, None, 0, 1, 5, 1e-8) == -1
    assert lib.rdis_hip_lm_plan_fetch_starts(None, None, None, None, None, None, None, None) == -1
    assert lib.rdis_hip_lm_plan_objective_device(None, None) == -1
    assert "#define RDIS_HIP_ABI_VERSION 1\n" in header
    for method in ("solve_starts", "solve_starts_population", "fetch_starts", "objective"):
        assert hasattr(capi.LmPlan, method)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lm_starts") / "lm_starts_layout_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", path, os.path.join(ROOT, "tests", "cpp", "lm_starts_layout_test.cpp")])
    return path


def _run(exe, mode, text=""):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return out.stdout.splitlines()


def test_layout_of_a_starts_solve(exe):
    """the program's own checks (field order, no overlap, 8-byte alignment, the winners' row after nstarts rows, best behind the
    rows, the row of N doubles in a start's budget, budgets of nothing, one start and all starts), and every figure it prints
    against the same arithmetic written out here"""
    rows = _run(exe, "layout")
    assert rows[-1] == "ok" and len(rows) == 6
    for row in rows[:-1]:
        w = row.split()
        assert w[0] == "lmstarts"
        nc, rd, cap, nfr, ws, N, n, per, o_res, o_hist, o_x, w_res, w_hist, w_x, o_best, total, start, s_ws, s_rows, work = (int(v) for v in w[1:])
        assert rd == 12
        res, hist, x = nc * 12 * 8, nc * cap * 4 * 8, nfr * 8                 # a row of each field, in bytes
        assert (o_res, o_hist, o_x) == (0, (n + 1) * res, (n + 1) * (res + hist))   # [n + 1][ncomp][12], [n + 1][ncomp][cap][4], [n + 1][nfree]
        assert (w_res, w_hist, w_x) == (n * res, o_hist + n * hist, o_x + n * x)   # the winners: row n of each
        assert o_best == (n + 1) * (res + hist + x) and o_best % 8 == 0       # best[ncomp] behind the rows
        assert total == o_best + (4 * nc + 7) // 8 * 8
        assert start == 8 * (ws + N)                                          # a start of a launch: its slices and its row of x
        assert (s_ws, s_rows, work) == (0, per * 8 * ws, per * start)         # [per][ws], [per][N]


def _lists():
    """free lists (N, free_ptr, free_vid): ascending, the components reversed, and free variables inside blocks next to constants"""
    asc = (45, [0, 9, 18, 45], list(range(45)))
    comps = [list(range(45 + 3 * p, 48 + 3 * p)) for p in range(30)][::-1]
    rev = (135, list(np.concatenate([[0], np.cumsum([len(c) for c in comps])])), [v for c in comps for v in c])
    sub = (135, [0, 45, 45, 51], list(range(0, 6)) + list(range(27, 36)) + list(range(45, 75)) + [100, 99, 98, 6, 7, 8])
    return {"ascending": asc, "reversed": rev, "sub-block": sub}


@pytest.mark.parametrize("kind", ["ascending", "reversed", "sub-block"])
def test_tables_of_a_free_list(kind, exe):
    N, fp, fv = _lists()[kind]
    assert len(set(fv)) == len(fv) == fp[-1]
    rows = _run(exe, "tables", "%d %d\n%s\n%s\n" % (N, len(fp) - 1, " ".join(map(str, fp)), " ".join(map(str, fv))))
    pos, comp_of = (np.array(r.split(), dtype=np.int64) for r in rows[:2])
    assert pos.shape == (N,) and comp_of.shape == (len(fv),)
    fv = np.array(fv)
    off = np.setdiff1d(np.arange(N), fv)
    assert np.all(pos[off] == -1) and np.all(pos[fv] >= 0)                     # -1 exactly off the free list
    assert np.array_equal(fv[pos[fv]], fv) and np.array_equal(pos[fv], np.arange(len(fv)))
    want = np.repeat(np.arange(len(fp) - 1), np.diff(fp))                      # comp_of matches free_ptr
    assert np.array_equal(comp_of, want)
    for k, c in enumerate(comp_of):
        assert fp[c] <= k < fp[c + 1]
    if kind == "reversed":
        assert np.any(np.diff(pos[np.sort(fv)]) < 0)                           # (pos is not monotone)


def _bits(a):
    return "\n".join(" ".join("%x" % struct.unpack("<Q", struct.pack("<d", v))[0] for v in row) for row in a)


def test_select_scan_against_numpy(exe):
    """the kernel's scan (lm_starts_best over a component's fret, with the result rows' strides) against the rule in numpy, on
    tables that hold ties, -0.0 against +0.0, single NaNs, an all-NaN column, infinities, and one start alone"""
    nan, inf = float("nan"), float("inf")
    cols = [
        ([3.0, 1.0, 2.0, 1.5], 1),              # plain
        ([2.0, 1.0, 1.0, 1.0], 1),              # a tie: the lowest index
        ([1.0, 1.0, 1.0, 1.0], 0),
        ([0.0, -0.0, 0.0, -0.0], 0),            # -0.0 against +0.0 is a tie
        ([1.0, -0.0, 0.0, 2.0], 1),
        ([1.0, 0.0, -0.0, 2.0], 1),
        ([nan, 5.0, 4.0, 6.0], 2),              # single NaNs never win
        ([4.0, nan, 4.0, 3.0], 3),
        ([nan, nan, nan, 7.0], 3),
        ([nan, nan, 7.0, nan], 2),
        ([nan, nan, nan, nan], 0),              # all NaN: 0
        ([nan, inf, inf, nan], 1),              # an infinity is a number
        ([inf, -inf, nan, -inf], 1),
        ([5.0, 4.0, 3.0, 2.0], 3),              # the last start
    ]
    table = np.array([c for c, _ in cols]).T
    want = np.array([b for _, b in cols])
    assert np.array_equal(K.select(table), want)                               # (the numpy rule itself, on the literal cases)
    got = np.array(_run(exe, "select", "%d %d\n%s\n" % (table.shape + (_bits(table),)))[0].split(), dtype=np.int64)
    assert np.array_equal(got, want)
    # random tables with many ties, NaNs and signed zeros; S = 1 .. 9
    rng = np.random.default_rng(5)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.0, -3.0, nan, nan, inf, 1e-300])
    for nstarts in (1, 2, 3, 9):
        t = rng.choice(pool, size=(nstarts, 200))
        got = np.array(_run(exe, "select", "%d %d\n%s\n" % (t.shape + (_bits(t),)))[0].split(), dtype=np.int64)
        assert np.array_equal(got, K.select(t)), nstarts
        if nstarts == 1:
            assert np.all(got == 0)


# the winners' spread over the six starts and the smallest gap, as measured when the shapes were chosen
SPREAD = {"ladybug-5-30-points": ([4, 6, 4, 4, 7, 5], 1.6e-4), "ladybug-5-30-cameras": ([1, 0, 1, 0, 2, 1], 2.3e-2),
          "synthetic-6x3x40": ([2, 0, 2, 0, 1, 1], 2.6e-2), "synthetic-2x16x60": ([0, 0, 0, 0, 1, 1], 7.7e-2)}


@pytest.mark.parametrize("name", K.ORACLE_NAMES)
def test_the_gpu_tests_inputs_discriminate(name):
    """the oracle (model 1) from the six starts of a shape: at least two distinct winners occur, and no component's best fret is
    closer than 1e-6 (relative) to its second -- a device whose frets agree with the oracle's to _compare's 1e-8 picks the same
    winners, and a select that ignored the values would be seen.  (Model 2 on the point shape converges every start to one
    minimum, gaps of 1e-13: it serves == comparisons only.)"""
    f = K.oracle_frets(name, 1)
    comps = S.shape(name)[1]
    assert f.shape == (K.NSTARTS, len(comps)) and not np.any(np.isnan(f))
    best = K.select(f)
    spread = np.bincount(best, minlength=K.NSTARTS).tolist()
    gap = K.smallest_gap(f)
    print("LM starts, %s, model 1: winners per start %s, smallest gap %.1e" % (name, spread, gap))
    assert len(set(best.tolist())) >= 2
    assert gap >= 1e-6
    assert spread == SPREAD[name][0] and 0.5 * SPREAD[name][1] <= gap <= 2.0 * SPREAD[name][1]
    X = K.rows(name)
    free = np.concatenate([fr for fr, _ in comps])
    for s in range(1, K.NSTARTS):                                              # the starts differ from one another where they are free
        for t in range(s):
            assert np.count_nonzero(X[s, free] != X[t, free]) > 0.9 * len(free)
