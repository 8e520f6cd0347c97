"""rdis_amd/csrc/lm_rules.hpp without a GPU (tests/cpp/lm_rules_test.cpp): the rules the Levenberg-Marquardt entries of the C ABI
share, each against a restatement of what the entries did when every one of them carried its own copy -- the two block-layout
scans as numpy, the two result-row loops as numpy, and the six readers' refusals as a literal table of the twelve messages."""
import os
import subprocess

import numpy as np
import pytest

from rdis_amd import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lm_rules") / "lm_rules_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", path, os.path.join(ROOT, "tests", "cpp", "lm_rules_test.cpp")])
    return path


def _run(exe, mode, text=""):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return out.stdout.splitlines()


# ---- block layout ------------------------------------------------------------------------------------------------------------------
def _layout_of_both_scans(N, cam, pt):
    """(ncams, what rdis_hip_lm_optimize's scan let pass, lm_batch_tables' `layout` flag) as the two entries computed them"""
    F = len(cam)
    minpt = min([2 ** 31 - 1] + [int(v) for v in pt])
    ncams = minpt // 9 if F > 0 else 0
    fits = [c % 9 == 0 and c < 9 * ncams and (p - 9 * ncams) % 3 == 0 for c, p in zip(cam.tolist(), pt.tolist())]
    optimize_passes = all(fits)                                      # (no factor: the loop refuses nothing)
    layout = F > 0 and (N - 9 * ncams) % 3 == 0
    if layout:
        layout = all(fits)
    return ncams, optimize_passes, layout


def _layout_cases():
    pp = P.load_bal(ncams=5, npts=30)
    cam, pt, N = pp.cam_vid0, pp.pt_vid0, pp.nvars
    i64 = lambda v: np.array(v, dtype=np.int64)
    off_cam, off_pt = cam.copy(), pt.copy()
    off_cam[3] += 1                                                  # a camera id that is no multiple of 9
    off_pt[len(pt) // 2] += 1                                        # a point id off the 3-grid (not the lowest: ncams stays 5)
    return {
        "ladybug-5-30": (N, cam, pt),
        "no-factor": (N, i64([]), i64([])),
        "camera-off-the-9-grid": (N, off_cam, pt),
        "point-off-the-3-grid": (N, cam, off_pt),
        "tail-no-whole-point-blocks": (N + 1, cam, pt),              # N - 9 ncams is no multiple of 3
        "camera-at-the-points": (N, np.concatenate([cam, i64([45])]), np.concatenate([pt, i64([48])])),
        "first-point-block-inside-a-camera": (N, i64([0, 9]), i64([22, 25])),   # minpt 22: ncams 2, (22 - 18) % 3 != 0
    }


def test_block_layout_is_both_entries_scans(exe):
    cases = _layout_cases()
    text = "".join("%d %d %s %s\n" % (N, len(cam), " ".join(map(str, cam.tolist())), " ".join(map(str, pt.tolist()))) for N, cam, pt in cases.values())
    rows = _run(exe, "layout", text)
    assert len(rows) == len(cases)
    seen = set()
    for (name, (N, cam, pt)), row in zip(cases.items(), rows):
        ncams, fit, whole = (int(v) for v in row.split())
        want_ncams, optimize_passes, layout = _layout_of_both_scans(N, cam, pt)
        assert ncams == want_ncams, name
        assert bool(fit) == optimize_passes, name                                  # rdis_hip_lm_optimize refuses on this flag alone
        assert bool(whole) == ((N - 9 * want_ncams) % 3 == 0), name
        assert (len(cam) > 0 and bool(whole) and bool(fit)) == layout, name         # lm_batch_tables' flag from F > 0 and both
        seen.add((len(cam) > 0, bool(fit), bool(whole)))
    assert cases["ladybug-5-30"][0] == 135 and rows[0] == "5 1 1" and rows[1] == "0 1 1"
    assert {(True, True, True), (False, True, True), (True, False, True), (True, True, False)} <= seen


# ---- result rows -------------------------------------------------------------------------------------------------------------------
ROWS, NCOMP, RES = 3, 2, 12
SENTINEL, SENTINEL_N = -7.5, -7


def _result_block(cap, rng):
    """3 rows x 2 components of result rows; the record counts lie below the cap, at it and above it (and at zero)"""
    n = ROWS * NCOMP
    res = rng.standard_normal((n, RES))
    res[:, 10] = [0, 1, 3, 4, 5, 9]                                  # against a cap of 4: below, below, below, at, above, above
    hist = rng.standard_normal((n, cap, 4))
    return res, hist


def _rows_restated(res, hist, cap, mask):
    """the loop rdis_hip_lm_batch and lm_plan_download each had, on sentinel-filled destinations"""
    n = len(res)
    fret, delta, info8 = np.full(n, SENTINEL), np.full(n, SENTINEL), np.full((n, 8), SENTINEL)
    nhist, hist4 = np.full(n, SENTINEL_N, dtype=np.int64), np.full((n, cap, 4), SENTINEL)
    for cc in range(n):
        r = res[cc]
        if mask & 1:
            fret[cc] = r[0]
        if mask & 2:
            delta[cc] = r[0] - r[1]
        if mask & 4:
            info8[cc] = r[2:10]
        if mask & 8:
            nhist[cc] = int(r[10])
        if mask & 16 and cap > 0:
            k = min(int(r[10]), cap)
            hist4[cc, :k] = hist[cc, :k]
    return fret, delta, info8, nhist, hist4


@pytest.mark.parametrize("cap", [0, 4])
def test_result_rows_are_both_entries_loops(cap, exe):
    rng = np.random.default_rng(20 + cap)
    res, hist = _result_block(cap, rng)
    masks = [1, 2, 4, 8, 16, 31]                                     # every output pointer alone, and all together
    hexes = lambda a: " ".join(float(v).hex() for v in np.asarray(a).ravel())
    text = "".join("%d %d %d %s %s\n" % (ROWS * NCOMP, cap, m, hexes(res), hexes(hist)) for m in masks)
    lines = _run(exe, "rows", text)
    assert len(lines) == 5 * len(masks)
    for i, m in enumerate(masks):
        got = lines[5 * i:5 * i + 5]
        want = _rows_restated(res, hist, cap, m)
        for bit, (g, w) in enumerate(zip(got, want)):
            if not m >> bit & 1:
                assert g == "-"
            elif bit == 3:
                assert [int(v) for v in g.split()] == w.tolist()
            else:
                assert np.array([float.fromhex(v) for v in g.split()]).tobytes() == w.ravel().tobytes(), (cap, m, bit)
    if cap > 0:                                                      # entries beyond min(nhist, cap) keep the sentinel, the ones below are the source's
        h = _rows_restated(res, hist, cap, 16)[4]
        assert np.all(h[0] == SENTINEL) and np.all(h[1, 1:] == SENTINEL) and np.all(h[1, 0] == hist[1, 0]) and np.all(h[2, 3] == SENTINEL)
        assert h[3:].tobytes() == hist[3:].tobytes()


# ---- last-solve refusals -----------------------------------------------------------------------------------------------------------
# reader: (the kinds of last solve it reads, its message before any solve, its message after a solve of another kind); kinds:
# 0 none, 1 rdis_hip_lm_plan_solve, 2 a population solve, 3 a multi-start solve.  The order is lm_rules.hpp's enum LmReader.
REFUSALS = [
    ("fetch", {1, 3}, "lm_plan_fetch: nothing was solved yet",
     "lm_plan_fetch: the last solve was a population solve (rdis_hip_lm_plan_fetch_population)"),
    ("fetch_population", {2}, "lm_plan_fetch_population: nothing was solved yet",
     "lm_plan_fetch_population: the last solve was not a population solve (rdis_hip_lm_plan_fetch)"),
    ("fetch_starts", {3}, "lm_plan_fetch_starts: nothing was solved yet",
     "lm_plan_fetch_starts: the last solve was not a multi-start solve (rdis_hip_lm_plan_fetch, rdis_hip_lm_plan_fetch_population)"),
    ("objective_device", {1, 3}, "lm_plan_objective_device: nothing was solved yet",
     "lm_plan_objective_device: the last solve was a population solve (its members have no common objective)"),
    ("summary_device", {1, 3}, "lm_plan_summary: nothing was solved yet",
     "lm_plan_summary: the last solve was a population solve (its members have no common summary)"),
    ("summary_population_device", {2}, "lm_plan_summary_population: nothing was solved yet",
     "lm_plan_summary_population: the last solve was not a population solve (rdis_hip_lm_plan_summary)"),
]


def test_last_solve_refusals_are_the_six_entries_messages(exe):
    lines = _run(exe, "refusals")
    assert len(lines) == 6 * 4
    for reader, (_, allowed, nothing, wrong) in enumerate(REFUSALS):
        for kind in range(4):
            want = "-" if kind in allowed else nothing if kind == 0 else wrong
            assert lines[4 * reader + kind] == "%d %d %s" % (reader, kind, want)
    assert len({m for r in REFUSALS for m in r[2:]}) == 12
