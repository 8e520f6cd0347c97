"""The level driver on Levenberg-Marquardt plans (optBA's useCGD = false) without a GPU: where a component goes
(rdis_amd/host/lm_routing.h, a pure host rule: tests/cpp/lm_routing_test.cpp), that the level trees of the shapes
tests/test_gpu_lm_levels.py runs hand the optimiser the classes that file is meant to cover -- oracle/levels.py on the CPU; if a
shape drifted, the GPU tests would silently stop covering a class --, and that the library, the header and the binding name the
step summary's two entries."""
import os
import subprocess

import numpy as np
import pytest

from rdis_amd import capi

import lm_levels_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lm_levels") / "lm_routing_test")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", path, os.path.join(ROOT, "tests", "cpp", "lm_routing_test.cpp")])
    return path


def _run(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return [int(v) for v in out.stdout.split()]


PLAN, SINGLE = 0, 1
# (active cameras, factors, LMsingleMinFactors) -> route
ROUTES = [
    ((0, 0, 0), PLAN), ((0, 7, 0), PLAN), ((1, 385, 0), PLAN), ((16, 10, 0), PLAN), ((17, 1072, 0), PLAN),
    ((64, 5, 0), PLAN), ((65, 5, 0), SINGLE), ((89, 1071, 0), SINGLE), ((1000, 1, 0), SINGLE),
    # threshold 0 (off) never sends a component of at most 64 cameras away, however many factors it has
    ((46, 30594, 0), PLAN), ((64, 10 ** 9, 0), PLAN), ((5, 121, -1), PLAN),
    # threshold t sends exactly the components with at least t factors
    ((5, 120, 121), PLAN), ((5, 121, 121), SINGLE), ((5, 122, 121), SINGLE), ((0, 3, 3), SINGLE), ((0, 2, 3), PLAN),
    ((46, 30594, 30594), SINGLE), ((46, 30593, 30594), PLAN), ((64, 1, 1), SINGLE), ((64, 0, 1), PLAN),
    # beyond 64 cameras the threshold does not matter
    ((65, 0, 10 ** 6), SINGLE), ((65, 10, 1), SINGLE),
]


def test_routing_rule(exe):
    got = _run(exe, "route", "".join("%d %d %d\n" % k for k, _ in ROUTES))
    assert got[0] == capi.LM_WIDE_MAX_CAMERAS == K.WIDE_MAX_CAMERAS == 64
    assert got[1:] == [r for _, r in ROUTES]
    # ... and over a grid against the rule written out: more than 64 cameras, or a threshold that is on and reached
    grid = [(c, f, t) for c in (0, 1, 16, 17, 63, 64, 65, 66, 200) for f in (0, 1, 9, 10, 11, 5000) for t in (0, 1, 10, 11, 5001)]
    got = _run(exe, "route", "".join("%d %d %d\n" % k for k in grid))[1:]
    assert got == [int(c > 64 or (t > 0 and f >= t)) for c, f, t in grid]


def test_active_cameras_of_a_free_list(exe):
    """camera blocks among a component's free variables: ids below 9 * ncams, nine a camera; sorted lists (what the level tree
    hands over), a partly free camera, points only, and an unsorted list with a camera named twice"""
    cases = [
        (5, list(range(45)) + [45, 46, 47], 5),
        (5, [45, 46, 47], 0),
        (5, [], 0),
        (20, [9, 10, 11, 27, 180, 181, 182], 2),
        (90, list(range(0, 810, 9)), 90),
        (5, [40, 3, 41, 20, 4, 46], 3),
    ]
    for ncams, vids, want in cases:
        assert _run(exe, "cameras", "%d %d\n%s\n" % (ncams, len(vids), " ".join(map(str, vids)))) == [want], (ncams, vids)


def _classes(name):
    return [(d, k, sorted(set(c[3] for c in comps))) for d, k, comps in K.shapes(name)]


def _big(name, launch):
    """the components of a launch that are not single points, as (cameras, points, factors)"""
    return [c[:3] for c in K.shapes(name)[launch][2] if not (c[0] == 0 and c[1] == 1)]


def test_level_tree_shapes_cover_the_classes():
    # ladybug 5/30 and 8/30: one separator (class 1 / class 2), 29 single points
    for name, sep, cls in (("ladybug-5-30", (5, 1, 121), 1), ("ladybug-8-30", (8, 1, 164), 2)):
        s = K.shapes(name)
        assert [(d, k, len(c)) for d, k, c in s] == [(0, 0, 1), (1, 1, 29)]
        assert s[0][2] == [sep + (cls,)] and all(c == (0, 1, c[2], 0) for c in s[1][2])
    # ladybug 8/300's point plan: more components than the summary kernel has lanes
    s = K.shapes("ladybug-8-300")
    assert len(s) == 2 and len(s[1][2]) == 299 > 256 and set(c[3] for c in s[1][2]) == {0}
    # ladybug 20/120: a separator of 17 camera blocks -- the wide class -- and leaves of mixed classes
    assert K.shapes("ladybug-20-120")[0][2] == [(17, 1, 1072, 3)]
    assert _big("ladybug-20-120", 1) == [(2, 7, 89), (1, 25, 385)] and len(K.shapes("ladybug-20-120")[1][2]) == 89
    assert _classes("ladybug-20-120") == [(0, 0, [3]), (1, 1, [0, 1])]
    # ... with sepPiecePct 0.5: four launches a sweep, separators at depths 0 and 1, leaves at depths 1 and 2
    s = K.shapes("ladybug-20-120-pieces")
    assert [(d, k) for d, k, _ in s] == [(0, 0), (1, 0), (1, 1), (2, 1)]
    assert s[0][2] == [(14, 1, 965, 2)] and s[1][2] == [(3, 1, 122, 1)]
    assert _classes("ladybug-20-120-pieces")[2:] == [(1, 1, [0]), (2, 1, [0, 1])]
    # ladybug 49/300: a wide separator and a wide leaf beside a class-2 one
    assert K.shapes("ladybug-49-300")[0][2] == [(21, 1, 2622, 3)]
    assert _big("ladybug-49-300", 1) == [(17, 35, 416), (8, 65, 1157)]
    # the synthetic 160 x 400 problem: a separator of 89 camera blocks, beyond every plan; leaves of all four classes
    s = K.shapes("synthetic-160-400")
    assert s[0][2] == [(89, 1, 1071, K.BEYOND)]
    big = _big("synthetic-160-400", 1)
    assert (24, 51, 204) in big and (10, 23, 92) in big and (8, 21, 84) in big and (6, 18, 72) in big
    assert _classes("synthetic-160-400") == [(0, 0, [K.BEYOND]), (1, 1, [0, 1, 2, 3])]
    assert sum(1 for _, _, comps in s for c in comps if c[3] == K.BEYOND) == 1


ENTRIES = ["rdis_hip_lm_plan_summary_device", "rdis_hip_lm_plan_summary"]


def test_library_header_and_binding_name_the_summary_entries():
    lib = capi.load_library()
    with open(os.path.join(ROOT, "include", "rdis_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None and "int %s(" % name in header
    assert "#define RDIS_HIP_LM_SUMMARY_DOUBLES 16\n" in header and capi.LM_SUMMARY_DOUBLES == 16
    assert "#define RDIS_HIP_ABI_VERSION 1\n" in header
    assert lib.rdis_hip_lm_plan_summary_device(None, None) == -1 and lib.rdis_hip_lm_plan_summary(None, None) == -1
    assert hasattr(capi.LmPlan, "summary")
    # the caller-side entry documents the switch
    with open(os.path.join(ROOT, "include", "rdis_optba.h")) as fh:
        optba = fh.read()
    for word in ("useCGD", "LMmodel", "LMsingleMinFactors"):
        assert word in optba
