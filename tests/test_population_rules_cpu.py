"""rdis_amd/csrc/population_rules.hpp without a GPU (tests/cpp/population_rules_test.cpp): the rules the population entries of the
C ABI share, each against the messages the entries carried when every one of them typed its own copy.  Every message here is a
literal copied from that text and compared whole; tests/test_gpu_population_refusals.py walks the same ones through the library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("population_rules") / "population_rules_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", path, os.path.join(ROOT, "tests", "cpp", "population_rules_test.cpp")])
    return path


def _run(exe, mode, text=""):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return out.stdout.splitlines()


# ---- member and value range ----------------------------------------------------------------------------------------------------------
# (first, count, n, has_vid, nmembers, N) -> None: in range, or (code, what follows "who: ")
RANGE_CASES = [
    ((0, 4, 135, 0, 4, 135), None),
    ((0, 0, 0, 0, 4, 135), None),
    ((4, 0, 135, 0, 4, 135), None),                                   # first == nmembers with count == 0 passes
    ((3, 1, 135, 0, 4, 135), None),
    ((4, 1, 135, 0, 4, 135), (EINVAL, "members out of range")),
    ((5, 0, 135, 0, 4, 135), (EINVAL, "members out of range")),
    ((-1, 1, 135, 0, 4, 135), (EINVAL, "members out of range")),
    ((0, -1, 135, 0, 4, 135), (EINVAL, "members out of range")),
    ((3, 2, 135, 0, 4, 135), (EINVAL, "members out of range")),
    ((1, "max", 135, 0, 4, 135), (EINVAL, "members out of range")),   # count > nmembers - first: nothing is added, nothing overflows
    (("max", "max", 135, 0, 4, 135), (EINVAL, "members out of range")),
    (("max", 0, 135, 0, "max", 135), None),
    ((0, "max", 0, 0, "max", 135), None),                             # (no value: 0 is not too many)
    (("min", 1, 135, 0, 4, 135), (EINVAL, "members out of range")),
    ((0, "min", 135, 0, 4, 135), (EINVAL, "members out of range")),
    ((0, 4, 136, 0, 4, 135), (EINVAL, "n > nvars")),
    ((0, 4, 136, 1, 4, 135), None),                                   # a list may be longer than nvars (its ids are checked where they are staged)
    ((0, 0, 136, 0, 4, 135), (EINVAL, "n > nvars")),
    ((0, 5, 136, 0, 4, 135), (EINVAL, "members out of range")),       # the members first
    ((0, 3000000000, 3000000, 1, 4000000000, 135), (ERANGE, "too many values")),      # 9.0e15 exactly
    ((0, 3000000000, 2999999, 1, 4000000000, 135), None),
    ((0, 3000000000, 3000000, 0, 4000000000, 3000000), (ERANGE, "too many values")),
    ((0, 3000000000, 3000001, 0, 4000000000, 3000000), (EINVAL, "n > nvars")),        # n > nvars before too many
]
WHO = ["population_set_x", "population_get_x", "population_sample", "population_eval_grad"]


def test_range_refusals_are_the_entries_messages(exe):
    text = "".join("%s %s\n" % (who, " ".join(map(str, args))) for who in WHO for args, _ in RANGE_CASES)
    lines = _run(exe, "range", text)
    assert len(lines) == len(WHO) * len(RANGE_CASES)
    it = iter(lines)
    for who in WHO:
        for args, want in RANGE_CASES:
            assert next(it) == ("0 -" if want is None else "%d %s: %s" % (want[0], who, want[1])), (who, args)
    # whole strings, as the entries typed them
    i = [a for a, _ in RANGE_CASES].index((4, 1, 135, 0, 4, 135))
    assert lines[i] == "-1 population_set_x: members out of range"
    assert lines[len(RANGE_CASES) + [a for a, _ in RANGE_CASES].index((0, 4, 136, 0, 4, 135))] == "-1 population_get_x: n > nvars"
    assert lines[2 * len(RANGE_CASES) + len(RANGE_CASES) - 4] == "-5 population_sample: too many values"


def test_too_many_is_one_bound(exe):
    cases = [((2 ** 31 - 1, 1), "0 0"), ((2 ** 31, 1), "0 1"), ((2 ** 31, 0), "0 1"), ((3000000000, 3000000), "1 1"),
             ((1000000, 9000000000), "1 1"), ((1000000, 8999999999), "0 0"), ((1, 9 * 10 ** 15), "1 1"), ((1, 9 * 10 ** 15 - 1), "0 0"),
             (("max", "max"), "1 1"), ((0, "max"), "0 0")]
    lines = _run(exe, "many", "".join("%s %s\n" % c for c, _ in cases))
    assert lines == [w for _, w in cases]


# ---- permutation ---------------------------------------------------------------------------------------------------------------------
def test_permutation_refusals_carry_their_indices(exe):
    cases = [
        ([0, 1, 2, 3], "-"),
        ([3, 2, 1, 0], "-"),
        ([2, 0, 3, 1], "-"),
        ([], "-"),
        ([0], "-"),
        ([0, 4, 1, 2], "population_permute: order[1] = 4 is out of range (the population has 4 members)"),
        ([-1, 0, 1, 2], "population_permute: order[0] = -1 is out of range (the population has 4 members)"),
        ([0, 1, 2, "max"], "population_permute: order[3] = 9223372036854775807 is out of range (the population has 4 members)"),
        ([1], "population_permute: order[0] = 1 is out of range (the population has 1 members)"),
        ([2, 0, 2, 1], "population_permute: member 2 is named twice (order[2]): not a permutation"),      # at its second position
        ([0, 0, 0, 0], "population_permute: member 0 is named twice (order[1]): not a permutation"),
        ([1, 1, 9, 0], "population_permute: member 1 is named twice (order[1]): not a permutation"),      # the first fault in list order
        ([1, 9, 1, 0], "population_permute: order[1] = 9 is out of range (the population has 4 members)"),
    ]
    lines = _run(exe, "permute", "".join("%d %s\n" % (len(o), " ".join(map(str, o))) for o, _ in cases))
    assert lines == [w for _, w in cases]


# ---- sampling intervals --------------------------------------------------------------------------------------------------------------
TOGETHER = "population_set_sampling: lo and hi are given together (both NULL: the problem's domains)"
INTERVAL = "population_set_sampling: variable %d: the sampling interval must be finite with lo <= hi"


def test_sampling_refusals(exe):
    ok_lo, ok_hi = [-1.0, 0.0, 2.5], [1.0, 0.0, 3.0]                 # (lo == hi is an interval)
    cases = [
        (0, ok_lo, ok_hi, "-"),
        (3, ok_lo, ok_hi, "-"),                                       # both NULL: the problem's domains, nothing to refuse
        (1, ok_lo, ok_hi, TOGETHER),
        (2, ok_lo, ok_hi, TOGETHER),
        (1, ["nan", 0, 0], ok_hi, TOGETHER),                          # (before any interval is looked at)
        (0, [-1.0, 0.5, 2.5], [1.0, 0.25, 3.0], INTERVAL % 1),
        (0, ok_lo, [1.0, 0.0, "inf"], INTERVAL % 2),
        (0, ["-inf", 0.0, 2.5], ok_hi, INTERVAL % 0),
        (0, ["nan", 0.0, 2.5], ok_hi, INTERVAL % 0),
        (0, ok_lo, [1.0, "nan", 3.0], INTERVAL % 1),
        (0, [-1.0, 9.0, "nan"], ok_hi, INTERVAL % 1),                 # the first such variable
    ]
    text = "".join("3 %d %s %s\n" % (w, " ".join(map(str, lo)), " ".join(map(str, hi))) for w, lo, hi, _ in cases)
    lines = _run(exe, "sampling", text)
    assert lines == [w for *_, w in cases]
    assert INTERVAL % 1 == "population_set_sampling: variable 1: the sampling interval must be finite with lo <= hi"


# ---- "no current values" -------------------------------------------------------------------------------------------------------------
NO_VALUES = [
    "population_best: the population has no current values (evaluate first: rdis_hip_population_eval or _eval_device after the last "
    "population_set_x / plan_solve_population)",
    "population_assign_best: the population has no current values (evaluate first: rdis_hip_population_eval or _eval_device after the last "
    "population_set_x / plan_solve_population)",
    "population_sort: the population has no current values (evaluate first: rdis_hip_population_eval or _eval_device after the last "
    "population_set_x / population_sample / plan_solve_population)",
]


def test_no_current_values_is_each_readers_text(exe):
    assert _run(exe, "novalues") == ["%d %s" % (r, m) for r, m in enumerate(NO_VALUES)]
    assert "population_sample" in NO_VALUES[2] and "population_sample" not in NO_VALUES[0] + NO_VALUES[1]   # the two texts differ
