"""rdis_amd/csrc/plan_index.hpp -- the index a plan is created from: validation of the caller's component lists, v2s_ptr /
slot_base / slot_pos, the slots' component-local indices, the heaviest-first order, the camera-block tables, the packed int32
block -- without a GPU.  tests/cpp/plan_index_test.cpp runs plan_index_check + plan_index_build on the problems and calls given
here; its tables are compared entry for entry with restate() below (numpy, written from the tables' definitions: a lookup of every
slot's variable in the free list, a stable sort by that position), and every refusal with its exact code and message."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EOVERLAP, ERANGE = -1, -4, -5
BLOCK = ("order", "free_ptr", "free_vid", "fac_ptr", "fac_id", "v2s_ptr", "slot_base", "slot_pos", "cb_ptr", "cb", "cb_li")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("plan_index") / "plan_index_test")
    subprocess.check_call([hipcc, "-x", "c++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "plan_index_test.cpp")],
                          stderr=subprocess.DEVNULL)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# problems and calls

class BA:
    """four cameras (blocks of 9 at 0, 9, 18, 27), eight points (blocks of 3 from 36), two variables in no block"""
    kind = "ba"
    N = 62
    PAIRS = [(0, 0), (1, 2), (1, 0), (0, 2), (2, 3), (0, 3), (3, 4), (0, 4), (3, 1), (1, 1), (2, 7), (1, 2), (2, 5), (3, 5)]

    def __init__(self):
        self.cam = np.array([9 * c for c, _ in self.PAIRS])
        self.pt = np.array([36 + 3 * q for _, q in self.PAIRS])
        self.F = len(self.PAIRS)
        self.block_of = np.full(self.N, -1)
        self.block_of[:36] = 9 * (np.arange(36) // 9)
        self.ncam_blocks = 4

    def vars_of(self, f):
        return np.concatenate([self.cam[f] + np.arange(9), self.pt[f] + np.arange(3)])

    def text(self):
        return "problem ba %d %d %s %s %d %s\n" % (self.N, self.F, _j(self.cam), _j(self.pt), self.ncam_blocks, _j(self.block_of))


class NLP:
    """thirteen variables, factors of arity 1, 2 and 5"""
    kind = "nlp"
    N = 13
    ROWS = [[0], [1, 2], [3, 4, 5, 6, 7], [2, 8], [8], [9, 10], [10, 3, 8, 11, 6]]

    def __init__(self):
        self.F = len(self.ROWS)
        self.rowptr = np.concatenate([[0], np.cumsum([len(r) for r in self.ROWS])])
        self.vid = np.concatenate(self.ROWS)
        self.block_of = np.full(self.N, -1)
        self.ncam_blocks = 0

    def vars_of(self, f):
        return np.array(self.ROWS[f])

    def text(self):
        return "problem nlp %d %d %s %d %s\n" % (self.N, self.F, _j(self.rowptr), len(self.vid), _j(self.vid))


def _j(a):
    return " ".join(str(int(x)) for x in a)


def _csr(lists):
    return [0] + list(np.cumsum([len(x) for x in lists])), [x for part in lists for x in part]


# Bundle adjustment, five components (free variables, factors), in this order:
#   no factors (point 7, which only the unlisted factor 10 reads);
#   point 3 and the FIRST rotation variable of camera 2 alone, three factors;
#   camera 1 with four of its nine variables free, two of them rotation variables (10, 11; not 9), listed out of order, and
#     point 2, five factors out of id order;
#   no free variables, one factor over constants;
#   camera 3 whole, listed out of order, and two of point 4's three variables, three factors (as many as the second: stable order).
# Camera 0 and points 0, 1, 5 are constants that several components read.
BA_COMPS = [([57, 58, 59], []),
            ([45, 46, 47, 18], [5, 4, 12]),
            ([11, 10, 16, 13, 42, 43, 44], [11, 1, 2, 3, 9]),
            ([], [0]),
            ([31, 27, 35, 28, 29, 30, 34, 33, 32, 49, 48], [6, 7, 8])]
BA_ORDER = [2, 1, 4, 3, 0]
# Nonlinear products, four components: no factors; {1, 0} under three factors; no free variables; {5, 4, 7} under three factors.
# Variables 2, 3, 6, 8, 9, 10, 11 are constants, 8 read by three of the components.
NLP_COMPS = [([12], []), ([1, 0], [1, 0, 3]), ([], [4]), ([5, 4, 7], [6, 2, 5])]
NLP_ORDER = [1, 3, 2, 0]


def call_text(free_lists, fac_lists, free_ptr=None, fac_ptr=None, null_free=False, null_fac=False):
    fp, fv = _csr(free_lists)
    gp, gi = _csr(fac_lists)
    fp = fp if free_ptr is None else free_ptr
    gp = gp if fac_ptr is None else fac_ptr
    return "call %d %s %s %s %s\n" % (len(fp) - 1, _j(fp), "-1" if null_free else "%d %s" % (len(fv), _j(fv)),
                                      _j(gp), "-1" if null_fac else "%d %s" % (len(gi), _j(gi)))


def comps_text(comps):
    return call_text([c[0] for c in comps], [c[1] for c in comps])


def run(exe, text):
    """the program's answers, one per call: (code, message, tables or None)"""
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok"
    answers, i = [], 0
    while i < len(lines) - 1:
        head = lines[i].split(" ", 2)
        assert head[0] == "rc"
        code, message, tables = int(head[1]), head[2] if len(head) > 2 else "", None
        i += 1
        if code == 0:
            tables = {}
            while lines[i] != "end":
                parts = lines[i].split()
                tables[parts[0]] = np.array(parts[1:], dtype=np.int64)
                i += 1
            i += 1
        answers.append((code, message, tables))
    return answers


# ---------------------------------------------------------------------------------------------------------------------
# the restatement

def restate(pb, comps):
    free_ptr, free_vid = (np.array(a, dtype=np.int64) for a in _csr([c[0] for c in comps]))
    fac_ptr, fac_id = (np.array(a, dtype=np.int64) for a in _csr([c[1] for c in comps]))
    ncomp, nfree = len(comps), len(free_vid)
    where = np.full(pb.N, -1, dtype=np.int64)                 # a variable's position in the plan's free list
    where[free_vid] = np.arange(nfree)
    slot_vars = [pb.vars_of(f) for f in fac_id]
    arity = np.array([len(v) for v in slot_vars], dtype=np.int64)
    sv = np.concatenate(slot_vars) if len(slot_vars) else np.zeros(0, dtype=np.int64)
    g = where[sv]                                             # per listed slot
    slot_comp = np.repeat(np.repeat(np.arange(ncomp), np.diff(fac_ptr)), arity)
    free = np.flatnonzero(g >= 0)
    slot_pos = np.full(len(sv), -1, dtype=np.int64)           # variable-major: a stable sort of the free slots by variable
    slot_pos[free[np.argsort(g[free], kind="stable")]] = np.arange(len(free))
    t = {"free_ptr": free_ptr, "free_vid": free_vid, "fac_ptr": fac_ptr, "fac_id": fac_id,
         "v2s_ptr": np.concatenate([[0], np.cumsum(np.bincount(g[free], minlength=nfree))]),
         "slot_base": np.concatenate([[0], np.cumsum(arity)]), "slot_pos": slot_pos,
         "slot_li": np.where(g >= 0, g - free_ptr[slot_comp], -1) if pb.kind == "ba" else np.zeros(0, dtype=np.int64),
         "order": np.array(sorted(range(ncomp), key=lambda c: -(fac_ptr[c + 1] - fac_ptr[c])), dtype=np.int64),
         "counts": np.array([len(sv), len(free)])}
    cb_ptr, cb, cb_li = [0], [], []
    for free_list, _ in comps:
        local = {v: i for i, v in enumerate(free_list)}
        rot = {int(pb.block_of[v]) for v in free_list if pb.block_of[v] >= 0 and v - pb.block_of[v] < 3} if pb.ncam_blocks else set()
        for b in sorted(rot):
            cb.append(b)
            cb_li += [local.get(b + k, -1) for k in range(3)]
        cb_ptr.append(len(cb))
    t.update(cb_ptr=np.array(cb_ptr, dtype=np.int64), cb=np.array(cb, dtype=np.int64), cb_li=np.array(cb_li, dtype=np.int64))
    t["offsets"] = np.concatenate([[0], np.cumsum([len(t[k]) for k in BLOCK])])[:-1]
    t["blk"] = np.concatenate([t[k] for k in BLOCK])
    return t, sv, where


def compare(pb, comps, got, order):
    want, sv, where = restate(pb, comps)
    # the block's parts, by the offsets the program printed
    ends = list(got["offsets"][1:]) + [len(got["blk"])]
    for name, a, b in zip(BLOCK, got["offsets"], ends):
        assert np.array_equal(got["blk"][a:b], want[name]), name
    for name in ("free_ptr", "free_vid", "fac_ptr", "fac_id", "v2s_ptr", "slot_li", "order", "counts", "offsets", "blk"):
        assert np.array_equal(got[name], want[name]), name
    assert list(got["order"]) == order
    # structure: the free slots' positions are a permutation of 0 .. ngfac-1, variable by variable, a variable's in listed order
    nslots, ngfac = got["counts"]
    pos = got["blk"][got["offsets"][7]:got["offsets"][7] + nslots]
    free = np.flatnonzero(pos >= 0)
    assert np.array_equal(np.sort(pos[free]), np.arange(ngfac)) and np.all(pos[where[sv] < 0] == -1)
    by_pos = free[np.argsort(pos[free])]
    assert np.array_equal(where[sv[by_pos]], np.repeat(np.arange(len(got["free_vid"])), np.diff(got["v2s_ptr"])))
    same = where[sv[by_pos]][1:] == where[sv[by_pos]][:-1]
    assert np.all(by_pos[1:][same] > by_pos[:-1][same])
    return want


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["ba", "nlp"])
def test_tables_are_the_restatement(exe, layout):
    pb, comps, order = (BA(), BA_COMPS, BA_ORDER) if layout == "ba" else (NLP(), NLP_COMPS, NLP_ORDER)
    (code, message, got), = run(exe, pb.text() + comps_text(comps))
    assert (code, message) == (0, "")
    want = compare(pb, comps, got, order)
    if layout == "ba":
        # what the layout is there to reach
        assert list(want["cb"]) == [18, 9, 27] and list(want["cb_li"]) == [3, -1, -1, -1, 1, 0, 1, 3, 4] and list(want["cb_ptr"]) == [0, 0, 1, 2, 2, 3]
        assert len(want["slot_li"]) == 12 * 12 and want["counts"][1] > 0 and np.any(want["slot_li"] < 0)
    else:
        assert len(got["slot_li"]) == 0 and sorted(set(np.diff(want["slot_base"]))) == [1, 2, 5] and not want["cb_ptr"].any()
    # one component alone, and no component at all
    (code, _, got), (code0, _, got0) = run(exe, pb.text() + comps_text(comps[2:3]) + comps_text([]))
    assert code == 0 and code0 == 0
    compare(pb, comps[2:3], got, [0])
    compare(pb, [], got0, [])


def _mutated(comps, c, what, value):
    """the components with component c's free (what = 0) or factor (1) list replaced"""
    out = [list(x) for x in comps]
    out[c][what] = value
    return [tuple(x) for x in out]


def ba_refusals():
    C = BA_COMPS
    frees, facs = [c[0] for c in C], [c[1] for c in C]
    fp, gp = _csr(frees)[0], _csr(facs)[0]
    return [
        (call_text(frees, facs, free_ptr=[1] + fp[1:]), EINVAL, "plan_create: bad CSR"),
        (call_text(frees, facs, fac_ptr=[2] + gp[1:]), EINVAL, "plan_create: bad CSR"),
        (call_text(frees, facs, null_free=True), EINVAL, "plan_create: bad CSR"),
        (call_text(frees, facs, null_fac=True), EINVAL, "plan_create: bad CSR"),
        (call_text([[]], [[]], free_ptr=[0, -1]), EINVAL, "plan_create: bad CSR"),
        # pointer arrays whose last entry is the bound: nothing else is touched before the check
        (call_text([[]], [[]], free_ptr=[0, (1 << 31) // 5]), ERANGE, "plan_create: too large"),
        (call_text([[]], [[]], fac_ptr=[0, ((1 << 31) - 16) // 12]), ERANGE, "plan_create: too large"),
        (call_text(frees, facs, free_ptr=[fp[0], fp[2], fp[1]] + fp[3:]), EINVAL, "plan_create: ptr not monotone"),
        (call_text(frees, facs, fac_ptr=[gp[0], gp[1], gp[3], gp[2]] + gp[4:]), EINVAL, "plan_create: ptr not monotone"),
        (comps_text(_mutated(C, 0, 0, [57, 62, 59])), EINVAL, "plan_create: free variable id out of range"),
        (comps_text(_mutated(C, 4, 0, [31, -1])), EINVAL, "plan_create: free variable id out of range"),
        (comps_text(_mutated(C, 0, 0, [57, 58, 59, 16])), EOVERLAP, "plan_create: variable 16 is free in two components (or listed twice)"),
        (comps_text(_mutated(C, 1, 0, [45, 46, 47, 18, 46])), EOVERLAP, "plan_create: variable 46 is free in two components (or listed twice)"),
        (comps_text(_mutated(C, 3, 1, [0, 14])), EINVAL, "plan_create: factor id out of range"),
        (comps_text(_mutated(C, 3, 1, [-1])), EINVAL, "plan_create: factor id out of range"),
        (comps_text(_mutated(C, 3, 1, [0, 4])), EOVERLAP, "plan_create: factor 4 listed twice"),
        (comps_text(_mutated(C, 1, 1, [5, 4, 5])), EOVERLAP, "plan_create: factor 5 listed twice"),
        # factor 10 reads camera 2 (free in component 1) and point 7 (free in component 0); factor 13 camera 3 (component 4)
        (comps_text(_mutated(C, 3, 1, [0, 10])), EOVERLAP, "plan_create: factor 10 of component 3 reads a free variable of component 1"),
        (comps_text(_mutated(C, 2, 1, [11, 1, 2, 3, 9, 13])), EOVERLAP, "plan_create: factor 13 of component 2 reads a free variable of component 4"),
    ]


def nlp_refusals():
    C = NLP_COMPS
    return [
        (comps_text(_mutated(C, 2, 1, [4, 7])), EINVAL, "plan_create: factor id out of range"),
        (comps_text(_mutated(C, 0, 0, [12, 0])), EOVERLAP, "plan_create: variable 0 is free in two components (or listed twice)"),
        (comps_text(_mutated(C, 2, 1, [4, 5])), EOVERLAP, "plan_create: factor 5 listed twice"),   # (5 reads constants only)
        # factor 1 reads variable 1, free in component 1, and is listed by component 2
        (comps_text([([12], []), ([1, 0], [0, 3]), ([], [4, 1]), ([5, 4, 7], [6, 2, 5])]), EOVERLAP,
         "plan_create: factor 1 of component 2 reads a free variable of component 1"),
    ]


@pytest.mark.parametrize("layout", ["ba", "nlp"])
def test_refusals_and_the_stamp_rule(exe, layout):
    """every refusal with its code and message; between them the valid call on the SAME scratch arrays, whose tables must be the
    ones a fresh scratch gives (the marks a refused call left are of an older stamp)"""
    pb, comps, order, refusals = (BA(), BA_COMPS, BA_ORDER, ba_refusals()) if layout == "ba" else (NLP(), NLP_COMPS, NLP_ORDER, nlp_refusals())
    valid = comps_text(comps)
    answers = run(exe, pb.text() + valid + "".join(text + valid for text, _, _ in refusals))
    assert len(answers) == 1 + 2 * len(refusals)
    fresh = answers[0][2]
    compare(pb, comps, fresh, order)
    for k, (_, code, message) in enumerate(refusals):
        assert answers[1 + 2 * k][:2] == (code, message), (k, answers[1 + 2 * k][:2])
        again = answers[2 + 2 * k]
        assert again[:2] == (0, "")
        assert fresh.keys() == again[2].keys() and all(np.array_equal(fresh[n], again[2][n]) for n in fresh), k


def test_too_many_slots_of_a_nonlinear_product_plan(exe):
    """the second "too large": one listed factor whose row claims 2^31 - 8 variables -- the slot count is refused before any
    slot is read"""
    text = "problem nlp 1 1 0 %d 0\n" % ((1 << 31) - 8) + call_text([[]], [[0]])
    assert run(exe, text) == [(ERANGE, "plan_create: too large", None)]
