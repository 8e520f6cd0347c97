"""The references of the component-labelling tests, pinned against each other without a device: the lists
that tests/component_graphs.py derives from its constructions, its validator check_lists, the oracle's
sequential union-find (ro_components) and, where scipy is installed, scipy's connected_components -- at the
small sizes and at the sizes beyond the device's capped grid that tests/test_gpu_components.py compares the
device with.  Index work: exact."""
import numpy as np
import pytest

import component_graphs as G
from oracle import oracle as O

SMALL, LARGE = G.small_cases(), G.large_cases()

# large cases that share a problem: one oracle problem each (creating it is what takes the time)
LARGE_GROUPS = {
    "chain-past-cap": ["chain-past-cap", "chain-past-cap-cut1000"],
    "rows-past-cap-singletons": ["rows-past-cap-singletons"],
    "rows-past-cap-components": ["rows-past-cap-components"],
    "chain5000-factors-past-cap": ["chain5000-factors-past-cap"],
    "ba16x349611x3": ["ba16x349611x3-cameras", "ba16x349611x3-points", "ba16x349611x3-none"],
    "star300000": ["star300000-first", "star300000-last", "star300000-middle"],
    "merge18": ["merge18"],
}


def _pin(names, table):
    orc = last = None
    for name in names:
        pp, a, exp = table[name]()
        G.check_lists(pp, a, exp)
        if last is None or not G.same_problem(last, pp):
            orc, last = O.OracleProblem(pp), pp
        got = orc.components(a)
        G.check_lists(pp, a, got)
        assert G.same(got, exp), name
    return pp, a, exp


def test_every_large_case_is_in_a_group():
    assert sorted(n for g in LARGE_GROUPS.values() for n in g) == sorted(LARGE)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_constructions_equal_oracle(name):
    _pin([name], SMALL)


@pytest.mark.parametrize("group", sorted(LARGE_GROUPS))
def test_large_constructions_equal_oracle(group):
    _pin(LARGE_GROUPS[group], LARGE)


def test_constructions_have_the_shapes_they_promise():
    """the sizes the docstrings state, read off the expected lists"""
    _, _, e = G.chain(4097, 64, 0)
    sizes = np.diff(e[0])
    assert sizes.shape[0] == 65 and sizes[0] == 1 and np.all(sizes[1:] == 63)          # 64 segments of 63 and 4097 % 64 = 1
    assert np.all(np.diff(e[1][e[0][1:-1]]) > 0)                                       # equal sizes: by smallest id
    _, _, e = G.chain(G.PAST_CAP, 1000, 11)
    sizes = np.diff(e[0])
    assert sizes.shape[0] == 1049 and sizes[0] == 833 and np.all(sizes[1:] == 999)
    pp, _, e = G.chain(G.PAST_CAP, 0, 11)
    assert len(e[0]) == 2 and e[0][1] == pp.nvars == G.PAST_CAP and e[2][1] == pp.nfac == G.PAST_CAP - 1
    pp, _, e = G.chain(5000, 100, 14, parallel=G.PAST_CAP - 4999)
    assert pp.nfac == G.PAST_CAP and pp.nvars == 5000 and np.all(np.diff(e[0]) == 99) and e[2][-1] == pp.nfac
    pp, a, e = G.star(3000, 2999, True, 0)
    assert a.sum() == 1 and np.all(np.diff(e[0]) == 1) and np.all(np.diff(e[2]) == 1) and len(e[0]) == 3000
    assert np.array_equal(e[1], np.arange(2999))
    _, _, e = G.merge_tree(12, 0, open_levels=5)
    assert np.all(np.diff(e[0]) == 128) and len(e[0]) == 33 and np.all(np.diff(e[2]) == 127)
    _, _, e = G.grid(64, 48, (10, 40), (30,), 0)
    sizes, smallest = np.diff(e[0]), e[1][e[0][:-1]]
    assert sorted(sizes) == sorted([10 * 30, 10 * 17, 29 * 30, 29 * 17, 23 * 30, 23 * 17])
    assert np.all(np.diff(sizes) > 0) and smallest[1] == 0 and smallest[0] == 31       # size order against id order: the block
    assert np.sum(np.diff(smallest) < 0) >= 2                                          # with variable 0 is not the first
    pp, a, e = G.rows(G.WIDE_ROWS, 12)
    sizes = np.diff(e[0])
    assert pp.nvars == G.PAST_CAP and pp.nfac < 5000 and sizes[-1] == 70_000 > 65_535 and np.all(sizes[:-1] <= 2)
    assert np.sum(np.diff(e[2]) == 0) > 900_000 and a.sum() == 6
    pp, a, e = G.rows(G.WIDER_ROWS, 13)
    assert len(e[0]) - 1 > G.GRID_CAP and np.diff(e[0])[-1] == 70_000
    pp, _, e = G.rows(dict(high_arity=100_000, nvars=100_100), 5)
    assert pp.nfac == 1 and np.diff(pp.rowptr)[0] == 100_000 and np.diff(e[0])[-1] == 100_000 and len(e[0]) == 102
    pp, a, e = G.rows(G.EDGE_ROWS, 0)
    ar = np.diff(pp.rowptr)
    assert (ar == 0).sum() == 40 and (ar == 1).sum() == 300 and ar.max() == 700
    lead = a[pp.vid[pp.rowptr[:-1][ar > 0]]]                                           # rows that begin with an assigned variable ...
    live = np.bincount(G.entries(pp)[0][a[pp.vid] == 0], minlength=pp.nfac) > 0
    assert (lead[live[ar > 0]] == 1).sum() >= 150 and (~live).sum() == 40 + 30          # ... and still have a free one; constants
    pp, a, e = G.ba_points(16, 349_611, 3, "cameras", 15)
    assert pp.nfac == G.PAST_CAP and np.all(np.diff(e[0]) == 3) and np.all(np.diff(e[2]) == 3) and len(e[0]) == 349_612
    assert np.array_equal(e[1], 144 + np.arange(3 * 349_611))
    _, _, e = G.ba_points(16, 349_611, 3, "points", 15)
    assert np.all(np.diff(e[0]) == 9) and len(e[0]) == 17 and e[2][-1] == G.PAST_CAP and np.array_equal(e[1], np.arange(144))
    _, _, e = G.ba_points(16, 349_611, 3, "none", 15)
    assert len(e[0]) == 2 and e[2][1] == G.PAST_CAP


def test_partition_agrees_with_scipy():
    """component count and partition against connected_components on the variable-factor bipartite graph"""
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    cases = [SMALL[n] for n in sorted(SMALL)] + [LARGE["chain-past-cap-cut1000"], LARGE["rows-past-cap-singletons"]]
    for build in cases:
        pp, a, exp = build()
        N, F = pp.nvars, pp.nfac
        row, vid = G.entries(pp)
        live = a[vid] == 0
        g = sp.coo_matrix((np.ones(int(live.sum()), np.int8), (vid[live], N + row[live])), shape=(N + F, N + F)).tocsr()
        _, lab = csgraph.connected_components(g, directed=False)
        free = np.flatnonzero(a == 0)
        # name every component by its smallest variable id, on both sides
        ncomp = len(exp[0]) - 1
        assert np.unique(lab[free]).shape[0] == ncomp, pp.meta
        small_sp = np.full(lab.max() + 1, N, np.int64)
        np.minimum.at(small_sp, lab[free], free)
        name_exp = np.empty(N, np.int64)
        name_exp[exp[1]] = np.repeat(exp[1][exp[0][:-1]], np.diff(exp[0]))
        assert np.array_equal(small_sp[lab[free]], name_exp[free]), pp.meta


def test_validator_rejects_wrong_lists():
    """check_lists has teeth: one defect of each kind it names"""
    pp, a, exp = G.rows(G.EDGE_ROWS, 1)
    G.check_lists(pp, a, exp)
    fp, fv, cp, ci = (x.copy() for x in exp)

    def rejected(lists):
        with pytest.raises(AssertionError):
            G.check_lists(pp, a, lists)

    rejected((fp, fv[:-1], cp, ci))                                      # a variable missing (and the ptr end)
    w = fv.copy(); w[0] = w[1]; rejected((fp, w, cp, ci))                # a variable twice, another missing
    w = fv.copy(); w[0] = np.flatnonzero(a)[0]; rejected((fp, w, cp, ci))    # an assigned variable listed
    two = int(np.flatnonzero(np.diff(fp) >= 2)[0])                       # the first component with two variables
    w = fv.copy(); w[fp[two]], w[fp[two] + 1] = w[fp[two] + 1], w[fp[two]]; rejected((fp, w, cp, ci))   # ids descend
    w = fv.copy(); w[0], w[-1] = w[-1], w[0]; rejected((fp, w, cp, ci))  # a variable in another component
    w = ci.copy(); w[0], w[-1] = w[-1], w[0]; rejected((fp, fv, cp, w))  # a factor in another component
    dead = np.setdiff1d(np.arange(pp.nfac), ci)[0]
    w = ci.copy(); w[0] = dead; rejected((fp, fv, cp, w))                # a factor without an unassigned variable listed
    rejected((fp, fv, cp[:-1], ci))
    # two components of equal size in the wrong order: every list is consistent, only the order rule is broken
    one = np.flatnonzero(np.diff(fp) == 1)
    i = int(one[0]); assert one[1] == i + 1
    w, v = fv.copy(), ci.copy()
    w[fp[i]], w[fp[i + 1]] = fv[fp[i + 1]], fv[fp[i]]
    f0, f1 = ci[cp[i]:cp[i + 1]], ci[cp[i + 1]:cp[i + 2]]
    q = cp.copy(); q[i + 1] = cp[i] + len(f1)
    v[cp[i]:cp[i + 2]] = np.concatenate([f1, f0])
    rejected((fp, w, q, v))
    # a larger component before a smaller one
    big = (fp[-1] - np.diff(fp)[-1])
    n_last = int(np.diff(fp)[-1])
    w = np.concatenate([fv[big:], fv[:big]])
    p = np.concatenate([[0], n_last + fp[:-1]])
    nf_last = int(np.diff(cp)[-1])
    v = np.concatenate([ci[len(ci) - nf_last:], ci[:len(ci) - nf_last]])
    q = np.concatenate([[0], nf_last + cp[:-1]])
    rejected((p, w, q, v))


def test_sinusoid_lists_by_the_tree_recurrence():
    """the by-construction lists of the one library problem the device test feeds to a plan, under random masks"""
    from rdis_amd import problems as P
    pp = P.make_high_dim_sinusoid()
    orc = O.OracleProblem(pp)
    rng = np.random.default_rng(29)
    for frac in (0.0, 0.2, 0.35, 0.6, 0.9):
        a = (rng.random(pp.nvars) < frac).astype(np.uint8)
        exp = G.sinusoid_expected(pp, a)
        G.check_lists(pp, a, exp)
        assert G.same(orc.components(a), exp)


def test_oracle_on_masks_no_construction_knows():
    """random masks on a chain (what the device's call-sequence test compares with the oracle): the oracle's lists pass
    the validator, and there are as many components as maximal runs of unassigned positions along the chain"""
    pp, _, _ = G.chain(4097, 0, 0)
    perm = np.random.default_rng(0).permutation(pp.nvars)      # chain()'s first draw: position -> variable id
    assert set(map(tuple, np.sort(pp.vid.reshape(-1, 2), axis=1))) == set(map(tuple, np.sort(np.stack([perm[:-1], perm[1:]], axis=1), axis=1)))
    orc = O.OracleProblem(pp)
    rng = np.random.default_rng(5)
    for frac in (0.0, 0.1, 0.5, 0.9, 1.0):
        a = (rng.random(pp.nvars) < frac).astype(np.uint8) if 0.0 < frac < 1.0 else np.full(pp.nvars, int(frac), np.uint8)
        got = orc.components(a)
        G.check_lists(pp, a, got)
        along = a[perm] == 0
        assert len(got[0]) - 1 == int(along[0]) + int(np.sum(along[1:] & ~along[:-1]))
