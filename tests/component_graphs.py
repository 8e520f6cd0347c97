"""Factor graphs whose connected components are known by construction, for the tests of the component
labelling (rdis_hip_components on the device, ro_components in the oracle).

Every generator returns (PackedProblem, assigned, expected): expected = (free_ptr, free_vid, fac_ptr,
fac_id) in the library's convention -- components ordered by (number of variables, smallest variable id),
ids ascending inside a list, a factor filed under the component of its unassigned variables, a factor
without one in no list.  The generator knows the group of every variable from how it laid the graph out;
expected_from_groups() turns that into the four arrays by sorting.  No union-find and no graph search
anywhere in this module: what is checked here is independent of both implementations under test.

check_lists() validates any four such arrays against a problem without knowing the answer (everything
but maximality -- that nothing is wrongly split -- which equality with `expected` gives).

Values (x0, coeff, obs) are arbitrary finite numbers: only indices matter.  A plain helper module: no
fixtures, no pytest settings."""
from __future__ import annotations

import numpy as np

from rdis_amd.problems import KIND_BA, KIND_NLP, PackedProblem

I64 = np.int64
GRID_CAP = 4096 * 256          # work items of one pass of components.hip's capped launches
PAST_CAP = GRID_CAP + 257      # the smallest interesting size beyond it: a second pass, not a multiple of 256


# ---------------------------------------------------------------------------------------------------
# from groups to lists, and the validator
# ---------------------------------------------------------------------------------------------------

def entries(pp):
    """(row, vid): every (factor, variable) incidence of the problem, both kinds"""
    if pp.kind == KIND_BA:
        F = pp.nfac
        row = np.repeat(np.arange(F, dtype=I64), 12)
        vid = np.concatenate([pp.cam_vid0[:, None] + np.arange(9, dtype=I64)[None, :],
                              pp.pt_vid0[:, None] + np.arange(3, dtype=I64)[None, :]], axis=1).reshape(-1)
        return row, vid
    row = np.repeat(np.arange(pp.nfac, dtype=I64), np.diff(pp.rowptr))
    return row, np.asarray(pp.vid, dtype=I64)


def _csr(sorted_comp, ncomp):
    return np.concatenate([[0], np.cumsum(np.bincount(sorted_comp, minlength=ncomp))]).astype(I64)


def expected_from_groups(pp, assigned, group):
    """group[v]: any integer label, equal for two unassigned variables exactly when the construction put
    them into one component (ignored where assigned[v])"""
    a = np.asarray(assigned) != 0
    N, F = pp.nvars, pp.nfac
    free = np.flatnonzero(~a).astype(I64)                       # ascending ids
    if free.size == 0:
        return np.zeros(1, I64), np.zeros(0, I64), np.zeros(1, I64), np.zeros(0, I64)
    labels, first, inv, size = np.unique(np.asarray(group)[free], return_index=True, return_inverse=True, return_counts=True)
    smallest = free[first]                                      # free ascends: the first member met is the smallest
    order = np.lexsort((smallest, size))                        # by size, then by smallest id
    rank = np.empty(labels.shape[0], I64)
    rank[order] = np.arange(labels.shape[0], dtype=I64)
    comp_of_free = rank[inv.reshape(-1)]
    by_comp = np.argsort(comp_of_free, kind="stable")           # stable: ids stay ascending inside a component
    free_vid, free_ptr = free[by_comp], _csr(comp_of_free, labels.shape[0])
    comp_of_var = np.full(N, -1, I64)
    comp_of_var[free] = comp_of_free
    row, vid = entries(pp)
    e = comp_of_var[vid]
    comp_of_fac = np.full(F, -1, I64)
    comp_of_fac[row[e >= 0]] = e[e >= 0]                        # (all unassigned variables of a row agree: check_lists proves it)
    listed = np.flatnonzero(comp_of_fac >= 0).astype(I64)
    fac_id = listed[np.argsort(comp_of_fac[listed], kind="stable")]
    return free_ptr, free_vid, _csr(comp_of_fac[listed], labels.shape[0]), fac_id


def check_lists(pp, assigned, lists):
    """AssertionError unless `lists` is a labelling of pp under `assigned` in the library's convention;
    knows nothing of connectivity beyond 'the unassigned variables of a factor share a component'"""
    free_ptr, free_vid, fac_ptr, fac_id = (np.asarray(x, dtype=I64) for x in lists)
    a = np.asarray(assigned) != 0
    N, F = pp.nvars, pp.nfac
    nc = free_ptr.shape[0] - 1
    assert nc >= 0 and fac_ptr.shape[0] == nc + 1, "ptr arrays of different length"
    assert free_ptr[0] == 0 and fac_ptr[0] == 0 and free_ptr[-1] == free_vid.shape[0] and fac_ptr[-1] == fac_id.shape[0], "ptr ends"
    nvars, nfacs = np.diff(free_ptr), np.diff(fac_ptr)
    assert np.all(nvars >= 1) and np.all(nfacs >= 0), "a component without a variable, or a ptr that descends"
    # every unassigned variable exactly once, nothing else
    assert np.array_equal(np.sort(free_vid), np.flatnonzero(~a)), "free_vid is not the set of unassigned variables, each once"
    comp_var = np.repeat(np.arange(nc, dtype=I64), nvars)
    comp_fac = np.repeat(np.arange(nc, dtype=I64), nfacs)
    comp_of_var = np.full(N, -1, I64)
    comp_of_var[free_vid] = comp_var
    # every factor with an unassigned variable exactly once, no other factor
    row, vid = entries(pp)
    live = ~a[vid]
    has_free = np.bincount(row[live], minlength=F) > 0
    assert np.array_equal(np.sort(fac_id), np.flatnonzero(has_free)), "fac_id is not the set of factors with an unassigned variable, each once"
    # all unassigned variables of a listed factor lie in that factor's component
    comp_of_fac = np.full(F, -1, I64)
    comp_of_fac[fac_id] = comp_fac
    assert np.array_equal(comp_of_var[vid[live]], comp_of_fac[row[live]]), "a factor reaches a variable of another component"
    # ids ascend inside each list
    assert np.all(np.diff(comp_var * (N + 1) + free_vid) > 0), "free_vid does not ascend inside a component"
    assert np.all(np.diff(comp_fac * (F + 1) + fac_id) > 0), "fac_id does not ascend inside a component"
    # components by (number of variables, smallest id)
    if nc > 1:
        smallest = free_vid[free_ptr[:-1]]
        ds, dm = np.diff(nvars), np.diff(smallest)
        assert np.all((ds > 0) | ((ds == 0) & (dm > 0))), "components are not ordered by (size, smallest id)"


def same(a, b):
    return len(a) == len(b) == 4 and all(np.array_equal(np.asarray(x, dtype=I64), np.asarray(y, dtype=I64)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------

def _nlp(rng, nvars, arity, flat, meta):
    """rows given by their lengths and their concatenated variable ids"""
    arity = np.asarray(arity, dtype=I64)
    rowptr = np.concatenate([[0], np.cumsum(arity)]).astype(I64)
    flat = np.asarray(flat, dtype=I64)
    assert rowptr[-1] == flat.shape[0] and (flat.size == 0 or (flat.min() >= 0 and flat.max() < nvars))
    nnz, F = flat.shape[0], arity.shape[0]
    return PackedProblem(kind=KIND_NLP, x0=rng.uniform(-1.0, 1.0, nvars), lo=np.full(nvars, -5.0), hi=np.full(nvars, 5.0),
                         coeff=rng.uniform(0.5, 2.0, F), rowptr=rowptr, vid=flat, expo=np.ones(nnz), cons=np.zeros(nnz),
                         sine=np.zeros(nnz, np.uint8), meta=meta)


def _shuffle_rows(rng, arity, flat):
    """the same rows in a random order (factor ids carry no structure then)"""
    arity, flat = np.asarray(arity, dtype=I64), np.asarray(flat, dtype=I64)
    start = np.concatenate([[0], np.cumsum(arity)])[:-1]
    order = rng.permutation(arity.shape[0])
    new_arity = arity[order]
    new_start = np.concatenate([[0], np.cumsum(new_arity)])[:-1]
    src = np.repeat(start[order] - new_start, new_arity) + np.arange(flat.shape[0], dtype=I64)
    return new_arity, flat[src]


def _pairs(rng, u, v):
    """arity-2 rows {u[i], v[i]}, either variable first"""
    flip = rng.random(u.shape[0]) < 0.5
    return np.stack([np.where(flip, v, u), np.where(flip, u, v)], axis=1).reshape(-1)


# ---------------------------------------------------------------------------------------------------
# the generators
# ---------------------------------------------------------------------------------------------------

def chain(n, cut_every=0, seed=0, parallel=0):
    """factors {v_i, v_i+1} along a random permutation of the ids, factor ids shuffled; `parallel` further
    factors repeat edges drawn at random.  cut_every = 0: one component of n; else every cut_every-th
    variable along the chain is assigned: segments of cut_every - 1, and one of n % cut_every at the end.
    (The problem depends on n, seed and parallel only: one upload serves every cut_every.)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n).astype(I64)                       # position along the chain -> variable id
    edge = np.concatenate([np.arange(n - 1, dtype=I64), rng.integers(0, n - 1, parallel, dtype=I64)])
    edge = edge[rng.permutation(edge.shape[0])]
    pp = _nlp(rng, n, np.full(edge.shape[0], 2, I64), _pairs(rng, perm[edge], perm[edge + 1]),
              {"generator": "chain", "n": n, "seed": seed, "parallel": parallel})
    pos = np.arange(n, dtype=I64)
    assigned, group = np.zeros(n, np.uint8), np.zeros(n, I64)
    if cut_every > 0:
        assigned[perm[pos % cut_every == cut_every - 1]] = 1
        group[perm] = pos // cut_every
    return pp, assigned, expected_from_groups(pp, assigned, group)


def star(n, hub, hub_assigned=False, seed=0):
    """every factor {hub, leaf}, leaves in random order, the hub first or second in its row.  One component
    of n; with the hub assigned n - 1 singletons, each with one arity-2 factor reduced to one free variable."""
    rng = np.random.default_rng(seed)
    leaves = np.delete(np.arange(n, dtype=I64), hub)
    leaves = leaves[rng.permutation(n - 1)]
    pp = _nlp(rng, n, np.full(n - 1, 2, I64), _pairs(rng, np.full(n - 1, hub, I64), leaves),
              {"generator": "star", "n": n, "hub": hub, "seed": seed})
    assigned = np.zeros(n, np.uint8)
    assigned[hub] = 1 if hub_assigned else 0
    group = np.arange(n, dtype=I64) if hub_assigned else np.zeros(n, I64)
    return pp, assigned, expected_from_groups(pp, assigned, group)


def merge_tree(levels, seed=0, open_levels=0):
    """a complete binary tree of unions over 2^levels leaves (random ids): at level l every block of 2^l
    leaves gets one factor joining a random member of its left half to one of its right half; factor ids
    in random order.  open_levels = k leaves the top k levels out: 2^k components of equal size, whose
    order is decided by their smallest ids alone."""
    rng = np.random.default_rng(seed)
    n = 1 << levels
    ident = rng.permutation(n).astype(I64)                      # leaf -> variable id
    us, vs = [], []
    for l in range(1, levels - open_levels + 1):
        half, nblocks = 1 << (l - 1), n >> l
        base = np.arange(nblocks, dtype=I64) << l
        us.append(base + rng.integers(0, half, nblocks, dtype=I64))
        vs.append(base + half + rng.integers(0, half, nblocks, dtype=I64))
    u, v = np.concatenate(us), np.concatenate(vs)
    order = rng.permutation(u.shape[0])
    pp = _nlp(rng, n, np.full(u.shape[0], 2, I64), _pairs(rng, ident[u[order]], ident[v[order]]),
              {"generator": "merge_tree", "levels": levels, "seed": seed, "open_levels": open_levels})
    group = np.empty(n, I64)
    group[ident] = np.arange(n, dtype=I64) >> (levels - open_levels)
    assigned = np.zeros(n, np.uint8)
    return pp, assigned, expected_from_groups(pp, assigned, group)


def grid(h, w, cut_rows, cut_cols, seed=0):
    """a 4-neighbour lattice, variable r * w + c (no relabelling: the blocks' smallest ids are part of the
    construction), factor ids shuffled.  The rows cut_rows and the columns cut_cols are assigned whole; the
    rectangular blocks between them are the components.  The caller chooses cuts that leave blocks of
    different sizes with the largest block holding variable 0 or the like: size order against id order
    (asserted here: some larger block has a smaller smallest id than some smaller block)."""
    rng = np.random.default_rng(seed)
    r, c = np.divmod(np.arange(h * w, dtype=I64), w)
    right, down = np.flatnonzero(c < w - 1), np.flatnonzero(r < h - 1)
    u, v = np.concatenate([right, down]), np.concatenate([right + 1, down + w])
    order = rng.permutation(u.shape[0])
    pp = _nlp(rng, h * w, np.full(u.shape[0], 2, I64), _pairs(rng, u[order], v[order]),
              {"generator": "grid", "h": h, "w": w, "seed": seed})
    cut_r, cut_c = np.zeros(h, bool), np.zeros(w, bool)
    cut_r[list(cut_rows)] = True
    cut_c[list(cut_cols)] = True
    assigned = (cut_r[r] | cut_c[c]).astype(np.uint8)
    band_r, band_c = np.cumsum(cut_r), np.cumsum(cut_c)         # the band a row / column lies in
    group = band_r[r] * (w + 1) + band_c[c]
    exp = expected_from_groups(pp, assigned, group)
    sizes, smallest = np.diff(exp[0]), exp[1][exp[0][:-1]]
    assert np.unique(sizes).shape[0] > 1 and np.any(np.diff(smallest) < 0), "cuts leave no block ordered against its id"
    return pp, assigned, exp


ROWS_DEFAULTS = dict(nvars=0, high_arity=0, arity_one=0, arity_one_vars=0, arity_zero=0, repeats=0, leaders=0, leader_k=0,
                     assigned_rows=0)


def rows(spec, seed=0):
    """the edge shapes of a row, any mix of them in one problem (random variable ids, random factor order):

      high_arity      one factor over this many variables of its own: one component
      arity_one       this many arity-1 factors over arity_one_vars variables (several per variable): singletons
      arity_zero      this many factors without a variable: in no component
      repeats         units of three variables a, b, c with the rows [a, a, b], [b, a, b, b], [c, c, c], [c, c]:
                      a variable listed two and three times; components {a, b} and {c}
      leaders         rows [s .. s, u, w] that begin with k = 0 .. leader_k assigned variables s (k cycles over
                      the rows): components {u, w}; the only assigned variables are the leader_k separators
      assigned_rows   rows over two separators only: in no component
      nvars           the total; what the above leaves over is touched by no factor: singletons with empty lists"""
    s = dict(ROWS_DEFAULTS)
    s.update(spec)
    assert set(s) == set(ROWS_DEFAULTS), "unknown key in spec"
    rng = np.random.default_rng(seed)
    H, n1f, n0, R, L, K, A = (int(s[k]) for k in ("high_arity", "arity_one", "arity_zero", "repeats", "leaders", "leader_k", "assigned_rows"))
    n1v = int(s["arity_one_vars"]) or (max(n1f // 2, 1) if n1f else 0)
    assert (L == 0 or K >= 0) and (A == 0 or K >= 2)
    # slots (ids before the relabelling), block by block
    o_h, o_1, o_r, o_s, o_l = np.cumsum([0, H, n1v, 3 * R, K])
    used = int(o_l + 2 * L)
    n = max(int(s["nvars"]), used)
    group, assigned = np.arange(n, dtype=I64), np.zeros(n, np.uint8)
    arity, flat = [], []
    if H:
        arity.append([H]); flat.append(o_h + rng.permutation(H))
        group[o_h:o_h + H] = o_h
    if n1f:
        arity.append(np.ones(n1f, I64)); flat.append(o_1 + rng.integers(0, n1v, n1f, dtype=I64))
    if n0:
        arity.append(np.zeros(n0, I64))
    if R:
        a = o_r + 3 * np.arange(R, dtype=I64)
        b, c = a + 1, a + 2
        arity.append(np.tile(np.array([3, 4, 3, 2], I64), R))
        flat.append(np.stack([a, a, b, b, a, b, b, c, c, c, c, c], axis=1).reshape(-1))
        group[b] = a
    if K:
        assigned[o_s:o_s + K] = 1
    if L:
        k = np.arange(L, dtype=I64) % (K + 1)
        ar = k + 2
        start = np.concatenate([[0], np.cumsum(ar)])[:-1]
        ri = np.repeat(np.arange(L, dtype=I64), ar)
        j = np.arange(int(ar.sum()), dtype=I64) - start[ri]
        u = o_l + 2 * np.arange(L, dtype=I64)
        arity.append(ar)
        flat.append(np.where(j < k[ri], o_s + (ri + j) % max(K, 1), np.where(j == k[ri], u[ri], u[ri] + 1)))
        group[u + 1] = u
    if A:
        i = np.arange(A, dtype=I64)
        arity.append(np.full(A, 2, I64)); flat.append(np.stack([o_s + i % K, o_s + (i + 1) % K], axis=1).reshape(-1))
    arity = np.concatenate([np.asarray(x, dtype=I64) for x in arity]) if arity else np.zeros(0, I64)
    flat = np.concatenate([np.asarray(x, dtype=I64) for x in flat]) if flat else np.zeros(0, I64)
    relabel = rng.permutation(n).astype(I64)                    # slot -> variable id
    arity, flat = _shuffle_rows(rng, arity, relabel[flat])
    pp = _nlp(rng, n, arity, flat, {"generator": "rows", "spec": s, "seed": seed})
    g, a_ = np.empty(n, I64), np.empty(n, np.uint8)
    g[relabel], a_[relabel] = group, assigned
    return pp, a_, expected_from_groups(pp, a_, g)


def ba_points(ncams, npts, k, assign="cameras", seed=0):
    """bundle adjustment built directly: point p is seen by the k cameras s_p, s_p + 1, ... (mod ncams), s_p = p
    for the first ncams points (so that the cameras hang together) and random after; observations in random
    order.  assign = "cameras": npts components of 3 variables and k factors, in id order; "points": one
    component of 9 variables per camera; "none": one component.  (One problem per (ncams, npts, k, seed).)"""
    assert 2 <= k <= ncams <= npts and assign in ("cameras", "points", "none")
    rng = np.random.default_rng(seed)
    s = np.concatenate([np.arange(ncams, dtype=I64), rng.integers(0, ncams, npts - ncams, dtype=I64)])
    cam = ((s[:, None] + np.arange(k, dtype=I64)[None, :]) % ncams).reshape(-1)
    pt = np.repeat(np.arange(npts, dtype=I64), k)
    order = rng.permutation(npts * k)
    cam, pt = cam[order], pt[order]
    n = 9 * ncams + 3 * npts
    pp = PackedProblem(kind=KIND_BA, x0=rng.uniform(-1.0, 1.0, n), lo=np.full(n, -10.0), hi=np.full(n, 10.0),
                       cam_vid0=9 * cam, pt_vid0=9 * ncams + 3 * pt, obs=rng.uniform(-100.0, 100.0, (npts * k, 2)),
                       meta={"ncams": ncams, "npts": npts, "generator": "ba_points", "seed": seed})
    v = np.arange(n, dtype=I64)
    assigned = np.zeros(n, np.uint8)
    if assign == "cameras":
        assigned[:9 * ncams] = 1
    elif assign == "points":
        assigned[9 * ncams:] = 1
    block = np.where(v < 9 * ncams, v // 9, ncams + (v - 9 * ncams) // 3)   # a camera or a point: free as a whole
    group = np.zeros(n, I64) if assign == "none" else block
    return pp, assigned, expected_from_groups(pp, assigned, group)


def sinusoid_expected(pp, assigned):
    """the lists of rdis_amd.problems.make_high_dim_sinusoid (arities 1 and 2: every factor over a variable alone or
    over a variable and its parent in the k-ary tree) under any mask, by the tree's own recurrence, level by level:
    a variable belongs with its parent when both are unassigned, else it heads a group of its own"""
    h, k = pp.meta["h"], pp.meta["k"]
    assert pp.meta["generator"] == "sinusoid" and np.diff(pp.rowptr).max() == 2
    a = np.asarray(assigned) != 0
    head = np.arange(pp.nvars, dtype=I64)
    lo = 1
    for level in range(1, h + 1):
        v = np.arange(lo, lo + k ** level, dtype=I64)
        parent = (v - 1) // k
        head[v] = np.where(~a[v] & ~a[parent], head[parent], v)
        lo += k ** level
    assert lo == pp.nvars
    return expected_from_groups(pp, assigned, head)


def same_problem(p, q):
    """two generator calls gave the same problem (so that one upload can serve both masks)"""
    if p.kind != q.kind or p.nvars != q.nvars or p.nfac != q.nfac:
        return False
    if p.kind == KIND_BA:
        return np.array_equal(p.cam_vid0, q.cam_vid0) and np.array_equal(p.pt_vid0, q.pt_vid0)
    return np.array_equal(p.rowptr, q.rowptr) and np.array_equal(p.vid, q.vid)


# ---------------------------------------------------------------------------------------------------
# the cases both test files run (one table: the CPU file pins expected == oracle for exactly what the
# device is compared with)
# ---------------------------------------------------------------------------------------------------

EDGE_ROWS = dict(nvars=2500, high_arity=700, arity_one=300, arity_one_vars=120, arity_zero=40, repeats=60, leaders=240, leader_k=5,
                 assigned_rows=30)

# 1 048 833 variables, some thousand factors: nearly all singletons with empty factor lists, one component of
# 70 000 variables from a single factor (a count beyond 16 bits in the 64-bit sort key)
WIDE_ROWS = dict(nvars=PAST_CAP, high_arity=70_000, arity_one=1500, arity_one_vars=900, arity_zero=300, repeats=200, leaders=900,
                 leader_k=6, assigned_rows=100)
# ... and the same with 72 000 more variables, so that the NUMBER OF COMPONENTS passes the cap as well (1 049 728)
WIDER_ROWS = dict(WIDE_ROWS, nvars=PAST_CAP + 72_000)


def small_cases():
    """name -> zero-argument builder, sizes of a few hundred to a few thousand, several seeds"""
    c = {}
    for seed in (0, 1, 2):
        c[f"chain4097-s{seed}"] = lambda seed=seed: chain(4097, 0, seed)
        c[f"chain4097-cut64-s{seed}"] = lambda seed=seed: chain(4097, 64, seed)
        c[f"merge12-s{seed}"] = lambda seed=seed: merge_tree(12, seed)
        c[f"merge12-open5-s{seed}"] = lambda seed=seed: merge_tree(12, seed, open_levels=5)
        c[f"rows-edge-s{seed}"] = lambda seed=seed: rows(EDGE_ROWS, seed)
        c[f"grid64x48-s{seed}"] = lambda seed=seed: grid(64, 48, (10, 40), (30,), seed)
    c["chain4097-cut7"] = lambda: chain(4097, 7, 3)
    c["chain300-parallel5000"] = lambda: chain(300, 10, 4, parallel=5000)
    for name, hub in (("first", 0), ("last", 2999), ("middle", 1500)):
        c[f"star3000-{name}"] = lambda hub=hub: star(3000, hub, False, hub)
        c[f"star3000-{name}-assigned"] = lambda hub=hub: star(3000, hub, True, hub)
    c["rows-one-factor-100000"] = lambda: rows(dict(high_arity=100_000, nvars=100_100), 5)
    c["rows-untouched-only"] = lambda: rows(dict(nvars=777), 6)
    c["rows-arity-zero-only"] = lambda: rows(dict(nvars=300, arity_zero=500), 7)
    for assign in ("cameras", "points", "none"):
        c[f"ba7x500x3-{assign}"] = lambda assign=assign: ba_points(7, 500, 3, assign, 8)
    return c


def large_cases():
    """name -> builder, at the sizes where the capped grid takes a second pass (or the device is filled);
    cases that share a problem follow each other"""
    c = {}
    c["chain-past-cap"] = lambda: chain(PAST_CAP, 0, 11)
    c["chain-past-cap-cut1000"] = lambda: chain(PAST_CAP, 1000, 11)
    c["rows-past-cap-singletons"] = lambda: rows(WIDE_ROWS, 12)
    c["rows-past-cap-components"] = lambda: rows(WIDER_ROWS, 13)
    c["chain5000-factors-past-cap"] = lambda: chain(5000, 100, 14, parallel=PAST_CAP - 4999)
    for assign in ("cameras", "points", "none"):
        c[f"ba16x349611x3-{assign}"] = lambda assign=assign: ba_points(16, 349_611, 3, assign, 15)
    for name, hub in (("first", 0), ("last", 299_999), ("middle", 150_000)):
        c[f"star300000-{name}"] = lambda hub=hub: star(300_000, hub, False, 16)
    c["merge18"] = lambda: merge_tree(18, 17)
    return c
