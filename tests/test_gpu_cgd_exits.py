"""Every exit of the CGD minimiser on every solver kind and every many-solve entry: the cases of tests/cgd_exit_cases.py side by
side in ONE plan, the kind forced with plan options at these small shapes and confirmed with plan.info.  Each kind: the stated
code and roll-back flag per case, the contract of CGDSubspaceOptimizer::optimize (cgd_exit_cases.check_contract), the same bits
twice, the two ordinary components' bits unchanged by the edge cases beside them, the device's decisions replayed through the
oracle (check_replay), and == on (fret, delta, x, iters, status, nfeval, ngeval) with the restatement tests/test_gpu_parity.py
compares that solver with.

code x solver kind: reached by (cases of cgd_exit_cases; "all kinds" = LDS-resident with its two options, plain, point-major
alone / in groups of two, cooperative in its four settings and side by side, the grid solver)
    0 ftol          flat, blocked, exact, three-factors on all kinds; flat / two-factors on the tiny-component solver (4 and 16
                    lanes); flat on the wide point-major group and on the plain solver's nonlinear-product body; ordinary at ftol = 1
    1 gtol          one-factor on all kinds and on the tiny-component solver
    2 gg == 0       gg-zero (ftol < 0, an underflowing square) on the plain solver's nonlinear-product body; unreachable for ftol >= 0
    3 itmax         ordinary at maxiters = 1 on all kinds (and at 25 iterations where the solver's order of sums gets there)
    4 Brent's 100   unreached by the inputs tried (test_cgd_exits_cpu.py::test_code_4_search)
    5 NaN           nan on all kinds, rolled back; a point in its camera's plane on the tiny-component solver; the NaN row of
                    solve_starts / solve_population
    6 empty         empty, beside every kind (the plain solver's kernel returns it)
    7 exchange      never provoked: asserted absent everywhere

Mutations (a scratch build each, run once on this file; they change a decision, not an address):
    an equal value counts as worse (`fu <= fx` made `fu < fx` in CgdMachine::hot, hot_post and S_DB_EVAL): 20 of the 24 tests fail --
      flat, blocked and exact on every kind (the call counts and, for exact, x part from the restatement; flat and blocked
      no longer pass "stays at the clamped start" with code 0 after 30 / 26 calls), the wide group, both nonlinear-product
      cases and their many-solve rows.  Passing: the many-solve rows of bundle adjustment and the agreement of the four
      cooperative settings -- they compare the device with itself.
    finish_request() without RF_RESTORE (the roll-back's value taken at step 0 of the last line, not at the start): 19 fail --
      the nan case on every kind (fret / delta, and x on some), the NaN rows of solve_starts / solve_population and the tiny
      population; the flat-line tests, which never roll back, pass."""
import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import capi, problems as P
from test_gpu_solver import check_replay

import cgd_exit_cases as X

pytestmark = pytest.mark.gpu

OFF = {"coop_min_factors": 0, "coop_group_min_factors": 0}      # no cooperative group


def _lds(pp, v, f, plan):
    return O.OracleProblem.device_lds_default(pp, v, f, threads=64)


def _coop(pp, v, f, plan):
    return O.OracleProblem.device_default(pp, v, f, lanes_per_workgroup=128 if plan.info("pipelined") else 256)


# kind: (options, the plan.info key that counts its components, the restatement test_gpu_parity.py compares it with, the problem)
KINDS = {
    "LDS-resident": ({}, "components_lds", _lds, "combined"),
    "LDS-resident, factor_rounding": ({"factor_rounding": 1}, "components_lds",
                                      lambda pp, v, f, plan: O.OracleProblem.device_parity(pp, emulate_stale_cache=False), "no-empty"),
    # (fused arithmetic with the cache emulation: no restatement in test_gpu_parity.py -- check_replay and check_contract carry it)
    "LDS-resident, emulate_stale_cache": ({"emulate_stale_cache": 1}, "components_lds", None, "no-empty"),
    "LDS-resident, both": ({"factor_rounding": 1, "emulate_stale_cache": 1}, "components_lds",
                           lambda pp, v, f, plan: O.OracleProblem.device_parity(pp), "no-empty"),
    "plain": ({**OFF, "lds_resident": 0, "ptm_stream": 0}, "components_plain", lambda pp, v, f, plan: O.OracleProblem.device_wg_default(pp, v, f), "combined"),
    "point-major": ({**OFF, "ptm_stream": 2, "ptm_group": 1}, "components_point_major",
                    lambda pp, v, f, plan: O.OracleProblem.device_ptm_default(pp, fac=f), "combined"),
    "point-major x2": ({**OFF, "ptm_stream": 2, "ptm_group": 2, "ptm_threads": 256}, "components_point_major",
                       lambda pp, v, f, plan: O.OracleProblem.device_ptm_default(pp, fac=f, threads=256, group=2), "combined"),
    "tiny, four lanes": ({"quad_min_components": 1}, "components_tiny", lambda pp, v, f, plan: O.OracleProblem.device_group_default(pp, 4), "tiny"),
    "tiny, sixteen lanes": ({"row_min_components": 1}, "components_tiny", lambda pp, v, f, plan: O.OracleProblem.device_group_default(pp, 16), "tiny"),
    "tiny shapes, neither option": ({}, "components_lds", _lds, "tiny"),
    "cooperative": ({"coop_min_factors": 1, "coop_pipeline": 1, "coop_speculate": 1}, "components_cooperative", _coop, "combined"),
    "cooperative, no speculation": ({"coop_min_factors": 1, "coop_pipeline": 1, "coop_speculate": 0}, "components_cooperative", _coop, "combined"),
    "cooperative, plain layout": ({"coop_min_factors": 1, "coop_pipeline": 0, "coop_speculate": 1}, "components_cooperative", _coop, "combined"),
    "cooperative, plain layout, no speculation": ({"coop_min_factors": 1, "coop_pipeline": 0, "coop_speculate": 0}, "components_cooperative", _coop, "combined"),
    "cooperative groups side by side": ({"coop_group_min_factors": 1}, "components_cooperative", _coop, "combined"),
    "grid": ({"coop_min_factors": 1, "force_stream": 1, "ptm_stream": 0}, "components_grid_stream",
             lambda pp, v, f, plan: O.OracleProblem.device_wg_default(pp, v, f, grid_workgroups=plan.info("grid_stream_workgroups")), "combined"),
}
FIELDS = ("fret", "delta", "x", "iters", "status", "nfeval", "ngeval")
COOP_RESULTS = {}


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=k in ("fret", "delta", "x")) for k in FIELDS)


def _plan(gctx, cb, opts, trace=True):
    g = capi.Problem(gctx, cb.pp)
    plan = capi.Plan(g, *cb.csr)
    for k, v in opts.items():
        plan.set_option(k, v)
    if trace:
        plan.set_option("trace_records", 4096)
        plan.set_option("dump_iters", 25)
    return g, plan


def _solve(g, plan, cb, maxiters, ftol):
    g.set_x(cb.pp.x0)
    plan.set_start(cb.pp.x0[cb.csr[1]])
    plan.solve(maxiters, ftol)
    return plan.fetch(), g.get_x()


def _component(cb, r, c):
    f0, f1 = int(cb.csr[0][c]), int(cb.csr[0][c + 1])
    return type("R", (), {"x": r.x[f0:f1], "fret": r.fret[c:c + 1], "delta": r.delta[c:c + 1], "iters": r.iters[c:c + 1], "status": r.status[c:c + 1],
                          "nfeval": r.nfeval[c:c + 1], "ngeval": r.ngeval[c:c + 1]})


def _equals_oracle(bad, sub, want, what):
    nan = np.isnan(want.fret)
    bad.check((sub.fret[0] == want.fret or (nan and np.isnan(sub.fret[0]))) and sub.delta[0] == want.delta, what, "fret, delta ==", sub.fret[0], want.fret, sub.delta[0], want.delta)
    got, ref = (int(sub.iters[0]), int(sub.status[0]), int(sub.nfeval[0]), int(sub.ngeval[0])), (want.iters, want.status, want.nfeval, want.ngeval)
    bad.check(got == ref, what, "iters, status, nfeval, ngeval ==", got, ref)
    bad.check(sub.x.tobytes() == want.x.tobytes(), what, "x ==", sub.x[:3], want.x[:3])


def _check_solve(cb, plan, r, after, maxiters, ftol, make, expected):
    pp = cb.pp
    bad = X.check_contract(pp, cb.comps, r, after, names=cb.names)
    for c, ((v, f), name) in enumerate(zip(cb.comps, cb.names)):
        sub = _component(cb, r, c)
        code, rolled = int(r.status[c]) & 0xFF, bool(int(r.status[c]) & X.ROLLED_BACK)
        want_code, want_rolled = expected(name)
        bad.check(rolled == want_rolled and (want_code is None or code == want_code), name, "code, rolled back", code, rolled, int(r.iters[c]))
        if make is not None:
            # (a run that met a NaN too: the restatement goes on exactly as long -- like the device it takes f at step 0 of a line
            # from the line before, unless the cache is emulated, and the two differ once a direction is not finite)
            _equals_oracle(bad, sub, make(pp, v, f, plan).cgd(v, f, x=pp.x0[v], maxiters=maxiters, ftol=ftol), (name, maxiters, ftol))
        if code in (5, 6) or want_code == 5:
            continue                       # (nothing was traced; a NaN compares equal to nothing)
        tr, n = plan.get_trace(c, 4096)
        bad.check(n <= 4096, name, "the trace fits", n)
        try:
            if name == "exact" or (name == "one-factor" and maxiters > 1):
                # values of 1e-23 ... 1e-29 are what is left of pixel-scale numbers cancelling: no bound in units of the factor
                # values applies to them.  The decisions do not care: fed the device's scalars the oracle asks for the same steps.
                # (one-factor's first line search, where its values are of ordinary size, goes through check_replay in the
                # maxiters = 1 solve)
                rep = O.OracleProblem(pp).replay(tr, free_vid=v, fac=f, x=pp.x0[v], maxiters=maxiters, ftol=ftol)
                assert rep.step_mismatches == 0 and rep.tag_mismatches == 0 and rep.underrun == 0 and rep.consumed == len(tr), rep
                assert rep.reason == code and rep.iters == int(r.iters[c]), rep
                continue
            # (the fuzz test's bounds: a run that leaves by the gradient test has sums that are rounding noise to 1e-4)
            itol, vtol = (1e-3, 1e-3) if code in (1, 2) else (1e-8, 1e-7)
            check_replay(pp, (tr, plan.get_vectors(c, 25)[:maxiters]), sub, maxiters, ftol=ftol, free_vid=v, fac_id=f, x=pp.x0[v],
                         iter_tol=itol, far_tol=1e-2, near_scale=10.0, vec_tol=vtol)
        except AssertionError as e:
            bad.check(False, name, (maxiters, ftol), "replay", str(e)[:600])
    return bad


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_exit_on_every_solver_kind(kind, gctx):
    opts, key, make, which = KINDS[kind]
    cb = {"combined": X.combined, "no-empty": X.without_empty, "tiny": X.tiny}[which]()
    g, plan = _plan(gctx, cb, opts)
    nonempty = sum(1 for _, f in cb.comps if len(f) > 0)
    assert plan.info(key) == (len(cb.comps) if key == "components_plain" else nonempty), {k: plan.info(k) for k in ("components_lds", "components_plain", "components_tiny")}
    assert plan.info("components_plain") == (len(cb.comps) if key == "components_plain" else len(cb.comps) - nonempty)
    if kind.startswith("cooperative"):
        assert plan.info("pipelined") == (0 if "plain layout" in kind else 1)
    first, bad = None, X.Problems()
    for maxiters, ftol in (X.SOLVES[:1] if which == "tiny" else X.SOLVES):
        (r, after), (r2, after2) = _solve(g, plan, cb, maxiters, ftol), _solve(g, plan, cb, maxiters, ftol)
        bad.check(_same(r, r2) and np.array_equal(after, after2, equal_nan=True), "the same bits twice", (maxiters, ftol))
        if kind.startswith("point-major"):
            assert plan.info("point_major_group") == (2 if kind == "point-major x2" else 1)
        if which != "tiny":
            expected = lambda name: X.expected(name, maxiters, ftol)
        else:
            expected = lambda name: X.TINY_EXPECT[name]
        bad += [((maxiters, ftol),) + b for b in _check_solve(cb, plan, r, after, maxiters, ftol, make, expected)]
        first = first or r
    plan.close(); g.close()
    assert not bad, "\n".join(repr(b) for b in bad)
    if which != "tiny":
        # the ordinary components alone, same options: the edge cases beside them changed nothing
        pair = X.plain_pair()
        g2, plan2 = _plan(gctx, pair, opts, trace=False)
        rp, _ = _solve(g2, plan2, pair, *X.SOLVES[0])
        for i, c in enumerate(X.ORDINARY):
            a, b = _component(cb, first, c), _component(pair, rp, i)
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in FIELDS), (c, a.fret, b.fret)
        plan2.close(); g2.close()
    if kind.startswith("cooperative") and "side by side" not in kind:
        COOP_RESULTS[kind] = first


def test_the_four_cooperative_settings_agree_bit_for_bit(gctx):
    """pipelined or not, guessing or not: every case, nfeval / ngeval included -- on the flat cases every trial comes back EQUAL,
    the side of the Predictor's guess that ordinary runs do not take.  (The results of the four tests above, or, run alone, its
    own solves.)"""
    cb = X.combined()
    for kind in [k for k in KINDS if k.startswith("cooperative") and "side by side" not in k]:
        if kind not in COOP_RESULTS:
            g, plan = _plan(gctx, cb, KINDS[kind][0], trace=False)
            COOP_RESULTS[kind] = _solve(g, plan, cb, *X.SOLVES[0])[0]
            plan.close(); g.close()
    assert len(COOP_RESULTS) == 4
    ref = COOP_RESULTS["cooperative"]
    for kind, r in COOP_RESULTS.items():
        assert _same(ref, r), kind


def test_the_wide_point_major_group_on_a_flat_line(gctx):
    """one component on a wide group (more than 16 workgroups of 512 lanes), built as test_wide_point_major_group_on_one_large_component
    builds its smallest -- force_stream and a group size by option -- on the smallest block that gives every workgroup a chunk of
    points: 6 cameras x 2048 points, lo = hi = x0"""
    pp = X.flat(P.make_synthetic_ba(1, 6, 2048, obs_per_pt=3)).single_component()
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    for k, v in {"force_stream": 1, "ptm_group": 32, "trace_records": 4096, "dump_iters": 25}.items():
        plan.set_option(k, v)
    runs = []
    for _ in range(2):
        g.set_x(pp.x0); plan.set_start(pp.x0); plan.solve(25, 3e-8)
        runs.append(plan.fetch())
    r = runs[0]
    assert plan.info("components_point_major") == 1 and plan.info("point_major_wide") == 1
    K, nt = plan.info("point_major_group"), plan.info("point_major_threads")
    assert K > 16 and nt == 512
    assert _same(r, runs[1])
    assert (int(r.status[0]), int(r.iters[0]), int(r.nfeval[0]), int(r.ngeval[0]), r.delta[0]) == (0, 0, 30, 26, 0.0)
    assert r.x.tobytes() == pp.x0.tobytes() and g.get_x().tobytes() == pp.x0.tobytes()
    want = O.OracleProblem.device_ptm_default(pp, threads=nt, group=K, wide=True).cgd(x=pp.x0, maxiters=25)
    bad = X.Problems()
    _equals_oracle(bad, _component(X.Combined(pp, None, None, (np.array([0, pp.nvars]),), None), r, 0), want, "wide")
    assert not bad, bad
    tr, n = plan.get_trace(0, 4096)
    check_replay(pp, (tr[:n], plan.get_vectors(0, 25)), r, 25)


@pytest.mark.parametrize("case", ["flat", "gg-zero"])
def test_the_plain_solver_on_nonlinear_products(case, gctx):
    """the plain solver's nonlinear-product body: load_poly() with lo = hi = x0 (code 0 after 30 / 26 calls), and the one
    input found that leaves by gg == 0 (cgd_exit_cases.gg_zero: ftol < 0)"""
    if case == "flat":
        pp, maxiters, ftol, code = X.flat(P.load_poly()), 25, 3e-8, 0
    else:
        c = X.case("gg-zero")
        pp, maxiters, ftol, code = c.pp, c.maxiters, c.ftol, c.code
    pp.single_component()
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.set_option("trace_records", 4096)
    plan.set_option("dump_iters", 25)
    runs = []
    for _ in range(2):
        g.set_x(pp.x0); plan.set_start(pp.x0); plan.solve(maxiters, ftol)
        runs.append(plan.fetch())
    r = runs[0]
    assert plan.info("components_plain") == 1 and _same(r, runs[1])
    assert (int(r.status[0]), int(r.iters[0]), r.delta[0]) == (code, 0, 0.0) and r.x.tobytes() == pp.x0.tobytes() and g.get_x().tobytes() == pp.x0.tobytes()
    if case == "flat":
        assert (int(r.nfeval[0]), int(r.ngeval[0])) == (30, 26)
    want = O.OracleProblem.device_wg_default(pp).cgd(x=pp.x0, maxiters=maxiters, ftol=ftol)
    bad = X.Problems()
    _equals_oracle(bad, _component(X.Combined(pp, None, None, (np.array([0, pp.nvars]),), None), r, 0), want, case)
    assert not bad, bad
    tr, n = plan.get_trace(0, 4096)
    check_replay(pp, (tr[:n], plan.get_vectors(0, 25)), r, maxiters, ftol=ftol)


# ---- the many-solve entries against plan_solve from the same start, == per (row, component) --------------------------------------
def _rows_by_plan_solve(g, plan, cb, rows, maxiters=25, ftol=3e-8):
    out = []
    for row in rows:
        g.set_x(row)
        plan.set_start(row[cb.csr[1]])
        plan.solve(maxiters, ftol)
        out.append(plan.fetch())
    return out


def _rows_equal(bad, m, single):
    for s, r in enumerate(single):
        for k in FIELDS:
            a, b = getattr(m, k)[s], getattr(r, k)
            bad.check(np.array_equal(a, b, equal_nan=k in ("fret", "delta", "x")), "row", s, k, "== plan_solve", a if a.size < 12 else "", b if b.size < 12 else "")


def _check_rows(cb, rows, nan_row, m, single, best=None):
    bad = X.Problems()
    fp = cb.csr[0]
    _rows_equal(bad, m, single)
    bad.check(not np.any((m.status & 0xFF) == 7), "an exchange gave up")
    for c, ((v, f), name) in enumerate(zip(cb.comps, cb.names)):
        for s in range(len(rows)):
            start = X.clamp(cb.pp, v, rows[s][v])
            code = int(m.status[s, c]) & 0xFF
            nan = name == "room" and s == nan_row
            if name in ("flat", "empty") or nan or (name == "blocked" and np.array_equal(rows[s][v], cb.pp.x0[v])):   # (blocked: from x0 only)
                bad.check(m.x[s, fp[c]:fp[c + 1]].tobytes() == start.tobytes() and m.delta[s, c] == 0.0, name, s, "comes back as its clamped start", m.delta[s, c])
            bad.check((code == 6) == (name == "empty") and (code == 5) == nan, name, s, "code", code)
        if name == "room":
            bad.check((int(m.status[nan_row, c]) & X.ROLLED_BACK) and np.isnan(m.fret[nan_row, c]), name, "the NaN row is rolled back", m.fret[nan_row, c])
            if best is not None:
                bad.check(int(best[c]) != nan_row, name, "the selection picked the NaN row", best)
    return bad


MANY_BODIES = {
    "LDS-resident": ({}, "components_lds", None),
    "point-major": ({**OFF, "ptm_stream": 2, "ptm_group": 1}, "components_point_major", "population_point_major"),
}


@pytest.mark.parametrize("body", list(MANY_BODIES))
def test_many_solve_entries_equal_plan_solve_row_by_row(body, gctx):
    """Plan.solve_starts (LDS-resident body) and Plan.solve_population (LDS-resident; point-major with its option) on rows =
    {the ordinary start, the truth, a NaN start}: every (row, component) == plan_solve from that row; the flat and blocked
    domains hold for every row; the best-start selection never picks the NaN row, whose entries come back as its clamped start"""
    opts, key, pop_option = MANY_BODIES[body]
    cb, rows, nan_row = X.many()
    g, plan = _plan(gctx, cb, opts, trace=False)
    assert plan.info(key) == sum(1 for _, f in cb.comps if len(f) > 0)
    single = _rows_by_plan_solve(g, plan, cb, rows)
    if pop_option is None:
        g.set_x(cb.pp.x0)
        plan.solve_starts(np.ascontiguousarray(rows[:, cb.csr[1]]), 25, 3e-8)
        m = plan.fetch_starts()
        bad = _check_rows(cb, rows, nan_row, m, single, best=m.best)
        assert not bad, "\n".join(repr(b) for b in bad)
        kept, after = plan.fetch(), g.get_x()
        for c in range(len(cb.comps)):       # the plan's ordinary outputs and the problem's x: the start kept
            assert np.array_equal(_component(cb, kept, c).x, m.x[int(m.best[c]), cb.csr[0][c]:cb.csr[0][c + 1]]) and kept.fret[c] == m.fret[int(m.best[c]), c]
        assert np.array_equal(after[cb.csr[1]], kept.x)
    else:
        plan.set_option(pop_option, 1)
    g.set_x(cb.pp.x0)
    pop = capi.Population(g, x=rows)
    plan.solve_population(pop, 25, 3e-8)
    m = plan.fetch_population()
    bad = _check_rows(cb, rows, nan_row, m, single)
    assert not bad, "\n".join(repr(b) for b in bad)
    assert np.array_equal(pop.get_x()[:, cb.csr[1]], m.x, equal_nan=True)
    pop.close(); plan.close(); g.close()


def test_population_on_the_tiny_component_solver(gctx):
    """population_tiny: members = {the start, the truth} of the tiny cases (the flat point's domain holds for both; the point in
    its camera's plane stays there in the start's row) == plan_solve from each member"""
    cb = X.tiny()
    rows = np.stack([cb.pp.x0, cb.pp.x0])
    pts = np.concatenate([v for (v, _), n in zip(cb.comps, cb.names) if n != "nan"])
    rows[1, pts] = cb.x_true[pts]
    g, plan = _plan(gctx, cb, {"quad_min_components": 1, "population_tiny": 1}, trace=False)
    assert plan.info("components_tiny") == len(cb.comps)
    single = _rows_by_plan_solve(g, plan, cb, rows)
    g.set_x(cb.pp.x0)
    pop = capi.Population(g, x=rows)
    plan.solve_population(pop, 25, 3e-8)
    m = plan.fetch_population()
    bad = X.Problems()
    _rows_equal(bad, m, single)
    assert not bad, "\n".join(repr(b) for b in bad)
    c = cb.names.index("nan")
    assert np.all((m.status[:, c] & 0xFF) == 5) and np.all(m.delta[:, c] == 0.0)
    pop.close(); plan.close(); g.close()


def test_many_solve_entries_on_the_plain_nonlinear_product_body(gctx):
    """solve_starts and, with population_plain, solve_population on load_poly() with lo = hi = x0: rows anywhere are clamped
    to the one point of the domain, every row ends with code 0 after 30 / 26 calls == plan_solve"""
    pp = X.flat(P.load_poly()).single_component()
    cb = X.Combined(pp, [(np.arange(pp.nvars, dtype=np.int64), np.arange(pp.nfac, dtype=np.int64))], ["flat"],
                    (pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id), None)
    rows = np.stack([pp.x0, pp.x0 + 1.0, pp.x0 - 2.0])
    g, plan = _plan(gctx, cb, {"population_plain": 1}, trace=False)
    assert plan.info("components_plain") == 1
    single = _rows_by_plan_solve(g, plan, cb, rows)
    g.set_x(pp.x0)
    plan.solve_starts(rows, 25, 3e-8)
    ms = plan.fetch_starts()
    g.set_x(pp.x0)
    pop = capi.Population(g, x=rows)
    plan.solve_population(pop, 25, 3e-8)
    mp = plan.fetch_population()
    for m in (ms, mp):
        bad = X.Problems()
        _rows_equal(bad, m, single)
        assert not bad, "\n".join(repr(b) for b in bad)
        assert np.all(m.status == 0) and np.all(m.iters == 0) and np.all(m.nfeval == 30) and np.all(m.ngeval == 26) and np.all(m.delta == 0.0)
        assert all(m.x[s].tobytes() == pp.x0.tobytes() for s in range(3))
    assert int(ms.best[0]) == 0
    pop.close(); plan.close(); g.close()


def test_many_solve_entries_with_a_nan_row_on_the_nonlinear_product_body(gctx):
    """sqrt(x) + x^2 on [-5, 5] (test_empty_factor_list_and_nan's function): the row x = -1 starts at a NaN and comes back restored
    with delta 0 from solve_starts and, with population_plain, solve_population -- the roll-back of the plain solver's two
    many-solve kernels; every row == plan_solve, and the selection does not keep the NaN row"""
    pp = P._pack_nlp([(1.0, [(0, 0.5, 0.0, 0)]), (1.0, [(0, 2.0, 0.0, 0)])], np.array([1.0]), np.array([-5.0]), np.array([5.0]), {}).single_component()
    cb = X.Combined(pp, [(np.arange(1, dtype=np.int64), np.arange(2, dtype=np.int64))], ["sqrt"],
                    (pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id), None)
    rows = np.array([[-1.0], [1.0], [2.0]])
    g, plan = _plan(gctx, cb, {"population_plain": 1}, trace=False)
    assert plan.info("components_plain") == 1
    single = _rows_by_plan_solve(g, plan, cb, rows)
    g.set_x(pp.x0)
    plan.solve_starts(rows, 25, 3e-8)
    ms = plan.fetch_starts()
    g.set_x(pp.x0)
    pop = capi.Population(g, x=rows)
    plan.solve_population(pop, 25, 3e-8)
    mp = plan.fetch_population()
    for m in (ms, mp):
        bad = X.Problems()
        _rows_equal(bad, m, single)
        bad.check((int(m.status[0, 0]) & 0xFF) == 5 and (int(m.status[0, 0]) & X.ROLLED_BACK), "the NaN row: code 5, rolled back", m.status[0, 0])
        bad.check(np.isnan(m.fret[0, 0]) and m.delta[0, 0] == 0.0 and m.x[0, 0] == -1.0, "the NaN row: its start, delta 0", m.fret[0, 0], m.delta[0, 0], m.x[0, 0])
        bad.check(np.all(m.delta <= 0.0) and not np.any(np.isnan(m.fret[1:])), "the finite rows", m.delta, m.fret)
        assert not bad, "\n".join(repr(b) for b in bad)
    assert int(ms.best[0]) != 0
    pop.close(); plan.close(); g.close()
