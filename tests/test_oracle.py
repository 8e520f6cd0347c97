"""Pins the CPU oracle (oracle/rdis_oracle.c) before anything is compared with it:

* against the reference's golden values (tests/golden/reference_golden.json): per-factor values and
  partials, the full objective and gradient, and the four recorded CGD runs -- all bit for bit,
* against the reference's own documented minima of data/testpoly.txt,
* bit for bit against the reference's minimize_nrc.h built as oracle/_ref.
"""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from rdis_amd import problems as P


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


# ---------------------------------------------------------------- BA factor
def test_ba_factor0_value_and_gradient(golden):
    g0 = golden["ba_factor0"]
    vals = np.array(g0["cam"] + g0["pt"])
    e = O.ba_factor_eval(vals, *g0["obs"])
    assert e == g0["E"]                      # same expression order -> bit-exact
    # the reference's forward chain restated operation by operation: bit-exact
    e1, gref = O.ba_factor_grad_ref(vals, *g0["obs"])
    assert e1 == g0["E"] and list(gref) == g0["grad"]
    e2, g = O.ba_factor_grad(vals, *g0["obs"])
    assert e2 == g0["E"]
    # adjoint-mode derivative vs the reference's forward chain rule: rounding only
    assert rel(g, g0["grad"]) < 1e-13


def _seq_norm(g):
    s = 0.0
    for v in g:
        s += float(v) * float(v)
    return float(np.sqrt(s))


def test_two_oracle_derivatives_agree_on_every_ladybug_factor():
    """The oracle holds two derivatives of the reprojection factor: the reference's forward chain
    (bit-exact against the reference's recorded partials and runs) and an adjoint sweep derived
    independently from the camera model (the derivation the device kernels share).  They are
    compared here on all 31843 factors of ladybug, at the BAL start and at a perturbed point, so a
    derivation error in either would show."""
    p = P.load_bal()
    rng = np.random.default_rng(11)
    for x in (p.x0, p.x0 * (1 + 1e-2 * rng.standard_normal(p.nvars))):
        o = O.OracleProblem(p, derivative="refchain")
        o.assign(None, x)
        a = o.grad_each_ba()
        o.set_derivative("adjoint")
        b = o.grad_each_ba()
        assert a.shape == b.shape == (31843, 12) and not np.array_equal(a, b)
        d = np.max(np.abs(a - b), axis=1) / np.max(np.abs(a), axis=1)
        assert d.max() < 2e-14, (d.max(), int(d.argmax()))
        o.set_derivative("refchain")
        ga = o.gradient()
        o.set_derivative("adjoint")
        gb = o.gradient()
        assert np.max(np.abs(ga - gb)) < 1e-13 * np.max(np.abs(ga))


def test_ba_gradient_matches_central_differences():
    p = P.load_bal(ncams=5, npts=30)
    o = O.OracleProblem(p)
    g = o.grad_each_ba()
    rng = np.random.default_rng(3)
    for f in rng.choice(p.nfac, 8, replace=False):
        vals = np.concatenate([p.x0[p.cam_vid0[f]:p.cam_vid0[f] + 9], p.x0[p.pt_vid0[f]:p.pt_vid0[f] + 3]])
        for k in range(12):
            h = 1e-6 * max(1.0, abs(vals[k])) if k not in (7, 8) else 1e-9
            a, b = vals.copy(), vals.copy()
            a[k] += h
            b[k] -= h
            fd = (O.ba_factor_eval(a, *p.obs[f]) - O.ba_factor_eval(b, *p.obs[f])) / (2 * h)
            assert abs(fd - g[f, k]) <= 2e-4 * max(abs(g[f, k]), 1e-3), (f, k)


def test_ba_theta_zero_branch():
    # theta == 0 takes the first-order branch P = q + r x q (reference .cpp:304-329)
    vals = np.array([0, 0, 0, 0.1, -0.2, -3.0, 400.0, -3e-7, 5e-13, 0.3, -0.4, 0.5])
    e, g = O.ba_factor_grad(vals, 10.0, -20.0)
    assert np.isfinite(e) and np.all(np.isfinite(g))
    tiny = vals.copy()
    tiny[0] = 1e-9
    e2, g2 = O.ba_factor_grad(tiny, 10.0, -20.0)
    assert abs(e - e2) < 1e-6 * e
    assert rel(g[3:], g2[3:]) < 1e-6


def test_ladybug_full_eval_and_gradient(golden):
    gl = golden["ladybug_full"]
    p = P.load_bal()
    assert (p.nvars, p.nfac) == (gl["nvars"], gl["nfac"])
    o = O.OracleProblem(p)
    each = o.eval_each()
    assert each[1] == gl["E_factor1"] and each[31842] == gl["E_factor31842"]
    assert o.eval() == gl["f_xinit"]
    g = o.gradient()                       # reference-order derivative, factor-order sums: bit-exact
    assert _seq_norm(g) == gl["grad_norm2"]
    assert list(g[0:9]) == gl["grad_0_8"] and list(g[441:444]) == gl["grad_441_443"]
    assert g[23768] == gl["grad_23768"]
    o.set_derivative("adjoint")
    g2 = o.gradient()
    gmax = np.max(np.abs(g))
    assert np.max(np.abs(g2 - g)) < 1e-13 * gmax
    o.set_derivative("refchain")
    # the reference's sorted-vector merge and dense accumulation are the same sum
    sub = np.arange(0, 4000, dtype=np.int64)
    assert np.array_equal(o.gradient(sub, merge=True), o.gradient(sub, merge=False))


def test_bal_subsets_match_reference_sizes(golden):
    for key in ("ladybug_5_30", "ladybug_49_500", "ladybug_49_2000"):
        c = golden["cgd"][key]
        p = P.load_bal(ncams=c["ncams"], npts=c["npts"])
        assert (p.nvars, p.nfac) == (c["nvars"], c["nfac"])
    c = golden["cgd"]["ladybug_5_30"]
    o = O.OracleProblem(P.load_bal(ncams=5, npts=30))
    assert o.eval() == c["f0"] and _seq_norm(o.gradient()) == c["grad_norm2"]


# ---------------------------------------------------------------- NLP / poly
def test_testpoly_known_answers(golden):
    t = golden["testpoly"]
    p = P.load_poly()
    assert (p.nvars, p.nfac) == (t["nvars"], t["nfac"])
    assert list(p.lo) == t["lo"] and list(p.hi) == t["hi"]
    o = O.OracleProblem(p)
    o.assign(None, np.array([1.0, -2.0]))
    assert o.eval() == t["f_1_m2"]
    o.assign(None, np.array([-4.6601, -4.6601]))
    assert o.eval() == t["f_m46601"]
    # the reference's documented minima (data/testpoly.txt:17-22), 4 digits
    for fmin, a, b in t["documented_minima"]:
        o.assign(None, np.array([a, b]))
        assert abs(o.eval() - fmin) < 2e-4


def test_testpoly_cgd_golden(golden):
    t = golden["testpoly"]
    o = O.OracleProblem(P.load_poly())
    for case in t["cgd"]:
        r = o.cgd(x=np.array(case["start"]), maxiters=t["cgd_maxiters"])
        assert r.fret == case["fret"], case          # converged: bit-exact
        if "x" in case:
            assert list(r.x) == case["x"]
        assert r.status in (0, 1, 2)


def test_sinusoid_shape_and_derivative(golden):
    s = P.make_high_dim_sinusoid()
    assert (s.nvars, s.nfac) == (golden["sinusoid"]["nvars"], golden["sinusoid"]["nfac"])
    assert np.sum(np.diff(s.rowptr) == 1) == 242 and np.sum(np.diff(s.rowptr) == 2) == 120
    o = O.OracleProblem(s)
    x = np.random.default_rng(1).uniform(-6.28, 6.28, s.nvars)
    o.assign(None, x)
    g = o.gradient()
    for j in (0, 5, 39, 120):
        a, b = x.copy(), x.copy()
        a[j] += 1e-6
        b[j] -= 1e-6
        o.assign(None, a)
        fa = o.eval()
        o.assign(None, b)
        fb = o.eval()
        assert abs((fa - fb) / 2e-6 - g[j]) < 1e-6 * max(1, abs(g[j]))


def test_sinusoid_full_domain_start_fixture():
    """the committed start of config 2 (tests/golden/sinusoid_start.json, generated by
    tests/golden/make_sinusoid_start.py): uniform over the whole domain like optSinusoid's
    (src/optimize_sinusoid.cpp:154-165)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sinusoid_start.json")) as fh:
        d = json.load(fh)
    s = P.make_high_dim_sinusoid()
    x0 = np.array(d["x0"])
    assert len(x0) == s.nvars == 121 and d["lo"] == s.lo[0] and d["hi"] == s.hi[0]
    assert abs(s.hi[0] - 10 * 2.000001 * 3.141592653) < 1e-4            # +-10 tp, as the generator prints it (OptimizableFunctionGenerator.cpp:660-760)
    assert np.all(x0 >= s.lo) and np.all(x0 <= s.hi) and x0.max() - x0.min() > 100
    o = O.OracleProblem(s)
    o.assign(None, x0)
    assert abs(o.eval() - 17126.136253546265) < 1e-9
    r = O.OracleProblem(s).cgd(x=x0, maxiters=25)
    assert r.fret < 0.2 * r.finit and np.any((r.x == s.lo) | (r.x == s.hi))   # a bound is active at the end


# ---------------------------------------------------------------- minimiser
def _rosen(x):
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2))


def _rosen_g(x):
    g = np.zeros_like(x)
    g[:-1] = -400 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2 * (1 - x[:-1])
    g[1:] += 200 * (x[1:] - x[:-1] ** 2)
    return g


def _minimiser_cases(maxiters):
    rng = np.random.default_rng(maxiters)
    return [(_rosen, _rosen_g, rng.uniform(-2, 2, 6)),
            (lambda x: float(np.sum(np.cos(x) + 0.05 * x * x)), lambda x: -np.sin(x) + 0.1 * x,
             rng.uniform(-6, 6, 9)),
            (lambda x: float(np.sum((x - 1.5) ** 4)), lambda x: 4 * (x - 1.5) ** 3, rng.uniform(-3, 3, 3)),
            (lambda x: 0.0 * x[0] + 7.0, lambda x: np.zeros_like(x), np.array([1.0, 2.0]))]


def _ba_minimiser_case():
    p = P.load_bal(ncams=5, npts=30)
    o = O.OracleProblem(p, emulate_stale_cache=False)

    def f(x):
        o.assign(None, np.clip(x, p.lo, p.hi))
        return o.eval()

    def g(x):
        o.assign(None, np.clip(x, p.lo, p.hi))
        return o.gradient()
    return f, g, p.x0


def _reference_frprmn(key, f, g, x0, maxiters):
    """the reference's minimiser on (f, g, x0): run live from oracle/_ref where it is built (and then the recorded result must be
    the same), else the recorded result of the same case"""
    # what the reference's nrc::Frprmn (oracle/_ref) returned on the same case, recorded by tests/golden/make_reference_frprmn.py
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_frprmn.json")) as fh:
        rec = json.load(fh)[key]
    assert np.array_equal(np.array(rec["x0"]), x0)
    want = (rec["reason"], np.array(rec["x"]), rec["fret"], rec["iter"])
    if O.ref_available():
        b = O.ref_frprmn(f, g, x0, maxiters, 3e-8)
        assert b[0] == want[0] and np.array_equal(b[1], want[1]) and b[2] == want[2] and b[3] == want[3]
        return b
    return want


@pytest.mark.parametrize("maxiters", [1, 2, 7, 25, 400])
def test_minimiser_bit_exact_vs_reference_header(maxiters):
    """restated Frprmn/linmin/Dbrent/bracket == the reference's minimize_nrc.h"""
    for k, (f, g, x0) in enumerate(_minimiser_cases(maxiters)):
        a = O.frprmn(f, g, x0, maxiters, 3e-8)
        b = _reference_frprmn("maxiters_%d_case_%d" % (maxiters, k), f, g, x0, maxiters)
        assert a[0] == b[0] or (b[0] == 0 and a[0] in (0, 1, 2))
        assert np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


def test_minimiser_bit_exact_on_bundle_adjustment():
    f, g, x0 = _ba_minimiser_case()
    a = O.frprmn(f, g, x0, 25, 3e-8)
    b = _reference_frprmn("ladybug_5_30", f, g, x0, 25)
    assert a[0] == b[0] == 3                       # "Too many iterations in frprmn"
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] == 24


# ---------------------------------------------------------------- CGD wrapper
@pytest.mark.parametrize("key", ["ladybug_5_30", "ladybug_49_500", "ladybug_49_2000", "ladybug_full"])
def test_reference_recorded_cgd_runs_bit_exact(golden, key):
    """The four CGD runs the reference itself produced in this container (BASELINE.md 2:
    unmodified reference sources, g++ -O2, glibc libm) are reproduced exactly: end value, evaluation
    counts, end point.  25 unconverged CG iterations on bundle adjustment amplify a one-ulp
    difference to percents (test_cgd_is_chaotic below), so equality of the end value after
    500-800 dependent evaluations pins every rounding on the way: the forward-chain derivative
    (BundleAdjustmentFactor.cpp:351-554), the factor-order sums (OptimizableFunction.cpp:118,
    248-262; State.h:174-194), the stale-cache rule (Variable.cpp:70-76) and the minimiser."""
    c = golden["cgd"][key]
    p = P.load_bal(ncams=c["ncams"], npts=c["npts"])
    r = O.OracleProblem(p).cgd(maxiters=c["maxiters"], ftol=3e-8)
    assert r.fret == c["fret"] and r.nfeval == c["nfeval"]
    assert r.status == 3 and r.iters == c["maxiters"] - 1          # "Too many iterations in frprmn"
    if "ngeval" in c:
        assert r.ngeval == c["ngeval"]
    if "f0" in c:
        assert r.finit == c["f0"]
    if "delta" in c:
        assert r.delta == c["delta"]
    if "x_0_2" in c:
        assert list(r.x[:3]) == c["x_0_2"]


def test_recorded_runs_need_every_reference_detail(golden):
    """drop any one of the reference's rounding-relevant details and the recorded end point is lost"""
    c = golden["cgd"]["ladybug_5_30"]
    p = P.load_bal(ncams=5, npts=30)
    for kw in (dict(derivative="adjoint"), dict(emulate_stale_cache=False)):
        r = O.OracleProblem(p, **kw).cgd(maxiters=25)
        assert r.fret != c["fret"] and abs(r.fret - c["fret"]) < 0.05 * c["fret"]


def test_device_arithmetic_switches_are_the_only_difference(golden):
    """The CPU side of the end-to-end == tests (tests/test_gpu_parity.py): the oracle with its three named switches for the
    device's factor arithmetic.  (1) With the switches off it is the reference-pinned oracle (the recorded run, ==).
    (2) Each switch alone leaves every factor's value / partials within last places of the reference's arithmetic -- the
    reciprocals move values (1e-11 of a value that is a cancelled residual), the two derivative forms move partials by 2e-15 of
    a row's largest entry, the angle routine does not move a single one of ladybug's 49 cameras at x0 (it is below 1 ulp, like
    the C library's).  (3) With all three on, 25 iterations from x0 end where tests/golden/parity_end_values.json says -- numbers
    that do not depend on the machine (no C-library transcendental is left on the path) and that the device's parity option
    reproduces bit for bit on the GPU."""
    import json
    c = golden["cgd"]["ladybug_5_30"]
    p = P.load_bal(ncams=5, npts=30)
    assert O.OracleProblem(p, derivative="refchain", arithmetic="reference").cgd(maxiters=25).fret == c["fret"]
    full = P.load_bal()
    ref = O.OracleProblem(full)
    f0, g0 = ref.eval_each(), ref.grad_each_ba()
    rowmax = np.max(np.abs(g0), axis=1, keepdims=True)
    for kw, moves_f, tol_f, tol_g in ((dict(arithmetic="reciprocal"), True, 1e-10, 1e-10), (dict(arithmetic="sincos_angle"), False, 0.0, 0.0),
                                      (dict(derivative="adjoint_device"), False, 0.0, 1e-14)):
        o = O.OracleProblem(full, **kw)
        f, g = o.eval_each(), o.grad_each_ba()
        assert bool(np.any(f != f0)) == moves_f and np.max(np.abs(f - f0) / np.abs(f0)) <= tol_f, kw
        assert np.max(np.abs(g - g0) / rowmax) <= tol_g, kw
    with open(os.path.join(os.path.dirname(__file__), "golden", "parity_end_values.json")) as fh:
        want = json.load(fh)
    for key in ("ladybug_5_30_stale_cache", "ladybug_5_30"):
        w = want[key]
        pp = P.load_bal(ncams=w["ncams"], npts=w["npts"]).single_component()
        r = O.OracleProblem.device_parity(pp, emulate_stale_cache=w["emulate_stale_cache"]).cgd(x=pp.x0, maxiters=w["maxiters"])
        assert (r.fret, r.delta, r.iters, r.status, r.nfeval, r.ngeval) == (w["fret"], w["delta"], w["iters"], w["status"], w["nfeval"], w["ngeval"])
        assert list(r.x[:3]) == w["x_0_2"] and r.x[-1] == w["x_last"]
        assert r.fret != c["fret"] and abs(r.fret - c["fret"]) < 0.05 * c["fret"]     # another member of the chaotic family


def test_device_arithmetic_end_value_on_full_ladybug():
    """... and BASELINE config 4: 85993.13597324853 after 805 evaluations (the reference's arithmetic: 83227.60422775625 after 825)"""
    import json
    with open(os.path.join(os.path.dirname(__file__), "golden", "parity_end_values.json")) as fh:
        w = json.load(fh)["ladybug_full_stale_cache"]
    pp = P.load_bal().single_component()
    r = O.OracleProblem.device_parity(pp).cgd(x=pp.x0, maxiters=25)
    assert (r.fret, r.iters, r.nfeval, r.ngeval) == (w["fret"], w["iters"], w["nfeval"], w["ngeval"])
    assert list(r.x[:3]) == w["x_0_2"] and r.x[-1] == w["x_last"]


@pytest.mark.parametrize("key", ["ladybug_49_500_default_path", "ladybug_full_default_path"])
def test_sum_topology_switch_reproduces_the_default_paths_fixture(key):
    """The fourth named switch, RO_SUM_TOPOLOGY_COOPERATIVE: the device's cooperative solvers add their sums as trees (a wave of 64
    as a balanced tree, the waves' sums taken l, l + 64, ... by lane l, the slope factor by factor, gg / dgg by owner lane, a
    wave-owned variable's partials strided over a wave).  With it and the three arithmetic switches the oracle ends where
    tests/golden/parity_end_values.json says -- on full ladybug 89607.17144518998 after 798 evaluations, which is the number the
    benchmarked DEFAULT path prints (the GPU suite asserts device == this oracle live; bench.py compares its timed solve with the
    fixture).  Helpers first: the balanced tree of 64 equals what the device's butterfly leaves in every lane (a + b == b + a), and
    the topology's sums equal the plain ones to rounding."""
    import json
    with open(os.path.join(os.path.dirname(__file__), "golden", "parity_end_values.json")) as fh:
        w = json.load(fh)[key]
    pp = P.load_bal(ncams=w["ncams"], npts=w["npts"]).single_component()
    o = O.OracleProblem.device_default(pp)
    plain = O.OracleProblem(pp, emulate_stale_cache=False, derivative="adjoint_device", arithmetic="device")
    assert abs(o.eval() - plain.eval()) <= 1e-12 * plain.eval() and o.eval() != plain.eval()
    go, gp = o.gradient(), plain.gradient()
    assert np.max(np.abs(go - gp)) <= 1e-12 * np.max(np.abs(gp))
    r = o.cgd(x=pp.x0, maxiters=w["maxiters"])
    assert (r.fret, r.delta, r.iters, r.status, r.nfeval, r.ngeval) == (w["fret"], w["delta"], w["iters"], w["status"], w["nfeval"], w["ngeval"])
    assert list(r.x[:3]) == w["x_0_2"] and r.x[-1] == w["x_last"]


def test_lds_topology_with_the_host_compiled_arithmetic_reproduces_its_fixture():
    """The DEFAULT batch path (configs 3, 5-S) contracts a * b + c into fused multiply-adds; a C restatement compiled by another
    compiler cannot promise those bits, so the oracle takes the factor arithmetic from outside (ro_set_factor_arithmetic):
    rdis_amd/csrc/factors.hpp itself compiled for the HOST by the same front end (tests/cpp/factors_host.hip; per factor == the
    device under -m gpu).  With it and RO_SUM_TOPOLOGY_LDS (the LDS-resident solver's trees) the oracle ends where
    tests/golden/parity_end_values.json says: 25.168503286225235 after 540 evaluations on ladybug 5 / 30 -- what smoke() and the
    bench line's configs block print --, and the first components of the synthetic decomposition.  The plugged-in arithmetic
    agrees with the built-in one to rounding (the same model, fused)."""
    import json
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc to compile factors.hpp for the host")
    with open(os.path.join(os.path.dirname(__file__), "golden", "parity_end_values.json")) as fh:
        fx = json.load(fh)
    w = fx["ladybug_5_30_default_path"]
    pp = P.load_bal(ncams=5, npts=30).single_component()
    o = O.OracleProblem.device_lds_default(pp)
    ref = O.OracleProblem(pp, emulate_stale_cache=False)
    fe, fr = o.eval_each(), ref.eval_each()
    assert np.max(np.abs(fe - fr) / np.abs(fr)) < 1e-9 and np.any(fe != fr)
    r = o.cgd(x=pp.x0, maxiters=25)
    assert (r.fret, r.delta, r.iters, r.status, r.nfeval, r.ngeval) == (w["fret"], w["delta"], w["iters"], w["status"], w["nfeval"], w["ngeval"])
    assert list(r.x[:3]) == w["x_0_2"] and r.x[-1] == w["x_last"]
    ws = fx["synthetic_S_default_path"]
    ps = P.make_synthetic_ba(8, 3, 40)
    for c in range(8):
        fv, fc = ps.component(c)
        rc = O.OracleProblem.device_lds_default(ps, free_vid=fv, fac=fc).cgd(free_vid=fv, fac=fc, x=ps.x0[fv], maxiters=25)
        assert rc.fret == ws["fret"][c] and rc.nfeval == ws["nfeval"][c], c


def test_point_major_topology_reproduces_its_fixture():
    """RO_SUM_TOPOLOGY_PTM -- the point-major streaming solver's layout and sums (BASELINE config 5-L), with factors.hpp compiled for
    the host for both forms of the arithmetic -- ends where tests/golden/parity_end_values.json says: component 0 of the synthetic
    49 x 7776 x 4 decomposition under one workgroup of 768 lanes and as a pair of 512 (the device returns the same bits under -m
    gpu, tests/test_gpu_parity.py).  The plan's point order is restated in oracle.py (ptm_point_order): by number of factors
    descending, whole chunks of 64 dealt over sixteen runs; the matrix form agrees with the vector form to rounding."""
    import json
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc to compile factors.hpp for the host")
    with open(os.path.join(os.path.dirname(__file__), "golden", "parity_end_values.json")) as fh:
        fx = json.load(fh)
    pp = P.make_synthetic_ba(1, 49, 7776, obs_per_pt=4)
    fv, fc = pp.component(0)
    cams, pts = O.ptm_point_order(pp.cam_vid0[fc], pp.pt_vid0[fc])
    assert len(cams) == 49 and len(pts) == 7776 and len(set(pts.tolist())) == 7776 and not np.array_equal(pts, np.sort(pts))
    for w in fx["synthetic_L_default_path"]["runs"]:
        if w["component"] != 0 or w["group"] > 2:
            continue
        o = O.OracleProblem.device_ptm_default(pp, fac=fc, threads=w["threads"], group=w["group"])
        rc = o.cgd(free_vid=fv, fac=fc, x=pp.x0[fv], maxiters=25)
        assert (rc.fret, rc.iters, rc.nfeval, rc.ngeval) == (w["fret"], w["iters"], w["nfeval"], w["ngeval"]), w
    # the matrix form's value at x0 against the reference-order sum of the vector form: the same model
    o = O.OracleProblem.device_ptm_default(pp, fac=fc)
    ref = O.OracleProblem(pp, emulate_stale_cache=False)
    r0 = o.cgd(free_vid=fv, fac=fc, x=pp.x0[fv], maxiters=0)
    assert abs(r0.finit - ref.eval(fc)) <= 1e-11 * abs(r0.finit)


def test_plain_solver_topology_reproduces_the_nonlinear_product_fixtures():
    """BASELINE configs 1 and 2 (testpoly; the high-dimensional sinusoid from the committed start): the oracle with the device's sine
    / cosine (factors.hpp's nlp_sin / nlp_cos compiled for the host, ro_set_trig), its third and fourth power by multiplication
    (RO_ARITH_POW_SMALL_INT) and the plain workgroup solver's sums (RO_SUM_TOPOLOGY_WG) ends where
    tests/golden/parity_end_values.json says -- what the device returns under -m gpu and what the bench line's configs rows compare
    with.  The device's sine agrees with the C library's to an ulp."""
    import ctypes as C
    import json
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc to compile factors.hpp for the host")
    here = os.path.dirname(__file__)
    with open(os.path.join(here, "golden", "parity_end_values.json")) as fh:
        fx = json.load(fh)
    with open(os.path.join(here, "golden", "sinusoid_start.json")) as fh:
        sin_x0 = np.array(json.load(fh)["x0"])
    for key, pp in (("testpoly_default_path", P.load_poly().single_component()), ("sinusoid_default_path", P.make_high_dim_sinusoid().single_component())):
        if key.startswith("sinusoid"):
            pp.x0 = sin_x0
        w = fx[key]
        r = O.OracleProblem.device_wg_default(pp).cgd(x=pp.x0, maxiters=25)
        assert (r.fret, r.delta, r.iters, r.status, r.nfeval, r.ngeval) == (w["fret"], w["delta"], w["iters"], w["status"], w["nfeval"], w["ngeval"]), key
        assert list(r.x[:2]) == w["x_0_2"] and r.x[-1] == w["x_last"]
    L = O.factors_host()[0]
    L.fh_sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    sn, cs = C.c_double(), C.c_double()
    for v in np.random.default_rng(0).uniform(-70.0, 70.0, 2000):
        L.fh_sincos(float(v), C.byref(sn), C.byref(cs))
        assert abs(sn.value - np.sin(v)) <= 2.3e-16 and abs(cs.value - np.cos(v)) <= 2.3e-16


def test_remaining_solver_restatements_reproduce_their_fixtures():
    """one pin each for the oracle's other restatements of device solvers (the device returns the same bits under -m gpu,
    tests/test_gpu_parity.py): the tiny-component solver (RO_SUM_TOPOLOGY_GROUP), bundle adjustment on the plain solver and on the grid
    solver (RO_SUM_TOPOLOGY_WG, ro_set_stream_topology), a wide point-major group with local camera numbering (ro_set_ptm_local),
    and the public evaluation entry points' sums (ro_eval_device_ba, ro_eval_grad_device_ba)"""
    import json
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc to compile factors.hpp for the host")
    with open(os.path.join(os.path.dirname(__file__), "golden", "parity_end_values.json")) as fh:
        fx = json.load(fh)
    lb = P.load_bal()
    fp, fv, cp, ci = P.ba_alternation_plans(lb)[1]
    v, f = fv[fp[0]:fp[1]], ci[cp[0]:cp[1]]
    r = O.OracleProblem.device_group_default(lb, lanes=16).cgd(free_vid=v, fac=f, x=lb.x0[v], maxiters=25)
    w = fx["ladybug_point_0_tiny_solver"]
    assert (r.fret, r.nfeval, r.ngeval) == (w["fret"], w["nfeval"], w["ngeval"])
    s530 = P.load_bal(ncams=5, npts=30).single_component()
    for key, kw in (("ladybug_5_30_plain_solver", {}), ("ladybug_5_30_grid_solver_3_workgroups", {"grid_workgroups": 3})):
        r = O.OracleProblem.device_wg_default(s530, **kw).cgd(x=s530.x0, maxiters=25)
        assert (r.fret, r.nfeval, r.ngeval) == (fx[key]["fret"], fx[key]["nfeval"], fx[key]["ngeval"]), key
    w24 = P.make_synthetic_ba(1, 24, 30000, obs_per_pt=4).single_component()
    o = O.OracleProblem.device_ptm_default(w24, local_cus=256)
    r = o.cgd(x=w24.x0, maxiters=3)
    w = fx["synthetic_24_30000_local_cameras"]
    assert (len(o._wg_chunk0) - 1, r.fret, r.nfeval, r.ngeval) == (w["workgroups"], w["fret"], w["nfeval"], w["ngeval"])
    o = O.OracleProblem.device_eval(lb)
    fe, ge = o.eval_grad_device()
    w = fx["ladybug_public_evaluation"]
    assert fe == w["value"] == o.eval_device() and list(ge[:3]) == w["g_0_2"] and ge[-1] == w["g_last"] and float(np.abs(ge).sum()) == w["g_abs_sum"]
    ref = O.OracleProblem(lb, emulate_stale_cache=False)
    assert abs(fe - ref.eval()) <= 1e-12 * fe and np.max(np.abs(ge - ref.gradient())) <= 1e-11 * np.max(np.abs(ge))


def test_cgd_is_chaotic():
    """25 unconverged CG iterations are a chaotic map of the start point: a 1e-15 relative
    perturbation moves the end value by far more than 1e-6 relative, while one line minimisation
    is reproducible to Brent's own tolerance"""
    p = P.load_bal(ncams=5, npts=30)
    frets = []
    rng = np.random.default_rng(0)
    for _ in range(5):
        q = P.load_bal(ncams=5, npts=30)
        q.x0 = q.x0 * (1 + 1e-15 * rng.standard_normal(q.nvars))
        frets.append(O.OracleProblem(q).cgd(maxiters=25).fret)
    assert max(frets) - min(frets) > 1e-4 * np.mean(frets)
    a = O.OracleProblem(p).cgd(maxiters=1).fret
    q = P.load_bal(ncams=5, npts=30)
    q.x0 = q.x0 * (1 + 1e-15 * rng.standard_normal(q.nvars))
    assert abs(O.OracleProblem(q).cgd(maxiters=1).fret - a) < 1e-6 * a


def test_cgd_contract_details():
    p = P.load_poly()
    o = O.OracleProblem(p)
    # empty factor list: returns 0, delta 0, x untouched (CGDSubspaceOptimizer.cpp:26-29)
    r = o.cgd(fac=np.zeros(0, dtype=np.int64), x=np.array([3.0, 4.0]))
    assert (r.fret, r.delta, r.status) == (0.0, 0.0, 6) and list(r.x) == [3.0, 4.0]
    # start outside the domain is clamped before the first evaluation
    r = o.cgd(x=np.array([100.0, -100.0]), maxiters=50)
    o2 = O.OracleProblem(p)
    o2.assign(None, np.array([8.0, -9.0]))
    assert r.finit == o2.eval()
    assert np.all(r.x >= p.lo) and np.all(r.x <= p.hi) and r.delta <= 0
    # a sub-function: only x0 free, only the factors that mention x0
    fac = np.array([0, 1, 5], dtype=np.int64)
    o3 = O.OracleProblem(p)
    o3.assign(None, np.array([0.0, 2.0]))
    r = o3.cgd(free_vid=np.array([0]), fac=fac, x=np.array([0.0]), maxiters=50)
    assert abs(r.x[0] - (-4.6601175)) < 1e-5 and o3.get_x()[1] == 2.0


# ---------------------------------------------------------------- data formats either side of the path
def test_bal_save_load_round_trip(tmp_path):
    pp = P.load_bal(ncams=5, npts=30)
    x = pp.x0 * (1 + 1e-3 * np.random.default_rng(0).standard_normal(pp.nvars))
    f = str(tmp_path / "state.txt")
    P.save_bal(pp, f, x)
    q = P.load_bal(f)
    assert np.array_equal(q.x0, x) and np.array_equal(q.obs, pp.obs)
    assert np.array_equal(q.cam_vid0, pp.cam_vid0) and np.array_equal(q.pt_vid0, pp.pt_vid0)


def test_alternation_decompositions_are_independent_components():
    pp = P.load_bal(ncams=49, npts=500)
    for (free_ptr, free_vid, fac_ptr, fac_id), block, nblk in zip(P.ba_alternation_plans(pp), (9, 3), (49, 500)):
        assert len(free_ptr) == nblk + 1 and np.array_equal(np.sort(fac_id), np.arange(pp.nfac))   # every factor once
        owner = np.repeat(np.arange(nblk), np.diff(fac_ptr))
        blk_of = (pp.cam_vid0[fac_id] // 9) if block == 9 else ((pp.pt_vid0[fac_id] - 441) // 3)
        assert np.array_equal(owner, blk_of)                       # a factor belongs to the component of its block
        for c in (0, nblk // 2, nblk - 1):
            assert np.all(np.diff(fac_id[fac_ptr[c]:fac_ptr[c + 1]]) > 0)   # ascending factor ids (Component.cpp:78-79)
            assert np.array_equal(free_vid[free_ptr[c]:free_ptr[c + 1]], (0 if block == 9 else 441) + block * c + np.arange(block))


# ---- connected components of the residual factor graph (Component::createChildren) -------------
def _scipy_components(pp, assigned):
    """independent implementation: scipy's connected_components on the bipartite variable-factor graph"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n, f = pp.nvars, pp.nfac
    if pp.kind == 0:
        rows = np.repeat(np.arange(f), 12)
        cols = np.concatenate([pp.cam_vid0[:, None] + np.arange(9), pp.pt_vid0[:, None] + np.arange(3)], axis=1).reshape(-1)
    else:
        rows = np.repeat(np.arange(f), np.diff(pp.rowptr))
        cols = pp.vid
    keep = assigned[cols] == 0
    g = coo_matrix((np.ones(keep.sum()), (cols[keep], n + rows[keep])), shape=(n + f, n + f))
    _, lab = connected_components(g, directed=False)
    comps = {}
    for v in np.where(assigned == 0)[0]:
        comps.setdefault(lab[v], ([], []))[0].append(int(v))
    has_edge = np.zeros(f, bool)
    has_edge[rows[keep]] = True
    for k in np.where(has_edge)[0]:                      # a factor without an unassigned variable is in no component
        comps[lab[n + k]][1].append(int(k))
    order = sorted(comps.values(), key=lambda c: (len(c[0]), c[0][0]))
    return order


@pytest.mark.parametrize("case", ["ladybug_cams", "ladybug_random", "synthetic", "sinusoid", "none", "all"])
def test_components_match_scipy(case):
    rng = np.random.default_rng(5)
    if case.startswith("ladybug"):
        pp = P.load_bal(ncams=49, npts=300)
        a = np.zeros(pp.nvars, np.uint8)
        if case == "ladybug_cams":
            a[:9 * 46] = 1                               # 46 of 49 cameras assigned (the PaToH cut of SURVEY 3.2b)
        else:
            a[rng.random(pp.nvars) < 0.6] = 1
    elif case == "synthetic":
        pp = P.make_synthetic_ba(7, 3, 10)
        a = np.zeros(pp.nvars, np.uint8); a[rng.random(pp.nvars) < 0.2] = 1
    elif case == "sinusoid":
        pp = P.make_high_dim_sinusoid()
        a = np.zeros(pp.nvars, np.uint8); a[rng.random(pp.nvars) < 0.3] = 1
    else:
        pp = P.load_bal(ncams=5, npts=30)
        a = np.full(pp.nvars, 1 if case == "all" else 0, np.uint8)
    fp, fv, cp, ci = O.OracleProblem(pp).components(a)
    ref = _scipy_components(pp, a)
    assert len(fp) - 1 == len(ref)
    for c, (vs, fs) in enumerate(ref):                   # index work: exact
        assert list(fv[fp[c]:fp[c + 1]]) == vs
        assert list(ci[cp[c]:cp[c + 1]]) == sorted(fs)
    # every unassigned variable exactly once; factors with an unassigned variable exactly once
    assert sorted(fv) == list(np.where(a == 0)[0])
    assert len(set(ci)) == len(ci)
    if case == "none":
        assert len(fp) == 2 and fp[1] == pp.nvars and cp[1] == pp.nfac
    if case == "all":
        assert len(fp) == 1 and len(fv) == 0 and len(ci) == 0


def test_components_isolated_variable_and_constant_factor():
    # x2 appears in no factor; the last factor has no variables at all
    terms = [(2.0, [(0, 1.0, 0.0, 0), (1, 1.0, 0.0, 0)]), (1.0, [(3, 2.0, 0.0, 0)]), (-7.0, [])]
    q = P._pack_nlp(terms, np.zeros(4), np.full(4, -5.0), np.full(4, 5.0), {})
    fp, fv, cp, ci = O.OracleProblem(q).components(np.zeros(4, np.uint8))
    # by (size, smallest id): {2} (no factors), {3} (factor 1), {0,1} (factor 0)
    assert list(fp) == [0, 1, 2, 4] and list(fv) == [2, 3, 0, 1]
    assert list(cp) == [0, 0, 1, 2] and list(ci) == [1, 0]


# ---- Levenberg-Marquardt restatement (parity unpinned, oracle/lm_oracle.py) ----------------------
def test_lm_oracle_least_squares_problem_and_descent():
    from oracle import lm_oracle as LM
    pp = P.load_bal(ncams=5, npts=30)
    o = O.OracleProblem(pp, emulate_stale_cache=False)
    fv, fc = np.arange(pp.nvars), np.arange(pp.nfac)
    e, J = LM.residuals_and_jacobian(o, fv, fc)
    assert abs(0.5 * e @ e - o.eval()) <= 1e-12 * o.eval()              # sum e_j^2 / 2 is the objective (LMSubspaceOptimizer.cpp:196-200)
    assert np.max(np.abs(J.T @ e - o.gradient())) <= 1e-10 * np.max(np.abs(o.gradient()))   # J^T e is its gradient (:258-275)
    r = LM.lm_optimize(o, maxiters=25)
    acc = [h for h in r.history if h[3]]
    assert r.stop == 3 and r.iters == 25 and len(acc) == 25
    assert all(b[2] < a[2] for a, b in zip(acc, acc[1:])) and r.fret < 0.05 * r.finit
    assert np.all(r.x >= pp.lo) and np.all(r.x <= pp.hi)


def test_slope_association_moves_the_population():
    """Why the device's end values on ladybug 5 / 30 (BASELINE config 3) are a population of their own, found in round 5.
    The reference forms a trial's slope as gradient times direction, sum_v (sum_f partial_fv) xi_v (Df1dim::df,
    minimize_nrc.h:439-447); the device's fused trials add factor by factor, sum_f (sum_k partial_fk xi_k) -- the same number
    to the last place or two.  But Dbrent's secant steps here run between trial points 1e-17 apart, where the difference of two
    slopes cancels ten digits, and the association moves every such step the same way: with the oracle's switch
    ro_set_experiment(2) the FIRST line minimisation ends lower on almost every one-ulp start (by 6e-9: Brent's tolerance, not
    rounding noise, and one-sided), and after 25 iterations the population has moved -- to where the device's is (lower
    quartile 25.15 against 25.11; tests/test_gpu_solver.py::test_end_values_distribution_matches_oracle).
    Nothing else tried moves it: stale cache, derivative formula, sum order of the value, reciprocals, contraction."""
    import json
    from concurrent.futures import ThreadPoolExecutor
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "end_values.json")) as fh:
        fx = json.load(fh)
    pp = P.load_bal(ncams=5, npts=30)
    n = 512

    def start(k):
        rng = np.random.default_rng([fx["seed"], 100000 + k])
        return np.nextafter(pp.x0, np.where(rng.random(pp.x0.shape) < 0.5, -np.inf, np.inf))

    def run(maxit):
        with ThreadPoolExecutor(4) as ex:
            return np.array(list(ex.map(lambda k: O.OracleProblem(pp, emulate_stale_cache=False).cgd(x=start(k), maxiters=maxit).fret, range(n))))
    base1, base25 = run(1), run(25)
    O.lib().ro_set_experiment(2)
    try:
        alt1, alt25 = run(1), run(25)
    finally:
        O.lib().ro_set_experiment(0)
    d1 = (alt1 - base1) / base1
    assert np.mean(d1 < 0) >= 0.85 and -2e-8 < np.median(d1) < -1e-9, (np.mean(d1 < 0), np.median(d1))   # one-sided, at Brent's tolerance
    ks = lambda a, b: np.max(np.abs(np.searchsorted(np.sort(a), np.concatenate([a, b]), side="right") / len(a) -
                                    np.searchsorted(np.sort(b), np.concatenate([a, b]), side="right") / len(b)))
    oe = np.array(fx["ladybug_5_30"]["end_values"])
    crit = 1.358 * np.sqrt((n + len(oe)) / (n * len(oe)))
    print("k = 1: share of starts ending lower %.2f, median %.2e; k = 25: quartiles %s (by factor) against %s; KS against the fixture %.3f / %.3f, critical %.3f" % (
        np.mean(d1 < 0), np.median(d1), np.quantile(alt25, [0.25, 0.5, 0.75]), np.quantile(base25, [0.25, 0.5, 0.75]), ks(alt25, oe), ks(base25, oe), crit))
    assert ks(base25, oe) <= crit                    # the oracle as it is: the fixture's population (other starts)
    assert ks(alt25, oe) > crit                      # with the device's association: another one
    assert np.quantile(alt25, 0.25) > np.quantile(base25, 0.25) + 0.02


def test_nlp_exponential_values_only():
    """useExponential (NonlinearProductFactor.cpp:140, 204): a flagged factor is coeff * exp(-product); the
    reference's computeGradient asserts the flag off (:110), the restatement's derivative is NaN there."""
    s = P.make_high_dim_sinusoid()
    rng = np.random.default_rng(3)
    x = rng.uniform(-3.0, 3.0, s.nvars)
    o = O.OracleProblem(s)
    o.assign(None, x)
    idx = np.arange(s.nfac, dtype=np.int64)
    plain = o.eval_each(idx)
    flags = (rng.random(s.nfac) < 0.4).astype(np.uint8)
    o.set_exponential(flags)
    e = o.eval_each(idx)
    want = np.where(flags != 0, s.coeff * np.exp(-plain / s.coeff), plain)
    assert np.array_equal(e[flags == 0], plain[flags == 0])
    assert np.allclose(e, want, rtol=4e-16 * 8, atol=0)
    assert o.eval() == pytest.approx(float(np.sum(want)), rel=1e-13)
    assert np.any(np.isnan(o.gradient()))
    o.set_exponential(None)
    assert np.array_equal(o.eval_each(idx), plain) and np.all(np.isfinite(o.gradient()))


def test_population_follows_the_order_of_the_slope_sum():
    """The committed oracle samples of full ladybug's end values (tests/golden/end_values.json; make_end_values.py,
    make_end_values_slope.py): four variants of ONE algorithm over the same 320 one-ulp starts.  The two that add a trial's
    slope factor by factor -- in list order, and as a balanced tree -- differ in nothing but the order of that sum and part
    with KS 0.19 (critical 0.107): the reason a device whose slope is a parallel reduction is measured against the family's
    spread, and the plain test is asserted only where the sum is formed in the reference's order (factor_rounding = 1)."""
    import json
    from scipy import stats
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "end_values.json")))["ladybug_full"]
    ref, con = np.array(fx["end_values"]), np.array(fx["end_values_contracted"])
    lst, tree = np.array(fx["end_values_slope_by_factor"]), np.array(fx["end_values_slope_by_factor_tree"])
    assert len(ref) == len(con) == len(lst) == len(tree) == 320
    crit = 1.358 * np.sqrt(2 / 320)
    ks = lambda a, b: stats.ks_2samp(a, b).statistic
    assert ks(lst, tree) > 1.5 * crit and ks(ref, tree) > 1.5 * crit and ks(ref, con) > 1.5 * crit
    assert ks(ref, lst) < crit                       # (the association alone, in list order, is not told apart at this n)
    for v in (con, lst, tree):                       # ... while every quartile of every variant stays within 1 % of the reference's
        assert np.all(np.abs(np.quantile(v, [0.25, 0.5, 0.75]) / np.quantile(ref, [0.25, 0.5, 0.75]) - 1) < 0.01)
    # one run with the tree-order switch reproduces the fixture's entry (the generator's code path)
    pp = P.load_bal()
    sys_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_end_values", os.path.join(sys_path, "make_end_values.py"))
    mev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mev)
    O.lib().ro_set_experiment(6)
    try:
        got = O.OracleProblem(pp, sum_order="pairwise").cgd(x=mev.start(pp.x0, 3), maxiters=25, ftol=3e-8).fret
    finally:
        O.lib().ro_set_experiment(0)
    assert got == tree[3]
