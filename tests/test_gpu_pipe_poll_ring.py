"""The pipelined solver's collector with several polls of a slot in flight (solver_pipe.hpp: PipeSync::sweep_ring, plan options
coop_poll_inflight / coop_poll_stagger).  The ring samples the slot being swept more often; the slots, the re-arming rule and the
order of every sum are those of the one-poll loop, so every bit of a solve is the same -- whatever the first-poll delay, the issue
interval, with guesses or without, for one group or several in a launch, and when a line search ends while polls are in flight.

The ring is entered only by a value+slope sweep that had to wait for its own lanes.  On every shape here that happens in every
variant: a fresh trial's sweep is ordered before the lanes have evaluated it (some 40 of the 130 to 250 sweeps of a solve; all of
them with coop_speculate = 0, where nothing is evaluated ahead).  profiles/pipe_poll_ring_test_shapes_coverage.txt has the counts
of a timing build per shape and variant (tools/gpu_probe_ring_coverage.py: 22 to 50 ring polls looked at in workgroup 0 with
guesses, 131 to 319 without, none with coop_poll_inflight = 0).  A release build carries no counters, so the test cannot assert it."""
import copy
import json
import os

import numpy as np
import pytest

from rdis_amd import capi, problems as P

pytestmark = pytest.mark.gpu

STAGGER_MIN, STAGGER_MAX = 0, 64      # the range rdis_hip_plan_set_option accepts for coop_poll_stagger
EXIT_SYNC_TIMEOUT = 7

VARIANTS = (
    ("plain", {"coop_pipeline": 0}),
    ("one poll", {"coop_pipeline": 1, "coop_poll_inflight": 0}),
    ("ring", {"coop_pipeline": 1, "coop_poll_inflight": 1}),
    ("ring, no delay", {"coop_pipeline": 1, "coop_poll_inflight": 1, "coop_poll_delay": 0}),
    ("ring, long delay", {"coop_pipeline": 1, "coop_poll_inflight": 1, "coop_poll_delay": 64}),
    ("ring, no guesses", {"coop_pipeline": 1, "coop_poll_inflight": 1, "coop_speculate": 0}),
    ("ring, smallest stagger", {"coop_pipeline": 1, "coop_poll_inflight": 1, "coop_poll_stagger": STAGGER_MIN}),
    ("ring, largest stagger", {"coop_pipeline": 1, "coop_poll_inflight": 1, "coop_poll_stagger": STAGGER_MAX}),
)


def _whole(pp):
    return (np.array([0, pp.nvars]), np.arange(pp.nvars, dtype=np.int64), np.array([0, pp.nfac]), np.arange(pp.nfac, dtype=np.int64))


def _tight_bounds():
    # every seventh variable may move 1e-4 of its size up, every eleventh down: the bounds bite
    tight = copy.deepcopy(P.load_bal(ncams=49, npts=500))
    idx = np.arange(tight.nvars)
    tight.hi = np.where(idx % 7 == 0, tight.x0 + 1e-4 * np.abs(tight.x0) + 1e-9, tight.hi)
    tight.lo = np.where(idx % 11 == 0, tight.x0 - 1e-4 * np.abs(tight.x0) - 1e-9, tight.lo)
    return tight


def _shape(name):
    if name == "22 workgroups":            # 44 entries: a lane's first load is real, the other seven clamp to entry 0
        pp = P.make_synthetic_ba(1, 3, 900, obs_per_pt=3)
    elif name == "35 workgroups":          # 4400 factors, 70 entries: a few lanes own a second entry
        pp = P.make_synthetic_ba(1, 4, 1100, obs_per_pt=4)
    elif name == "one factor beyond a workgroup":
        pp = P.make_synthetic_ba(1, 2, 1153, obs_per_pt=2)
    elif name == "five groups":            # cgd_pipe_kernel: five groups side by side in one launch
        pp = P.make_synthetic_ba(5, 3, 900, obs_per_pt=3)
        return pp, (pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id)
    else:
        pp = _tight_bounds()
    return pp, _whole(pp)


def _solve(gctx, g, pp, comps, opts, iters, ftol, trace):
    g.set_x(pp.x0)
    plan = capi.Plan(g, *comps)
    for k, v in {"coop_min_factors": 1000, **opts}.items():
        plan.set_option(k, v)
    if trace:
        plan.set_option("trace_records", 4096)
    plan.set_start(None)
    plan.solve(iters, ftol)
    r = plan.fetch()
    ncomp = len(comps[0]) - 1
    tr = [plan.get_trace(c, 4096) for c in range(ncomp)] if trace else []
    out = (r, g.get_x(), tr, plan.last_kernel_ms()[1], plan.info("pipelined"))
    plan.close()
    return out


def _same(a, b, what):
    (ra, xa, ta, _, _), (rb, xb, tb, _, _) = a, b
    assert np.array_equal(ra.fret, rb.fret) and np.array_equal(ra.x, rb.x) and np.array_equal(xa, xb), what
    assert np.array_equal(ra.iters, rb.iters) and np.array_equal(ra.status, rb.status), what
    assert np.array_equal(ra.nfeval, rb.nfeval) and np.array_equal(ra.ngeval, rb.ngeval), what
    assert len(ta) == len(tb), what
    for (tra, ca), (trb, cb) in zip(ta, tb):
        assert ca == cb and np.array_equal(tra[:min(ca, 4096)], trb[:min(cb, 4096)]), what


@pytest.mark.parametrize("shape", ["22 workgroups", "35 workgroups", "one factor beyond a workgroup", "five groups", "active bounds"])
def test_ring_gives_the_bits_of_the_one_poll_loop_and_of_the_plain_solver(gctx, shape):
    pp, comps = _shape(shape)
    g = capi.Problem(gctx, pp)
    out = {label: _solve(gctx, g, pp, comps, opts, 8, 3e-8, True) for label, opts in VARIANTS}
    ref = out["plain"]
    assert np.all(ref[0].delta <= 0) and np.all(ref[0].nfeval > 20), shape
    for label, res in out.items():
        assert np.all((res[0].status & 0xFF) != EXIT_SYNC_TIMEOUT), (shape, label)     # no exchange gave up
        assert res[3] == 1, (shape, label)                                            # one launch
        assert res[4] == (0 if label == "plain" else 1), (shape, label)
        _same(ref, res, (shape, label))


def test_ring_hands_over_at_a_lines_end_as_the_plain_solver_does(gctx):
    """To EXIT_FTOL: at the end of a line search the collector is still following the chain of guesses, and the sweep it abandons
    returns with polls in flight -- they are drained before the ring is used again."""
    pp, comps = _shape("22 workgroups")
    g = capi.Problem(gctx, pp)
    plain = _solve(gctx, g, pp, comps, {"coop_pipeline": 0}, 600, 1e-4, False)
    assert (plain[0].status[0] & 0xFF) == 0          # EXIT_FTOL: the exit this case is about
    for label, opts in VARIANTS[2:]:
        res = _solve(gctx, g, pp, comps, opts, 600, 1e-4, False)
        assert res[3] == 1 and res[4] == 1, label
        _same(plain, res, label)


def test_ring_on_full_ladybug_ends_at_the_committed_end_values(gctx):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parity_end_values.json")) as fh:
        w = json.load(fh)["ladybug_full_default_path"]
    pp = P.load_bal().single_component()
    g = capi.Problem(gctx, pp)
    plan = capi.Plan(g)
    plan.set_option("coop_poll_inflight", 1)
    plan.set_start(pp.x0)
    plan.solve(25, 3e-8)
    r = plan.fetch()
    assert plan.info("pipelined") == 1 and plan.info("coop_poll_inflight") == 1 and plan.last_kernel_ms()[1] == 1
    assert r.fret[0] == w["fret"] and int(r.nfeval[0]) == w["nfeval"] and int(r.ngeval[0]) == w["ngeval"]
    assert [float(v) for v in r.x[:3]] == w["x_0_2"] and float(r.x[-1]) == w["x_last"]
    plan.close()
