"""rdis_hip_plan_set_option through the library, on ladybug 5 cameras / 30 points (the smoke problem): every value the table of
tests/test_plan_options_cpu.py says is refused raises with that message, an unknown name raises, the poll options read back
through plan.info, and setting and resetting options that leave the partition alone does not change what a solve returns."""
import numpy as np
import pytest

from rdis_amd import capi, problems as P
from test_plan_options_cpu import ROWS, UNKNOWN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan(gctx):
    pp = P.load_bal(ncams=5, npts=30).single_component()
    plan = capi.Plan(capi.Problem(gctx, pp))
    plan.set_start(pp.x0)
    return plan


def test_refused_values_raise_with_the_message(plan):
    refused = [(r, v) for r in ROWS for v in r["refused"]]
    assert len(refused) >= len([r for r in ROWS if not r["flag"]])
    for r, v in refused:
        with pytest.raises(capi.RdisHipError) as e:
            plan.set_option(r["name"], v)
        assert e.value.code == -1 and str(e.value) == str(capi.RdisHipError(-1, r["message"])), (r["name"], v)
    with pytest.raises(capi.RdisHipError) as e:
        plan.set_option(UNKNOWN, 1)
    assert e.value.code == -1 and str(e.value) == str(capi.RdisHipError(-1, "unknown option " + UNKNOWN))


def test_poll_options_read_back(plan):
    for name, value in (("coop_poll_delay", 7), ("coop_poll_inflight", 1), ("coop_poll_stagger", 5)):
        plan.set_option(name, value)
        assert plan.info(name) == value
    for r in ROWS:
        if r["name"].startswith("coop_poll_"):
            plan.set_option(r["name"], r["default"])
            assert plan.info(r["name"]) == r["default"]


def test_clean_options_set_and_reset_leave_the_solve_alone(plan):
    def solve():
        plan.solve(25, 3e-8)
        r = plan.fetch()
        return (r.x.tobytes(), r.fret.tobytes(), r.delta.tobytes(), r.iters.tobytes(), r.status.tobytes(), r.nfeval.tobytes(), r.ngeval.tobytes())
    first = solve()
    assert np.frombuffer(first[2], dtype=np.float64)[0] < 0
    defaults = {r["name"]: r["default"] for r in ROWS}
    for name, other in (("starts_workspace_bytes", 0), ("population_plain", 1), ("lds_matrix", 1)):
        plan.set_option(name, other)
        plan.set_option(name, defaults[name])
    assert solve() == first
