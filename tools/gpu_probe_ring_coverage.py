"""exploratory: do the shapes of tests/test_gpu_pipe_poll_ring.py reach PipeSync::sweep_ring?  With a -DRDIS_COOP_TIMING build
(RDIS_PROBE_LIB; tools/build_pipe_variant.sh timing -DRDIS_COOP_TIMING) prints, per shape and variant of the test, the
collector's completed sweeps, those that waited for their own lanes, and the ring polls it looked at (counter 43) in workgroup 0
of the launch's first group."""
import sys, os
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from rdis_amd import capi
if os.environ.get("RDIS_PROBE_LIB"):
    capi.LIB_PATH = os.path.abspath(os.environ["RDIS_PROBE_LIB"])
import test_gpu_pipe_poll_ring as T
ctx = capi.Context(0)
for shape in ("22 workgroups", "35 workgroups", "one factor beyond a workgroup", "five groups", "active bounds"):
    pp, comps = T._shape(shape)
    g = capi.Problem(ctx, pp)
    for label, opts in T.VARIANTS[1:]:
        g.set_x(pp.x0)
        plan = capi.Plan(g, *comps)
        for k, v in {"coop_min_factors": 1000, **opts}.items():
            plan.set_option(k, v)
        plan.set_start(None)
        plan.solve(8, 3e-8); r = plan.fetch()
        tm = plan.debug_counters()
        print("%-30s %-24s sweeps %4d, waited for own lanes %4d, ring polls looked at %4d, status %s" % (
            shape, label, tm[5], tm[34], tm[43], sorted(set(int(s) & 0xFF for s in r.status))), flush=True)
        plan.close()
