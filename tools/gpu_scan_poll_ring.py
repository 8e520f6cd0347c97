"""exploratory: the collector's poll ring (solver_pipe.hpp: sweep_ring) on full ladybug -- kernel time of one solve of 25 iterations
under coop_poll_inflight x coop_poll_stagger x coop_poll_delay, for the library RDIS_PROBE_LIB names (one per PIPE_POLLS:
tools/build_pipe_variant.sh pollsN -DRDIS_PIPE_POLLS=N).  Best and median of --reps solves per setting, whole scan twice."""
import sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdis_amd import problems as P, capi
if os.environ.get("RDIS_PROBE_LIB"):
    capi.LIB_PATH = os.path.abspath(os.environ["RDIS_PROBE_LIB"])
label = sys.argv[1] if len(sys.argv) > 1 else "default build"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
ctx = capi.Context(0)
pp = P.load_bal().single_component()
g = capi.Problem(ctx, pp)
plan = capi.Plan(g)
settings = [(0, 4, d) for d in (0, 2, 4, 8, 16)] + [(1, s, d) for s in (2, 4, 8, 16) for d in (0, 2, 4, 8, 16)]
for rnd in range(2):
    for inflight, stagger, delay in settings:
        for k, v in (("coop_poll_inflight", inflight), ("coop_poll_stagger", stagger), ("coop_poll_delay", delay)):
            plan.set_option(k, v)
        plan.set_start(pp.x0)
        ms = []
        for rep in range(reps):
            plan.solve(25, 3e-8); r = plan.fetch()
            ms.append(plan.last_kernel_ms()[0])
        print("%s round %d inflight %d stagger %2d delay %2d: kernel best %.4f median %.4f ms | fret %.6f nfeval %d status %d" % (
            label, rnd, inflight, stagger if inflight else 0, delay, min(ms), float(np.median(ms)), r.fret[0], r.nfeval[0], r.status[0]), flush=True)
