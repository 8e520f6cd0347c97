#!/usr/bin/env python3
"""Headline benchmark: subspace-solver iterations per second on ladybug bundle
adjustment (BASELINE.json metric), one process per GPU.

A step = one pass of the hot path over one batch: CGDSubspaceOptimizer::optimize
(SSmaxit 25, ftol 3e-8) over the workload's components, from the start state that
is already resident in HBM, including the D2H of the results.  An iteration = one
Frprmn outer iteration (one line minimisation), summed over components.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the headline line.  --full adds
everything else the line has carried (CPU baselines, the comparisons with the committed CPU
fixtures, the latency floor, the objective band, the strong-scaling, all-components, configs,
large-component and normal-equations blocks).  --dump-outputs DIR writes what the last timed
step returned (solution, per-component results, objective) as DIR/<name>.npy in float64.

Workloads (--workload):
  ladybug-full   BASELINE config 4 (default, the metric's configuration): all 23769
                 variables and 31843 factors of ladybug-49-7776 as one component.
                 For N > 1 every rank solves one such component (N independent
                 components of a block-diagonal problem; weak scaling) and the
                 top-level objective is summed with an RCCL all-reduce.  With --full the
                 line also carries a "strong_scaling" block for every N: north_star's fixed
                 1000-component synthetic decomposition shared out over the N ranks
                 (STRONG below), and at N = 1 "cpu_baseline" and "objective_band".
  synthetic-S    BASELINE config 5: 1000 independent 3-camera x 40-point components
                 per rank (one workgroup each, one launch).
  (--scaling strong: the synthetic decompositions keep their total size and are sharded over the ranks)
  synthetic-L    the same generator at ladybug's size (the throughput point):
                 --components (default 256) independent 49-camera x 7776-point components of
                 31104 observations per rank -- 8.0e6 factors; one workgroup each, one launch.
  ladybug-components  the component mix RDIS reaches on ladybug once a separator is assigned
                 (SURVEY.md 3.2b): 7776 single-point components (3 variables, 2-29 factors,
                 cameras fixed), one launch.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md)


def measured_traffic(workload: str):
    """HBM bytes per solver launch from the PMC counters (rocprofv3 --pmc FETCH_SIZE and,
    in a separate pass, --pmc WRITE_SIZE; KiB units; FETCH doubled per MI355X_MICROARCH.md
    section HBM), as recorded in profiles/traffic.json by tools/collect_traffic.py for the
    same bench command.  None when no such record exists for this workload."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as fh:
            rec = json.load(fh).get(workload)
        return None if rec is None else float(rec["hbm_bytes_per_launch"])
    except (OSError, ValueError, KeyError):
        return None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="ladybug-full", choices=["ladybug-full", "synthetic-S", "synthetic-L", "ladybug-components", "large-component"])
    ap.add_argument("--large-shape", default="64x2000000x4", help="large-component: cameras x points x observations per point of the one component")
    ap.add_argument("--no-configs", action="store_true", help="skip the configs block (BASELINE configs 1, 2, 3, 5-S)")
    ap.add_argument("--no-large-component", action="store_true", help="skip the large_component block (one component larger than ladybug)")
    ap.add_argument("--components", type=int, default=256, help="synthetic-L: components per rank (weak) / in total (strong)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="strong: the synthetic workloads keep their total size (synthetic-S: 1000 components, synthetic-L: "
                         "--components) and every rank takes a contiguous share of the components")
    ap.add_argument("--maxiters", type=int, default=25)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-strong-scaling", action="store_true", help="skip the strong_scaling block (the fixed 1000-component decomposition)")
    ap.add_argument("--strong-size", default="L", choices=sorted(STRONG_SIZES), help="component size of the strong_scaling block")
    ap.add_argument("--no-objective-band", action="store_true")
    ap.add_argument("--no-all-components", action="store_true", help="skip the all_components block (the recursion's whole call mix)")
    ap.add_argument("--opt", action="append", default=[], help="plan option name=value")
    ap.add_argument("--collective", default="c-abi", choices=["c-abi", "torch"],
                    help="how the ranks' objective all-reduce runs: the library's own RCCL entry points (default; no torch in the process) or torch.distributed")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: CPU baselines, comparisons with the CPU fixtures, latency floor, objective band and the other "
                         "blocks (strong scaling, all components, configs, large component, normal equations); the --no-* options trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float64, at most 64 MB in all)")
    return ap.parse_args()


def build_problem(workload: str, rank: int, components: int = 256, world: int = 1, strong: bool = False, large_shape: str = "64x2000000x4"):
    from rdis_amd import problems as P
    if workload == "large-component":
        c, pn, k = (int(v) for v in large_shape.split("x"))
        return P.make_synthetic_ba(1, c, pn, obs_per_pt=k, first_comp=rank).single_component()
    if strong:   # a fixed decomposition, sharded: components are generated from their ids, so a rank builds only its own
        if workload not in ("synthetic-S", "synthetic-L"):
            raise SystemExit("--scaling strong needs a decomposable workload (synthetic-S / synthetic-L)")
        total = 1000 if workload == "synthetic-S" else components
        lo, hi = rank * total // world, (rank + 1) * total // world
        if hi <= lo:
            raise SystemExit(f"--scaling strong: {total} components do not cover {world} ranks")
        if workload == "synthetic-S":
            return P.make_synthetic_ba(hi - lo, 3, 40, first_comp=lo)
        return P.make_synthetic_ba(hi - lo, 49, 7776, obs_per_pt=4, first_comp=lo)
    if workload == "synthetic-L":
        return P.make_synthetic_ba(components, 49, 7776, obs_per_pt=4, first_comp=components * rank)
    if workload == "ladybug-full":
        return P.load_bal().single_component()
    if workload == "ladybug-components":
        pp = P.load_bal()
        _, pts = P.ba_alternation_plans(pp)
        pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id = pts
        return pp
    return P.make_synthetic_ba(1000, 3, 40, first_comp=1000 * rank)


# The strong-scaling workload of north_star ("1000-component synthetic decomposition"): a FIXED
# decomposition of 1000 independent bundle-adjustment components, sharded over the ranks.  Size of
# a component ("L", the default): SURVEY 8d's config-5-L -- 49 cameras x 7776 points x 4 observations
# per point = 31104 factors, 23769 variables, ladybug's own size; 3.1e7 factors / 2.4e7 variables in
# all, the size at which the path streams from HBM.  One GPU works through its 1000 components a
# workgroup each (four rounds of 256 compute units); at eight GPUs a rank has 125, fewer than compute
# units, and four workgroups share a component (solver_ptm.hpp: cgd_ptmg_kernel) -- that is what lets the
# time keep falling with the number of ranks.  "small": 8 cameras x 512 points x 4 = 2048 factors (round 2's
# block): a component fits one compute unit's LDS and an evaluation is 2 us of arithmetic, too little
# to share between workgroups -- 125 components use 125 compute units, and a launch lasts as long as
# its slowest component's chain of ~460 evaluations.
STRONG_SIZES = {"L": {"components": 1000, "ncams": 49, "npts": 7776, "obs_per_pt": 4},
                "small": {"components": 1000, "ncams": 8, "npts": 512, "obs_per_pt": 4}}
STRONG = dict(STRONG_SIZES["L"])


def strong_scaling_shard(rank: int, world: int, components: int = None):
    """(problem, CSR of this rank's components, their ids, per-rank factor loads): the whole fixed
    decomposition is generated on every rank (components come from their ids: identical
    everywhere) and shared out by dist.rank_decomposition -- longest-processing-time by factor
    count, the same partition on every rank, no communication."""
    from rdis_amd import problems as P
    from rdis_amd.dist import rank_decomposition
    pp = P.make_synthetic_ba(components or STRONG["components"], STRONG["ncams"], STRONG["npts"], obs_per_pt=STRONG["obs_per_pt"])
    free_ptr, free_vid, fac_ptr, fac_id, mine = rank_decomposition(pp, rank, world)
    w = np.diff(pp.comp_fac_ptr)
    loads = np.array([int(w[part].sum()) for part in P.shard_components(pp.ncomp, w, world)])
    return pp, (free_ptr, free_vid, fac_ptr, fac_id), mine, loads


import contextlib
import ctypes


@contextlib.contextmanager
def _stdout_to_stderr():
    """RCCL announces its version on the process's STDOUT when it is first used: the contract's one JSON line must stay the only
    thing there, so file descriptor 1 points at stderr meanwhile"""
    sys.stdout.flush()
    keep = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)   # (the library writes through C's buffered stdout: out with it while 1 is still stderr)
        os.dup2(keep, 1)
        os.close(keep)


class RcclCollective:
    """The ranks' one exchange through the library's own C ABI (include/rdis_hip.h: rdis_hip_comm_*, rdis_hip_allreduce_objective
    -- ncclAllReduce over RCCL / xGMI on the solver's stream): no torch in the process.  The 128-byte communicator id travels from
    rank 0 to the others through a file in /dev/shm named after the launcher's pid and port (one node, as the contract says)."""
    name = "rccl through the C ABI (rdis_hip_allreduce_objective)"

    def __init__(self, capi, ctx, rank, world):
        if os.environ.get("RDIS_BENCH_NO_RCCL") == "1":   # (tests: the fallback below)
            raise RuntimeError("RDIS_BENCH_NO_RCCL=1")
        self.ctx = ctx
        key = "rdis_bench_id_%s_%d" % (os.environ.get("MASTER_PORT", "0"), os.getppid() if world > 1 else os.getpid())
        path = os.path.join("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp", key)
        if rank == 0:
            with _stdout_to_stderr():
                uid = capi.Comm.unique_id()
            with open(path + ".tmp", "wb") as fh:
                fh.write(uid)
            os.replace(path + ".tmp", path)
        else:
            t0 = time.time()
            while True:
                try:
                    if time.time() - os.path.getmtime(path) < 600:
                        with open(path, "rb") as fh:
                            uid = fh.read()
                        if len(uid) == 128:
                            break
                except OSError:
                    pass
                if time.time() - t0 > 300:
                    raise RuntimeError("no communicator id from rank 0 at " + path)
                time.sleep(0.01)
        with _stdout_to_stderr():
            self.comm = capi.Comm(ctx, world, rank, uid)
            self.comm.barrier()
        if rank == 0:
            try:
                os.remove(path)
            except OSError:
                pass

    def reduce_objective(self, plan):
        plan.allreduce_objective(self.comm, fetch=False)   # in place on the device, behind the solve on its stream

    def barrier_sync(self):
        self.comm.barrier()
        self.ctx.synchronize()

    def allreduce(self, values, op="sum"):
        return [float(v) for v in self.comm.allreduce(values, op)]

    def close(self):
        self.comm.barrier()
        self.comm.close()


class FileCollective:
    """Last resort when RCCL cannot be brought up through the C ABI (the library missing, the communicator refused): the ranks' few
    scalars through files in /dev/shm -- one node, as the contract says.  No device collective: the objective is read back and summed
    on the host (one 8-byte copy a step more than the RCCL paths).  The bench line names the collective it ran with."""
    name = "host files in /dev/shm (fallback: RCCL could not be initialised through the C ABI)"

    def __init__(self, ctx, rank, world, why=""):
        self.ctx, self.rank, self.world, self.seq, self.why = ctx, rank, world, 0, why
        base = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
        self.key = os.path.join(base, "rdis_bench_fc_%s_%d" % (os.environ.get("MASTER_PORT", "0"), os.getppid() if world > 1 else os.getpid()))
        self._obj = {}

    def _path(self, seq, rank):
        return "%s_%d_%d" % (self.key, seq, rank)

    def allreduce(self, values, op="sum"):
        self.seq += 1
        mine = np.asarray(list(values), dtype=np.float64)
        tmp = self._path(self.seq, self.rank) + ".tmp"
        with open(tmp, "wb") as fh:
            fh.write(mine.tobytes())
        os.replace(tmp, self._path(self.seq, self.rank))
        acc = None
        t0 = time.time()
        for r in range(self.world):
            while True:
                try:
                    with open(self._path(self.seq, r), "rb") as fh:
                        b = fh.read()
                    if len(b) == mine.nbytes:
                        break
                except OSError:
                    pass
                if time.time() - t0 > 600:
                    raise RuntimeError("rank %d never wrote %s" % (r, self._path(self.seq, r)))
                time.sleep(0.0005)
            v = np.frombuffer(b, dtype=np.float64)
            acc = v.copy() if acc is None else (np.maximum(acc, v) if op == "max" else acc + v)   # rank order: the same bits everywhere
        old = self._path(self.seq - 2, self.rank)   # (everybody has read what is two exchanges old)
        if self.seq > 2 and os.path.exists(old):
            os.remove(old)
        return [float(x) for x in acc]

    def reduce_objective(self, plan):
        self._obj[id(plan)] = self.allreduce([plan.objective()])[0]

    def objective(self, plan):
        return self._obj.get(id(plan), plan.objective())

    def barrier_sync(self):
        self.ctx.synchronize()
        self.allreduce([0.0])

    def close(self):
        # a last exchange, a marker "I have read it", and rank 0 -- the last to leave -- removes what is left once every marker is there
        import glob
        self.allreduce([0.0])
        open("%s_done_%d" % (self.key, self.rank), "w").close()
        if self.rank == 0:
            t0 = time.time()
            while len(glob.glob(self.key + "_done_*")) < self.world and time.time() - t0 < 60:
                time.sleep(0.001)
            for f in glob.glob(self.key + "_*"):
                try:
                    os.remove(f)
                except OSError:
                    pass


class TorchCollective:
    """the same through torch.distributed (backend "nccl" = RCCL): the fallback, --collective torch"""
    name = "rccl through torch.distributed"

    def __init__(self, ctx, torch, dist, local_rank):
        self.ctx, self.torch, self.dist, self.dev = ctx, torch, dist, f"cuda:{local_rank}"
        self.views = {}

    def reduce_objective(self, plan):
        t = self.views.get(id(plan))
        if t is None:
            class _Dev:
                def __init__(self, ptr):
                    self.__cuda_array_interface__ = {"shape": (1,), "typestr": "<f8", "data": (ptr, False), "version": 2}
            t = self.views[id(plan)] = self.torch.as_tensor(_Dev(plan.objective_device_ptr()), device=self.dev)
        self.dist.all_reduce(t)

    def barrier_sync(self):
        self.dist.barrier()
        self.torch.cuda.synchronize()
        self.ctx.synchronize()

    def allreduce(self, values, op="sum"):
        t = self.torch.tensor(list(values), dtype=self.torch.float64, device=self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX if op == "max" else self.dist.ReduceOp.SUM)
        return [float(v) for v in t.tolist()]

    def close(self):
        self.dist.barrier()
        self.dist.destroy_process_group()


def run_strong_scaling(ctx, rank, world, coll, maxiters, steps=3, warmup=1, cpu=False):
    """the strong-scaling block of the bench line: the fixed 1000-component decomposition solved by
    all ranks together; barrier + synchronize around exactly `steps` solves, MAX over ranks"""
    from rdis_amd import capi, problems as P
    pp, csr, mine, loads = strong_scaling_shard(rank, world)
    prob = capi.Problem(ctx, pp)
    plan = capi.Plan(prob, *csr)
    plan.set_start(pp.x0[csr[1]])

    keep = [None]

    def step():
        plan.solve(maxiters, 3e-8)
        if coll is not None:
            coll.reduce_objective(plan)
        keep[0] = plan.fetch(out=keep[0])   # (the caller's result arrays are its own: written again every step, like the reference's xval)
        return keep[0]

    def sync():
        if coll is not None:
            coll.barrier_sync()
        ctx.synchronize()
    for _ in range(warmup):
        r = step()
    sync()
    kms, iters, abytes = 0.0, 0, 0.0
    Fc, Nc = np.diff(csr[2]).astype(np.float64), np.diff(csr[0]).astype(np.float64)
    t0 = time.perf_counter()
    for _ in range(steps):
        r = step()
        kms += plan.last_kernel_ms()[0]
        iters += int(np.sum(r.iters.astype(np.int64) + 1))
        # value-only evaluations 24F + 8N + 8 bytes, value + slope / gradient 24F + 16N + 8
        abytes += float(np.sum((r.nfeval - r.ngeval).clip(0) * (24 * Fc + 8 * Nc + 8) + r.ngeval * (24 * Fc + 16 * Nc + 8)))
    sync()
    dt = time.perf_counter() - t0
    objective = coll.objective(plan) if hasattr(coll, "objective") else plan.objective()
    kmax = kms / steps
    if coll is not None:
        dt, kmax = coll.allreduce([dt, kmax], "max")
        iters = coll.allreduce([float(iters)])[0]
    ncu = 256
    max_comps = max(len(part) for part in P.shard_components(pp.ncomp, np.diff(pp.comp_fac_ptr), world))
    out = {"workload": (f"fixed decomposition of {pp.ncomp} independent synthetic BA components x ({STRONG['ncams']} cameras, "
                        f"{STRONG['npts']} points, {pp.nfac // pp.ncomp} observations), SSmaxit {maxiters}, shared out over {world} rank(s) "
                        "by factor count (longest processing time first), no data-path collective, objective all-reduced"),
           "scaling": "strong", "n_gpus": world, "components_total": int(pp.ncomp), "factors_total": int(pp.nfac),
           "variables_total": int(pp.nvars), "components_rank0": int(len(mine)),
           "value": iters / dt, "unit": "iters/s", "steps": steps, "ms_per_step": dt / steps * 1e3,
           "kernel_ms_max_over_ranks": kmax, "objective": objective,
           "load_imbalance": float(loads.max() / loads.mean()), "factors_per_rank": [int(v) for v in loads],
           # rounds of one workgroup per compute unit a rank's launch needs; below one round workgroups share a component
           "workgroup_rounds": int(-(-int(max_comps) // ncu)), "workgroups_per_component": int(plan.info("point_major_group")),
           "exit_status_histogram": {capi.EXIT_NAMES[int(k)]: int(v) for k, v in zip(*np.unique(r.status & 0xFF, return_counts=True))},
           # rank 0's launch against the HBM roofline: this is the workload whose state does not fit the caches
           # (1.4 MB streamed per component and trial point), HIP events around the solver kernel
           "roofline": {"bound": "hbm", "achieved": abytes / (kms * 1e-3) / 1e9 if kms > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": (abytes / (kms * 1e-3) / 1e9 if kms > 0 else 0.0) / HBM_PEAK_GBS,
                        "traffic": measured_traffic("synthetic-L-1000") if STRONG["npts"] == 7776 and world == 1 else None,
                        "traffic_is": "counter passes of this launch's own shape -- 1000 such components, bench.py --workload synthetic-L --components 1000 in the "
                                      "profile round (profiles/traffic.json); not collected in this run",
                        "kernel": "cgd_ptm_kernel / cgd_ptmg_kernel (solver_ptm.hpp)", "kernel_ms_avg": kms / max(steps, 1),
                        "algorithmic_bytes_per_launch": abytes / max(steps, 1), "rank": 0}}
    plan.close()
    if world == 1 and cpu:
        # the CPU leg of this block: the oracle (a port, one core) on the first three of the 1000 components
        from oracle import oracle as O
        o = O.OracleProblem(pp)
        t0c = time.perf_counter()
        cits, cfe = 0, 0
        for c in range(3):
            fv, fc = pp.component(c)
            ro = o.cgd(free_vid=fv, fac=fc, x=pp.x0[fv], maxiters=maxiters)
            cits += ro.iters + 1; cfe += ro.nfeval
        dtc = time.perf_counter() - t0c
        out["cpu_baseline"] = {"value": cits / dtc, "unit": "iters/s", "cores": 1, "kind": "port", "f_evals_per_s": cfe / dtc,
                               "sample": "the first 3 of the %d components, dense gradient accumulation" % pp.ncomp}
        # ... and what the launch above returned for those components against CPU runs of the oracle with the point-major solver's own
        # arithmetic, layout and sums (oracle/rdis_oracle.h: RO_SUM_TOPOLOGY_PTM): the same bits or not
        if out["workgroups_per_component"] == 1 and STRONG["npts"] >= 2048:
            where = {int(c): i for i, c in enumerate(mine)}
            same = []
            for c in range(3):
                fv, fc = pp.component(c)
                w = O.OracleProblem.device_ptm_default(pp, fac=fc).cgd(free_vid=fv, fac=fc, x=pp.x0[fv], maxiters=maxiters)
                i = where[c]
                same.append(bool(float(r.fret[i]) == w.fret and int(r.nfeval[i]) == w.nfeval and int(r.ngeval[i]) == w.ngeval))
            out["components_bit_identical_to_cpu"] = {"components": [0, 1, 2], "identical": same,
                                                      "what": "fret, f and gradient evaluation counts of the timed launch == the oracle's run with the "
                                                              "device's factor arithmetic (factors.hpp for the host) and the point-major solver's sums"}
    if world == 1:
        out["emulated_ranks"] = emulated_ranks(capi, prob, pp, maxiters, out["ms_per_step"], cpu=cpu, kernel_ms_world1=kmax)
    prob.close()
    return out


def emulated_ranks(capi, prob, pp, maxiters, ms_world1, steps=3, cpu=False, kernel_ms_world1=None):
    """rank 0's share of the fixed decomposition for world = 2, 4, 8, run on THIS one GPU: what one GPU of such a job
    does per step -- solve + fetch of its own results (the start is resident, as in the block above; the 8-byte
    all-reduce is not emulated) -- wall clock around exactly `steps` steps after one warm-up, and the ratio to
    the one-rank step above.  The shard is dist.rank_decomposition's (longest processing time first, identical on
    every rank); with 125 components a GPU has fewer components than compute units and K workgroups share each."""
    from rdis_amd.dist import rank_decomposition
    rows = [{"world": 1, "components_rank0": int(pp.ncomp), "ms_per_step": ms_world1, "kernel_ms": kernel_ms_world1, "ratio_to_world1": 1.0}]
    # (round 6: every emulated step carries the objective's all-reduce through the C ABI over a communicator of one rank -- RCCL's
    # launch and its place on the solver's stream are in the step; what a real job adds is the wire)
    comm = None
    try:
        with _stdout_to_stderr():
            comm = capi.Comm(prob.ctx, 1, 0, capi.Comm.unique_id())
    except Exception:
        comm = None
    for world in (2, 4, 8):
        fp, fv, cp, ci, mine = rank_decomposition(pp, 0, world)
        plan = capi.Plan(prob, fp, fv, cp, ci)
        plan.set_start(pp.x0[fv])
        plan.solve(maxiters, 3e-8); r = plan.fetch()
        if comm is not None:
            plan.allreduce_objective(comm, fetch=False)
        t0 = time.perf_counter()
        kms = 0.0
        for _ in range(steps):
            plan.solve(maxiters, 3e-8)
            if comm is not None:
                plan.allreduce_objective(comm, fetch=False)
            r = plan.fetch(out=r)
            kms += plan.last_kernel_ms()[0]
        ms = (time.perf_counter() - t0) / steps * 1e3
        rows.append({"world": world, "components_rank0": int(len(mine)), "ms_per_step": ms, "kernel_ms": kms / steps,
                     "workgroups_per_component": int(plan.info("point_major_group")), "ratio_to_world1": ms_world1 / ms,
                     "objective_rank0": float(r.fret.sum()), "all_reduce_in_the_step": comm is not None})
        if kernel_ms_world1:   # (a step = the kernel + the copy of the share's solution to the host: the ratio of the kernels alone beside it)
            rows[-1]["kernel_ratio_to_world1"] = kernel_ms_world1 / (kms / steps)
        if cpu and STRONG["npts"] >= 2048 and not plan.info("point_major_wide") and plan.info("components_point_major") == len(mine):
            # the share's first component against a CPU run of the oracle with this launch's group (RO_SUM_TOPOLOGY_PTM)
            from oracle import oracle as O
            K, nt = int(plan.info("point_major_group")), int(plan.info("point_major_threads"))
            v, f = fv[fp[0]:fp[1]], ci[cp[0]:cp[1]]
            w = O.OracleProblem.device_ptm_default(pp, fac=f, threads=nt, group=K).cgd(free_vid=v, fac=f, x=pp.x0[v], maxiters=maxiters)
            rows[-1]["first_component_bit_identical_to_cpu"] = bool(float(r.fret[0]) == w.fret and int(r.nfeval[0]) == w.nfeval and int(r.ngeval[0]) == w.ngeval)
            rows[-1]["lanes_per_workgroup"] = nt
        plan.close()
    if comm is not None:
        comm.close()
    return rows


def lm_block(ctx, maxiters, steps=5):
    """north_star's per-component normal-equation solve: Levenberg-Marquardt on full ladybug with pixel residuals (lm_solver.hip --
    block J^T J, Schur complement on the cameras, the dense 441 x 441 system factored on the device; fp64 MFMA in the Schur product
    and the trailing updates, where the work is a true contraction).  Wall clock of `steps` solves of `maxiters` iterations; what
    the matrix cores do in them is in profiles/ (kernel stats and SQ_INSTS_MFMA counter passes of tools/gpu_lm_profile.py)."""
    from rdis_amd import capi, problems as P
    pp = P.load_bal()
    g = capi.Problem(ctx, pp)
    g.set_x(pp.x0); r = g.lm_optimize(maxiters=maxiters, model=2)
    t0 = time.perf_counter()
    for _ in range(steps):
        g.set_x(pp.x0)
        r = g.lm_optimize(maxiters=maxiters, model=2)
    dt = (time.perf_counter() - t0) / steps
    g.close()
    return {"workload": "Levenberg-Marquardt with pixel residuals, ladybug-49-7776 (23769 variables, 63686 residuals), %d iterations from x0" % maxiters,
            "reference": "src/optimizers/LMSubspaceOptimizer.cpp (levmar, not in the reference tree: parity unpinned; oracle/lm_oracle.py restates the published algorithm)",
            "ms_per_solve": dt * 1e3, "iterations": int(r.iters), "damped_solves": int(r.nsolve), "value": (int(r.iters)) / dt, "unit": "iters/s",
            "objective_start": float(r.fret - r.delta), "objective_end": float(r.fret), "camera_blocks": int(r.camera_blocks), "point_blocks": int(r.point_blocks),
            "matrix_cores": "v_mfma_f64_16x16x4_f64 in k_schur / k_cam / k_trail (lm_solver.hip); kernel stats and SQ_INSTS_MFMA / SQ_VALU_MFMA_BUSY_CYCLES "
                            "counter passes: profiles/r06_lm_ladybug_kernel_stats.csv, profiles/r06_lm_ladybug_pmc_mfma.txt"}


def latency_floor():
    """the pieces of ONE dependent evaluation of the cooperative solvers, measured on this device by tools/microbench/eval_floor
    (built by __graft_entry__.build()): a wave's factor arithmetic, its wave sums, one store-to-load hop between compute units,
    one step of the control logic.  None when the binary is not there."""
    import subprocess
    exe = os.path.join(ROOT, "tools", "microbench", "bin", "eval_floor")
    if not os.path.exists(exe):
        return None
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        return json.loads(out.stdout.strip().splitlines()[-1])
    except Exception:   # (a measurement aid: never the reason a bench run fails)
        return None


def _timed_solves(plan, x0, maxiters, steps):
    plan.set_start(x0); plan.solve(maxiters, 3e-8); r = plan.fetch()
    kms, nfe, nge, its = 0.0, 0, 0, 0
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.set_start(x0)
        plan.solve(maxiters, 3e-8)
        r = plan.fetch(out=r)
        kms += plan.last_kernel_ms()[0]
        nfe += int(r.nfeval.sum()); nge += int(r.ngeval.sum()); its += int((r.iters.astype(np.int64) + 1).sum())
    dt = time.perf_counter() - t0
    return r, dt, kms, nfe, nge, its


def configs_block(ctx, maxiters: int, cpu: bool):
    """One row per BASELINE.json config that is not the headline (config 4) or the strong-scaling block (config 5-L): iterations/s
    over all components, f-evals/s, final objective, the solver kernel the dispatcher picked, and a one-core CPU leg (the oracle, a
    port: the same workload, or the stated sample of it).  SURVEY 8d / BASELINE.md section 3."""
    from rdis_amd import capi, problems as P
    with open(os.path.join(ROOT, "tests", "golden", "sinusoid_start.json")) as fh:
        sin_x0 = np.array(json.load(fh)["x0"])

    def sinusoid():
        pp = P.make_high_dim_sinusoid()
        pp.x0 = sin_x0
        return pp.single_component()
    cases = [
        ("config 1: testpoly (data/testpoly.txt, 2 variables; the reference runs it on the CPU path only)", lambda: P.load_poly().single_component(), 200, None,
         "src/main.cpp:180-197"),
        ("config 2: optSinusoid default high-dim sinusoid (121 variables, 362 nonlinear-product factors, one component), committed full-domain start",
         sinusoid, 100, None, "src/optimize_sinusoid.cpp:99-233"),
        ("config 3: ladybug-49-7776 --ncams 5 --npts 30 as one subspace solve (135 variables, 121 factors)", lambda: P.load_bal(ncams=5, npts=30).single_component(), 100, None,
         "src/bundleadjust/optBA.cpp:117-330"),
        ("config 5-S: synthetic decomposable BA, 1000 components x (3 cameras, 40 points, 120 observations), one launch", lambda: P.make_synthetic_ba(1000, 3, 40), 10, 250,
         "src/OptimizableFunctionGenerator.cpp:660-760"),
    ]
    kinds = ("components_cooperative", "components_grid_stream", "components_tiny", "components_lds", "components_point_major", "components_plain")
    rows = []
    fixtures = {"config 1": "testpoly_default_path", "config 2": "sinusoid_default_path", "config 3": "ladybug_5_30_default_path",
                "config 5": "synthetic_S_default_path"}
    for label, make, steps, cpu_sample, ref in cases:
        fixture_key = next((v for k, v in fixtures.items() if label.startswith(k)) if maxiters == 25 else iter(()), None)
        pp = make()
        prob = capi.Problem(ctx, pp)
        plan = capi.Plan(prob)
        x0 = pp.x0[pp.comp_free_vid]
        r, dt, kms, nfe, nge, its = _timed_solves(plan, x0, maxiters, steps)
        row = {"config": label, "reference": ref, "components": int(pp.ncomp), "factors": int(pp.nfac), "variables": int(pp.nvars), "steps": steps,
               "value": its / dt, "unit": "iters/s", "ms_per_step": dt / steps * 1e3, "kernel_ms": kms / steps,
               "f_evals_per_s": nfe / dt, "grad_evals_per_s": nge / dt, "final_objective": float(r.fret.sum()),
               "exit_status_histogram": {capi.EXIT_NAMES[int(k)]: int(v) for k, v in zip(*np.unique(r.status & 0xFF, return_counts=True))},
               "solver": {k[len("components_"):]: int(plan.info(k)) for k in kinds if plan.info(k)}}
        plan.close(); prob.close()
        # the timed default path against the committed CPU fixture (the oracle with the device's factor arithmetic and the sums of the
        # solver the dispatcher picks: the LDS-resident one for configs 3 and 5-S, the plain workgroup solver for configs 1 and 2;
        # tests/golden/make_parity_end_values.py) -- no oracle in this comparison
        if fixture_key is not None:
            try:
                with open(os.path.join(ROOT, "tests", "golden", "parity_end_values.json")) as fh:
                    w = json.load(fh)[fixture_key]
                wf = np.atleast_1d(np.array(w["fret"], dtype=np.float64))
                wn = np.atleast_1d(np.array(w["nfeval"], dtype=np.int64))
                row["bit_identical_to_cpu_fixture"] = bool(np.array_equal(r.fret, wf) and np.array_equal(r.nfeval.astype(np.int64), wn))
            except (OSError, KeyError, ValueError):
                pass
        if cpu:
            from oracle import oracle as O
            o = O.OracleProblem(pp)
            ncomp = pp.ncomp if cpu_sample is None else min(cpu_sample, pp.ncomp)
            reps = max(1, int(20000 // max(pp.nfac * ncomp // max(pp.ncomp, 1), 1))) if pp.ncomp == 1 else 1
            t0 = time.perf_counter()
            cits, cfe, cobj = 0, 0, 0.0
            for _ in range(reps):
                cobj = 0.0
                for c in range(ncomp):
                    fv, fc = pp.component(c)
                    o.assign(None, pp.x0)
                    ro = o.cgd(free_vid=fv, fac=fc, x=pp.x0[fv], maxiters=maxiters)
                    cits += ro.iters + 1; cfe += ro.nfeval; cobj += ro.fret
            dtc = time.perf_counter() - t0
            row["cpu_baseline"] = {"value": cits / dtc, "unit": "iters/s", "cores": 1, "kind": "port", "f_evals_per_s": cfe / dtc,
                                   "sample": ("the workload %d time(s)" % reps) if ncomp == pp.ncomp else "the first %d of %d components" % (ncomp, pp.ncomp),
                                   "final_objective_of_the_sample": cobj}
        rows.append(row)
    return {"what": "BASELINE.json configs 1, 2, 3 and 5-S on one GPU, SSmaxit %d (config 4: the headline; config 5-L: strong_scaling; the recursion over all "
                    "components of configs 3 and 4: all_components)" % maxiters, "rows": rows}


LARGE_SHAPES = [("8e6 factors", 64, 2000000, 4), ("1.2e6 observations", 120, 300000, 4),
                ("356 cameras x 226730 points (more cameras than the LDS holds: local camera numbering)", 356, 226730, 6)]


def large_component(ctx, maxiters: int, cpu: bool, steps: int = 2):
    """ONE bundle-adjustment component larger than ladybug (the larger BAL problems): the wide point-major group
    (solver_ptm.hpp, cgd_ptmg_kernel<512, ., true>: a workgroup per compute unit on the one component) that since round 6 takes
    what is too large for the register-resident cooperative solver when its cameras fit the LDS.  Per shape: `steps` timed solves
    of SSmaxit iterations from the resident start (solve + fetch), the kernel's HIP-event time, its algorithmic bytes (24F + 8N + 8
    a value, 24F + 16N + 8 a value + slope or gradient) against the HBM peak, and a one-core CPU sample (the oracle, ONE CG
    iteration of the same component)."""
    from rdis_amd import capi, problems as P
    rows = []
    for label, C_, Pn, K_ in LARGE_SHAPES:
        pp = P.make_synthetic_ba(1, C_, Pn, obs_per_pt=K_).single_component()
        prob = capi.Problem(ctx, pp)
        plan = capi.Plan(prob)
        plan.set_start(pp.x0)
        t0 = time.perf_counter()
        plan.solve(maxiters, 3e-8); r = plan.fetch(want_x=False)     # (the first solve builds the solver's tables)
        first = time.perf_counter() - t0
        kms, nfe, nge, its = 0.0, 0, 0, 0
        t0 = time.perf_counter()
        for _ in range(steps):
            plan.set_start(pp.x0)
            plan.solve(maxiters, 3e-8)
            r = plan.fetch(want_x=False)
            kms += plan.last_kernel_ms()[0]
            nfe += int(r.nfeval[0]); nge += int(r.ngeval[0]); its += int(r.iters[0]) + 1
        dt = time.perf_counter() - t0
        F, N = pp.nfac, pp.nvars
        abytes = (nfe - nge) * (24.0 * F + 8 * N + 8) + nge * (24.0 * F + 16 * N + 8)
        ach = abytes / (kms * 1e-3) / 1e9
        row = {"shape": label, "cameras": C_, "points": Pn, "factors": int(F), "variables": int(N), "steps": steps,
               "value": its / dt, "unit": "iters/s", "ms_per_solve": dt / steps * 1e3, "kernel_ms": kms / steps,
               "f_evals_per_solve": nfe / steps, "us_per_evaluation": kms * 1e3 / max(nfe, 1), "f_evals_per_s": nfe / dt,
               "final_objective": float(r.fret[0]), "first_solve_s": first,
               "workgroups": int(plan.info("point_major_group")), "wide_group": int(plan.info("point_major_wide")),
               "cameras_in_a_workgroups_lds": int(plan.info("point_major_local_cameras")) or C_,
               "solver": "cgd_ptmg_kernel<512, ., true> (solver_ptm.hpp)" if plan.info("components_point_major") else
                         "cgd_stream_kernel (solver_stream.hpp)" if plan.info("components_grid_stream") else "other",
               "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                            "traffic": measured_traffic("large-component-%dx%dx%d" % (C_, Pn, K_)),
                            "kernel_ms_avg": kms / steps, "algorithmic_bytes_per_launch": abytes / steps}}
        plan.close()
        prob.close()
        if cpu:
            from oracle import oracle as O
            t0 = time.perf_counter()
            ro = O.OracleProblem(pp).cgd(maxiters=1)
            dtc = time.perf_counter() - t0
            row["cpu_baseline"] = {"value": (ro.iters + 1) / dtc, "unit": "iters/s", "cores": 1, "kind": "port",
                                   "sample": "ONE CG iteration of the same component (%d f-evals), dense gradient accumulation" % ro.nfeval,
                                   "f_evals_per_s": ro.nfeval / dtc}
        rows.append(row)
    return {"what": "one bundle-adjustment component larger than ladybug on one GPU, SSmaxit %d" % maxiters, "rows": rows}


def host_cpu():
    """model name and core count of the box the CPU leg runs on"""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as fh:
            for ln in fh:
                if ln.startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    return {"model": model, "logical_cores": os.cpu_count() or 1, "usable_cores": usable}


def objective_band(plan, pp, maxiters: int, k_dev: int = 320):
    """End values over one-ulp-perturbed starts: the device's draws next to the ORACLE'S COMMITTED samples
    (tests/golden/end_values.json, generated by tests/golden/make_end_values.py: 320 end values of the
    reference-faithful CPU oracle compiled like the reference -- its first entry is the reference's recorded run bit
    for bit -- and 320 of the same oracle compiled with contraction, an equally valid rounding of the same algorithm).
    25 unconverged CG iterations are a chaotic map of the start, so one run's end value is a draw from a distribution,
    and that distribution depends on the evaluator's rounding: the oracle's two samples part with KS 0.21
    (tests/test_gpu_solver.py::test_end_values_distribution_matches_oracle).  Outside the
    timed region; nothing under oracle/ runs here."""
    with open(os.path.join(ROOT, "tests", "golden", "end_values.json")) as fh:
        fx = json.load(fh)
    oe = np.array(fx["ladybug_full"]["end_values"])
    oc = np.array(fx["ladybug_full"].get("end_values_contracted", []))

    def ulp(x, k):
        rng = np.random.default_rng([fx["seed"], 200000 + k])
        return np.nextafter(x, np.where(rng.random(x.shape) < 0.5, -np.inf, np.inf))
    def draw(opts, n=None):
        for k, v in opts.items():
            plan.set_option(k, v)
        out, kms = [], 0.0
        for k in range(k_dev if n is None else n):
            plan.set_start((pp.x0 if k == 0 else ulp(pp.x0, k))[pp.comp_free_vid])
            plan.solve(maxiters, 3e-8)
            out.append(float(plan.fetch().fret.sum()))
            kms += plan.last_kernel_ms()[0]
        return np.array(out), kms / len(out)
    # the default (the cooperative solvers round like the reference's build) and the same solver with fused multiply-adds
    de, ms_ref = draw({"factor_rounding": -1})
    df, ms_fma = draw({"factor_rounding": 0})
    # ... and a short sample of the parity option (the reference's slope: one sequential sum per trial, 0.18 s a solve; the full
    # sample and the plain two-sample test are tests/test_gpu_solver.py::test_end_values_distribution_matches_oracle)
    dp, ms_par = draw({"factor_rounding": 1}, n=24)
    plan.set_option("factor_rounding", -1)
    plan.set_start(pp.x0[pp.comp_free_vid])

    def ks(a, b):
        a, b = np.sort(a), np.sort(b)
        allv = np.concatenate([a, b])
        return float(np.max(np.abs(np.searchsorted(a, allv, side="right") / len(a) - np.searchsorted(b, allv, side="right") / len(b))))
    q = lambda v: {"n": int(len(v)), "min": float(v.min()), "q25": float(np.quantile(v, 0.25)), "median": float(np.median(v)),
                   "q75": float(np.quantile(v, 0.75)), "max": float(v.max())}
    out = {"what": "final objective over starts moved by one unit in the last place (first entry: the unperturbed start)",
           "device": dict(q(de), rounding="products rounded before they are added, like the reference's build (plan option factor_rounding: the default "
                                          "of the cooperative solvers)", kernel_ms=ms_ref),
           "device_fused_multiply_add": dict(q(df), rounding="factor_rounding = 0", kernel_ms=ms_fma, ks_vs_oracle=ks(df, oe),
                                             ks_vs_oracle_contracted=ks(df, oc) if len(oc) else None),
           "oracle_fixture": dict(q(oe), unperturbed=float(oe[0]), file="tests/golden/end_values.json"),
           "ks_device_vs_oracle": ks(de, oe),
           "ks_critical_alpha_0.05": float(1.358 * np.sqrt((len(de) + len(oe)) / (len(de) * len(oe)))),
           "reference_recorded": 83227.604227756252,
           "device_parity_option": dict(q(dp), rounding="factor_rounding = 1: the reference's rounding AND every sum added in the reference's order",
                                        kernel_ms=ms_par, ks_vs_oracle=ks(dp, oe),
                                        ks_critical_alpha_0_05=float(1.358 * np.sqrt((len(dp) + len(oe)) / (len(dp) * len(oe))))),
           "parity_option": "plan option factor_rounding = 1 adds every sum in the reference's order (two sequential sums per trial: 0.4 s a solve, "
                            "so only 24 draws here: device_parity_option; its == with the CPU oracle: value_parity_option); under -m gpu, tests/test_gpu_solver.py::test_end_values_distribution_matches_oracle asserts the plain two-sample "
                            "test for it on this workload (measured KS 0.056 at n = 320, critical 0.107) and, for the default drawn here, that the device is no "
                            "further from the oracle than the oracle's own rounding variants are from one another (DESIGN.md section 6)"}
    if len(oc):
        out["oracle_fixture_contracted"] = dict(q(oc), what="the same oracle compiled with -ffp-contract=fast -mfma: an equally valid rounding")
        out["ks_device_vs_oracle_contracted"] = ks(de, oc)
        out["ks_oracle_vs_oracle_contracted"] = ks(oc, oe)
    return out


def parity_option(plan, pp, maxiters: int):
    """The same workload under the PARITY option (plan options factor_rounding = 1, emulate_stale_cache = 1): every product
    rounded before it is added, every sum in the reference's order, the reference's factor cache.  Its end state is compared, ==,
    with the committed CPU fixture tests/golden/parity_end_values.json -- what the CPU oracle returns with its three named
    switches for the device's factor arithmetic on (written by tests/golden/make_parity_end_values.py, pinned by the CPU suite;
    nothing under oracle/ runs here).  Outside the timed region."""
    with open(os.path.join(ROOT, "tests", "golden", "parity_end_values.json")) as fh:
        w = json.load(fh)["ladybug_full_stale_cache"]
    plan.set_option("factor_rounding", 1)
    plan.set_option("emulate_stale_cache", 1)
    best, r = None, None
    for _ in range(2):
        plan.set_start(pp.x0[pp.comp_free_vid])
        t = time.perf_counter()
        plan.solve(maxiters, 3e-8)
        r = plan.fetch()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    ms = plan.last_kernel_ms()[0]
    plan.set_option("factor_rounding", -1)
    plan.set_option("emulate_stale_cache", 0)
    plan.set_start(pp.x0[pp.comp_free_vid])
    same = (float(r.fret[0]) == w["fret"] and int(r.iters[0]) == w["iters"] and int(r.nfeval[0]) == w["nfeval"] and
            int(r.ngeval[0]) == w["ngeval"] and [float(v) for v in r.x[:3]] == w["x_0_2"] and float(r.x[-1]) == w["x_last"])
    return {"value": (int(r.iters[0]) + 1) / best, "unit": "iters/s", "ms_per_solve": best * 1e3, "kernel_ms": ms,
            "final_objective": float(r.fret[0]), "f_evals": int(r.nfeval[0]), "grad_evals": int(r.ngeval[0]),
            "cpu_fixture": {"final_objective": w["fret"], "f_evals": w["nfeval"], "grad_evals": w["ngeval"], "file": "tests/golden/parity_end_values.json"},
            "bit_identical_to_cpu_fixture": bool(same),
            "what": "plan options factor_rounding = 1 + emulate_stale_cache = 1: the reference's rounding, every sum in the reference's order, its factor "
                    "cache; == the CPU oracle with its three named switches for the device's factor arithmetic (own sincos of the rotation angle, "
                    "reciprocals, adjoint sweep) after 25 iterations from x0, no re-synchronisation (tests/test_gpu_parity.py; DESIGN.md section 6). "
                    "A parity option: two sequential sums per trial"}


def plugin_call(prob, pp, maxiters: int, reps: int = 5):
    """What ONE HipCGDSubspaceOptimizer::optimize call of an unchanged caller costs on the same workload:
    rdis_hip_cgd_batch -- the decomposition handed over as host id lists, validated, indexed and uploaded,
    the start copied in, the solve, the results copied out; nothing kept between calls (no plan)."""
    x0 = np.ascontiguousarray(pp.x0[pp.comp_free_vid])
    best, iters = float("inf"), 0
    for _ in range(reps):
        t = time.perf_counter()
        r = prob.cgd_batch(pp.comp_free_ptr, pp.comp_free_vid, pp.comp_fac_ptr, pp.comp_fac_id, x0, maxiters, 3e-8)
        dt = time.perf_counter() - t
        if dt < best:
            best, iters = dt, int(np.sum(r.iters.astype(np.int64) + 1))
    return {"what": "one-shot rdis_hip_cgd_batch on this workload (host id lists in, results out, no resident plan); best of %d" % reps,
            "ms": best * 1e3, "iters_per_s": iters / best}


def all_components(device: int, maxiters: int):
    """BASELINE's metric in its "(all components)" form: every subspace-optimizer call the recursion makes on ladybug --
    separator blocks, leaves, single points -- through include/rdis_optba.h (librdis_host.so: optBA's core with
    HipRDISLevelOptimizer::optimizeReferenceSchedule in RDISOptimizer's place, src/RDISOptimizer.cpp:253-334, 1067), next
    to the reference's own run as BASELINE.md section 2 records it.  Outside the headline's timed region.  The cut
    (a degree-ordered separator instead of PaToH) and the restarts' values (per node, not one shared generator) are not
    the reference's, so the two runs make different calls: what compares is the rate and the end value."""
    import ctypes as C
    import gzip
    import shutil
    import tempfile
    from rdis_amd import problems as P
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run_hist.restype = C.c_int
    lib.rdis_optba_run_hist.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                        C.c_int32, C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_double), C.c_int32]
    names = [b"SSmaxit", b"SSftol", b"maxCalls"]
    ref = {"ladybug 5 cameras / 30 points": {"calls": 731, "seconds_in_calls": 0.197, "final_objective": 18.443091288282886,
                                             "source": "BASELINE.md section 2 (reference built in the survey container, Xeon 2.1 GHz, 1 core)"},
           "ladybug-49-7776 full": {"calls": 13850, "seconds_in_calls": 282.0, "final_objective": 102978.259,
                                    "note": "stopped by its 240 s timeout", "source": "BASELINE.md section 2"}}
    rows = []
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ladybug.txt")
        with gzip.open(P.LADYBUG_PATH, "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        for label, nc, npnt in (("ladybug 5 cameras / 30 points", 5, 30), ("ladybug-49-7776 full", 0, 0)):
            # twice: under the schedule's own end (budget 200 000 calls), and with the REFERENCE'S number of calls as the budget
            for budget, what in ((200000.0, "the schedule to its own end"), (float(ref[label]["calls"]), "budget = the reference run's number of calls")):
                vals = [float(maxiters), 3e-8, budget]
                out = (C.c_double * 10)()
                hist = (C.c_double * (7 * 8))()
                best = None
                for _ in range(2):   # (the second run finds the device warm)
                    t = time.perf_counter()
                    rc = lib.rdis_optba_run_hist(path.encode(), nc, npnt, 1, len(names), (C.c_char_p * len(names))(*names),
                                                 (C.c_double * len(vals))(*vals), device, out, None, hist, 8)
                    wall = time.perf_counter() - t
                    if rc != 0:
                        return {"error": "rdis_optba_run returned %d on %s" % (rc, label)}
                    o = [float(v) for v in out]
                    if best is None or o[5] < best["seconds"]:
                        best = {"problem": label, "run": what, "subspace_optimizer_calls": int(o[2]), "cg_iterations": int(o[3]),
                                "launches": int(o[4]), "calls_per_launch": o[2] / max(o[4], 1.0), "seconds": o[5],
                                "iters_per_s": o[3] / o[5] if o[5] > 0 else 0.0, "calls_per_s": o[2] / o[5] if o[5] > 0 else 0.0,
                                "f_evals": int(o[8]), "initial_objective": o[1], "final_objective": o[0],
                                "decomposition_seconds": o[6], "tree_nodes": int(o[7]), "seconds_with_load_and_upload": wall,
                                "calls_by_depth": [{"depth": d, "nodes": int(hist[7 * d]), "free_variables": int(hist[7 * d + 1]),
                                                    "initial_values": int(hist[7 * d + 2]), "iterative_improvement": int(hist[7 * d + 3]),
                                                    "random_restart": int(hist[7 * d + 4]), "no_progress_beyond_steptol": int(hist[7 * d + 5]),
                                                    "new_minima": int(hist[7 * d + 6])} for d in range(8) if hist[7 * d]],
                                "reference_run": ref[label]}
                rows.append(best)
    return {"what": "the recursion's whole call mix under the reference's per-node schedule (iterative improvement + random restarts, "
                    "nRRperLvl 2), SSmaxit %d: Sigma CG iterations over all subspace-optimizer calls / wall time of the optimisation" % maxiters,
            "not_the_references": "the cut (degree-ordered separator, not PaToH) and the restart values (splitmix64 per node, not one "
                                  "shared mt19937): different calls than the reference's run, same rules (oracle/levels.py replays them)",
            "why_more_calls_than_the_reference": "SURVEY 3.2b: the reference's 731 calls on 5 / 30 are 80 of the top block (48 variables: the same block this "
                                                 "cut finds) + 651 of single points, i.e. 8 point calls per top call where the tree has 29 points -- its branch "
                                                 "and bound (out of scope, DESIGN.md section 7) skips the children of evaluations that cannot improve.  Here every "
                                                 "evaluation of a node runs all its children's loops (calls_by_depth), and the top block's iterative improvement "
                                                 "goes on for as long as its own solve gains more than steptol -- 1 600 steps on 5 / 30, of which 5 are new minima: "
                                                 "the end value is reached within the first 300 calls (the budgeted run: the reference's own number of calls)",
            "runs": rows}


def algorithmic_bytes(pp, nfeval: int, ngeval: int) -> float:
    """value-only evaluation 24F + 8N + 8 bytes, value+gradient
    24F + 16N + 8 (16 B observation + two int32 indices per factor, x read and g
    written once per variable); every df call of the reference is counted as one
    fused unit with the operator() call that precedes it."""
    tot = 0.0
    for c in range(pp.ncomp):
        F = int(pp.comp_fac_ptr[c + 1] - pp.comp_fac_ptr[c])
        N = int(pp.comp_free_ptr[c + 1] - pp.comp_free_ptr[c])
        nf, ng = int(nfeval[c]), int(ngeval[c])
        tot += max(nf - ng, 0) * (24 * F + 8 * N + 8) + ng * (24 * F + 16 * N + 8)
    return tot


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def dump_outputs(directory: str, arrays: dict, suffix: str = "", limit: int = DUMP_LIMIT_BYTES) -> None:
    """--dump-outputs: every array as directory/<name><suffix>.npy in float64.  When they would exceed `limit` bytes together, an
    array longer than its share is replaced by a sample at sorted indices drawn with a fixed seed (the same indices for the same
    length in every run), written beside it as <name>_sample_index."""
    os.makedirs(directory, exist_ok=True)
    out = {k: np.ascontiguousarray(v, dtype=np.float64).ravel() for k, v in arrays.items() if v is not None}
    if sum(v.nbytes for v in out.values()) > limit:
        cap = max(1, (limit - 4096) // 8 // (2 * len(out)))   # (4096: the .npy headers)
        for k in list(out):
            if out[k].size > cap:
                idx = np.sort(np.random.default_rng(20260101).choice(out[k].size, cap, replace=False))
                out[k] = out[k][idx]
                out[k + "_sample_index"] = idx.astype(np.float64)
    for k, v in out.items():
        np.save(os.path.join(directory, k + suffix + ".npy"), v)


def cpu_baseline(pp, maxiters: int):
    """the oracle (a port of the reference's algorithm) on this box's host cores,
    single-threaded like the reference; bounded to a few tens of seconds"""
    from oracle import oracle as O
    ncores = 1
    if pp.ncomp > 1:
        # about 2e5 factors' worth of components (10-20 s): 1000 small ones, 6 of ladybug's size
        ncomp = min(pp.ncomp, 1000, max(1, int(2e5 // max(pp.nfac // pp.ncomp, 1))))
        o = O.OracleProblem(pp)
        t = time.perf_counter()
        its = 0
        for c in range(ncomp):
            fv, fc = pp.component(c)
            r = o.cgd(free_vid=fv, fac=fc, x=pp.x0[fv], maxiters=maxiters)
            its += r.iters + 1
        dt = time.perf_counter() - t
        sample = f"first {ncomp} of {pp.ncomp} components, dense gradient accumulation"
        extra = {}
    else:
        o = O.OracleProblem(pp)
        t = time.perf_counter()
        r = o.cgd(maxiters=maxiters)
        dt = time.perf_counter() - t
        its = r.iters + 1
        sample = f"the full workload once ({its} iterations), dense gradient accumulation"
        # the reference's own cost model: sorted (vid,value)-vector merge per factor (State.h:157-210)
        o2 = O.OracleProblem(pp)
        t = time.perf_counter()
        r2 = o2.cgd(maxiters=1, merge=True)
        dt2 = time.perf_counter() - t
        extra = {"reference_cost_model": {"value": (r2.iters + 1) / dt2, "unit": "iters/s",
                                          "sample": "1 iteration with the reference's per-factor sorted-vector gradient merge",
                                          "final_objective": r2.fret}}
        extra["final_objective"] = r.fret
    out = {"value": its / dt, "unit": "iters/s", "cores": ncores, "kind": "port", "sample": sample, "host": host_cpu()}
    out.update(extra)
    return out


def self_launch(n: int) -> None:
    """`python bench.py --gpus N` without a launcher: re-run this command as N ranks under
    torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1 at a free port), pass their
    output through, and print rank 0's JSON line last."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        t = ln.strip()
        if t.startswith("{") and '"metric"' in t:
            try:
                json.loads(t)
                line = t
                continue
            except ValueError:
                pass
        print(ln, file=sys.stderr)
    if proc.returncode != 0 or line is None:
        sys.exit(f"bench.py --gpus {n}: the ranks exited with {proc.returncode}" + ("" if line else " and printed no result line"))
    print(line, flush=True)


def dry_dist(a, rank: int, world: int) -> None:
    """RDIS_BENCH_DRY_DIST=gloo (tests, no GPU): the distributed mechanics of the bench -- process
    group, barrier, the MAX-over-ranks clock, the summed iteration count, rank 0's line last -- with
    the rank's LPT shard of the strong-scaling decomposition standing in for the device work."""
    import torch
    import torch.distributed as dist
    dist.init_process_group(os.environ["RDIS_BENCH_DRY_DIST"])
    STRONG.update(STRONG_SIZES["small"])   # (the mechanics, not the size)
    _, csr, mine, loads = strong_scaling_shard(rank, world, components=64)
    dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    dist.barrier()
    tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    it = torch.tensor([float(len(mine)), float(csr[2][-1])], dtype=torch.float64)
    dist.all_reduce(it)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "subspace-solver iters/sec (all components), ladybug BA", "dry_run": True, "value": None,
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "seconds_max_over_ranks": float(tt.item()),
                          "components_all_ranks": int(it[0].item()), "factors_all_ranks": int(it[1].item()),
                          "factors_per_rank": [int(v) for v in loads]}), flush=True)


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(a.gpus)          # `python bench.py --gpus N`: start the N ranks ourselves
    if a.gpus > 1 and world != a.gpus:
        sys.exit(f"--gpus {a.gpus} needs one process per GPU: launch with torch.distributed.run "
                 f"--nproc-per-node {a.gpus} (WORLD_SIZE is {world})")
    if os.environ.get("RDIS_BENCH_DRY_DIST"):
        return dry_dist(a, rank, world)
    coll = None
    want_coll = world > 1 or os.environ.get("RDIS_BENCH_FORCE_DIST") == "1"   # the env var exercises the RCCL path on one GPU
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch = dist = None
    if want_coll and a.collective == "torch":
        import torch  # before the HIP library: one HIP runtime per process
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from rdis_amd import capi
    ctx = capi.Context(local_rank)
    if want_coll and a.collective == "torch":
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)  # solver + all-reduce on one stream
        coll = TorchCollective(ctx, torch, dist, local_rank)
    elif want_coll:
        try:
            coll = RcclCollective(capi, ctx, rank, world)       # (no torch in this process)
        except Exception as exc:   # (every rank sees the same failure: the library is missing or refuses the communicator)
            print("bench: RCCL through the C ABI failed (%s); the ranks' scalars go through host files" % exc, file=sys.stderr)
            coll = FileCollective(ctx, rank, world, why=str(exc))

    pp = build_problem(a.workload, rank, a.components, world, a.scaling == "strong", a.large_shape)
    prob = capi.Problem(ctx, pp)
    plan = capi.Plan(prob)
    for kv in a.opt:
        k, v = kv.split("=")
        plan.set_option(k, int(v))
    plan.set_start(pp.x0[pp.comp_free_vid])

    xstart_host = np.ascontiguousarray(pp.x0[pp.comp_free_vid])
    kept = [None]

    def step():
        # the metric is the optimize() / optimize_batch() wall time INCLUDING the H2D copy of the
        # start point; the decomposition (plan) is resident, as it is for a caller that solves it again
        plan.set_start(xstart_host)
        plan.solve(a.maxiters, 3e-8)
        if coll is not None:
            coll.reduce_objective(plan)  # top-level objective = sum over components (RDISOptimizer.cpp:1491-1494)
        kept[0] = plan.fetch(out=kept[0])   # (into the caller's own arrays, like the reference's xval)
        return kept[0]

    def sync():
        if coll is not None:
            coll.barrier_sync()
        ctx.synchronize()

    for _ in range(a.warmup):
        r = step()
    sync()
    kms, klaunch, iters_done = 0.0, 0, 0
    nfe = np.zeros(pp.ncomp, dtype=np.int64)
    nge = np.zeros(pp.ncomp, dtype=np.int64)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        r = step()
        ms, nl = plan.last_kernel_ms()
        kms += ms
        klaunch += nl
        iters_done += int(np.sum(r.iters.astype(np.int64) + 1))
        nfe += r.nfeval
        nge += r.ngeval
    sync()
    dt = time.perf_counter() - t0
    objective_sum = coll.objective(plan) if hasattr(coll, "objective") else plan.objective()  # after the all-reduce: whole-job objective

    if coll is not None:
        dt = coll.allreduce([dt], "max")[0]
        total_iters, total_nfe, total_nge = coll.allreduce([float(iters_done), float(nfe.sum()), float(nge.sum())])
    else:
        total_iters, total_nfe, total_nge = float(iters_done), float(nfe.sum()), float(nge.sum())

    if a.dump_outputs:   # what a caller of the timed path receives from its last step (rank 0 unsuffixed, every other rank _rank<r>)
        dump_outputs(a.dump_outputs, {"x": r.x, "fret": r.fret, "delta": r.delta, "iters": r.iters, "status": r.status,
                                      "nfeval": r.nfeval, "ngeval": r.ngeval, "objective": np.array([objective_sum])},
                     suffix="" if rank == 0 else "_rank%d" % rank, limit=DUMP_LIMIT_BYTES // world)

    if rank == 0:
        abytes = algorithmic_bytes(pp, nfe, nge)
        achieved = abytes / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
        line = {
            "metric": "subspace-solver iters/sec (all components), ladybug BA",
            "value": total_iters / dt, "unit": "iters/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": a.scaling, "full": bool(a.full),
            "vs_baseline": None, "dtype": "f64", "data": "synthetic" if a.workload.startswith("synthetic") else "ladybug-49-7776 (BAL file)",
            "config": {"workload": ("ladybug-49-7776 full, CGD over all 23769 variables / 31843 factors, SSmaxit 25, ftol 3e-8; "
                                    "one such component per GPU") if a.workload == "ladybug-full" else
                       "ladybug-49-7776 with the cameras fixed: 7776 single-point components per GPU, SSmaxit 25" if a.workload == "ladybug-components" else
                       f"synthetic decomposable BA: {pp.ncomp} components x (49 cameras, 7776 points, 31104 observations) per GPU, SSmaxit 25" if a.workload == "synthetic-L" else
                       f"one synthetic BA component of {a.large_shape} (cameras x points x observations per point) per GPU, SSmaxit {a.maxiters}" if a.workload == "large-component" else
                       "synthetic decomposable BA: 1000 components x (3 cameras, 40 points, 120 observations) per GPU, SSmaxit 25",
                       "decomposition": (f"strong scaling: the components of the whole decomposition are shared out over {world} rank(s); "
                                         "rank 0's share is reported below") if a.scaling == "strong" else "weak scaling: the workload is per GPU",
                       "components_per_gpu": pp.ncomp, "factors_per_gpu": pp.nfac, "variables_per_gpu": pp.nvars,
                       "parallelism": f"{world} x independent components, all-reduce of the objective",
                       "collective": coll.name if coll is not None else "none (one rank)"},
            "final_objective": float(r.fret.sum()), "objective_sum_all_ranks": objective_sum,
            "f_evals_per_s": total_nfe / dt, "grad_evals_per_s": total_nge / dt,
            "exit_status_histogram": {capi.EXIT_NAMES[int(k)]: int(v) for k, v in
                                      zip(*np.unique(r.status & 0xFF, return_counts=True))},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": measured_traffic(a.workload if a.workload != "large-component" else "large-component-" + a.large_shape),
                         "traffic_source": "profiles/traffic.json (PMC passes of the same command in the profile round; not collected in this run)",
                         "kernel": "cgd solver kernel(s)", "kernel_ms_avg": kms / max(klaunch, 1),
                         "algorithmic_bytes_per_launch": abytes / max(klaunch, 1),
                         # what governs a single-component solve is not bandwidth but the chain of dependent
                         # evaluations: us per evaluation against the floor of one evaluation
                         # (factor arithmetic of one wave + wave reduction + one store->load hop between compute
                         # units + sweep + one step of the control logic, tools/microbench)
                         "latency": ({"evals": float(nfe.sum()) / max(a.steps, 1), "us_per_eval": kms / max(a.steps, 1) * 1e3 / max(float(nfe.sum()) / max(a.steps, 1), 1.0),
                                      "what": "measured in this run: solver-kernel time per dependent evaluation of the one component (the chain, not bandwidth, "
                                              "governs a single-component solve: DESIGN.md 3.2b; cycle stamps of the pipeline's three sides: profiles/r02_g_pipe_ladybug_stamps.txt)"}
                                     if pp.ncomp == 1 else None)},
        }
        if a.full and world == 1 and pp.ncomp == 1 and line["roofline"]["latency"] is not None:
            fl = latency_floor()
            if fl is not None:
                lat = line["roofline"]["latency"]
                lat["floor_us"] = fl["floor_us"]
                lat["floor"] = fl
                lat["floor_over_measured"] = fl["floor_us"] / lat["us_per_eval"] if lat["us_per_eval"] > 0 else None
                lat["floor_note"] = ("the floor is that of a strictly serial chain (step -> arithmetic -> reduce -> hop); the pipelined solver evaluates "
                                     "guessed Brent steps ahead of its control logic (84 % of them hold), which is how the measured figure reaches the "
                                     "serial floor although every evaluation also pays a sweep over 1000 granules and a request hand-over")
        if a.full and a.workload == "ladybug-full" and a.maxiters == 25 and not a.opt:
            # the headline solve against the committed CPU fixture: what the oracle returns with its four named switches on (the
            # device's factor arithmetic x 3 and the cooperative solvers' sum trees; tests/golden/make_parity_end_values.py, pinned by
            # the CPU suite, asserted live under -m gpu by tests/test_gpu_parity.py).  Nothing under oracle/ runs here.
            try:
                with open(os.path.join(ROOT, "tests", "golden", "parity_end_values.json")) as fh:
                    w = json.load(fh)["ladybug_full_default_path"]
                line["final_objective_parity"] = {
                    "cpu_fixture": {"final_objective": w["fret"], "f_evals": w["nfeval"], "grad_evals": w["ngeval"], "file": "tests/golden/parity_end_values.json"},
                    "bit_identical_to_cpu_fixture": bool(float(r.fret[0]) == w["fret"] and int(r.nfeval[0]) == w["nfeval"] and int(r.ngeval[0]) == w["ngeval"] and
                                                         [float(v) for v in r.x[:3]] == w["x_0_2"] and float(r.x[-1]) == w["x_last"]),
                    "what": "the timed solve's end state == the CPU oracle's with four named switches (own sincos of the rotation angle, reciprocals, adjoint "
                            "sweep, the device's sum trees): DESIGN.md section 6.0; the reference's own arithmetic ends at 83227.604227756252"}
            except (OSError, KeyError, ValueError):
                pass
        if a.full and world == 1:
            line["plugin_call"] = plugin_call(prob, pp, a.maxiters)
            if a.workload == "ladybug-full" and a.maxiters == 25:
                line["value_parity_option"] = parity_option(plan, pp, a.maxiters)
        if a.full and not a.no_cpu_baseline and world == 1:   # the CPU leg is timed at N = 1 only
            line["cpu_baseline"] = cpu_baseline(pp, a.maxiters)
            if a.workload == "ladybug-full" and not a.no_objective_band and a.maxiters == 25:
                line["objective_band"] = objective_band(plan, pp, a.maxiters)
    plan.close()
    prob.close()
    # (--full) north_star's scaling workload, in the command the driver runs: for every N, N = 1 included
    if a.full and a.workload == "ladybug-full" and not a.no_strong_scaling:
        STRONG.clear(); STRONG.update(STRONG_SIZES[a.strong_size])
        ss = run_strong_scaling(ctx, rank, world, coll, a.maxiters, cpu=not a.no_cpu_baseline and world == 1)
        if rank == 0:
            line["strong_scaling"] = ss
    if a.full and a.workload == "ladybug-full" and world == 1 and not a.no_all_components:
        line["all_components"] = all_components(local_rank, a.maxiters)
    if a.full and a.workload == "ladybug-full" and world == 1 and not a.no_configs:
        line["configs"] = configs_block(ctx, a.maxiters, cpu=not a.no_cpu_baseline)
    if a.full and a.workload == "ladybug-full" and world == 1 and not a.no_large_component:
        line["large_component"] = large_component(ctx, a.maxiters, cpu=not a.no_cpu_baseline)
    if a.full and a.workload == "ladybug-full" and world == 1 and not a.no_configs:
        line["normal_equations"] = lm_block(ctx, a.maxiters)
    import ctypes
    ctypes.CDLL(None).fflush(None)   # every rank: nothing buffered (RCCL's banner) may surface after rank 0's JSON
    sys.stdout.flush()
    if coll is not None:
        coll.close()
    ctx.close()
    if rank == 0:
        # RCCL prints a version banner through C stdio, which is flushed at exit when stdout is a
        # pipe: push it out now, so that the JSON really is the last line of stdout
        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        print(json.dumps(line), flush=True)  # the last line of stdout


if __name__ == "__main__":
    main()
