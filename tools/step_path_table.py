"""One steady step of the headline command as its stream saw it, from a rocprofv3 run with HIP-API, kernel and memory-copy
tracing (no counters):

   rocprofv3 --hip-runtime-trace --kernel-trace --memory-copy-trace --output-format csv -d DIR -o step -- \
       python bench.py --gpus 1 --steps 20 --warmup 5
   python tools/step_path_table.py DIR/step [step-from-the-end, default 2] > profiles/step_path_trace_<which>.txt

A step is set_start + solve + fetch of one plan.  The device operations of step k are those from the first upload behind solver
launch k - 1 to the last operation in front of the next upload; the host side is the HIP calls of the same stretch, cut into C calls
at hipSetDevice (every entry point of the library begins with it).  Times in microseconds from the step's first HIP call."""
from __future__ import annotations

import csv
import sys


def rows(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def main():
    stem = sys.argv[1]
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    ops = []
    for r in rows(stem + "_kernel_trace.csv"):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        ops.append({"what": "kernel " + name, "corr": int(r["Correlation_Id"]), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]),
                    "solver": "cgd_" in name})
    for r in rows(stem + "_memory_copy_trace.csv"):
        d = r["Direction"].replace("MEMORY_COPY_", "").replace("HOST_TO_DEVICE", "H2D").replace("DEVICE_TO_HOST", "D2H")
        ops.append({"what": "copy " + d, "corr": int(r["Correlation_Id"]), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]), "solver": False})
    ops.sort(key=lambda o: o["t0"])
    api = [{"fn": r["Function"], "corr": int(r["Correlation_Id"]), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])}
           for r in rows(stem + "_hip_api_trace.csv")]
    api.sort(key=lambda a: a["t0"])

    solvers = [i for i, o in enumerate(ops) if o["solver"]]
    i = solvers[-back]

    def first_upload_behind(j):   # index of the first H2D copy behind operation j, len(ops) if none
        for k in range(j + 1, len(ops)):
            if ops[k]["what"] == "copy H2D":
                return k
        return len(ops)
    lo, hi = first_upload_behind(solvers[-back - 1]), first_upload_behind(i)
    step = ops[lo:hi]
    by_corr = {a["corr"]: a for a in api}
    a_lo = by_corr[step[0]["corr"]]
    # the C call that enqueued the first upload begins at the hipSetDevice in front of it
    k0 = api.index(a_lo)
    while k0 > 0 and api[k0]["fn"] != "hipSetDevice":
        k0 -= 1
    t_zero = api[k0]["t0"]
    nxt = ops[hi]["corr"] if hi < len(ops) else None
    k1 = api.index(by_corr[nxt]) if nxt in by_corr else len(api)
    while k1 > k0 and api[k1 - 1]["fn"] != "hipSetDevice":
        k1 -= 1
    k1 = max(k1 - 1, k0 + 1)   # (up to, not including, the next step's hipSetDevice)

    us = lambda t: (t - t_zero) / 1e3
    print("stream operations of one steady step (us from the step's first HIP call)")
    print("%-58s %10s %10s %10s %10s" % ("operation", "start", "end", "length", "gap"))
    prev = None
    for o in step:
        gap = "" if prev is None else "%10.2f" % ((o["t0"] - prev["t1"]) / 1e3)
        print("%-58s %10.2f %10.2f %10.2f %10s" % (o["what"][:58], us(o["t0"]), us(o["t1"]), (o["t1"] - o["t0"]) / 1e3, gap))
        prev = o
    solver = [o for o in step if o["solver"]][0]
    print("first operation's start to last operation's end: %.2f us; the solver kernel %.2f us; the rest %.2f us"
          % ((step[-1]["t1"] - step[0]["t0"]) / 1e3, (solver["t1"] - solver["t0"]) / 1e3,
             (step[-1]["t1"] - step[0]["t0"] - solver["t1"] + solver["t0"]) / 1e3))
    print()
    print("host side: HIP calls of the same step, cut into C calls at hipSetDevice")
    calls, cur = [], None
    for a in api[k0:k1]:
        if a["fn"] == "hipSetDevice" or cur is None:
            cur = []
            calls.append(cur)
        cur.append(a)
    for grp in calls:
        fns = [a["fn"] for a in grp]
        label = ("plan_set_start" if any(a["corr"] == step[0]["corr"] for a in grp) else
                 "plan_solve" if "hipLaunchCooperativeKernel" in fns else
                 "plan_fetch" if any(f in ("hipStreamSynchronize", "hipEventSynchronize") for f in fns) and any(f.startswith("hipMemcpy") for f in fns) else
                 "plan_last_kernel_ms (the benchmark's)" if "hipEventElapsedTime" in fns else "other")
        print("%-40s start %9.2f  host time inside %9.2f us (first HIP call's start to the last one's end)"
              % (label, us(grp[0]["t0"]), (grp[-1]["t1"] - grp[0]["t0"]) / 1e3))
        for a in grp:
            print("    %-36s %9.2f %9.2f" % (a["fn"], us(a["t0"]), (a["t1"] - a["t0"]) / 1e3))
    print("whole step on the host, first HIP call to the next step's first: %.2f us" % ((api[k1]["t0"] - t_zero) / 1e3 if k1 < len(api) else float("nan")))


if __name__ == "__main__":
    main()
