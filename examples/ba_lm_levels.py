#!/usr/bin/env python3
"""optBA's --useCGD switch on full ladybug (49 cameras, 7776 points): the level driver (sweeps over the decomposition tree:
the 46-camera separator, then its 6561 children in one launch) through the C entry rdis_optba_run, once with the CGD subspace
optimiser (useCGD 1, the default) and once with Levenberg-Marquardt (useCGD 0: resident rdis_hip_lm_plans, a step's objective
from one 128-byte summary).  Prints the objective after every sweep -- a run of k sweeps for k = 1, 2, ...: the runs are
deterministic, so each is a prefix of the next -- and the time of the longest run.

  python examples/ba_lm_levels.py [sweeps] [SSmaxit] [LMmodel]"""
import ctypes as C
import gzip
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rdis_amd import problems as P  # noqa: E402


def main():
    sweeps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    maxit = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    model = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                   C.c_int32, C.c_void_p, C.c_void_p]
    tmp = tempfile.mkdtemp()
    try:
        path = os.path.join(tmp, "ladybug.txt")
        with gzip.open(P.LADYBUG_PATH, "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        for label, opts in (("useCGD 1 (CGD)", {"useCGD": 1.0}), ("useCGD 0 (Levenberg-Marquardt, LMmodel %d)" % model, {"useCGD": 0.0, "LMmodel": float(model)})):
            print(label)
            for k in range(1, sweeps + 1):
                o = dict(opts, SSmaxit=float(maxit), maxSweeps=float(k))
                names, vals = [n.encode() for n in o], list(o.values())
                out = np.zeros(10)
                rc = lib.rdis_optba_run(path.encode(), 0, 0, 0, len(names), (C.c_char_p * len(names))(*names), (C.c_double * len(vals))(*vals), 0,
                                        out.ctypes.data_as(C.c_void_p), None)
                assert rc == 0, rc
                if k == 1:
                    print("  start            %14.6f" % out[1])
                print("  after sweep %-2d   %14.6f" % (k, out[0]))
                if int(out[9]) < k:
                    print("  (the driver stopped after %d sweeps: the last gained less than steptol)" % int(out[9]))
                    break
            print("  %d subspace-optimizer calls in %d launches, %d iterations, %.1f ms (decomposition %.1f ms)" % (
                out[2], out[4], out[3], out[5] * 1e3, out[6] * 1e3))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
