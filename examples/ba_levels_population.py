#!/usr/bin/env python3
"""optBA's sample loop on full ladybug (49 cameras, 7776 points) as ONE run: 16 initial states drawn on the device from every
variable's sampling interval, the level driver's sweeps (the 46-camera separator, then its 6561 children) for all of them at once
-- every step one launch over the members still running, a member that has stopped is not solved again -- with
Levenberg-Marquardt, the two pixel residuals a factor (useCGD 0, LMmodel 2), through the C entry rdis_optba_run_samples.
Prints per member the start value, the final value and the sweeps, then the best.
With `cgd` as the last argument: the reference's default configuration instead, useCGD 1 -- the separator and the camera level
run on the cooperative solver, a cooperative group per (member, component) (the level option populationCooperative = 1;
without it this tree is refused).

  python examples/ba_levels_population.py [samples] [sweeps] [SSmaxit] [seed] [cgd]"""
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
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    sweeps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    maxit = int(sys.argv[3]) if len(sys.argv) > 3 else 25
    seed = int(sys.argv[4]) if len(sys.argv) > 4 else 20240611
    cgd = len(sys.argv) > 5 and sys.argv[5] == "cgd"
    lib = C.CDLL(os.path.join(ROOT, "rdis_amd", "lib", "librdis_host.so"))
    lib.rdis_optba_run_samples.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int32,
                                           C.c_int64, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    tmp = tempfile.mkdtemp()
    try:
        path = os.path.join(tmp, "ladybug.txt")
        with gzip.open(P.LADYBUG_PATH, "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        o = {"useCGD": 0.0, "LMmodel": 2.0, "SSmaxit": float(maxit), "maxSweeps": float(sweeps)}
        if cgd:
            o = {"useCGD": 1.0, "populationCooperative": 1.0, "SSmaxit": float(maxit), "maxSweeps": float(sweeps)}
        names, vals = [n.encode() for n in o], list(o.values())
        out, members = np.zeros(10), np.zeros((samples, 8))
        rc = lib.rdis_optba_run_samples(path.encode(), 0, 0, len(names), (C.c_char_p * len(names))(*names), (C.c_double * len(vals))(*vals), 0,
                                        samples, seed, 1, out.ctypes.data_as(C.c_void_p), members.ctypes.data_as(C.c_void_p), None)
        assert rc == 0, rc
        print("member        start value        final value  sweeps")
        for s, m in enumerate(members):
            print("  %4d   %16.6g   %16.6f   %5d" % (s, m[0], m[1], int(m[2])))
        best = int(np.nanargmin(members[:, 1]))
        print("best: member %d, %.6f (from %.6g)" % (best, out[0], out[1]))
        print("%d subspace-optimizer calls and %d iterations over all members, %d launches for the best member, %.1f ms (decomposition %.1f ms)" % (
            out[2], out[3], out[4], out[5] * 1e3, out[6] * 1e3))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
