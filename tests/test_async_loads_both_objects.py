"""tools/check_async_loads.py on both objects that hold the cooperative solvers.  tests/test_capi_cpu.py runs it on rdis_hip.o; the
benchmark's solve and the parity option run the reference-rounding instantiation, which is in refround_kernels.o -- with the collector's
poll ring (solver_pipe.hpp: sweep_ring) the loads it checks stay pending across branches and counted waits in both."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_granule_loads_of_both_instantiations_are_waited_for_before_use():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    for name in ("rdis_hip.o", "refround_kernels.o"):
        assert os.path.exists(os.path.join(ROOT, "rdis_amd", "lib", "obj", name)), name      # (the build leaves them there)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_async_loads.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 touched before" in out.stdout and " 0 reach a branch first" in out.stdout, out.stdout
    assert int(out.stdout.split()[0]) >= 300, out.stdout      # both objects were read: each holds well over a hundred such loads
