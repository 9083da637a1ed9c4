"""ldso_ba_load_marginalization_device's host planner (ldso_amd/csrc/marg_plan.cpp) checked by its own
C++ program, tests/cpp/test_marg_plan.cpp, which links the host-only objects and needs no GPU.  The
same source builds and runs under the address and undefined-behaviour sanitizers with `make -C
ldso_amd/csrc sanitize-marg-plan` (a stand-alone executable, not part of the suite)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_marg_plan")


def test_marg_plan_on_cpu(built):
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ok:" in p.stdout and " 0 failed" in p.stdout
