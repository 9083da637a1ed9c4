"""hip_owning.h's failed-allocation rule (ldso_amd/csrc/hip_owning.h: DevBuf, PinBuf, Event) checked by its
own C++ program, tests/cpp/test_owning.cpp, in an environment without a HIP device: every
allocation fails there, and a failed ensure must leave neither a pointer nor a capacity."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_owning")


def test_failed_allocations_leave_no_capacity(built):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # no device, wherever this runs
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120, env=env)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0 and "0 failure(s)" in p.stdout
