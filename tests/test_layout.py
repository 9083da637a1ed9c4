"""The window layout ldso_ba_load uploads (ldso_amd/csrc/layout.cpp: sharding, the residual bucket
sort, the k_linearize / k_point_sc work items, every base offset) checked on the CPU by its own
C++ program, tests/cpp/test_layout.cpp, which links the host-only objects and needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_layout")


def test_layout_on_cpu(built):
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0 and "0 failure(s)" in p.stdout
