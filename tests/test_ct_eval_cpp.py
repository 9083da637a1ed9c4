"""The coarse tracker's per-evaluation functions (ldso_amd/csrc/ct_eval.h: the hypothesis' constants, the Vec6
and the scaled H, b from the sums), which the host entry points and k_ct_track both call, checked on the
CPU by their own C++ program, tests/cpp/test_ct_eval.cpp, against the straightforward statements.  The
same source builds and runs under the address and undefined-behaviour sanitizers with `make -C
ldso_amd/csrc sanitize-ct-eval` (a stand-alone executable, not part of the suite)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_ct_eval")


def test_ct_eval_on_cpu(built):
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ok:" in p.stdout and " 0 failed" in p.stdout
