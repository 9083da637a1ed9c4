"""The C++ host face with incremental edits (EnergyFunctional::setIncrementalEdits: a structural change
becomes one ldso_ba_edit_window) driven by its own test program, tests/cpp/test_face_edits.cpp: the
keyframes of test_face_resident.cpp and a point removal on top, bit-identical to the same face
reloading the window, with edits applied and none fallen back."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_face_edits")


def run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    return p


def test_cpp_edits_switch_and_counters(built):
    p = run("--cpu")
    assert p.returncode == 0 and "0 failure(s)" in p.stdout


@pytest.mark.gpu
def test_cpp_incremental_face_matches_reload_bit_for_bit(built):
    p = run()
    assert p.returncode == 0 and "0 failure(s)" in p.stdout
