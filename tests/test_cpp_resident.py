"""The C++ host face with resident frames (include/ldso_amd/energy_functional.h: the frame store,
insertFrame from the coarse tracker, ldso_ba_load_frames on structural changes) driven by its own
test program, tests/cpp/test_face_resident.cpp: two keyframes of a 5-frame window, bit-identical to
the same face on the ldso_ba_load path, with no host -> device image bytes over the second."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_face_resident")


def run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    return p


def test_cpp_resident_bookkeeping_and_argument_checks(built):
    p = run("--cpu")
    assert p.returncode == 0 and "0 failure(s)" in p.stdout


@pytest.mark.gpu
def test_cpp_resident_face_matches_load_path_bit_for_bit(built):
    p = run()
    assert p.returncode == 0 and "0 failure(s)" in p.stdout
