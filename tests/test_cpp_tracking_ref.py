"""EnergyFunctional::setCoarseTrackingRef (include/ldso_amd/energy_functional.h) driven by its own
test program, tests/cpp/test_tracking_ref.cpp: one keyframe of a 5-frame window, the face's
device-built tracking reference bit-identical on every level to ldso_ct_make_reference fed from
residualCenter, residualState and the points' HdiF in the face's traversal order."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_tracking_ref")


def run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    return p


def test_cpp_tracking_ref_argument_checks(built):
    p = run("--cpu")
    assert p.returncode == 0 and "0 failure(s)" in p.stdout


@pytest.mark.gpu
def test_cpp_tracking_ref_matches_host_route_bit_for_bit(built):
    p = run()
    assert p.returncode == 0 and "0 failure(s)" in p.stdout
