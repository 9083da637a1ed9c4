"""The keyframe close through the C++ host face on the device (EnergyFunctional::flagPoints and
setDeviceMarginalization: ldso_ba_flag_points, ldso_ba_load_marginalization_device, one
ldso_ba_edit_window) driven by its own test program, tests/cpp/test_face_close.cpp: the keyframes of
test_face_resident.cpp with the full close, bit-identical to the same face on the host path, with no
residual read-back over the cycle and no edit fallen back."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_face_close")


def run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    return p


def test_cpp_close_switches_and_refusals(built):
    p = run("--cpu")
    assert p.returncode == 0 and "0 failure(s)" in p.stdout


@pytest.mark.gpu
def test_cpp_device_close_matches_host_close_bit_for_bit(built):
    p = run()
    assert p.returncode == 0 and "0 failure(s)" in p.stdout
