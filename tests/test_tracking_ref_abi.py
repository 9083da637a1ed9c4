"""The device-built tracking reference (ldso_ct_make_reference, ldso_ct_make_reference_ba,
ldso_ct_get_reference): what needs no GPU.  The symbols are exported and bound, null arguments are
refused before any HIP call, and the numpy restatement of makeCoarseDepthL0 that the GPU tests
compare with (tests/coarse_depth_ref.py) gives answers worked out by hand."""
import ctypes as C
import re
import subprocess

import numpy as np

import coarse_depth_ref as R
from ldso_amd import _lib as L

F = np.float32
NEW = ("ldso_ct_make_reference", "ldso_ct_make_reference_ba", "ldso_ct_get_reference")


def test_symbols_exported_and_bound(built):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ldso_ct_\w+)", out))
    bound = {name for name, _, _ in L.CT_ABI}
    for s in NEW:
        assert s in exported and s in bound, s
    lib = L.lib()
    for s in NEW:
        assert getattr(lib, s).argtypes is not None
    assert lib.ldso_ba_abi_version() == 7
    assert lib.ldso_ct_num_kernels() == 7


def test_null_arguments_are_refused_before_any_hip_call(built):
    lib = L.lib()
    c = np.zeros((1, 3), F)
    h = np.ones(1, F)
    n = np.zeros(6, np.int32)
    assert lib.ldso_ct_make_reference(None, None, 1, L.ptr(c, L.f32p), L.ptr(h, L.f32p), 1.0, 0.0, 0.0,
                                      L.ptr(n, L.i32p)) < 0
    assert b"null" in lib.ldso_ba_last_error()
    assert lib.ldso_ct_make_reference_ba(None, None, None, 0, -1, 1.0, 0.0, 0.0, L.ptr(n, L.i32p)) < 0
    assert b"null" in lib.ldso_ba_last_error()
    k = C.c_int32()
    assert lib.ldso_ct_get_reference(None, 0, C.byref(k), None, 0) < 0
    assert b"null" in lib.ldso_ba_last_error()


def test_level_sizes_follow_the_tracker_rule():
    assert R.level_sizes(320, 240) == [(320, 240), (160, 120), (80, 60)]
    assert R.level_sizes(332, 244) == [(332, 244), (166, 122), (83, 61)]
    assert R.level_sizes(322, 242) == [(322, 242), (161, 121)]  # odd halves stop the pyramid
    assert len(R.level_sizes(640, 480)) == 4
    assert R.level_sizes(1232, 368)[-1] == (77, 23)  # 5 levels: 154 x 46 is still above 5000 pixels


def _colors(w, h):
    return [np.full(wl * hl, 10.0 + l, F) for l, (wl, hl) in enumerate(R.level_sizes(w, h))]


def test_one_contribution_by_hand():
    # one contribution at (101, 77) of a 3-level size, idepth 0.5 (a power of two, so that
    # (0.5 * weight) / weight is 0.5 exactly whatever the weight)
    w, h = 320, 240
    pcs = R.make_coarse_depth(w, h, [[101.2, 76.6, 0.5]], [3.0], _colors(w, h))
    # level 0: the pixel and its four diagonal neighbours (sum / 1, num / 1), row-major
    # level 1: pixel (50, 38) and its diagonals; level 2: pixel (25, 19) and its axis neighbours
    want = [
        [(100, 76), (102, 76), (101, 77), (100, 78), (102, 78)],
        [(49, 37), (51, 37), (50, 38), (49, 39), (51, 39)],
        [(25, 18), (24, 19), (25, 19), (26, 19), (25, 20)],
    ]
    for l in range(3):
        assert pcs[l].dtype == F and pcs[l].shape == (5, 4)
        assert [(int(u), int(v)) for u, v in pcs[l][:, :2]] == want[l]
        assert np.all(pcs[l][:, 2] == F(0.5)) and np.all(pcs[l][:, 3] == F(10.0 + l))


def test_weight_is_the_double_quotient_then_sqrtf():
    assert R.weight_of(0.0) == np.sqrt(F(1e-3 / 1e-12))
    assert R.weight_of(1e-3) == np.sqrt(F(1e-3 / (float(F(1e-3)) + 1e-12)))
    # int(c + 0.5f) truncates: -0.7 + 0.5 -> pixel 0; -1.5 and w - 0.5 are outside
    assert R.pixel_of(-0.7, 0.2, 320, 240) == (0, 0)
    assert R.pixel_of(-1.5, 0.2, 320, 240) is None and R.pixel_of(319.5, 0.2, 320, 240) is None
    assert R.pixel_of(float("nan"), 0.2, 320, 240) is None


FIVE_CENTER, FIVE_HDI = R.FIVE_CENTER, R.FIVE_HDI


def test_five_fold_pixel_depends_on_the_order():
    w, h = 320, 240
    fwd = R.scatter(w, h, FIVE_CENTER, FIVE_HDI)
    rev = R.scatter(w, h, FIVE_CENTER[::-1], FIVE_HDI[::-1])
    wts = np.array([R.weight_of(x) for x in FIVE_HDI])
    assert wts.min() < 2e-3 and wts.max() > 5e2
    # by hand: the chain from 0 in the given order
    s = F(0)
    ws = F(0)
    for c, wt in zip(FIVE_CENTER, wts):
        s = F(s + F(c[2] * wt))
        ws = F(ws + wt)
    assert fwd[0][33, 57] == s and fwd[1][33, 57] == ws
    assert np.count_nonzero(fwd[1]) == 1
    # the reversed order gives other bits: a device sum in the wrong order cannot pass
    assert (fwd[0][33, 57], fwd[1][33, 57]) != (rev[0][33, 57], rev[1][33, 57])
    a = R.make_coarse_depth(w, h, FIVE_CENTER, FIVE_HDI, _colors(w, h))
    b = R.make_coarse_depth(w, h, FIVE_CENTER[::-1], FIVE_HDI[::-1], _colors(w, h))
    assert a[0].tobytes() != b[0].tobytes()
