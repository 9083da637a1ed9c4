"""The C ABI of frame ingestion (include/ldso_ct.h): the new entry points are exported and bound, every
refusal comes back negative with its message, and the kernel-timing slots are the seven they were."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from ldso_amd import _lib as L

NEW = ["ldso_ct_undistort_init", "ldso_ct_set_new_frame_raw", "ldso_ct_set_new_frame_raw_device",
       "ldso_ct_get_undistorted", "ldso_ct_undistort_make_remap", "ldso_ct_undistort_make_photometric"]
W, H = 64, 48


def refused(rc, text):
    msg = L.lib().ldso_ba_last_error().decode()
    assert rc < 0 and text in msg, (rc, msg)


def test_symbols_and_kernel_slots(built):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    bound = {name for name, _, _ in L.CT_ABI}
    for s in NEW:
        assert f" T {s}\n" in out and s in bound, s
    lib = L.lib()
    assert lib.ldso_ct_num_kernels() == 7
    assert "undistort" not in " ".join(lib.ldso_ct_kernel_name(i).decode() for i in range(7))
    assert C.sizeof(L.LdsoCtUndistortDesc) == 56


def test_null_arguments(built):
    lib = L.lib()
    d = L.LdsoCtUndistortDesc(w_org=W, h_org=H)
    raw = np.zeros(W * H, np.uint8)
    img = np.zeros(W * H, np.float32)
    refused(lib.ldso_ct_undistort_init(None, C.byref(d), None), "null argument")
    refused(lib.ldso_ct_set_new_frame_raw(None, raw.ctypes.data, 8, 1.0, 1.0, None, None), "null argument")
    refused(lib.ldso_ct_set_new_frame_raw_device(None, raw.ctypes.data, 8, 1.0, 1.0, None, None, None), "null argument")
    refused(lib.ldso_ct_get_undistorted(None, L.ptr(img, L.f32p)), "null argument")
    refused(lib.ldso_ct_undistort_make_photometric(None, 256, None, 8, 4, 2, None, None), "null argument")
    refused(lib.ldso_ct_undistort_make_remap(0, None, W, H, W, H, 0, None, None, None, None, None), "null argument")


@pytest.fixture(scope="module")
def tracker(built):
    from ldso_amd.tracker import CoarseTracker

    t = CoarseTracker(W, H)
    yield t
    t.close()


def _desc(keep, **kw):
    """A valid descriptor (a remap into a 20 x 10 source, a 256-entry LUT) with fields replaced."""
    w_org, h_org = kw.get("w_org", 20), kw.get("h_org", 10)
    a = dict(remap_x=np.full(W * H, 1.5, np.float32), remap_y=np.full(W * H, 2.5, np.float32),
             g=np.arange(256, dtype=np.float32), vignette_inv=np.ones(max(w_org * h_org, 1), np.float32))
    a.update({k: v for k, v in kw.items() if k in a})
    keep.append(a)
    d = L.LdsoCtUndistortDesc(w_org=w_org, h_org=h_org, g_depth=kw.get("g_depth", 256),
                              photometric_mode=kw.get("photometric_mode", 2), use_exposure=1)
    for k, v in a.items():
        setattr(d, k, L.ptr(v, L.f32p))
    return d


@pytest.mark.gpu
def test_raw_frame_before_init(tracker):
    lib = L.lib()
    raw = np.zeros(W * H, np.uint8)
    refused(lib.ldso_ct_set_new_frame_raw(tracker._h, raw.ctypes.data, 8, 1.0, 1.0, None, None),
            "ldso_ct_undistort_init not called")
    refused(lib.ldso_ct_set_new_frame_raw_device(tracker._h, raw.ctypes.data, 8, 1.0, 1.0, None, None, None),
            "ldso_ct_undistort_init not called")
    img = np.zeros(W * H, np.float32)
    refused(lib.ldso_ct_get_undistorted(tracker._h, L.ptr(img, L.f32p)), "ldso_ct_set_new_frame not called")


@pytest.mark.gpu
@pytest.mark.parametrize("kw, text", [
    (dict(w_org=1), "at least 2 x 2"),
    (dict(h_org=1), "at least 2 x 2"),
    (dict(g_depth=255), "g_depth must be at least 256"),
    (dict(remap_x=None), "one of them is NULL"),
    (dict(remap_y=None), "one of them is NULL"),
    (dict(remap_x=None, remap_y=None), "passthrough needs a raw image of the context's size 64x48"),
    (dict(photometric_mode=3), "photometric_mode out of range"),
    (dict(photometric_mode=-1), "photometric_mode out of range"),
    (dict(vignette_inv=None), "g needs vignette_inv"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_init_refusals(tracker, kw, text):
    keep = []
    d = _desc(keep, **kw)
    refused(L.lib().ldso_ct_undistort_init(tracker._h, C.byref(d), None), text)
    refused(L.lib().ldso_ct_undistort_init(tracker._h, None, None), "null argument")


@pytest.mark.gpu
def test_frame_refusals_after_init(tracker):
    lib = L.lib()
    keep = []
    outside = C.c_int32(-1)
    d = _desc(keep)
    assert lib.ldso_ct_undistort_init(tracker._h, C.byref(d), C.byref(outside)) == 0
    assert outside.value == 0
    raw = np.zeros(20 * 10, np.uint16)
    refused(lib.ldso_ct_set_new_frame_raw(tracker._h, None, 8, 1.0, 1.0, None, None), "null argument")
    refused(lib.ldso_ct_set_new_frame_raw(tracker._h, raw.ctypes.data, 12, 1.0, 1.0, None, None), "bits must be 8 or 16")
    refused(lib.ldso_ct_set_new_frame_raw(tracker._h, raw.ctypes.data, 16, 1.0, 1.0, None, None),
            "65536 entries of G: g_depth is 256")
    refused(lib.ldso_ct_set_new_frame_raw_device(tracker._h, raw.ctypes.data, 16, 1.0, 1.0, None, None, None),
            "65536 entries of G: g_depth is 256")
    # where the frame takes the first branch (exposure_time <= 0) no table is indexed: 16 bits are read
    e = C.c_float()
    assert lib.ldso_ct_set_new_frame_raw(tracker._h, raw.ctypes.data, 16, 0.0, 1.0, None, C.byref(e)) == 0
    assert e.value == 0.0
    # a refused init leaves the earlier tables in force
    bad = _desc(keep, photometric_mode=5)
    assert lib.ldso_ct_undistort_init(tracker._h, C.byref(bad), None) < 0
    assert lib.ldso_ct_set_new_frame_raw(tracker._h, raw.ctypes.data, 16, 0.0, 1.0, None, None) == 0
