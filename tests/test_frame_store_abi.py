"""Frame-store entry points of include/ldso_ba.h without a GPU: exported, bound, and refusing null
or invalid arguments before any HIP call (a context cannot exist without a device, so every check
that runs here runs ahead of the device)."""
import ctypes as C
import re
import subprocess

import numpy as np

from ldso_amd import _lib as L

NEW = ["ldso_ba_frames_reserve", "ldso_ba_frame_put", "ldso_ba_frame_put_device", "ldso_ba_frame_put_tracker",
       "ldso_ba_frame_drop", "ldso_ba_frame_get", "ldso_ba_load_frames", "ldso_ba_transfer_stats"]


def test_symbols_exported_and_bound(built):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ldso_ba_\w+)", out))
    bound = {name for name, _, _ in L.ABI}
    for name in NEW:
        assert name in exported and name in bound, name
    lib = L.lib()
    assert lib.ldso_ba_abi_version() == 7  # functions were added, nothing changed
    assert lib.ldso_ct_num_kernels() == 7  # the ingest kernels take no tracker timing slot


def test_null_and_invalid_arguments_are_refused(built):
    lib = L.lib()
    px = np.zeros(12, np.float32)
    ids = np.zeros(2, np.int64)
    st = np.zeros(4, np.int64)
    w = L.LdsoBaWindow()
    fake = C.c_void_p(px.ctypes.data)  # never dereferenced: the null context is refused first
    calls = [
        lambda: lib.ldso_ba_frames_reserve(None, 4, 160, 120),
        lambda: lib.ldso_ba_frame_put(None, 0, L.ptr(px, L.f32p)),
        lambda: lib.ldso_ba_frame_put_device(None, 0, fake, fake, None),
        lambda: lib.ldso_ba_frame_put_tracker(None, 0, fake),
        lambda: lib.ldso_ba_frame_put_tracker(None, 0, None),
        lambda: lib.ldso_ba_frame_drop(None, 0),
        lambda: lib.ldso_ba_frame_get(None, 0, L.ptr(px, L.f32p), None),
        lambda: lib.ldso_ba_load_frames(None, 1, C.byref(w), L.ptr(ids, L.i64p), 0, 1),
        lambda: lib.ldso_ba_transfer_stats(None, L.ptr(st, L.i64p)),
    ]
    for call in calls:
        assert call() < 0
        assert lib.ldso_ba_last_error()
    assert L.ERR_FRAME_STORE == -4 and L.ERR_GRADIENT_MISMATCH == -5


def test_error_carries_the_code(built):
    lib = L.lib()
    try:
        L.check(lib.ldso_ba_frame_drop(None, 0))
    except L.LdsoError as e:
        assert e.code == -1 and isinstance(e, RuntimeError) and "ldso_ba error -1" in str(e)
    else:
        raise AssertionError("a negative return must raise")
