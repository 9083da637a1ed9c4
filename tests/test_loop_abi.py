"""include/ldso_lc.h at the boundary, without a GPU: the library exports and the bindings bind every symbol
the header declares, the record layouts agree, and what can be refused before any HIP call is refused with
a message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import loop_ref as R
from ldso_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldso_lc.h")


def declared_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ldso_lc_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(built):
    syms = declared_symbols()
    assert len(syms) == 16
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ldso_lc_\w+)", out))
    assert not [s for s in syms if s not in exported]
    assert set(syms) == {name for name, _, _ in L.LC_ABI}
    lib = L.lib()
    assert lib.ldso_lc_abi_version() == L.LC_ABI_VERSION == 1
    assert lib.ldso_ba_abi_version() == 7  # the other two headers are as they were
    txt = open(HEADER).read()
    assert "#define LDSO_LC_ABI_VERSION 1" in txt and "#define LDSO_LC_GRID_SIZE 20" in txt


def test_record_layouts():
    assert L.LC_FEATURE_DTYPE == R.FEATURE_DTYPE and L.LC_FEATURE_DTYPE.itemsize == 56
    assert L.LC_MATCH_DTYPE == R.MATCH_DTYPE and L.LC_MATCH_DTYPE.itemsize == 12
    assert L.LC_PROJECTION_DTYPE == R.PROJECTION_DTYPE and L.LC_PROJECTION_DTYPE.itemsize == 80
    assert L.LC_FEATURE_DTYPE.fields["descriptor"][1] == 24 and L.LC_PROJECTION_DTYPE.fields["p_ref"][1] == 16


def test_refusals_before_any_hip_call(built):
    lib = L.lib()
    h = C.c_void_p()
    for args, word in (((0, 19, 120, 4, 100), b"small"), ((0, 160, 120, 0, 100), b"max_keyframes"),
                       ((0, 160, 120, 4, 0), b"max_features")):
        assert lib.ldso_lc_create(*args, C.byref(h)) < 0 and not h.value
        assert word in lib.ldso_ba_last_error()
    assert lib.ldso_lc_create(0, 160, 120, 4, 100, None) < 0
    n = C.c_int32(-7)
    z = np.zeros(8, np.int32)
    f = np.zeros(8, np.float32)
    d = np.zeros(8, np.float64)
    assert lib.ldso_lc_keyframe_put(None, 0, 0, None) < 0 and b"null" in lib.ldso_ba_last_error()
    assert lib.ldso_lc_keyframe_put_tracker(None, 0, None) < 0
    assert lib.ldso_lc_keyframe_update(None, 0, 0, None, None) < 0
    assert lib.ldso_lc_keyframe_set_bow(None, 0, 0, None, L.ptr(z, L.i32p), None) < 0
    assert lib.ldso_lc_keyframe_get(None, 0, 0, None, C.byref(n)) < 0
    assert lib.ldso_lc_keyframe_drop(None, 0) < 0
    assert lib.ldso_lc_search_brute_force(None, 0, 1, 50, 0, None, C.byref(n)) < 0
    assert lib.ldso_lc_search_brute_force_many(None, 0, 0, None, 50, None, None, None) < 0
    assert lib.ldso_lc_search_by_bow(None, 0, 1, 50, 0.6, 0, None, C.byref(n)) < 0
    assert lib.ldso_lc_make_idepth_map_ba(None, None, 0, -1, None) < 0 and b"null" in lib.ldso_ba_last_error()
    assert lib.ldso_lc_make_idepth_map(None, 0, None) < 0
    assert lib.ldso_lc_get_idepth_map(None, L.ptr(f, L.f32p)) < 0
    assert lib.ldso_lc_search_by_projection(None, 0, 1, L.ptr(f, L.f32p), L.ptr(d, L.f64p), 5.0, 50, 0, None,
                                            C.byref(n)) < 0
    assert n.value == -7  # a refused call writes nothing
    lib.ldso_lc_destroy(None)
