"""The keyframe-close entry points at the C-ABI boundary, no GPU: the symbols exist and are bound, the
ABI version is still 7 (functions were added, nothing changed), ldso_ba_default_flag_params gives
Setting.cc's values, and the refusals that need no context return < 0 with a message.  The refusals
that need a loaded context are in test_flag_parity and test_marg_device."""
import ctypes as C
import re
import os

import numpy as np

import edit_cases as ec
from ldso_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ldso_ba_default_flag_params", "ldso_ba_flag_points", "ldso_ba_load_marginalization_device", "ldso_ba_marg_plan_check")


def test_symbols_and_version(built):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "ldso_ba.h")).read()
    bound = {name for name, _, _ in L.ABI}
    for name in NEW:
        assert hasattr(lib, name) and name in bound and re.search(r"\b%s\(" % name, header), name
    assert lib.ldso_ba_abi_version() == L.ABI_VERSION == 7
    assert re.search(r"#define LDSO_BA_ABI_VERSION 7\b", header)
    for k, v in dict(ACTIVE=0, OUTLIER=1, OUT=2, MARGINALIZED=3).items():
        assert re.search(r"#define LDSO_BA_PT_%s %d\b" % (k, v), header) and getattr(L, "PT_" + k) == v


def test_default_flag_params(built):
    p = L.FlagParams.default()
    assert (p.min_good_active_res_for_marg, p.min_good_res_for_marg, p.min_idepth_h_marg, p.reserved_) == (3, 4, 50.0, 0)
    assert C.sizeof(L.FlagParams) == 16
    L.lib().ldso_ba_default_flag_params(None)  # tolerated


def last_error():
    return L.lib().ldso_ba_last_error().decode()


def test_calls_without_a_context_are_refused(built):
    lib = L.lib()
    ff = np.zeros(4, np.uint8)
    assert lib.ldso_ba_flag_points(None, 0, None, L.ptr(ff, L.u8p), None, None, None, None, None, None, None, None) < 0
    assert "bad arguments" in last_error()
    w = ec.window_of(ec.make_pool(), ec.base_sel(ec.make_pool()))
    s = w.c_struct(with_images=False)
    pts = np.zeros(1, np.int32)
    assert lib.ldso_ba_load_marginalization_device(None, None, 0, C.byref(s), 1, L.ptr(pts, L.i32p), None) < 0
    assert "bad arguments" in last_error()


def plan(w, pts, live=None, item_order=0):
    lib = L.lib()
    s = w.c_struct(with_images=False)
    pts = np.ascontiguousarray(pts, np.int32)
    rg = np.full(w.n_residuals + 1, -7, np.int32)
    pg = np.full(pts.size + 1, -7, np.int32)
    n_res, mism = C.c_int32(-1), C.c_int32(-1)
    rc = lib.ldso_ba_marg_plan_check(C.byref(s), int(pts.size), L.ptr(pts, L.i32p), L.ptr(live, L.u8p), item_order, 0,
                                     L.ptr(rg, L.i32p), L.ptr(pg, L.i32p), C.byref(n_res), C.byref(mism))
    return rc, rg, pg, n_res.value, mism.value


def test_marginalisation_plan_refusals_and_a_plan(built):
    pool = ec.make_pool()
    w = ec.window_of(pool, ec.base_sel(pool), rank=True)
    for pts, msg in (([0, w.n_points], "not a point of the parent"), ([-1], "not a point of the parent"), ([2, 5, 2], "twice")):
        rc, *_ = plan(w, pts)
        assert rc < 0 and msg in last_error(), (pts, last_error())
    rc, *_ = plan(w, [2, 5], item_order=2)
    assert rc < 0 and "ITEM_ORDER 2" in last_error()
    # a plan: every second point, every third residual dropped
    pts = np.arange(0, w.n_points, 2, dtype=np.int32)
    live = (np.arange(w.n_residuals) % 3 != 0).astype(np.uint8)
    rc, rg, pg, n_res, mism = plan(w, pts, live)
    assert rc == 0 and mism == 0
    want = sum(int(live[w.point_res_begin[p]:w.point_res_begin[p + 1]].sum()) for p in pts)
    assert n_res == want
    assert len(set(rg[:n_res])) == n_res and rg[:n_res].min() >= 0 and rg[:n_res].max() < w.n_residuals and rg[n_res] == -7
    assert len(set(pg[:pts.size])) == pts.size and pg[:pts.size].min() >= 0 and pg[:pts.size].max() < w.n_points
    rc, _, _, n_res, mism = plan(w, np.zeros(0, np.int32))
    assert (rc, n_res, mism) == (0, 0, 0)
