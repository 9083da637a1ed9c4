"""The coarse initializer's C ABI without a GPU: the new symbols are exported and bound, the structs of
include/ldso_ct.h have the sizes and offsets of the Python dtypes, every refusal returns < 0 with a message,
and ldso_ct_init_lm_step -- the host instantiation of the kernel's LM step -- equals the numpy restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import init_ref as IR
import track_ref as TR
from ldso_amd import _lib as L
from ldso_amd import tracker as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ldso_ct_init_default_params", "ldso_ct_init_check_points", "ldso_ct_init_set_first", "ldso_ct_init_get_points",
       "ldso_ct_init_set_points", "ldso_ct_init_eval", "ldso_ct_init_lm_step", "ldso_ct_init_opt_reg",
       "ldso_ct_init_track_frame", "ldso_ct_init_rank_counts", "ldso_ba_frame_put_initializer"]
f32 = np.float32


def test_new_symbols_are_exported_and_bound(built):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ldso_\w+)", out))
    assert not [s for s in NEW if s not in exported]
    bound = {name for name, _, _ in L.ABI + L.CT_ABI}
    assert not [s for s in NEW if s not in bound]
    lib = L.lib()
    assert lib.ldso_ba_abi_version() == L.ABI_VERSION == 7 and lib.ldso_ct_num_kernels() == 7


def test_struct_layouts_equal_the_dtypes(built, tmp_path):
    structs = {"ldso_ct_init_point": L.INIT_POINT_DTYPE, "ldso_ct_init_result": L.INIT_RESULT_DTYPE,
               "ldso_ct_init_step": L.INIT_STEP_DTYPE}
    params = np.dtype({"names": [n for n, _ in L.LdsoCtInitParams._fields_],
                       "formats": ["<f4", "<f4", "<f4", "<f4", ("<i4", (5,)), "<i4", "<f4"],
                       "offsets": [getattr(L.LdsoCtInitParams, n).offset for n, _ in L.LdsoCtInitParams._fields_],
                       "itemsize": C.sizeof(L.LdsoCtInitParams)})
    structs["ldso_ct_init_params"] = params
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ldso_ct.h"', "int main(void) {"]
    for s, dt in structs.items():
        lines.append(f'printf("{s} size %zu\\n", sizeof({s}));')
        for name in dt.names:
            lines.append(f'printf("{s} {name} %zu\\n", offsetof({s}, {name}));')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        if line:
            s, name, v = line.split()
            got[(s, name)] = int(v)
    for s, dt in structs.items():
        assert got[(s, "size")] == dt.itemsize, s
        for name in dt.names:
            assert got[(s, name)] == dt.fields[name][1], (s, name)
    assert L.INIT_POINT_DTYPE == IR.POINT_DTYPE
    p = T.init_params()
    assert (p.alpha_k, p.alpha_w, p.coupling_weight, p.fix_affine, p.huber_th) == (6.25, 22500.0, 1.0, 1, 9.0)
    assert p.reg_weight == f32(0.8) and list(p.max_iterations) == [5, 5, 10, 30, 50]


def good_lists():
    uv = [np.array([[10.1, 10.1], [20.1, 12.1], [30.1, 30.1], [40.1, 20.1]], f32), np.array([[8.1, 8.1], [15.1, 9.1]], f32)]
    nb, par = IR.knn_tables(uv)
    return IR.make_points(uv, nb, par)


def refused(call, word):
    lib = L.lib()
    rc = call()
    msg = lib.ldso_ba_last_error().decode()
    assert rc < 0 and word in msg, (rc, msg)


def check(levels, w=64, h=48):
    keep, n, pp = T._point_lists(levels)
    return L.lib().ldso_ct_init_check_points(len(keep), w, h, L.ptr(n, L.i32p), pp)


def test_point_list_refusals(built):
    assert check(good_lists()) == 0
    for field, lvl, value, word in [("neighbours", 0, 4, "neighbour"), ("neighbours", 1, -2, "neighbour"),
                                    ("parent", 0, 2, "parent"), ("parent", 0, -1, "parent"), ("parent", 1, 0, "top level"),
                                    ("u", 0, 1.9, "inside"), ("u", 0, 61.0, "inside"), ("v", 1, 21.5, "inside"),
                                    ("v", 0, np.nan, "inside"), ("u", 1, np.inf, "inside")]:
        pts = good_lists()
        if field == "neighbours":
            pts[lvl][field][1, 3] = value
        else:
            pts[lvl][field][1] = value
        refused(lambda: check(pts), word)
    pts = good_lists()
    refused(lambda: check([pts[0], pts[1][:0]]), "at least one point")
    refused(lambda: check([pts[0]] * 6), "1 to 5")
    lib = L.lib()
    refused(lambda: lib.ldso_ct_init_check_points(2, 64, 48, None, None), "null")
    refused(lambda: lib.ldso_ct_init_set_first(None, None, None), "null context")
    refused(lambda: lib.ldso_ct_init_get_points(None, 0, None, 0, None), "null context")
    refused(lambda: lib.ldso_ct_init_set_points(None, 0, 0, None), "null")
    refused(lambda: lib.ldso_ct_init_opt_reg(None, 0, 0.8, 1), "null context")
    refused(lambda: lib.ldso_ct_init_rank_counts(None, None), "null")
    refused(lambda: lib.ldso_ba_frame_put_initializer(None, 0, None), "null")


def lm_args(p):
    z64, z8 = np.zeros(64, f32), np.zeros(8, f32)
    Tm, ab = np.eye(4)[:3].copy(), np.zeros(2)
    inc, To, abo = np.zeros(8, f32), np.zeros((3, 4)), np.zeros(2)
    return [L.ptr(z64, L.f32p), L.ptr(z8, L.f32p), L.ptr(z64, L.f32p), L.ptr(z8, L.f32p), 0.1, 80, 60, L.ptr(Tm, L.f64p),
            L.ptr(ab, L.f64p), C.byref(p), L.ptr(inc, L.f32p), L.ptr(To, L.f64p), L.ptr(abo, L.f64p)], (z64, z8, Tm, ab, inc, To, abo)


def test_parameter_refusals(built):
    lib = L.lib()
    bad = [dict(alpha_k=0.0), dict(alpha_w=-1.0), dict(reg_weight=float("nan")), dict(coupling_weight=float("inf")),
           dict(huber_th=0.0), dict(max_iterations=(5, 5, -1, 30, 50)), dict(max_iterations=(5, 5, 10, 30, 1001)),
           dict(fix_affine=2)]
    for kw in bad:
        p = T.init_params(**kw)
        word = "max_iterations" if "max_iterations" in kw else ("fix_affine" if "fix_affine" in kw else "finite")
        args, keep = lm_args(p)
        refused(lambda: lib.ldso_ct_init_lm_step(*args), word)
        res = np.zeros(1, L.INIT_RESULT_DTYPE)
        refused(lambda: lib.ldso_ct_init_track_frame(None, C.byref(p), res.ctypes.data, None, 0, None), word)
        refused(lambda: lib.ldso_ct_init_eval(None, 0, None, None, C.byref(p), None, None, None, None, None, None), word)
    p = T.init_params(max_iterations=(0, 0, 0, 0, 0))
    args, keep = lm_args(p)
    assert lib.ldso_ct_init_lm_step(*args) == 0
    res = np.zeros(1, L.INIT_RESULT_DTYPE)
    refused(lambda: lib.ldso_ct_init_track_frame(None, C.byref(p), res.ctypes.data, None, 0, None), "null context")
    refused(lambda: lib.ldso_ct_init_eval(None, 0, None, None, None, None, None, None, None, None, None), "null context")
    args[5], args[6] = 0, 60
    refused(lambda: lib.ldso_ct_init_lm_step(*args), "level size")
    args, keep = lm_args(p)
    args[0] = None
    refused(lambda: lib.ldso_ct_init_lm_step(*args), "null")


@pytest.mark.parametrize("fix_affine", [1, 0])
def test_lm_step_equals_the_restatement(built, fix_affine):
    """The increment bit for bit; the pose within 4 ulp per entry (tests/test_track.py's bar: the restatement
    calls libm's sine and cosine, the library its own)."""
    rng = np.random.default_rng(11 + fix_affine)
    for trial in range(6):
        A = rng.standard_normal((40, 9))
        A[:, 6] *= 30
        A[:, 7] *= 0.5
        M = (A.T @ A * 10.0 ** rng.uniform(2, 6)).astype(f32)
        Asc = rng.standard_normal((40, 9)) * 0.4
        Msc = (Asc.T @ Asc * 10.0 ** rng.uniform(1, 4)).astype(f32)
        H, b, Hsc, bsc = M[:8, :8], M[:8, 8], Msc[:8, :8], Msc[:8, 8]
        lam = f32(10.0 ** rng.uniform(-4, 2))
        w, h = (320 >> trial % 3), (240 >> trial % 3)
        T0 = np.zeros((3, 4))
        T0[:, :3] = TR.q_matrix(TR.q_normalize(tuple(rng.standard_normal(4))))
        T0[:, 3] = rng.standard_normal(3) * 0.05
        aff = (f32(rng.standard_normal() * 0.1), f32(rng.standard_normal() * 3))
        inc, To, abo = T.init_lm_step(H, b, Hsc, bsc, lam, w, h, T0, aff, fix_affine=fix_affine)
        rinc, rpose, raff = IR.lm_step(H, b, Hsc, bsc, lam, w, h, TR.pose_from_matrix(T0), aff, bool(fix_affine))
        assert inc.tobytes() == rinc.tobytes(), (trial, inc, rinc)
        assert TR.pose_ulps(To, TR.pose_matrix(rpose)) <= 4
        assert f32(abo[0]) == raff[0] and f32(abo[1]) == raff[1]
        if fix_affine:
            assert inc[6] == 0 and inc[7] == 0
