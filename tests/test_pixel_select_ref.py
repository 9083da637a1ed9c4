"""Pixel selection (PixelSelector::makeMaps, FullSystem::makeNewTraces with setting_pointSelection 0):
what needs no GPU.  The numpy restatement the GPU tests compare with (tests/pixel_select_ref.py) is
pinned by properties that do not come from its own code, the test inputs are shown to reach every
branch of makeMaps and the direction-dependent cells of select, and the new entry points of
include/ldso_ct.h are exported, bound and refuse a NULL context."""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

import pixel_select_ref as R
from ldso_amd import _lib as L

F = np.float32
NEW = ("ldso_ct_select_default_params", "ldso_ct_select_init", "ldso_ct_select_potential", "ldso_ct_select_pixels",
       "ldso_ct_make_new_traces")


@functools.lru_cache(maxsize=None)
def frame(kind, w, h):
    return R.Frame(R.image(kind, w, h))


@functools.lru_cache(maxsize=None)
def maps(kind, w, h, density, potential):
    sel = R.Selector(R.pattern_of(w, h), potential)
    return sel.make_maps(frame(kind, w, h), density=density)


# ---- makeMaps' branches on the chosen inputs --------------------------------------------------
def test_more_points_recursion(built):
    m, st, tr = maps("blobs", 192, 128, 300, 3)
    p = tr["passes"]
    assert len(p) == 2 and p[0]["pot"] == 3 and p[0]["quotia"] > 1.25
    assert p[1]["pot"] == 1 and p[1]["quotia"] < 0.95  # then potential 1 with sub-selection
    assert st["passes"] == 2 and st["potential_used"] == 1
    assert st["num"] < st["n2"] + st["n3"] + st["n4"] and st["num"] == np.count_nonzero(m)


def test_fewer_points_recursion(built):
    m, st, tr = maps("blobs", 192, 128, 20, 2)
    p = tr["passes"]
    assert len(p) == 2 and p[0]["pot"] == 2 and p[0]["quotia"] < 0.25 and p[1]["pot"] >= 9


def test_no_recursion_with_subselection(built):
    m, st, tr = maps("blobs", 192, 128, 600, 1)
    p = tr["passes"]
    assert len(p) == 1 and 0.25 <= p[0]["quotia"] < 0.95
    assert st["num"] == np.count_nonzero(m) < np.count_nonzero(p[0]["map"])


def test_too_few_points_ends_without_subselection(built):
    m, st, tr = maps("blobs", 192, 128, 3000, 3)
    assert tr["passes"][-1]["quotia"] > 1.25
    assert st["num"] == st["n2"] + st["n3"] + st["n4"] == np.count_nonzero(m)


def test_unaligned_size_one_pass_and_subselection(built):
    m, st, tr = maps("blobs", 200, 136, 300, 3)
    assert len(tr["passes"]) == 1 and tr["passes"][0]["quotia"] < 0.95


def test_mixed_image_has_direction_dependent_cells(built):
    for w, h in R.SIZES:
        m, st, tr = maps("mixed", w, h, 300, 3)
        first = tr["passes"][0]
        assert first["info"]["blocked"] >= 100, first["info"]
        assert first["n"][0] > 100


def test_nan_image_drops_records_in_the_walk(built):
    for w, h in R.SIZES:
        sel = R.Selector(R.pattern_of(w, h), 3)
        rec, st, tr, walked = sel.make_new_traces(frame("nan", w, h), density=300)
        assert walked - rec.size >= 1 and rec.size >= 200, (walked, rec.size)
        assert np.all(np.isfinite(rec["energy_th"]))
        # row-major order of the walk
        key = rec["v"].astype(np.int64) * w + rec["u"].astype(np.int64)
        assert np.all(np.diff(key) > 0)


# ---- invariants that do not come from the restatement -----------------------------------------
@pytest.mark.parametrize("kind", ["blobs", "mixed", "nan"])
@pytest.mark.parametrize("size", R.SIZES)
def test_select_invariants(built, kind, size):
    w, h = size
    m, st, tr = maps(kind, w, h, 300, 3)
    fr, T, p = frame(kind, w, h), tr["tests"], tr["params"]
    first = tr["passes"][0]
    pot, m0 = first["pot"], first["map"]
    n2, n3, n4 = first["n"]
    assert np.count_nonzero(m0) == n2 + n3 + n4
    assert (np.count_nonzero(m0 == 1), np.count_nonzero(m0 == 2), np.count_nonzero(m0 == 4)) == (n2, n3, n4)
    assert set(np.unique(m0)) <= {0, 1, 2, 4}
    ys, xs = np.nonzero(m0)
    # nothing outside the border rule
    assert xs.min() >= 4 and xs.max() < w - 5 and ys.min() >= 4 and ys.max() <= h - 4
    # at most one pick of each type per cell of its level
    for t, side in ((1, pot), (2, 2 * pot), (4, 4 * pot)):
        yy, xx = np.nonzero(m0 == t)
        cells = (yy // side) * w + xx // side
        assert np.unique(cells).size == cells.size
    # no type-2 pick in a 2 pot block with a type-1 pick, no type-4 pick in a 4 pot block with either
    y1, x1 = np.nonzero(m0 == 1)
    y2, x2 = np.nonzero(m0 == 2)
    y4, x4 = np.nonzero(m0 == 4)
    b2 = lambda yy, xx, s: set(((yy // s) * w + xx // s).tolist())
    assert not (b2(y1, x1, 2 * pot) & b2(y2, x2, 2 * pot))
    assert not ((b2(y1, x1, 4 * pot) | b2(y2, x2, 4 * pot)) & b2(y4, x4, 4 * pot))
    # every type-1 pick is past its threshold (looked up here, not taken from the restatement)
    ag0 = fr.ag[0].reshape(h, w)
    sm = tr["smoothed"]
    th = sm[(x1 >> 5) + (y1 >> 5) * (w // 32)]
    assert np.all(ag0[y1, x1] > (th * F(p["th_factor"])).astype(F))
    if w % 32 or h % 32:
        assert np.all(sm[(w // 32) * (h // 32):] == 0)  # the entries makeHists never writes


def test_histogram_quantile_against_cumsum(built):
    for w, h in R.SIZES:
        m, st, tr = maps("blobs", w, h, 300, 3)
        ag0 = frame("blobs", w, h).ag[0].reshape(h, w)
        for (bx, by), hist in tr["hists"].items():
            blk = ag0[32 * by:32 * by + 32, 32 * bx:32 * bx + 32]
            yy, xx = np.mgrid[32 * by:32 * by + 32, 32 * bx:32 * bx + 32]
            ok = (xx >= 1) & (xx <= w - 2) & (yy >= 1) & (yy <= h - 2)
            g = np.minimum(np.sqrt(blk[ok]).astype(np.int64), 48)
            counts = np.bincount(g, minlength=49)
            assert hist[0] == ok.sum() and np.array_equal(hist[1:50], counts)
            share = int(F(ok.sum()) * F(0.5) + F(0.5))
            first_bin = int(np.argmax(np.cumsum(counts) > share))
            assert tr["ths"][by, bx] == F(first_bin) + F(7)


def test_flat_image_selects_nothing(built):
    w, h = 192, 128
    sel = R.Selector(R.pattern_of(w, h), 3)
    m, st, tr = sel.make_maps(R.Frame(np.full((h, w), 90.0, F)), density=300)
    assert np.count_nonzero(m) == 0 and st["num"] == 0
    assert sel.potential == 1 and st["potential_next"] == 1


def test_potential_persists(built):
    w, h = 192, 128
    sel = R.Selector(R.pattern_of(w, h), 3)
    seen = []
    for seed in (1, 2, 3):
        m, st, tr = sel.make_maps(R.Frame(R.image("blobs", w, h, seed=seed)), density=300)
        assert tr["passes"][0]["pot"] == (seen[-1] if seen else 3)
        seen.append(st["potential_next"])
        assert sel.potential == seen[-1]


# ---- the C ABI without a GPU ------------------------------------------------------------------
def test_symbols_exported_and_bound(built):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ldso_ct_\w+)", out))
    bound = {name for name, _, _ in L.CT_ABI}
    for s in NEW:
        assert s in exported and s in bound, s
    lib = L.lib()
    assert lib.ldso_ba_abi_version() == 7
    assert lib.ldso_ct_num_kernels() == 7


def test_default_params(built):
    p = L.LdsoCtSelectParams()
    L.lib().ldso_ct_select_default_params(C.byref(p))
    got = {k: getattr(p, k) for k, _ in p._fields_}
    assert got == dict(density=1500.0, recursions=1, th_factor=1.0, min_grad_hist_cut=0.5, min_grad_hist_add=7.0,
                       grad_downweight_per_level=0.75, select_direction_distribution=1)
    assert got == {k: type(got[k])(v) for k, v in R.DEFAULTS.items()}
    assert C.sizeof(L.LdsoCtSelectParams) == 28


def test_null_context_is_refused_with_a_message(built):
    lib = L.lib()
    pat = np.zeros(16, np.uint8)
    n = C.c_int32()
    st = np.zeros(len(L.SELECT_STATS), np.int32)
    assert lib.ldso_ct_select_init(None, L.ptr(pat, L.u8p), 3) < 0
    assert b"null" in lib.ldso_ba_last_error()
    assert lib.ldso_ct_select_potential(None, C.byref(n)) < 0
    assert b"null" in lib.ldso_ba_last_error()
    assert lib.ldso_ct_select_pixels(None, None, None, L.ptr(st, L.i32p)) < 0
    assert b"null" in lib.ldso_ba_last_error()
    assert lib.ldso_ct_make_new_traces(None, None, 0, 0, None, C.byref(n), L.ptr(st, L.i32p)) < 0
    assert b"null" in lib.ldso_ba_last_error()
