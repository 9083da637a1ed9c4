"""Corner detection (FeatureDetector::DetectCorners, makeNewTraces with setting_pointSelection 1): what
needs no GPU.  The cases the GPU test compares on (tests/corner_detect_ref.py) are shown to be well
posed on the restatement alone -- the grid values, corners next to non-corners, a suppressed
neighbour, a pick the tie rule decides, scores that are not finite -- the two parallel forms the
kernels use are checked against the literal ones, and the new entry points of include/ldso_ct.h are
exported and bound."""
import ctypes as C
import functools
import math
import re
import subprocess

import numpy as np
import pytest

import corner_detect_ref as R
from ldso_amd import _lib as L

F = np.float32
NEW = ("ldso_ct_corners_init", "ldso_ct_detect_corners")
SIZED = sorted(R.CASES)
ALL = [(kind,) + case for case in SIZED for kind in R.KINDS]


@functools.lru_cache(maxsize=None)
def frame(kind, w, h):
    return R.Frame(R.image(kind, w, h))


@functools.lru_cache(maxsize=None)
def detected(kind, w, h, n):
    return R.detect_corners(frame(kind, w, h), n, R.bit_pattern())


def sorted_scores(cell):
    return sorted(cell["scores"].tolist(), key=R.sort_key)


def test_umax_is_the_orb_table(built):
    assert R.UMAX == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    # the circular patch: symmetric under the transposition the constructor enforces
    for v, u in enumerate(R.UMAX):
        assert R.UMAX[u] >= v


@pytest.mark.parametrize("case", SIZED, ids=lambda c: f"{c[0]}x{c[1]}n{c[2]}")
def test_grid_values(built, case):
    w, h, n = case
    G = R.grid(w, h, n)
    if R.CASES[case] is not None:
        assert (G["gridsize"], G["k"]) == R.CASES[case]
    assert 1 <= G["gridsize"] <= 30 and R.TILE < G["gridsize"] / 2
    # the margins include/ldso_ct.h derives: 31 pixels on the left and top, 16 on the right and bottom
    g, skip = G["gridsize"], G["skip"]
    assert skip * g >= 31
    assert (G["gridX"] - skip) * g - 1 <= w - 17 and (G["gridY"] - skip) * g - 1 <= h - 17


def test_grid_values_of_the_named_cases(built):
    assert R.grid(200, 136, 340)["nfeat"] == F(1.0125)
    G = R.grid(*R.WIDE)
    assert (G["gridsize"], G["k"]) == (17, 1)
    assert R.grid(200, 136, 20)["gridsize"] == 37  # refused by the library
    # every gridsize up to 30 keeps the margins, none above does
    for g in range(1, 60):
        right = (30 // g) * g
        assert (right >= 16) == (g <= 30), g


@pytest.mark.parametrize("case", SIZED, ids=lambda c: f"{c[0]}x{c[1]}n{c[2]}")
def test_blobs_corners_noncorners_and_suppression(built, case):
    out = detected("blobs", *case)
    info, feat = out["info"], out["feat"]
    assert 0 < feat["is_corner"].sum() < feat.size
    assert (info["cand"] & (feat["is_corner"] == 0)).any()  # a corner candidate a neighbour suppressed
    G = info["grid"]
    edge = [c for c in info["cells"] if c["gx"] in (G["skip"], G["gridX"] - G["skip"] - 1) or
            c["gy"] in (G["skip"], G["gridY"] - G["skip"] - 1)]
    assert any((c["scores"] == 0).any() for c in info["cells"]) or any(c["scores"].size for c in edge)
    # non-corners carry nothing
    off = feat["is_corner"] == 0
    assert (feat["angle"][off] == 0).all() and not feat["descriptor"][off].any()
    assert feat["descriptor"][~off].any()


@pytest.mark.parametrize("case", SIZED, ids=lambda c: f"{c[0]}x{c[1]}n{c[2]}")
def test_tiles_tie_rule_decides_a_pick(built, case):
    out = detected("tiles", *case)
    k = out["stats"]["k"]
    decided = 0
    for c in out["info"]["cells"]:
        s = sorted_scores(c)
        if len(s) > k and R.bits(s[k - 1]) == R.bits(s[k]):
            decided += 1
            # the stable order: among the equal scores the earliest candidates are the picks
            tied = [i for i, v in enumerate(c["scores"].tolist()) if R.bits(v) == R.bits(s[k - 1])]
            last_pick = c["picks"][-1]
            assert last_pick in tied and all(i in c["picks"] for i in tied if i < last_pick)
    assert decided > 0


@pytest.mark.parametrize("case", SIZED, ids=lambda c: f"{c[0]}x{c[1]}n{c[2]}")
def test_nan_scores_sort_last(built, case):
    out = detected("nan", *case)
    mixed = 0
    for c in out["info"]["cells"]:
        s = c["scores"]
        fin = np.isfinite(s)
        if not fin.all() and fin.any():
            mixed += 1
        picked = s[c["picks"]]
        # no score that is not finite ahead of a finite one: such a pick means every finite one is picked
        if not np.isfinite(picked).all():
            assert fin.sum() <= np.isfinite(picked).sum()
            first_bad = np.flatnonzero(~np.isfinite(picked))[0]
            assert np.isfinite(picked[:first_bad]).all() and not np.isfinite(picked[first_bad:]).any()
    assert mixed > 0
    assert not np.isfinite(np.concatenate([c["scores"] for c in out["info"]["cells"]])).all()
    assert np.isfinite(out["info"]["max_score"])


@pytest.mark.parametrize("case", ALL, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}n{c[3]}")
def test_parallel_forms_equal_the_literal_ones(built, case):
    out = detected(*case)
    info, k = out["info"], out["stats"]["k"]
    xs, ys = out["xy"][:, 0], out["xy"][:, 1]
    lit = R.suppress_literal(xs, ys, out["feat"]["score"], info["cand"])
    assert np.array_equal(lit, out["feat"]["is_corner"].astype(bool))
    assert np.array_equal(lit, R.suppress_parallel(xs, ys, out["feat"]["score"], info["cand"]))
    for c in info["cells"]:
        s = c["scores"].tolist()
        assert R.picks_by_rank(s, k) == R.picks_by_sort(s, k) == c["picks"]
        assert len(c["picks"]) == min(len(s), k)


def test_angle_against_math_atan2(built):
    """The restatement's double atan2 (numpy) against Python's own: within the GPU test's allowance."""
    out = detected("blobs", 203, 139, 300)
    ci = np.flatnonzero(out["feat"]["is_corner"])
    _, m_01, m_10 = R.ic_angle(frame("blobs", 203, 139), out["xy"][ci, 0], out["xy"][ci, 1])
    own = np.array([F(math.atan2(float(a), float(b))) for a, b in zip(m_01, m_10)], F)
    assert np.array_equal(R.bits(own), R.bits(out["feat"]["angle"][ci]))


def test_descriptor_known_answer(built):
    """A ramp I = x: dIp[.][0] grows with the column, so with angle 0 (a = 1, b = 0) a comparison is
    p0 < p2 of its pattern row (col = p0, row = p1)."""
    w, h = 96, 64
    img = np.tile(np.arange(w, dtype=F), (h, 1))
    fr = R.Frame(img)
    pat = R.bit_pattern()
    d = R.descriptor(fr, 40, 32, F(0), pat)
    P = pat.reshape(256, 4)
    assert np.array_equal(np.unpackbits(d, bitorder="little").astype(bool), P[:, 0] < P[:, 2])
    # an angle that is not finite: every tap leaves the patch
    assert not R.descriptor(fr, 40, 32, F(np.nan), pat).any()


def test_symbols_exported_and_bound(built):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ldso_ct_\w+)", out))
    bound = {name for name, _, _ in L.CT_ABI}
    for s in NEW:
        assert s in exported and s in bound, s
    lib = L.lib()
    assert lib.ldso_ba_abi_version() == 7
    assert lib.ldso_ct_num_kernels() == 7
    assert L.FEATURE_DTYPE == R.FEATURE_DTYPE and L.FEATURE_DTYPE.itemsize == 48
    assert L.CORNER_STATS == R.STATS


def test_null_context_is_refused_with_a_message(built):
    lib = L.lib()
    n = C.c_int32()
    pat = R.bit_pattern()
    assert lib.ldso_ct_corners_init(None, L.ptr(pat, L.i32p)) < 0
    assert b"null" in lib.ldso_ba_last_error()
    assert lib.ldso_ct_detect_corners(None, 300, 0, 0, None, None, C.byref(n), None) < 0
    assert b"null" in lib.ldso_ba_last_error()
