"""The restatement of frame ingestion (tests/undistort_ref.py) on the CPU: known answers of the
restatement itself, the host helpers ldso_ct_undistort_make_remap / _make_photometric against it bit for
bit, and the checks that the cases of tests/test_undistort.py are well posed."""
import numpy as np
import pytest

import undistort_ref as R
from ldso_amd import _lib as L

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- known answers of the restatement -----------------------------------------------------------
def test_identity_remap_returns_the_photometric_value():
    w_org, h_org = 9, 7
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 256, w_org * h_org).astype(np.uint8)
    g = np.linspace(0, 255, 256).astype(f32) ** f32(1.1)
    vinv = rng.uniform(1, 2, w_org * h_org).astype(f32)
    w, h = w_org - 1, h_org - 1  # integer coordinates whose footprint is inside
    gy, gx = np.mgrid[0:h, 0:w]
    rm = (gx.ravel().astype(f32), gy.ravel().astype(f32))
    img, e, outside = R.undistort(raw, w_org, h_org, w, h, remap=rm, g=g, vignette_inv=vinv, exposure=0.5)
    want = (g[raw] * vinv).reshape(h_org, w_org)[:h, :w]
    assert outside == 0 and e == f32(0.5)
    assert np.array_equal(bits(img), bits(want))
    # the three branches of processFrame on one pixel
    assert R.photometric(raw, None, None, 2, True, 0.5, 0.5)[0][3] == f32(0.5) * f32(raw[3])
    assert R.photometric(raw, g, vinv, 1, True, 0.5, 0.5)[0][3] == g[raw[3]]
    assert R.photometric(raw, g, vinv, 2, True, 0.0, 0.5)[0][3] == f32(0.5) * f32(raw[3])
    assert R.photometric(raw, g, vinv, 2, False, 0.5, 1.0)[1] == 1


def test_hand_computed_blend():
    # source 3 x 2 = [[10, 20, 99], [30, 50, 99]], factor 1; the entry (0.25, 0.5):
    #   xxyy = 0.125; 0.125 * 50 + (0.5 - 0.125) * 30 + (0.25 - 0.125) * 20 + (1 - 0.25 - 0.5 + 0.125) * 10
    #   = 6.25 + 11.25 + 2.5 + 3.75 = 23.75, every step exact in float
    raw = np.array([10, 20, 99, 30, 50, 99], np.uint8)
    rm = (np.array([0.25, -1, 1.5, 0.25], f32), np.array([0.5, -1, 0.5, 1.0], f32))
    img, _, outside = R.undistort(raw, 3, 2, 2, 2, remap=rm)
    assert img[0, 0] == f32(23.75)
    assert img[0, 1] == 0  # the reference's own mark
    # (1.5, 0.5): columns 1 and 2, rows 0 and 1, all weights 0.25: 0.25 * 99 + 0.25 * 50 + 0.25 * 99 + 0.25 * 20 = 67
    assert img[1, 0] == f32(67)
    assert img[1, 1] == 0 and outside == 1  # (0.25, 1.0) needs row 2, which the source does not have


def test_footprint_rule():
    rx = np.array([0.5, 81.999, 82.0, 5.0, 5.0, 5.0, np.nan, np.inf, -0.5, -np.inf, 5.0], f32)
    ry = np.array([0.5, 59.999, 5.0, 60.0, 70.5, 59.5, 1.0, 1.0, 70.0, 1.0, np.nan], f32)
    ox, oy, n = R.footprint(rx, ry, 83, 61)
    rejected = np.array([0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 1], bool)
    assert n == rejected.sum()
    assert np.array_equal(ox[rejected], np.full(rejected.sum(), -1, f32)) and np.array_equal(oy[rejected], ox[rejected])
    assert np.array_equal(bits(ox[~rejected]), bits(rx[~rejected])) and np.array_equal(bits(oy[~rejected]), bits(ry[~rejected]))


# ---- the host helpers against the restatement ---------------------------------------------------
@pytest.mark.parametrize("depth, vdtype, mode", [(256, np.uint8, 2), (256, np.uint16, 1), (1000, np.uint8, 0),
                                                 (65536, np.uint16, 2)])
def test_make_photometric(built, depth, vdtype, mode):
    from ldso_amd import tracker

    g_raw, v = R._tables(depth, vdtype, True, seed=depth + mode)
    g, vinv = tracker.make_photometric(g_raw, v, mode)
    gr, vr = R.make_photometric(g_raw, v, mode)
    assert np.array_equal(bits(g), bits(gr))
    assert np.array_equal(bits(vinv), bits(vr))
    assert np.isinf(vinv).sum() == 2  # the zero pixels give inf, which is kept
    assert g[0] == 0 and g[-1] == 255 and (np.diff(g.astype(np.float64)) >= 0).all()
    if mode == 0:
        assert g[1] == f32(255) / f32(depth - 1)


def test_make_photometric_refusals(built):
    from ldso_amd import tracker

    g_raw, v = R._tables(256, np.uint8, False, seed=3)
    flat = g_raw.copy()
    flat[100] = flat[99]
    with pytest.raises(L.LdsoError, match="strictly increasing"):
        tracker.make_photometric(flat, v)
    with pytest.raises(ValueError, match="strictly increasing"):
        R.make_photometric(flat, v)
    with pytest.raises(L.LdsoError, match="at least 256"):
        tracker.make_photometric(g_raw[:255], v)
    with pytest.raises(L.LdsoError, match="photometric_mode"):
        tracker.make_photometric(g_raw, v, 3)


W_ORG, H_ORG, W, H = 40, 30, 32, 24
# the first line of a calibration text per model: absolute pixels, and the relative format for two of them
PARS = {
    "fov": [0.535, 0.669, 0.493, 0.500, 0.897],  # relative
    "radtan": [33.1, 33.4, 19.2, 14.6, -0.28, 0.07, 0.0002, 0.00002],
    "equidistant": [0.48, 0.64, 0.49, 0.51, -0.013, 0.02, -0.012, 0.002],  # relative
    "kannala_brandt": [24.0, 24.3, 19.6, 14.8, -0.02, 0.01, -0.004, 0.0005],
    "pinhole": [35.0, 35.5, 19.4, 14.7, 0.0],
}
OUT_K = (0.8, 1.0, 0.5, 0.5)  # the third line: a field of view that leaves the source at the corners only
REMAP_CASES = [(m, o) for m in R.MODELS for o in ("crop", OUT_K)] + [("pinhole", "none")]


@pytest.mark.parametrize("model, out", REMAP_CASES, ids=lambda v: v if isinstance(v, str) else "calib")
def test_make_remap(built, model, out):
    from ldso_amd import tracker

    w, h = (W_ORG, H_ORG) if out == "none" else (W, H)
    K, rx, ry, pt = tracker.make_remap(model, PARS[model], W_ORG, H_ORG, w, h, out)
    Kr, rxr, ryr, ptr = R.make_remap(model, PARS[model], W_ORG, H_ORG, w, h, out)
    assert K.tobytes() == np.asarray(Kr, np.float64).tobytes(), (K, Kr)
    assert np.array_equal(bits(rx), bits(rxr)) and np.array_equal(bits(ry), bits(ryr))
    assert pt == ptr == (out == "none")
    valid = rx >= 0
    print(model, out, "K", K, "valid", valid.mean())
    assert valid.mean() > 0.5  # the comparison is not one of -1 tables
    assert ((rx[valid] > 0) & (rx[valid] < W_ORG - 1) & (ry[valid] > 0) & (ry[valid] < W_ORG - 1)).all()
    if model != "pinhole":  # a distorted grid: the rows of the table are not straight lines
        assert np.unique(ry.reshape(h, w)[h // 4][valid.reshape(h, w)[h // 4]]).size > 1


def test_make_remap_refusals(built):
    from ldso_amd import tracker

    with pytest.raises(L.LdsoError, match="full"):
        tracker.make_remap("pinhole", PARS["pinhole"], W_ORG, H_ORG, W, H, "full")
    with pytest.raises(L.LdsoError, match="dimensions to match"):
        tracker.make_remap("pinhole", PARS["pinhole"], W_ORG, H_ORG, W, H, "none")
    with pytest.raises(L.LdsoError, match="2 x 2"):
        tracker.make_remap("pinhole", PARS["pinhole"], W_ORG, H_ORG, 1, H, "crop")
    lib = L.lib()
    assert lib.ldso_ct_undistort_make_remap(7, None, 4, 4, 4, 4, 0, None, None, None, None, None) < 0
    assert b"null argument" in lib.ldso_ba_last_error()


# ---- the GPU cases are well posed ---------------------------------------------------------------
@pytest.mark.parametrize("w, h", R.SIZES)
def test_seeded_remap_is_well_posed(w, h):
    w_org, h_org = R.SRC
    assert h_org < w_org and w_org % 2 == 1 and w_org % 64 and h_org % 64
    rx, ry, kinds = R.remap(w, h)
    fx, fy, outside = R.footprint(rx, ry, w_org, h_org)
    valid = fx >= 0
    assert valid.mean() >= 0.6
    assert (rx[kinds["minus_one"]] == -1).all() and kinds["minus_one"].size > 0
    ii = kinds["integer"]
    assert ii.size and (rx[ii] == np.floor(rx[ii])).all() and (ry[ii] == np.floor(ry[ii])).all() and valid[ii].all()
    assert (rx[kinds["right_edge"]] == f32(w_org - 1.001)).all() and valid[kinds["right_edge"]].all()
    assert (ry[kinds["bottom_edge"]] == f32(h_org - 1.001)).all() and valid[kinds["bottom_edge"]].all()
    bs = kinds["below_source"]
    # entries the reference's test (iy < wOrg - 1) keeps: they must come out 0 and be counted
    assert ((ry[bs] >= h_org - 1) & (ry[bs] < w_org - 1) & (rx[bs] > 0) & (rx[bs] < w_org - 1)).all()
    assert (ry[bs] == h_org - 1).any()
    rejected = np.concatenate([bs, kinds["last_column"], kinds["not_finite"]])
    assert not valid[rejected].any() and outside == rejected.size
    # the planted entries are the only ones the rule touches
    untouched = np.ones(rx.size, bool)
    untouched[rejected] = False
    assert np.array_equal(bits(fx[untouched]), bits(rx[untouched]))
    # nothing valid reads outside the source
    xi, yi = fx[valid].astype(int), fy[valid].astype(int)
    assert xi.min() >= 0 and yi.min() >= 0 and (xi + 1).max() <= w_org - 1 and (yi + 1).max() <= h_org - 1
    assert (xi + 1).max() == w_org - 1 and (yi + 1).max() == h_org - 1  # and the last row and column are read


@pytest.mark.parametrize("w, h", R.SIZES)
def test_cases_are_well_posed(w, h):
    rx, ry, kinds = R.remap(w, h)
    for name in R.CASES:
        c = R.case(name, w, h)
        img, e, outside = R.expected(name, w, h)
        assert img.shape == (h, w) and img.dtype == f32
        if c.init["remap"] is not None:
            assert outside == 14 and (img.ravel()[kinds["below_source"]] == 0).all()
            assert (img.ravel()[kinds["minus_one"]] == 0).all()
        assert (img != 0).mean() > 0.6
        assert (name in R.NAN_FREE) <= bool(np.isfinite(img).all())
    # case 1: NaN from 0 * inf under a zero raw value, inf under a non-zero one
    img = R.expected("u8_mode2", w, h)[0].ravel()
    assert np.isnan(img[kinds["at_nan_pixel"]]).all() and np.isposinf(img[kinds["at_inf_pixel"]]).all()
    assert R.case("u8_mode2", w, h).init["g"].size == 256 and R.case("u16_mode2", w, h).init["g"].size == 65536
    assert R.case("u16_mode2", w, h).raw.max() > 60000
    # case 3: the three ways into the first branch scale the raw value
    for name in ("mode0_factor", "exposure0_factor", "no_g_factor"):
        c = R.case(name, w, h)
        ii = kinds["integer"][0]
        src = int(rx[ii]) + int(ry[ii]) * R.SRC[0]
        assert R.expected(name, w, h)[0].ravel()[ii] == f32(0.5) * f32(c.raw[src])
    assert R.case("no_g_factor", w, h).init["g"] is None
    # case 4
    assert R.expected("no_use_exposure", w, h)[1] == 1 and R.expected("u8_mode2", w, h)[1] == float(f32(0.02))
    # case 5: the inf pixel's neighbours are finite, where a blend with weights 1, 0, 0, 0 would give NaN
    img = R.expected("passthrough_inf", w, h)[0]
    x, y = R.PIX_INF
    assert np.isposinf(img[y, x]) and np.isinf(img).sum() == 1 and not np.isnan(img).any()
