"""NumPy restatement of frame ingestion from the raw image: PhotometricUndistorter's tables and
processFrame (Undistort.cc:86-154, 190-230), Undistort::undistort's remap loop and passthrough copy
(:398-453), readFromFile's numeric part (:738-751, 802-868), makeOptimalK_crop (:558-668) and the five
models' distortCoordinates (:891-1125), with the footprint rule of include/ldso_ct.h.

Every step is written with its type: np.float32 arrays and scalars round as the reference's float
statements do, a step the reference lifts to double by a double literal is an explicit float64 step
rounded back once.  tanf / atanf / atan2f / sqrtf are the C library's, called through ctypes, so the host
helpers of libldso_ba.so can be compared bit for bit.  Nothing here reads the reference tree or the
library under test.

Also the seeded inputs of tests/test_undistort.py (remap, CASES, case), which test_undistort_ref.py
shows to be well posed on the CPU."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np

f32, f64 = np.float32, np.float64
MODELS = ("fov", "radtan", "equidistant", "kannala_brandt", "pinhole")

_libm = ctypes.CDLL("libm.so.6")
for _n, _k in (("tanf", 1), ("atanf", 1), ("sqrtf", 1), ("atan2f", 2)):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * _k


def _map(fn, *arrs):
    """A libm float function over float32 arrays, element by element."""
    arrs = np.broadcast_arrays(*[np.asarray(a, f32) for a in arrs])
    out = np.fromiter((fn(*v) for v in zip(*[a.ravel().tolist() for a in arrs])), f32, arrs[0].size)
    return out.reshape(arrs[0].shape)


def tanf(a):
    return _map(_libm.tanf, a)


def atanf(a):
    return _map(_libm.atanf, a)


def sqrtf(a):
    return _map(_libm.sqrtf, a)


def atan2f(a, b):
    return _map(_libm.atan2f, a, b)


# ---- distortCoordinates (Undistort.cc:891-1125) -------------------------------------------------
def distort(model, pars, K, xs, ys):
    """pars: parsOrg (float64), K: {fx, fy, cx, cy} of the output K (float64); xs, ys float32 -> float32."""
    xs, ys = np.asarray(xs, f32), np.asarray(ys, f32)
    fx, fy, cx, cy = (f32(pars[i]) for i in range(4))
    ofx, ofy, ocx, ocy = (f32(k) for k in K)
    c = [f32(pars[i]) for i in range(4, 8)]
    ix = (xs - ocx) / ofx
    iy = (ys - ocy) / ofy
    with np.errstate(all="ignore"):
        if model == "fov":
            dist = c[0]
            d2t = f32(2) * f32(tanf(dist / f32(2)))
            r = sqrtf(ix * ix + iy * iy)
            fac = np.where((r == 0) | (dist == 0), f32(1), atanf(r * d2t) / (dist * r)).astype(f32)
            return fx * fac * ix + cx, fy * fac * iy + cy
        if model == "radtan":
            k1, k2, r1, r2 = c
            mx2, my2, mxy = ix * ix, iy * iy, ix * iy
            rho2 = mx2 + my2
            rad = k1 * rho2 + k2 * rho2 * rho2
            d = lambda a: np.asarray(a, f64)  # noqa: E731
            xd = ((d(ix + ix * rad) + (2.0 * d(r1)) * d(mxy)) + d(r2) * (d(rho2) + 2.0 * d(mx2))).astype(f32)
            yd = ((d(iy + iy * rad) + (2.0 * d(r2)) * d(mxy)) + d(r1) * (d(rho2) + 2.0 * d(my2))).astype(f32)
            return fx * xd + cx, fy * yd + cy
        if model == "equidistant":
            k1, k2, k3, k4 = c
            r = sqrtf(ix * ix + iy * iy)
            theta = atanf(r)
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            thetad = theta * (f32(1) + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8)
            scaling = np.where(r.astype(f64) > 1e-8, thetad / r, f32(1)).astype(f32)
            return fx * ix * scaling + cx, fy * iy * scaling + cy
        if model == "kannala_brandt":
            k0, k1, k2, k3 = c
            rr = sqrtf(ix * ix + iy * iy)
            theta = atan2f(rr, f32(1))
            t2 = theta * theta
            t3 = t2 * theta
            t5 = t3 * t2
            t7 = t5 * t2
            t9 = t7 * t2
            r = theta + k0 * t3 + k1 * t5 + k2 * t7 + k3 * t9
            small = rr.astype(f64) < 1e-6
            return (np.where(small, fx * ix + cx, (r / rr) * fx * ix + cx).astype(f32),
                    np.where(small, fy * iy + cy, (r / rr) * fy * iy + cy).astype(f32))
        assert model == "pinhole"
        return fx * ix + cx, fy * iy + cy


# ---- makeOptimalK_crop (Undistort.cc:558-668) ---------------------------------------------------
def optimal_k_crop(model, pars, w_org, h_org, w, h):
    ident = np.array([1.0, 1.0, 0.0, 0.0])
    line = (np.arange(100000).astype(f32) - f32(50000)) / f32(10000)
    zero = np.zeros(100000, f32)

    def span(vals, bound):
        hit = line[(vals > 0) & (vals < f32(bound))]
        nz = hit[hit != 0]  # `if (min == 0) min = ...` takes the first hit that is not 0
        return (nz[0] if nz.size else f32(0)), (hit[-1] if hit.size else f32(0))

    minX, maxX = span(distort(model, pars, ident, line, zero)[0], w_org - 1)
    minY, maxY = span(distort(model, pars, ident, zero, line)[1], h_org - 1)
    minX, maxX, minY, maxY = (f32(f64(v) * 1.01) for v in (minX, maxX, minY, maxY))
    yv, xv = np.arange(h).astype(f32), np.arange(w).astype(f32)
    rounds = 0
    while True:
        ys = minY + (maxY - minY) * yv / (f32(h) - f32(1))
        inside = lambda v, bound: (v > 0) & (v < f32(bound))  # noqa: E731
        left = not inside(distort(model, pars, ident, np.full(h, minX, f32), ys)[0], w_org - 1).all()
        right = not inside(distort(model, pars, ident, np.full(h, maxX, f32), ys)[0], w_org - 1).all()
        xs = minX + (maxX - minX) * xv / (f32(w) - f32(1))
        top = not inside(distort(model, pars, ident, xs, np.full(w, minY, f32))[1], h_org - 1).all()
        bottom = not inside(distort(model, pars, ident, xs, np.full(w, maxY, f32))[1], h_org - 1).all()
        if (left or right) and (top or bottom):
            if (maxX - minX) > (maxY - minY):
                top = bottom = False
            else:
                left = right = False
        if left:
            minX = f32(f64(minX) * 0.995)
        if right:
            maxX = f32(f64(maxX) * 0.995)
        if top:
            minY = f32(f64(minY) * 0.995)
        if bottom:
            maxY = f32(f64(maxY) * 0.995)
        rounds += 1
        if rounds > 500:
            raise ValueError("no camera matrix within 500 rounds")
        if not (left or right or top or bottom):
            break
    K00 = f64((f32(w) - f32(1)) / (maxX - minX))
    K11 = f64((f32(h) - f32(1)) / (maxY - minY))
    return np.array([K00, K11, f64(-minX) * K00, f64(-minY) * K11])


# ---- readFromFile's numeric part (Undistort.cc:738-751, 802-868) --------------------------------
def make_remap(model, pars, w_org, h_org, w, h, out="crop"):
    """-> (K {fx, fy, cx, cy} float64, remap_x [h*w], remap_y [h*w], passthrough)"""
    p = np.zeros(8, f64)
    p[:len(pars)] = np.asarray(pars, f64)
    if model in ("fov", "pinhole"):
        p[5:] = 0
    if p[2] < 1 and p[3] < 1:  # the relative format
        p[0], p[1], p[2], p[3] = p[0] * w_org, p[1] * h_org, p[2] * w_org - 0.5, p[3] * h_org - 0.5
    passthrough = False
    if isinstance(out, str) and out == "crop":
        K = optimal_k_crop(model, p, w_org, h_org, w, h)
    elif isinstance(out, str) and out == "none":
        assert (w, h) == (w_org, h_org)
        K, passthrough = p[:4].copy(), True
    else:
        oc = np.asarray(out, f32)
        K = np.array([f64(oc[0] * f32(w)), f64(oc[1] * f32(h)), f64(oc[2] * f32(w)) - 0.5, f64(oc[3] * f32(h)) - 0.5])
    gy, gx = np.mgrid[0:h, 0:w]
    ix, iy = distort(model, p, K, gx.ravel().astype(f32), gy.ravel().astype(f32))
    ix, iy = ix.astype(f32).copy(), iy.astype(f32).copy()
    # "make rounding resistant", statement by statement: the fourth sets ix, the last bound is wOrg's
    ix[ix == 0] = f32(0.001)
    iy[iy == 0] = f32(0.001)
    ix[ix == f32(w_org - 1)] = f32(w_org - 1.001)
    ix[iy == f32(h_org - 1)] = f32(h_org - 1.001)
    ok = (ix > 0) & (iy > 0) & (ix < f32(w_org - 1)) & (iy < f32(w_org - 1))
    return K, np.where(ok, ix, f32(-1)).astype(f32), np.where(ok, iy, f32(-1)).astype(f32), passthrough


# ---- PhotometricUndistorter's tables (Undistort.cc:86-103, 120-154) -----------------------------
def make_photometric(g_raw, vignette, photometric_mode=2):
    """-> (G [g_depth], vignetteMapInv shaped as vignette); ValueError where the reference gives up."""
    G = np.asarray(g_raw, f32).ravel()
    if G.size < 256:
        raise ValueError("fewer than 256 entries")
    if (G[1:] <= G[:-1]).any():
        raise ValueError("G has to be strictly increasing")
    mn, mx = G[0], G[-1]
    g = (255.0 * (G - mn).astype(f64) / f64(mx - mn)).astype(f32)
    if photometric_mode == 0:
        g = f32(255) * np.arange(G.size).astype(f32) / f32(G.size - 1)
    v = np.asarray(vignette)
    assert v.dtype in (np.uint8, np.uint16)
    with np.errstate(all="ignore"):
        vmap = v.astype(f32) / f32(v.max())
        return g, f32(1) / vmap


# ---- the footprint rule (include/ldso_ct.h) -----------------------------------------------------
def footprint(remap_x, remap_y, w_org, h_org):
    """-> (remap_x, remap_y, count): an entry that is not finite, or whose 2 x 2 footprint is not inside the
    source, becomes (-1, -1) and is counted; one with xx < 0 is the reference's own mark and is kept."""
    rx, ry = np.asarray(remap_x, f32).ravel().copy(), np.asarray(remap_y, f32).ravel().copy()
    with np.errstate(invalid="ignore"):
        keep = rx < 0
        fin = np.isfinite(rx) & np.isfinite(ry) & (rx < f32(w_org)) & (ry > f32(-1)) & (ry < f32(h_org)) & ~keep
    xi = np.where(fin, rx, 0).astype(np.int64)  # truncation, as (int)xx
    yi = np.where(fin, ry, 0).astype(np.int64)
    inside = fin & (xi + 1 <= w_org - 1) & (yi >= 0) & (yi + 1 <= h_org - 1)
    bad = ~keep & ~inside
    rx[bad] = -1
    ry[bad] = -1
    return rx, ry, int(bad.sum())


# ---- processFrame and undistort (Undistort.cc:190-230, 398-453) ---------------------------------
def photometric(raw, g, vignette_inv, photometric_mode, use_exposure, exposure, factor):
    """-> (the photometric image [n_org] float32, ImageAndExposure::exposure_time)"""
    raw = np.asarray(raw).ravel()
    assert raw.dtype in (np.uint8, np.uint16)
    exposure = f32(exposure)
    if g is None or exposure <= 0 or photometric_mode == 0:
        data = f32(factor) * raw.astype(f32)
    else:
        data = np.asarray(g, f32)[raw]
        if photometric_mode == 2:
            with np.errstate(invalid="ignore"):
                data = data * np.asarray(vignette_inv, f32).ravel()
    return data.astype(f32), (exposure if use_exposure else f32(1))


def undistort(raw, w_org, h_org, w, h, remap=None, g=None, vignette_inv=None, photometric_mode=2, use_exposure=True,
              exposure=1.0, factor=1.0):
    """-> (image [h, w] float32, exposure_time, entries the footprint rule rejected)"""
    data, exp_out = photometric(raw, g, vignette_inv, photometric_mode, use_exposure, exposure, factor)
    assert data.size == w_org * h_org
    if remap is None:  # passthrough: a copy
        assert (w, h) == (w_org, h_org)
        return data.reshape(h, w).copy(), exp_out, 0
    rx, ry, outside = footprint(remap[0], remap[1], w_org, h_org)
    assert rx.size == ry.size == w * h
    valid = ~(rx < 0)
    xi, yi = np.where(valid, rx, 0).astype(np.int64), np.where(valid, ry, 0).astype(np.int64)
    xx = np.where(valid, rx, 0).astype(f32) - xi.astype(f32)
    yy = np.where(valid, ry, 0).astype(f32) - yi.astype(f32)
    xxyy = xx * yy
    s = xi + yi * w_org
    with np.errstate(invalid="ignore"):
        out = (xxyy * data[s + 1 + w_org] + (yy - xxyy) * data[s + w_org] + (xx - xxyy) * data[s + 1]
               + (f32(1) - xx - yy + xxyy) * data[s])
    assert out.dtype == f32
    return np.where(valid, out, f32(0)).astype(f32).reshape(h, w), exp_out, outside


# ---- the seeded inputs of the GPU tests ---------------------------------------------------------
SRC = (83, 61)  # w_org, h_org: odd, no multiple of 64, and h_org < w_org, so the footprint rule fires
SIZES = ((64, 48), (160, 120))  # one pyramid level, two levels
PIX_NAN, PIX_INF = (20, 30), (50, 11)  # source pixels (x, y) under a zero vignette: raw 0 there, raw 77 there


@functools.lru_cache(maxsize=None)
def remap(w, h, w_org=SRC[0], h_org=SRC[1], seed=1):
    """A seeded remap of w x h output pixels into the w_org x h_org source: uniform inside the reference's
    bounds, then planted entries of every kind the kernel and the footprint rule tell apart.  Returns
    (remap_x, remap_y, kinds): kinds maps a name to the planted indices."""
    rng = np.random.default_rng(seed)
    n = w * h
    rx = rng.uniform(0.001, w_org - 1.001, n).astype(f32)
    ry = rng.uniform(0.001, h_org - 1.001, n).astype(f32)
    idx = rng.permutation(n)
    kinds, at = {}, 0

    def plant(name, k, xs, ys):
        nonlocal at
        ii = idx[at:at + k]
        at += k
        rx[ii], ry[ii] = np.asarray(xs, f32), np.asarray(ys, f32)
        kinds[name] = ii

    k = n // 8
    plant("minus_one", k, -1, -1)
    plant("integer", 16, rng.integers(1, w_org - 2, 16), rng.integers(1, h_org - 2, 16))
    plant("at_nan_pixel", 1, PIX_NAN[0], PIX_NAN[1])
    plant("at_inf_pixel", 1, PIX_INF[0], PIX_INF[1])
    plant("right_edge", 4, f32(w_org - 1.001), rng.uniform(1, h_org - 2, 4))
    plant("bottom_edge", 4, rng.uniform(1, w_org - 2, 4), f32(h_org - 1.001))
    # what the reference keeps (iy < wOrg - 1) and would read past the source
    plant("below_source", 8, rng.uniform(1, w_org - 2, 8),
          np.concatenate([[h_org - 1, w_org - 1.5], rng.uniform(h_org - 1, w_org - 1.001, 6)]))
    plant("last_column", 2, w_org - 1, rng.uniform(1, h_org - 2, 2))
    plant("not_finite", 4, [np.nan, np.inf, 5.5, 7.25], [3.5, 4.5, np.nan, np.inf])
    for a in (rx, ry):
        a.setflags(write=False)
    return rx, ry, kinds


def _tables(depth, vignette_dtype, zeros, seed):
    """A strictly increasing response of `depth` entries and a vignette over SRC through make_photometric's
    restatement; zeros: the vignette is 0 at PIX_NAN and PIX_INF."""
    rng = np.random.default_rng(seed)
    g_raw = np.cumsum(rng.uniform(0.2, 1.8, depth)).astype(f32)
    top = np.iinfo(vignette_dtype).max
    v = rng.integers(top // 3, top + 1, SRC[0] * SRC[1]).astype(vignette_dtype)
    if zeros:
        for x, y in (PIX_NAN, PIX_INF):
            v[x + y * SRC[0]] = 0
    return g_raw, v


def _raw(dtype, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, n).astype(dtype)


# name -> (raw type, LUT depth or None, vignette zeros, mode, use_exposure, exposure, factor, passthrough)
CASES = {
    "u8_mode2": (np.uint8, 256, True, 2, True, 0.02, 1.0, False),
    "u16_mode2": (np.uint16, 65536, False, 2, True, 0.02, 1.0, False),
    "u8_mode1": (np.uint8, 256, False, 1, True, 0.02, 1.0, False),
    "mode0_factor": (np.uint8, 256, True, 0, True, 0.02, 0.5, False),
    "exposure0_factor": (np.uint8, 256, True, 2, True, 0.0, 0.5, False),
    "no_g_factor": (np.uint16, None, False, 2, True, 0.02, 0.5, False),
    "no_use_exposure": (np.uint8, 256, False, 2, False, 0.02, 1.0, False),
    "passthrough_inf": (np.uint8, 256, True, 2, True, 0.02, 1.0, True),
}
NAN_FREE = ("u16_mode2", "u8_mode1")  # finite images: the pyramid and tracking comparisons


@functools.lru_cache(maxsize=None)
def case(name, w, h):
    """The inputs of one case at context size w x h: raw, the keywords of CoarseTracker.undistort_init
    (init) and the frame's exposure and factor."""
    dtype, depth, zeros, mode, use_exposure, exposure, factor, passthrough = CASES[name]
    seed = 100 + sorted(CASES).index(name)
    w_org, h_org = (w, h) if passthrough else SRC
    raw = _raw(dtype, w_org * h_org, seed)
    g = vinv = None
    if depth is not None:
        g_raw, v = _tables(depth, np.uint16 if dtype == np.uint16 else np.uint8, zeros, seed + 50)
        if passthrough:  # a vignette of the context's size: one zero under a raw 77, its neighbours untouched
            v = np.resize(v, w_org * h_org).copy()
            v[v == 0] = 1
            v[PIX_INF[0] + PIX_INF[1] * w_org] = 0
        g, vinv = make_photometric(g_raw, v, mode)
    if zeros:
        raw[PIX_NAN[0] + PIX_NAN[1] * w_org] = 0
        raw[PIX_INF[0] + PIX_INF[1] * w_org] = 77
    raw.setflags(write=False)
    rm = None if passthrough else remap(w, h)[:2]
    init = dict(w_org=w_org, h_org=h_org, remap=rm, g=g, vignette_inv=vinv, photometric_mode=mode,
                use_exposure=use_exposure)
    return SimpleNamespace(name=name, w=w, h=h, raw=raw, init=init, exposure=exposure, factor=factor)


@functools.lru_cache(maxsize=None)
def expected(name, w, h):
    """The restatement's (image, exposure_time, rejected entries) of a case; computed once, left unchanged."""
    c = case(name, w, h)
    img, e, outside = undistort(c.raw, w=w, h=h, exposure=c.exposure, factor=c.factor, **c.init)
    img.setflags(write=False)
    return img, float(e), outside
