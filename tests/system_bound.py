"""Elementwise, rounding-bounded comparison of the stitched system HA, bA, Hsc, bsc.

dense_bound() rebuilds the window's normal equations in float64 from the oracle's per-residual
Jacobians (D), the same sums over the absolute values of every factor (B) and the number of
per-pixel addends behind every element (cnt).  A float-accumulated system S of the same addends
satisfies |S - D| <= r u B elementwise with u = 2^-24 and r of a few units, whatever the order of
the sums; the per-block Frobenius bar (test_gpu_parity.BLOCK_TOL = 1e-4) lets a small element or a
uniform low-order error pass that this does not.  assert_elementwise() applies two tiers:

  1. a priori: |G - D| <= (cnt + 16) u B, and G == 0 wherever B == 0.  Any order of cnt float
     addends errs by at most (cnt - 1) u sum|t|; the 16 covers the roundings in forming one addend
     (the two-term gradient products, the pre-sum over 8 pattern pixels, the product itself).  The
     adjoints are applied in double on both sides.  A violation is a wrong, missing or duplicated
     addend, never rounding.
  2. calibrated: the largest ratio |G - D| / (u B) of each quantity is at most 4 max(r_ref, 2),
     r_ref being the largest of the oracle's own four ratios on the same window.  The oracle's ratio
     ranges from 1.7 to 5.4 over windows of 200 to 1,700 residuals, and the device adds the same
     float addends in another order: a legitimate difference is of that size.  The floor is 8, one
     residual's eight addends.

The rebuild is vectorised per (host, target) bucket (numpy, no loop over pixels or residuals) and
cached by the content of its inputs.  On synth.S7 (12,000 residuals, 11,080 active) it takes 0.10 s
on one core and 0.008 s from the cache; on synth.S11 (67,524 active) 0.68 s and 0.06 s.  That is not
small against the oracle's own iteration() there (compiled code: 0.016 s on S7, 0.11 s on S11), but
below what a test spends on making the window (synth.make_window: 0.14 s on S7) and 500 times
faster per residual than the loop in test_oracle_kat.dense_system (0.74 s for 1,704 residuals).
"""
import hashlib

import numpy as np

U = 2.0 ** -24
KEYS = ("HA", "bA", "Hsc", "bsc")
ADDEND_ROUNDINGS = 16   # tier 1: roundings in forming one addend
REF_FACTOR = 4.0        # tier 2: device ratio <= REF_FACTOR * max(r_ref, REF_FLOOR)
REF_FLOOR = 2.0

J_OFF = dict(resF=0, Jpdxi=8, Jpdc=20, Jpdd=28, JIdx=30, JabF=46, JIdx2=62, JabJIdx=66, Jab2=70)


def unpack_J(row):
    return dict(resF=row[0:8], Jpdxi=row[8:20].reshape(2, 6), Jpdc=row[20:28].reshape(2, 4), Jpdd=row[28:30],
                JIdx=row[30:46].reshape(2, 8), JabF=row[46:62].reshape(2, 8))


def _rows(J, adH, adT, absolute):
    """Per residual and pattern pixel of one (host, target) bucket: the row's calib, host and target
    parts side by side [n, 8, 20], d r / d idepth [n, 8] and the residual [n, 8] (absolute: every
    factor's absolute value).  adH, adT: the bucket's 8 x 8 adjoints."""
    f = np.abs if absolute else (lambda x: x)
    n = J.shape[0]
    g = f(J[:, 30:46].reshape(n, 2, 8))                                # [n, 2, pixel]
    gx, gy = g[:, 0, :, None], g[:, 1, :, None]
    geo = f(J[:, 8:30].reshape(n, 1, 22))                              # Jpdxi[0], Jpdxi[1], Jpdc[0], Jpdc[1], Jpdd
    jrel = np.empty((n, 8, 8))
    jrel[:, :, :6] = gx * geo[:, :, 0:6] + gy * geo[:, :, 6:12]
    jrel[:, :, 6:] = f(J[:, 46:62].reshape(n, 2, 8)).transpose(0, 2, 1)
    row = np.empty((n, 8, 20))
    row[:, :, :4] = gx * geo[:, :, 12:16] + gy * geo[:, :, 16:20]
    row[:, :, 4:12] = (jrel.reshape(-1, 8) @ f(adH).T).reshape(n, 8, 8)
    row[:, :, 12:] = (jrel.reshape(-1, 8) @ f(adT).T).reshape(n, 8, 8)
    jd = gx[:, :, 0] * geo[:, :, 20] + gy[:, :, 0] * geo[:, :, 21]
    return row, jd, f(J[:, 0:8])


def _compute(w, J, flags, hdi, skip, jab_lin=None):
    N, D, P = w.n_frames, w.dim, w.n_points
    J = np.asarray(J, np.float64)
    # with a fixed affine mode linearize zeroes JabF after JabJIdx and Jab2 are summed: the H terms and
    # the Schur rows hold the unzeroed affine Jacobians (J), bA's products with the residual the zeroed ones (Jb)
    Jb = J
    if jab_lin is not None and not np.array_equal(J[:, 46:62], jab_lin):
        J = J.copy()
        J[:, 46:62] = jab_lin
    begin = np.asarray(w.point_res_begin, np.int64)
    pt = np.repeat(np.arange(P), np.diff(begin))
    act = (np.asarray(flags) & 1).astype(bool)
    if skip is not None:
        act = act.copy()
        act[skip] = False
    host = np.asarray(w.point_host, np.int64)[pt]
    tgt = np.asarray(w.res_target, np.int64)
    adH = np.asarray(w.ad_host, np.float64).reshape(-1, 8, 8)
    adT = np.asarray(w.ad_target, np.float64).reshape(-1, 8, 8)

    Dm = dict(HA=np.zeros((D, D)), bA=np.zeros(D))
    Bm = dict(HA=np.zeros((D, D)), bA=np.zeros(D))
    cnt = dict(HA=np.zeros((D, D)), bA=np.zeros(D))
    # per point: the coupling row sum_pixels row * jd, its absolute twin, the addend counts
    hpd, hpd_abs, hpd_cnt = np.zeros((P, D)), np.zeros((P, D)), np.zeros((P, D))
    hdd, bd, bd_abs, bd_cnt = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)

    pair = host + N * tgt
    for k in np.unique(pair[act]):
        sel = np.flatnonzero(act & (pair == k))
        h, t = int(k % N), int(k // N)
        idx = np.concatenate([np.arange(4), 4 + 8 * h + np.arange(8), 4 + 8 * t + np.arange(8)])
        n = len(sel)
        rows = lambda Jk, absolute: _rows(Jk, adH[k], adT[k], absolute)
        (row, jd, r), (rowa, jda, ra) = rows(J[sel], False), rows(J[sel], True)
        nz = (rowa > 0).astype(np.float64)
        ix = np.ix_(idx, idx)
        r2, ra2, nz2 = row.reshape(-1, 20), rowa.reshape(-1, 20), nz.reshape(-1, 20)
        rb2, rba2, nzb2 = r2, ra2, nz2   # the rows of bA
        if Jb is not J:
            rb2, rba2 = rows(Jb[sel], False)[0].reshape(-1, 20), rows(Jb[sel], True)[0].reshape(-1, 20)
            nzb2 = (rba2 > 0).astype(np.float64)
        # np.add.at: host == target would repeat indices
        np.add.at(Dm["HA"], ix, r2.T @ r2)
        np.add.at(Bm["HA"], ix, ra2.T @ ra2)
        np.add.at(cnt["HA"], ix, nz2.T @ nz2)
        np.add.at(Dm["bA"], idx, rb2.T @ r.reshape(-1))
        np.add.at(Bm["bA"], idx, rba2.T @ ra.reshape(-1))
        np.add.at(cnt["bA"], idx, nzb2.T @ (ra.reshape(-1) > 0).astype(np.float64))
        pi = (pt[sel][:, None], idx[None, :])
        np.add.at(hpd, pi, (row * jd[:, :, None]).sum(1))
        np.add.at(hpd_abs, pi, (rowa * jda[:, :, None]).sum(1))
        np.add.at(hpd_cnt, pi, (nz * (jda > 0)[:, :, None]).sum(1))
        np.add.at(hdd, pt[sel], (jd * jd).sum(1))
        np.add.at(bd, pt[sel], (jd * r).sum(1))
        np.add.at(bd_abs, pt[sel], (jda * ra).sum(1))
        np.add.at(bd_cnt, pt[sel], (jda * ra > 0).sum(1))

    if hdi is None:
        wgt = np.where(hdd > 0, 1.0 / np.where(hdd > 0, hdd, 1.0), 0.0)
    else:
        # scAddPoint(shiftPriorToZero = true): bdSumF = bd + priorF * deltaF, HdiF = 1 / (Hdd + priorF)
        wgt = np.asarray(hdi, np.float64)
        pd = np.asarray(w.point_data, np.float64)
        prior = pd[:, 4] * pd[:, 5]
        bd = bd + prior
        bd_abs = bd_abs + np.abs(prior)
        bd_cnt = bd_cnt + (prior != 0)
    Dm["Hsc"] = (hpd * wgt[:, None]).T @ hpd
    Dm["bsc"] = hpd.T @ (bd * wgt)
    Bm["Hsc"] = (hpd_abs * wgt[:, None]).T @ hpd_abs
    Bm["bsc"] = hpd_abs.T @ (bd_abs * wgt)
    # element (i, j) of one point's term is a product of two sums: the addends of both count
    z = ((hpd_abs > 0) & (wgt > 0)[:, None]).astype(np.float64)
    c = hpd_cnt * z
    cnt["Hsc"] = c.T @ z + z.T @ c
    zb = z * (bd_abs > 0)[:, None]
    cnt["bsc"] = (c * zb).sum(0) + zb.T @ bd_cnt
    return Dm, Bm, cnt, (hpd, hdd, bd)


_CACHE = {}


def dense_bound(w, J, res, hdi=None, skip=None, jab_lin=None):
    """(D, B, cnt), each a dict over HA, bA, Hsc, bsc, for the window w after a pass: J the oracle's
    jacobians() of that pass, res its residuals() (a residual counts when flags & 1), hdi the
    per-point HdiF of that pass (None: 1 / sum jd^2, without the inverse-depth prior).
    skip: residual indices left out of the rebuild (for tests that plant a defect).
    jab_lin: the oracle's jabf_lin() of that pass, for a pass under a fixed affine mode (where J's JabF is
    zeroed after H's sums were formed from it); None: J's own.
    The results are shared through a cache keyed by the inputs' content: treat them as read-only."""
    J = np.ascontiguousarray(J)
    flags = np.ascontiguousarray(res["flags"])
    dig = hashlib.blake2b(digest_size=16)
    for a in (J, flags, w.point_res_begin, w.point_host, w.res_target, w.ad_host, w.ad_target,
              None if hdi is None else np.asarray(hdi, np.float64), None if hdi is None else w.point_data[:, 4:6],
              None if skip is None else np.asarray(skip, np.int64), jab_lin):
        dig.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
        dig.update(b"|")
    key = (w.n_frames, w.n_points, dig.digest())
    if key not in _CACHE:
        if len(_CACHE) >= 8:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = _compute(w, J, flags, hdi, skip, jab_lin)[:3]
    return _CACHE[key]


def point_terms(w, J, res):
    """Per point (h_pd [P, D], H_dd [P], b_d [P]) of the float64 rebuild (no prior)."""
    return _compute(w, J, res["flags"], None, None)[3]


def ratios(G, D, B, mirrored=False):
    """Per quantity: (largest |G - D| / (u B) over the compared elements with B > 0, largest |G| over
    those with B == 0).  The compared elements are block_errors': the upper triangle of the diagonal
    blocks and the blocks above them, i.e. the matrix's upper triangle.  mirrored: a matrix that also
    carries its lower triangle must mirror the upper one exactly (the device expands a packed upper
    triangle; the oracle's stitch sums both triangles on their own, so its lower one is only close)."""
    out = {}
    for k in KEYS:
        g, d, b = np.asarray(G[k], np.float64), D[k], B[k]
        if g.ndim == 2:
            if mirrored and np.any(np.tril(g, -1)):
                assert np.array_equal(g, g.T), f"{k}: the lower triangle does not mirror the upper one"
            m = np.triu(np.ones(g.shape, bool))
            g, d, b = g[m], d[m], b[m]
        pos = b > 0
        r = float(np.max(np.abs(g[pos] - d[pos]) / (U * b[pos]))) if pos.any() else 0.0
        z = float(np.max(np.abs(g[~pos]))) if (~pos).any() else 0.0
        out[k] = (r, z)
    return out


def tier1_violations(G, D, B, cnt):
    """Per quantity the number of compared elements outside |G - D| <= (cnt + 16) u B (which, where
    B == 0, demands G == 0), and the worst excess |G - D| / ((cnt + 16) u B) over B > 0."""
    out = {}
    for k in KEYS:
        g, d, b, c = np.asarray(G[k], np.float64), D[k], B[k], cnt[k]
        if g.ndim == 2:
            m = np.triu(np.ones(g.shape, bool))
            g, d, b, c = g[m], d[m], b[m], c[m]
        bound = (c + ADDEND_ROUNDINGS) * U * b
        err = np.abs(g - d)
        pos = b > 0
        out[k] = (int(np.sum(~(err <= bound))), float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0)
    return out


def assert_elementwise(G, O, D, B, cnt, what):
    """Both tiers for the system G beside the oracle's O and the rebuild (D, B, cnt) of the same
    pass; prints one line with G's four ratios and the oracle's."""
    rg, ro = ratios(G, D, B, mirrored=True), ratios(O, D, B)
    t1 = tier1_violations(G, D, B, cnt)
    fmt = lambda r: " ".join(f"{k}={r[k][0]:.2f}" for k in KEYS)
    print(f"elementwise ratios {what}: device {fmt(rg)} | oracle {fmt(ro)}")
    for k in KEYS:
        assert rg[k][1] == 0.0, f"{what} {k}: |G| = {rg[k][1]:.3e} where no addend reaches (B == 0)"
        assert t1[k][0] == 0, (f"{what} {k}: {t1[k][0]} elements outside (cnt + {ADDEND_ROUNDINGS}) u B, "
                               f"worst at {t1[k][1]:.3g} of the bound: a wrong, missing or duplicated addend")
    r_ref = max(ro[k][0] for k in KEYS)
    limit = REF_FACTOR * max(r_ref, REF_FLOOR)
    for k in KEYS:
        assert rg[k][0] <= limit, f"{what} {k}: ratio {rg[k][0]:.2f} above {limit:.2f} (oracle's largest {r_ref:.2f})"
    return rg, ro


def check_system(G, ow, O, what):
    """assert_elementwise for G beside the oracle window ow after its pass (O its system)."""
    D, B, cnt = dense_bound(ow.window, ow.jacobians(), ow.residuals(), ow.points()["HdiF"], jab_lin=ow.jabf_lin())
    return assert_elementwise(G, O, D, B, cnt, what)


def oracle_reference(w, passes=1):
    """(O, D, B, cnt) of the window w after `passes` passes of the oracle: for tests that compare two
    device results with each other, each of which is held against the unsharded window's rebuild."""
    import oracle

    ow = oracle.OracleWindow(w, threads=0)
    for _ in range(passes):
        _, O = ow.iteration()
    D, B, cnt = dense_bound(ow.window, ow.jacobians(), ow.residuals(), ow.points()["HdiF"], jab_lin=ow.jabf_lin())
    ow.close()
    return O, D, B, cnt
