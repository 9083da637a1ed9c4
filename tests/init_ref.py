"""CoarseInitializer::trackFrame (src/frontend/CoarseInitializer.cc:45-183), the multiThreading == false
branch, restated in numpy float32 from the reference text, statement for statement: the checker of
ldso_ct_init_track_frame / ldso_ct_init_eval / ldso_ct_init_lm_step.  It shares no code with the library.

Per-point statements are vectorised over the points (elementwise float32 operations in the reference's
order, so every per-point value is the reference's bit for bit); everything a later point reads from an
earlier one (optReg, the top level's resetPoints, propagateUp's sums) is a plain sequential loop.
Accumulator9 / Accumulator11 / AccumulatorX are restated with their SSE lanes and their shift-up rule
(`acc_sum`): after 1001 updates a lane's sum moves up, so a sum is the sequential sum of 1001-update blocks.

An evaluation also returns the float32 terms that went into each sum, from which the tests form the exact
sum and the any-order bound (n - 1) 2^-24 sum|term| in float64.

The loop runs free (its own float32 LM step, `lm_step`) or replays a device log (`forced`: the logged
pose, affine pair and increment of every evaluation), in which case every per-point value must be the
device's bit for bit and every decision is still taken from this file's own sums.

Two fixed-size Eigen reductions (doStep's dot, inc.norm()) are written in their SSE packet order, as
include/ldso_ct.h states.
"""
import math
from fractions import Fraction

import numpy as np

import track_ref as R

f32 = np.float32
PATTERN = ((0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2))  # staticPattern[8]
TRI = [(r, c) for r in range(9) for c in range(r, 9)]
TRI_R = np.array([r for r, _ in TRI])
TRI_C = np.array([c for _, c in TRI])
WM = np.array([1, 1, 1, 0.5, 0.5, 0.5, 10, 1000], f32)  # SCALE_XI_ROT x3, SCALE_XI_TRANS x3, SCALE_A, SCALE_B
DEFAULTS = dict(alpha_k=2.5 * 2.5, alpha_w=150.0 * 150.0, reg_weight=0.8, coupling_weight=1.0,
                max_iterations=(5, 5, 10, 30, 50), fix_affine=1, huber_th=9.0)
POINT_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("idepth", "<f4"), ("ir", "<f4"), ("idepth_new", "<f4"),
                        ("energy", "<f4", (2,)), ("energy_new", "<f4", (2,)), ("last_hessian", "<f4"),
                        ("last_hessian_new", "<f4"), ("maxstep", "<f4"), ("outlier_th", "<f4"), ("my_type", "<f4"),
                        ("ir_sum_num", "<f4"), ("is_good", "<i4"), ("is_good_new", "<i4"), ("parent", "<i4"),
                        ("neighbours", "<i4", (10,))])
U = 2.0 ** -24  # float32 unit roundoff


# ---- accumulators ----------------------------------------------------------------------------------
def acc_sum(terms):
    """The value an accumulator's lane holds after finish(): terms [m, ...] float32 in update order, one
    row per update; numIn1 > 1000 moves the lane's sum up after every 1001st update."""
    terms = np.asarray(terms, f32)
    total = np.zeros(terms.shape[1:], f32)
    for s in range(0, terms.shape[0], 1001):
        total = np.add.accumulate(terms[s:s + 1001], axis=0, dtype=f32)[-1] + total
    return total


def sum_bound(terms, axis=0):
    """(exact sum, any-order bound) in float64 of float32 terms along axis."""
    t = np.asarray(terms, np.float64)
    n = t.shape[axis]
    return t.sum(axis=axis), max(n - 1, 0) * U * np.abs(t).sum(axis=axis)


# ---- small exact float32 helpers ---------------------------------------------------------------------
def _round_f32(fr):
    if fr == 0:
        return f32(0)
    c = f32(float(fr))
    cands = [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))]
    return min(cands, key=lambda z: (abs(Fraction(float(z)) - fr), int(np.asarray(z, f32).view(np.uint32)) & 1))


def fmaf(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return f32(a * b + c)
    return _round_f32(Fraction(a) * Fraction(b) + Fraction(c))


def dot8(a, b):
    """Eigen's 8-float dot in SSE packet order: p_k = a_k b_k + a_(k+4) b_(k+4), (p0 + p2) + (p1 + p3)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    p = a[..., :4] * b[..., :4] + a[..., 4:8] * b[..., 4:8]
    return (p[..., 0] + p[..., 2]) + (p[..., 1] + p[..., 3])


def norm8(a):
    return np.sqrt(dot8(a, a))


def ldlt_solve_f32(A, b):
    """Eigen::LDLT<Matrix<float, n, n>, Lower> (the pivoting of ct_lm.h's ldlt_solve_small), float32."""
    n = len(b)
    a = [[f32(A[i][j]) for j in range(n)] for i in range(n)]
    perm = list(range(n))
    for k in range(n):
        piv = k
        for i in range(k + 1, n):
            if abs(a[i][i]) > abs(a[piv][piv]):
                piv = i
        if piv != k:
            perm[k], perm[piv] = perm[piv], perm[k]
            for j in range(k):
                a[k][j], a[piv][j] = a[piv][j], a[k][j]
            for i in range(k + 1, piv):
                a[i][k], a[piv][i] = a[piv][i], a[i][k]
            for i in range(piv + 1, n):
                a[i][k], a[i][piv] = a[i][piv], a[i][k]
            a[k][k], a[piv][piv] = a[piv][piv], a[k][k]
        d = a[k][k]
        rd = f32(1) / d if d != 0 else f32(0)
        col = [a[i][k] for i in range(n)]
        for i in range(k + 1, n):
            for j in range(k + 1, i + 1):
                a[i][j] = fmaf(-(col[i] * col[j]), rd, a[i][j])
            a[i][k] = col[i] / d if d != 0 else f32(0)
    y = [f32(b[perm[i]]) for i in range(n)]
    for i in range(n):
        for j in range(i):
            y[i] = fmaf(-a[i][j], y[j], y[i])
    for i in range(n):
        y[i] = y[i] / a[i][i] if a[i][i] != 0 else f32(0)
    for j in range(n - 1, -1, -1):
        for i in range(j):
            y[i] = fmaf(-a[j][i], y[j], y[i])
    x = [f32(0)] * n
    for i in range(n):
        x[perm[i]] = y[i]
    return x


def se3_log_translation(pose):
    """SE3::log(pose).head<3>() (se3.hpp:220-253 with SO3::logAndTheta, so3.hpp:239-283)."""
    (x, y, z, w), t = pose
    sq = (x * x + y * y) + z * z
    n = math.sqrt(sq)
    if n < R.EPS:
        f = 2.0 / w - (2.0 * sq) / (w * (w * w))
    elif abs(w) < R.EPS:
        f = math.pi / n if w > 0 else -math.pi / n
    else:
        f = (2.0 * math.atan(n / w)) / n
    theta = f * n
    om = (f * x, f * y, f * z)
    W = R.hat(om)
    W2 = R.mm(W, W)
    if abs(theta) < R.EPS:
        c = 1.0 / 12.0
    else:
        half = 0.5 * theta
        c = (1.0 - (theta * math.cos(half)) / (2.0 * math.sin(half))) / (theta * theta)
    Vi = [[((1.0 if i == j else 0.0) - 0.5 * W[i][j]) + c * W2[i][j] for j in range(3)] for i in range(3)]
    return R.mv(Vi, t)


def lm_step(H, b, Hsc, bsc, lam, w, h, pose, aff, fix_affine=True):
    """CoarseInitializer.cc:95-116 -> (inc [8] float32, refToNew_new (q, t), (a, b) float32)."""
    with np.errstate(all="ignore"):
        H, b, Hsc, bsc = (np.asarray(x, f32) for x in (H, b, Hsc, bsc))
        lam = f32(lam)
        dl, sl, s = f32(1) + lam, f32(1) / (f32(1) + lam), f32(0.01) / f32(w * h)
        Hl = H.copy()
        for i in range(8):
            Hl[i, i] = Hl[i, i] * dl
        Hl = Hl - Hsc * sl
        bl = b - bsc * sl
        Hl = ((WM[:, None] * Hl) * WM[None, :]) * s
        bl = (WM * bl) * s
        n = 6 if fix_affine else 8
        x = ldlt_solve_f32([[Hl[i, j] for j in range(n)] for i in range(n)], [bl[i] for i in range(n)])
        inc = np.zeros(8, f32)
        for i in range(n):
            inc[i] = -(WM[i] * x[i])
        new_pose = R.se3_mul(R.se3_exp(tuple(float(v) for v in inc[:6])), pose)
        return inc, new_pose, (f32(aff[0]) + inc[6], f32(aff[1]) + inc[7])


def inc_bound(out, lam, w, h, fix_affine=True):
    """First-order bound, in float64, of what the any-order bounds of the sums behind H, b, Hsc and bsc can
    move the increment: |d inc| <= wM |Hl^-1| (|d bl| + |d Hl| |x|), entry by entry; returns its 2-norm."""
    def full(v):
        M = np.zeros((9, 9))
        M[TRI_R, TRI_C] = v
        M[TRI_C, TRI_R] = v
        return M

    lam = float(lam)
    sl, s = 1.0 / (1.0 + lam), 0.01 / (w * h)
    B, Bsc = full(sum_bound(out["acc9_terms"])[1]), full(sum_bound(out["sc_terms"])[1])
    n = 6 if fix_affine else 8
    wm = WM.astype(np.float64)[:n]
    scale = wm[:, None] * wm[None, :] * s
    H, Hsc = np.asarray(out["H"], np.float64)[:n, :n], np.asarray(out["Hsc"], np.float64)[:n, :n]
    Hl = (H + np.diag(np.diag(H)) * lam - Hsc * sl) * scale
    bl = (np.asarray(out["b"], np.float64)[:n] - np.asarray(out["bsc"], np.float64)[:n] * sl) * wm * s
    dHl = (B[:n, :n] * (1 + lam * np.eye(n)) + Bsc[:n, :n] * sl) * scale
    dbl = (B[:n, 8] + Bsc[:n, 8] * sl) * wm * s
    inv = np.linalg.inv(Hl)
    x = inv @ bl
    return float(np.linalg.norm(wm * (np.abs(inv) @ (dbl + dHl @ np.abs(x)))))


# ---- tables ------------------------------------------------------------------------------------------
def make_k(calib, levels):
    """makeK (:811-837): fx, cx per level in double, Ki = K.inverse() (Eigen's cofactor form) in double."""
    fx0, fy0, cx0, cy0 = (float(f32(c)) for c in calib)
    out = []
    fx, fy = fx0, fy0
    for l in range(levels):
        if l:
            fx, fy = fx * 0.5, fy * 0.5
        cx = cx0 if l == 0 else (cx0 + 0.5) / (1 << l) - 0.5
        cy = cy0 if l == 0 else (cy0 + 0.5) / (1 << l) - 0.5
        invdet = 1.0 / (fy * fx)
        Ki = np.array([[fy * invdet, 0 * invdet, (0 * cy - cx * fy) * invdet],
                       [0 * invdet, fx * invdet, (cx * 0 - fx * cy) * invdet],
                       [0 * invdet, 0 * invdet, (fx * fy - 0 * 0) * invdet]])
        out.append(dict(fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), Ki=Ki))
    return out


def knn_tables(levels_uv, k=10):
    """Neighbour and parent tables by brute force (makeNN, :839-906, without the kd-tree): the k nearest
    points of the level, the point itself included as nanoflann returns it, fewer than k padded with -1;
    the parent is the nearest point of the next level to uv / 2 - 1/4.  Ties go to the lower index."""
    nbrs, parents = [], []
    for l, uv in enumerate(levels_uv):
        uv = np.asarray(uv, np.float64)
        d = ((uv[:, None, :] - uv[None, :, :]) ** 2).sum(-1)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        nb = np.full((uv.shape[0], k), -1, np.int32)
        nb[:, :order.shape[1]] = order
        nbrs.append(nb)
        if l + 1 < len(levels_uv):
            up = np.asarray(levels_uv[l + 1], np.float64)
            q = uv * 0.5 - 0.25
            parents.append(np.argmin(((q[:, None, :] - up[None, :, :]) ** 2).sum(-1), axis=1).astype(np.int32))
        else:
            parents.append(np.full(uv.shape[0], -1, np.int32))
    return nbrs, parents


def make_points(levels_uv, nbrs, parents, my_type=1.0):
    """The records setFirst leaves (:695-715) for points at the given (x + 0.1, y + 0.1) positions."""
    out = []
    for uv, nb, par in zip(levels_uv, nbrs, parents):
        p = np.zeros(len(uv), POINT_DTYPE)
        p["u"], p["v"] = np.asarray(uv, f32)[:, 0], np.asarray(uv, f32)[:, 1]
        p["idepth"] = p["ir"] = 1
        p["is_good"] = 1
        p["my_type"] = my_type
        p["outlier_th"] = f32(8) * f32(12 * 12)  # patternNum * setting_outlierTH
        p["neighbours"], p["parent"] = nb, par
        out.append(p)
    return out


def sweep_ranks(nb):
    """The number of ranks of the library's optReg sweep for a neighbour table (include/ldso_ct.h)."""
    n = nb.shape[0]
    rank = np.zeros(n, np.int64)
    for i in range(n):
        for j in nb[i]:
            if 0 <= j < i:
                rank[i] = max(rank[i], rank[j] + 1)
        for j in nb[i]:
            if j > i:
                rank[j] = max(rank[j], rank[i] + 1)
    return int(rank.max()) + 1


def _interp(plane, ix, iy, ddx, ddy, wl):
    dxdy = ddx * ddy
    bp = ix + iy * wl
    return ((dxdy * plane[bp + 1 + wl] + (ddy - dxdy) * plane[bp + wl]) + (ddx - dxdy) * plane[bp + 1]) + \
        (((f32(1) - ddx) - ddy) + dxdy) * plane[bp]


class Initializer:
    """CoarseInitializer after setFirst.  first / new frames: per level dI [wl*hl][3] float32 (makeImages)."""

    def __init__(self, width, height, calib, first_dI, first_exposure, points, **params):
        self.p = dict(DEFAULTS, **params)
        self.levels = len(points)
        self.w = [width >> l for l in range(self.levels)]
        self.h = [height >> l for l in range(self.levels)]
        self.K = make_k(calib, self.levels)
        self.first = [np.ascontiguousarray(np.asarray(d, f32)[:, 0]) for d in first_dI[:self.levels]]
        self.first_exposure = f32(first_exposure)
        self.pts = [np.array(p, POINT_DTYPE) for p in points]
        nmax = max(p.size for p in self.pts)
        self.jb = np.zeros((nmax, 10), f32)
        self.jb_new = np.zeros((nmax, 10), f32)
        self.T = np.eye(4)[:3].copy()  # thisToNext = SE3(), as matrix3x4()
        self.aff = (f32(0), f32(0))
        self.snapped, self.frame_id, self.snapped_at = False, 0, 0
        # (kind, margin, bound) of every decision taken from a sum: the distance of the compared quantities and
        # what the any-order bounds of the sums behind them can move it (inc_norm: free runs only)
        self.margins = []

    # -- calcResAndGS (:186-342) --
    def calc_res_and_gs(self, lvl, T, aff, new_dI):
        p, pts, K = self.p, self.pts[lvl], self.K[lvl]
        n, wl, hl = pts.size, self.w[lvl], self.h[lvl]
        T = np.asarray(T, np.float64)
        Ki = K["Ki"]
        RKi = np.array([[(T[i, 0] * Ki[0, j] + T[i, 1] * Ki[1, j]) + T[i, 2] * Ki[2, j] for j in range(3)]
                        for i in range(3)]).astype(f32)
        t = T[:, 3].astype(f32)
        r2a, r2b = f32(math.exp(float(f32(aff[0])))), f32(aff[1])
        fxl, fyl, cxl, cyl = K["fx"], K["fy"], K["cx"], K["cy"]
        hub = f32(p["huber_th"])
        In, gx, gy = (np.ascontiguousarray(np.asarray(new_dI, f32)[:, k]) for k in range(3))
        Ir = self.first[lvl]
        with np.errstate(all="ignore"):
            # calculateAllResiduals (:391-518)
            was_good = pts["is_good"] != 0
            g = np.nonzero(was_good)[0]
            m = g.size
            u0, v0, idn = pts["u"][g], pts["v"][g], pts["idepth_new"][g]
            alive = np.ones(m, bool)
            ms = np.full(m, 1e10, f32)
            energy = np.zeros(m, f32)
            jb = np.zeros((m, 10), f32)
            J = np.zeros((m, 8, 9), f32)
            for k, (dx, dy) in enumerate(PATTERN):
                a = np.nonzero(alive)[0]
                x, y, idd = u0[a] + f32(dx), v0[a] + f32(dy), idn[a]
                P = [(RKi[r, 0] * x + RKi[r, 1] * y + RKi[r, 2] * f32(1)) + t[r] * idd for r in range(3)]
                u, v = P[0] / P[2], P[1] / P[2]
                Ku, Kv = fxl * u + cxl, fyl * v + cyl
                nid = idd / P[2]
                ok = (Ku > 1) & (Kv > 1) & (Ku < f32(wl - 2)) & (Kv < f32(hl - 2)) & (nid > 0)
                alive[a[~ok]] = False
                a, x, y, idd, u, v, Ku, Kv, nid, P2 = (q[ok] for q in (a, x, y, idd, u, v, Ku, Kv, nid, P[2]))
                ix, iy = Ku.astype(np.int32), Kv.astype(np.int32)
                ddx, ddy = Ku - ix.astype(f32), Kv - iy.astype(f32)
                h0, h1, h2 = (_interp(pl, ix, iy, ddx, ddy, wl) for pl in (In, gx, gy))
                jx, jy = x.astype(np.int32), y.astype(np.int32)
                rlR = _interp(Ir, jx, jy, x - jx.astype(f32), y - jy.astype(f32), wl)
                ok = np.isfinite(rlR) & np.isfinite(h0)
                alive[a[~ok]] = False
                a, u, v, nid, P2, h0, h1, h2, rlR = (q[ok] for q in (a, u, v, nid, P2, h0, h1, h2, rlR))
                residual = h0 - r2a * rlR - r2b
                absr = np.abs(residual)
                hw = np.where(absr < hub, f32(1), hub / absr).astype(f32)
                energy[a] = energy[a] + hw * residual * residual * (f32(2) - hw)
                dxdd = (t[0] - t[2] * u) / P2
                dydd = (t[1] - t[2] * v) / P2
                hw = np.where(hw < 1, np.sqrt(hw), hw).astype(f32)
                dxI, dyI = hw * h1 * fxl, hw * h2 * fyl
                Jk = np.stack([nid * dxI, nid * dyI, -nid * (u * dxI + v * dyI),
                               -u * v * dxI - (f32(1) + v * v) * dyI, (f32(1) + u * u) * dxI + u * v * dyI,
                               -v * dxI + u * dyI, -hw * r2a * rlR, -hw * f32(1), hw * residual], axis=1)
                dd = dxI * dxdd + dyI * dydd
                sx, sy = dxdd * fxl, dydd * fyl
                maxstep = f32(1) / np.sqrt(sx * sx + sy * sy)
                ms[a] = np.where(maxstep < ms[a], maxstep, ms[a])
                jb[a, :9] = jb[a, :9] + Jk * dd[:, None]
                jb[a, 9] = jb[a, 9] + dd * dd
                J[a, k] = Jk
            pts["maxstep"] = f32(1e10)
            pts["maxstep"][g] = ms
            self.jb_new[g] = jb
            good = alive & ~(energy > pts["outlier_th"][g] * f32(20))
            new_good = np.zeros(n, bool)
            new_good[g[good]] = True
            pts["is_good_new"] = new_good
            pts["energy_new"] = pts["energy"]
            pts["energy_new"][g[good], 0] = energy[good]
            e_terms = pts["energy"][:, 0].copy()
            e_terms[g[good]] = energy[good]
            Jg = J[good]  # [ng, 8, 9] in point order
            prod = Jg[:, :, TRI_R] * Jg[:, :, TRI_C]  # [ng, 8, 45]
            ng = Jg.shape[0]
            lanes = acc_sum(prod.reshape(ng * 2, 4, 45))  # two updateSSE per point: pixels 0-3, 4-7 in the lanes
            acc9 = ((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]
            accE = acc_sum(e_terms)
            # calculateAlphaEnergy (:376-389)
            gi = np.nonzero(new_good)[0]
            idg = pts["idepth_new"][gi]
            pts["energy_new"][gi, 1] = (idg - f32(1)) * (idg - f32(1))
            ea_terms = pts["energy"][:, 1].copy()
            ea_terms[gi] = pts["energy_new"][gi, 1]
            accEA = acc_sum(ea_terms)
            tsq = (T[0, 3] * T[0, 3] + T[1, 3] * T[1, 3]) + T[2, 3] * T[2, 3]
            tsq_term = f32(tsq * n)
            alphaEnergy = tsq_term + accEA
            alphaEnergy = alphaEnergy * f32(p["alpha_w"])
            cap = f32(p["alpha_k"]) * f32(n)
            _, ea_bound = sum_bound(ea_terms)
            self.margins.append(("alpha_cap", abs(float(alphaEnergy) - float(cap)), float(ea_bound) * p["alpha_w"]))
            if alphaEnergy > cap:
                alphaOpt, alphaEnergy = f32(0), cap
            else:
                alphaOpt = f32(p["alpha_w"])
            # calculateSC (:349-374)
            jbn = self.jb_new
            pts["last_hessian_new"][gi] = jbn[gi, 9]
            j8 = jbn[gi, 8] + alphaOpt * (idg - f32(1))
            j9 = jbn[gi, 9] + alphaOpt
            if alphaOpt == 0:
                cw = f32(p["coupling_weight"])
                j8 = j8 + cw * (idg - pts["ir"][gi])
                j9 = j9 + cw
            j9 = f32(1) / (f32(1) + j9)
            jbn[gi, 8], jbn[gi, 9] = j8, j9
            Js = np.concatenate([jbn[gi, :8], j8[:, None]], axis=1)  # [ng, 9]
            sc_terms = np.zeros((gi.size, 45), f32)
            k = 0
            for r in range(9):  # Accumulator9::updateSingleWeighted
                sc_terms[:, k] = Js[:, r] * Js[:, r] * j9
                k += 1
                Js[:, r] = Js[:, r] * j9
                for c in range(r + 1, 9):
                    sc_terms[:, k] = Js[:, c] * Js[:, r]
                    k += 1
            acc9sc = acc_sum(sc_terms)

            def full(v):
                M = np.zeros((9, 9), f32)
                M[TRI_R, TRI_C] = v
                M[TRI_C, TRI_R] = v
                return M

            M, Msc = full(acc9), full(acc9sc)
            H, b, Hsc, bsc = M[:8, :8].copy(), M[:8, 8].copy(), Msc[:8, :8].copy(), Msc[:8, 8].copy()
            an = alphaOpt * f32(n)
            tlog = np.array(se3_log_translation(R.pose_from_matrix(T)), np.float64).astype(f32)
            tl_terms = tlog * alphaOpt * f32(n)
            for k in range(3):
                H[k, k] = H[k, k] + an
                b[k] = b[k] + tl_terms[k]
            res = np.array([accE, alphaEnergy, f32(n)], f32)
        return dict(H=H, b=b, Hsc=Hsc, bsc=bsc, res=res, capped=bool(alphaOpt == 0), alpha_opt=alphaOpt,
                    acc9_terms=prod.reshape(ng * 8, 45), sc_terms=sc_terms, e_terms=e_terms, ea_terms=ea_terms,
                    diag_term=an, tlog_terms=tl_terms, tsq_term=tsq_term)

    # -- calcEC (:520-536) --
    def calc_ec(self, lvl):
        pts = self.pts[lvl]
        if not self.snapped:
            return np.array([0, 0, pts.size], f32), np.zeros((0, 2), f32)
        g = pts["is_good_new"] != 0
        rOld, rNew = pts["idepth"][g] - pts["ir"][g], pts["idepth_new"][g] - pts["ir"][g]
        terms = np.stack([rOld * rOld, rNew * rNew], axis=1).astype(f32)
        A = acc_sum(terms) if terms.shape[0] else np.zeros(2, f32)
        cw = f32(self.p["coupling_weight"])
        return np.array([cw * A[0], cw * A[1], f32(terms.shape[0])], f32), terms

    # -- optReg (:538-567) --
    def opt_reg(self, lvl):
        pts = self.pts[lvl]
        if not self.snapped:
            pts["ir"] = 1
            return
        rw = f32(self.p["reg_weight"])
        good, ir, idepth, nbs = pts["is_good"], pts["ir"], pts["idepth"], pts["neighbours"]
        for i in range(pts.size):
            if not good[i]:
                continue
            idnn = [ir[j] for j in nbs[i] if j != -1 and good[j]]
            if len(idnn) > 2:
                med = sorted(idnn)[len(idnn) // 2]  # std::nth_element(idnn, idnn + nnn / 2, idnn + nnn)
                ir[i] = (f32(1) - rw) * idepth[i] + rw * med

    # -- propagateUp (:570-604) / propagateDown (:606-631) --
    def propagate_up(self, src):
        ps, pt = self.pts[src], self.pts[src + 1]
        pt["ir"] = 0
        pt["ir_sum_num"] = 0
        for i in range(ps.size):
            if not ps["is_good"][i]:
                continue
            par = ps["parent"][i]
            pt["ir"][par] = pt["ir"][par] + ps["ir"][i] * ps["last_hessian"][i]
            pt["ir_sum_num"][par] = pt["ir_sum_num"][par] + ps["last_hessian"][i]
        with np.errstate(all="ignore"):
            m = pt["ir_sum_num"] > 0
            val = pt["ir"][m] / pt["ir_sum_num"][m]
            pt["idepth"][m] = val
            pt["ir"][m] = val
            pt["is_good"][m] = 1
        self.opt_reg(src + 1)

    def propagate_down(self, src):
        ps, pt = self.pts[src], self.pts[src - 1]
        with np.errstate(all="ignore"):
            par = ps[pt["parent"]]
            go = (par["is_good"] != 0) & ~(par["last_hessian"].astype(np.float64) < 0.1)
            bad = go & (pt["is_good"] == 0)
            for f in ("ir", "idepth", "idepth_new"):
                pt[f][bad] = par["ir"][bad]
            pt["is_good"][bad] = 1
            pt["last_hessian"][bad] = 0
            ok = go & ~bad
            new = (pt["ir"][ok] * pt["last_hessian"][ok] * f32(2) + par["ir"][ok] * par["last_hessian"][ok]) / \
                (pt["last_hessian"][ok] * f32(2) + par["last_hessian"][ok])
            for f in ("ir", "idepth", "idepth_new"):
                pt[f][ok] = new
        self.opt_reg(src - 1)

    # -- resetPoints (:739-761), doStep (:763-789), applyStep (:791-809) --
    def reset_points(self, lvl):
        pts = self.pts[lvl]
        pts["energy"] = 0
        pts["idepth_new"] = pts["idepth"]
        if lvl != self.levels - 1:
            return
        for i in range(pts.size):
            if pts["is_good"][i]:
                continue
            snd, sn = f32(0), f32(0)
            for j in pts["neighbours"][i]:
                if j == -1 or not pts["is_good"][j]:
                    continue
                snd = snd + pts["ir"][j]
                sn = sn + f32(1)
            if sn > 0:
                pts["is_good"][i] = 1
                pts["ir"][i] = pts["idepth"][i] = pts["idepth_new"][i] = snd / sn

    def do_step(self, lvl, lam, inc):
        pts = self.pts[lvl]
        n = pts.size
        g = pts["is_good"] != 0
        jb = self.jb[:n]
        with np.errstate(all="ignore"):
            b = jb[:, 8] + dot8(jb[:, :8], np.asarray(inc, f32)[None, :])
            step = -b * jb[:, 9] / (f32(1) + f32(lam))
            maxstep = f32(0.25) * pts["maxstep"]
            maxstep = np.where(maxstep > f32(1e10), f32(1e10), maxstep)
            step = np.where(step > maxstep, maxstep, step)
            step = np.where(step < -maxstep, -maxstep, step)
            new = pts["idepth"] + step
            new = np.where(new < f32(1e-3), f32(1e-3), new)
            new = np.where(new > f32(50), f32(50), new)
        pts["idepth_new"][g] = new[g].astype(f32)

    def apply_step(self, lvl):
        pts = self.pts[lvl]
        bad = pts["is_good"] == 0
        g = ~bad
        pts["idepth"][bad] = pts["ir"][bad]
        pts["idepth_new"][bad] = pts["ir"][bad]
        pts["energy"][g] = pts["energy_new"][g]
        pts["idepth"][g] = pts["idepth_new"][g]
        pts["last_hessian"][g] = pts["last_hessian_new"][g]
        pts["is_good"][g] = pts["is_good_new"][g]
        self.jb, self.jb_new = self.jb_new, self.jb

    # -- trackFrame (:45-183) --
    def track_frame(self, new_dI, new_exposure, forced=None, on_eval=None):
        """forced: the device's log (records with pose [12], aff [2], inc [8]): the poses, affine pairs and
        increments are taken from it instead of this file's LM step.  on_eval(k, lvl, T, aff, out, pre): called with
        each evaluation's results and the level's records as they stood before it.  Returns (result dict, log).
        As the library does, an accepted pose is kept as the matrix that was evaluated and re-enters the next
        step through Eigen's Quaternion(Matrix3) (include/ldso_ct.h)."""
        p = self.p
        log = []
        if not self.snapped:
            self.T[:, 3] = 0
            for pts in self.pts:
                pts["ir"] = 1
                pts["idepth_new"] = 1
                pts["last_hessian"] = 0
        cur_T, aff_cur = self.T.copy(), self.aff
        new_exposure = f32(new_exposure)
        if self.first_exposure > 0 and new_exposure > 0:
            aff_cur = (f32(math.log(float(new_exposure / self.first_exposure))), f32(0))
        latest = np.zeros(3, f32)
        iters = np.zeros(5, np.int32)

        def evaluate(lvl, T, aff, it, lam, inc):
            k = len(log)
            if forced is not None:
                T = np.asarray(forced[k]["pose"], np.float64).reshape(3, 4).copy()
                aff = (f32(forced[k]["aff"][0]), f32(forced[k]["aff"][1]))
            pre = self.pts[lvl].copy() if on_eval else None
            out = self.calc_res_and_gs(lvl, T, aff, new_dI[lvl])
            out["bound"] = float(sum_bound(out["e_terms"])[1]) + \
                (0.0 if out["capped"] else float(p["alpha_w"]) * float(sum_bound(out["ea_terms"])[1]))
            log.append(dict(lvl=lvl, iteration=it, accepted=0, alpha_capped=int(out["capped"]), snapped=int(self.snapped),
                            lam=f32(lam), pose=T, aff=aff, inc=np.array(inc, f32), res=out["res"],
                            reg_energy=np.zeros(3, f32), out=out))
            if on_eval:
                on_eval(k, lvl, T, aff, out, pre)
            return out, T, aff

        for lvl in range(self.levels - 1, -1, -1):
            if lvl < self.levels - 1:
                self.propagate_down(lvl + 1)
            self.reset_points(lvl)
            old, cur_T, aff_cur = evaluate(lvl, cur_T, aff_cur, -1, 0, np.zeros(8, f32))
            self.apply_step(lvl)
            lam, eps, fails, iteration = f32(0.1), f32(1e-4), 0, 0
            while True:
                if forced is not None:
                    inc = np.asarray(forced[len(log)]["inc"], f32)
                    new_T, new_aff = None, None
                else:
                    inc, new_pose, new_aff = lm_step(old["H"], old["b"], old["Hsc"], old["bsc"], lam, self.w[lvl],
                                                     self.h[lvl], R.pose_from_matrix(cur_T), aff_cur,
                                                     bool(p["fix_affine"]))
                    new_T = R.pose_matrix(new_pose)
                    self.margins.append(("inc_norm", abs(float(norm8(inc)) - 1e-4),
                                         inc_bound(old, lam, self.w[lvl], self.h[lvl], bool(p["fix_affine"]))))
                self.do_step(lvl, lam, inc)
                new, new_T, new_aff = evaluate(lvl, new_T, new_aff, iteration, lam, inc)
                resOld, resNew = old["res"], new["res"]
                reg, reg_terms = self.calc_ec(lvl)
                eNew = (resNew[0] + resNew[1] + reg[1])
                eOld = (resOld[0] + resOld[1] + reg[0])
                accept = bool(eOld > eNew)
                bound = old["bound"] + new["bound"]
                if reg_terms.shape[0]:
                    bound += float(p["coupling_weight"]) * float(sum_bound(reg_terms)[1].sum())
                self.margins.append(("accept", abs(float(eOld) - float(eNew)), bound))
                if accept:
                    if resNew[1] == f32(p["alpha_k"]) * f32(self.pts[lvl].size):
                        self.snapped = True
                    old, aff_cur, cur_T = new, new_aff, new_T
                    self.apply_step(lvl)
                    self.opt_reg(lvl)
                    lam = lam * f32(0.5)
                    fails = 0
                    if lam < f32(0.0001):
                        lam = f32(0.0001)
                else:
                    fails += 1
                    lam = lam * f32(4)
                    if lam > 10000:
                        lam = f32(10000)
                log[-1].update(accepted=int(accept), snapped=int(self.snapped), reg_energy=reg, reg_terms=reg_terms)
                iters[lvl] += 1
                nrm = norm8(inc)
                if not (nrm > eps) or iteration >= p["max_iterations"][lvl] or fails >= 2:
                    break
                iteration += 1
            latest = old["res"]
        self.T, self.aff = cur_T.copy(), aff_cur
        for i in range(self.levels - 1):
            self.propagate_up(i)
        self.frame_id += 1
        if not self.snapped:
            self.snapped_at = 0
        if self.snapped and self.snapped_at == 0:
            self.snapped_at = self.frame_id
        ret = bool(self.snapped and self.frame_id > self.snapped_at + 5)
        res = dict(this_to_next=cur_T.copy(), this_to_next_aff=np.array([float(aff_cur[0]), float(aff_cur[1])]),
                   latest_res=np.asarray(latest, f32), snapped=int(self.snapped), frame_id=self.frame_id,
                   snapped_at=self.snapped_at, ret=int(ret), iterations=iters)
        return res, log
