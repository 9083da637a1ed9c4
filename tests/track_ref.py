"""CoarseTracker::trackNewestCoarse (src/frontend/CoarseTracker.cc:61-310) on the visual-only path,
restated in plain Python from the reference text: the checker of ldso_ct_track / ldso_ct_lm_step.

It shares no code with the library.  The loop is parametrised by two callables,
    calc_res(lvl, T [3][4], (a, b), cutoff) -> (rs [6], state)      CoarseTracker::calcRes
    calc_gs(lvl, state, (a, b))             -> (H [8][8], b [8])    CoarseTracker::calcGSSSE
so the same statements run over the CPU oracle, or replay the evaluations a device run logged.
It returns the ABI's result (a dict over ldso_ct_track_result's fields) and step log (dicts over
ldso_ct_track_step's).  float members of the reference (lambda, extrapFac, levelCutoffRepeat, AffLight's
a and b) are numpy float32 here; the Sophus statements are those of tests/test_sophus_kat.py, copied.

The solve: FULL is the symmetric 8x8 system (upstream's Mat88 Hl = H; Hl.ldlt()), REFERENCE what this
fork's text evaluates to -- H lands in the upper triangle of a zero Hl, LDLT<., Lower> reads the lower
one, so D = diag(Hl): inc_i = bl_i / Hl_ii.
"""
import math

import numpy as np

EPS = 1e-10  # Sophus::Constants<double>::epsilon()
SOLVE_FULL, SOLVE_REFERENCE = 0, 1
f32 = np.float32
LIMIT = f32(0.001)  # lambdaExtrapolationLimit
SCALE = (0.5, 0.5, 0.5, 1.0, 1.0, 1.0, 10.0, 1000.0)  # SCALE_XI_TRANS x3, SCALE_XI_ROT x3, SCALE_A, SCALE_B

DEFAULTS = dict(coarse_cutoff_th=20.0, lambda_increase=4.0, lambda_decrease=0.5, affine_opt_mode_a=1e12,
                affine_opt_mode_b=1e8, max_iterations=(10, 20, 50, 50, 50), solve=SOLVE_FULL)


# ---- Sophus (tests/test_sophus_kat.py) ---------------------------------------------------------
def q_normalize(q):
    x, y, z, w = q
    n = math.sqrt((x * x + z * z) + (y * y + w * w))
    return (x / n, y / n, z / n, w / n)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def q_rotate(q, p):
    uv = cross(q[:3], p)
    uv = tuple(u + u for u in uv)
    c = cross(q[:3], uv)
    return tuple((p[i] + q[3] * uv[i]) + c[i] for i in range(3))


def q_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def q_from_matrix(R):
    t = (R[0][0] + R[1][1]) + R[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2][1] - R[1][2]) * t
        q[1] = (R[0][2] - R[2][0]) * t
        q[2] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    return tuple(q)


def hat(w):
    return [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]


def mm(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def mv(A, v):
    return tuple((A[i][0] * v[0] + A[i][1] * v[1]) + A[i][2] * v[2] for i in range(3))


def se3_exp(a):
    w = a[3:]
    theta_sq = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    theta = math.sqrt(theta_sq)
    if theta < EPS:
        po4 = theta_sq * theta_sq
        imag = (0.5 - (1.0 / 48.0) * theta_sq) + (1.0 / 3840.0) * po4
        real = (1.0 - (1.0 / 8.0) * theta_sq) + (1.0 / 384.0) * po4
    else:
        imag = math.sin(0.5 * theta) / theta
        real = math.cos(0.5 * theta)
    q = (imag * w[0], imag * w[1], imag * w[2], real)
    W = hat(w)
    W2 = mm(W, W)
    if theta < EPS:
        V = q_matrix(q)
    else:
        theta_sq_v = theta * theta
        s1 = (1.0 - math.cos(theta)) / theta_sq_v
        s2 = (theta - math.sin(theta)) / (theta_sq_v * theta)
        V = [[((1.0 if i == j else 0.0) + s1 * W[i][j]) + s2 * W2[i][j] for j in range(3)] for i in range(3)]
    return q, mv(V, a[:3])


def se3_mul(A, B):
    (ax, ay, az, aw), (bx, by, bz, bw) = A[0], B[0]
    q = q_normalize((((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz,
                     ((aw * bz + az * bw) + ax * by) - ay * bx, ((aw * bw - ax * bx) - ay * by) - az * bz))
    r = q_rotate(A[0], B[1])
    return q, tuple(A[1][i] + r[i] for i in range(3))


def pose_from_matrix(T):
    """SE3(R, t) from matrix3x4()."""
    T = np.asarray(T, np.float64)
    return q_from_matrix([[float(v) for v in T[i, :3]] for i in range(3)]), tuple(float(T[i, 3]) for i in range(3))


def pose_matrix(P):
    T = np.zeros((3, 4))
    T[:, :3] = q_matrix(P[0])
    T[:, 3] = P[1]
    return T


# ---- the solve -----------------------------------------------------------------------------------
def ldlt_solve(A, b):
    """Eigen::LDLT<., Lower>: symmetric diagonal pivoting (the largest |diagonal| first), reading the
    lower triangle of A only."""
    n = len(b)
    a = [[float(A[i][j]) if j <= i else float(A[j][i]) for j in range(n)] for i in range(n)]
    for i in range(n):  # only the lower triangle is the input
        for j in range(i + 1, n):
            a[i][j] = a[j][i]
    perm = list(range(n))
    for k in range(n):
        piv = max(range(k, n), key=lambda i: (abs(a[i][i]), -i))
        if piv != k:
            perm[k], perm[piv] = perm[piv], perm[k]
            a[k], a[piv] = a[piv], a[k]
            for r in a:
                r[k], r[piv] = r[piv], r[k]
        d = a[k][k]
        for i in range(k + 1, n):
            li = a[i][k] / d if d != 0 else 0.0
            for j in range(k + 1, n):
                a[i][j] -= li * a[k][j]
            a[i][k] = li
    y = [float(b[perm[i]]) for i in range(n)]
    for i in range(n):
        for j in range(i):
            y[i] -= a[i][j] * y[j]
    for i in range(n):
        y[i] = y[i] / a[i][i] if a[i][i] != 0 else 0.0
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= a[j][i] * y[j]
    x = [0.0] * n
    for i in range(n):
        x[perm[i]] = y[i]
    return x


def lm_increment(H, b, lam, params):
    """CoarseTracker.cc:130-184 with bl = -b: the increment of the affine mode's sub-system."""
    H = np.asarray(H, np.float64)
    b = np.asarray(b, np.float64)
    fix_a, fix_b = params["affine_opt_mode_a"] < 0, params["affine_opt_mode_b"] < 0
    if fix_a and fix_b:
        idx = [0, 1, 2, 3, 4, 5]
    elif fix_b:
        idx = [0, 1, 2, 3, 4, 5, 6]
    elif fix_a:
        idx = [0, 1, 2, 3, 4, 5, 7]  # HlStitch: row and column 7 in the place of 6
    else:
        idx = list(range(8))
    n = len(idx)
    dl = float(f32(1) + f32(lam))  # Hl(i, i) *= (1 + lambda) with a float lambda
    A = [[float(H[idx[i], idx[j]]) * (dl if i == j else 1.0) for j in range(n)] for i in range(n)]
    rhs = [-float(b[i]) for i in idx]
    if params["solve"] == SOLVE_REFERENCE:
        tol = 1.0 / np.finfo(np.float64).max
        x = [rhs[i] / A[i][i] if abs(A[i][i]) > tol else 0.0 for i in range(n)]
    else:
        x = ldlt_solve(A, rhs)
    inc = [0.0] * 8
    for i, k in enumerate(idx):
        inc[k] = x[i]
    return inc


def lm_step(H, b, lam, pose, aff, params):
    """CoarseTracker.cc:130-213 -> (inc [8], refToNew_new, aff_g2l_new): pose a (q, t) pair, aff float32."""
    with np.errstate(all="ignore"):
        inc = lm_increment(H, b, lam, params)
        lam = f32(lam)
        extrap = f32(1)
        if lam < LIMIT:
            extrap = np.sqrt(np.sqrt(LIMIT / lam))  # float32 throughout
        inc = [v * float(extrap) for v in inc]
        scaled = [inc[i] * SCALE[i] for i in range(8)]
        if not math.isfinite(sum(v * v for v in scaled)):
            inc = [0.0] * 8
            scaled = [0.0] * 8
        new_pose = se3_mul(se3_exp(tuple(scaled[:6])), pose)
        new_aff = (f32(float(aff[0]) + scaled[6]), f32(float(aff[1]) + scaled[7]))
    return inc, new_pose, new_aff


def from_to_vec_exposure(exp_f, exp_t, a_f, b_f, a_t, b_t):
    """AffLight::fromToVecExposure (AffLight.h:27-35), float."""
    exp_f, exp_t = f32(exp_f), f32(exp_t)
    if exp_f == 0 or exp_t == 0:
        exp_f = exp_t = f32(1)
    a = f32(np.exp(f32(a_t) - f32(a_f))) * exp_t / exp_f
    return f32(a), f32(f32(b_t) - a * f32(b_f))


# ---- the loop ------------------------------------------------------------------------------------
def track(calc_res, calc_gs, ref_to_new, aff, coarsest_lvl, min_res_for_abort, ref_frame=(1.0, 1.0, 0.0, 0.0),
          **params):
    """trackNewestCoarse.  ref_frame: (lastRef->ab_exposure, newFrame->ab_exposure, lastRef_aff_g2l a, b)."""
    p = dict(DEFAULTS, **params)
    mA, mB = f32(p["affine_opt_mode_a"]), f32(p["affine_opt_mode_b"])
    T_in = np.array(np.asarray(ref_to_new, np.float64)[:3, :4])
    res = dict(ref_to_new=T_in.copy(), aff=np.array([float(f32(aff[0])), float(f32(aff[1]))]),
               last_residuals=np.full(5, np.nan), flow=np.full(3, 1000.0), ok=0, reason=0, abort_level=-1,
               iterations=np.zeros(5, np.int32), repeated_level=-1)
    log = []
    cur = pose_from_matrix(T_in)
    aff_cur = (f32(aff[0]), f32(aff[1]))
    have_repeated = False
    lvl = int(coarsest_lvl)

    def evaluate(pose, ab, cutoff, it, lam, inc):
        T = pose_matrix(pose)
        rs, state = calc_res(lvl, T, (float(ab[0]), float(ab[1])), float(cutoff))
        rs = np.array(rs, np.float64)
        log.append(dict(lvl=lvl, iteration=it, accepted=0, cutoff_th=float(cutoff), lam=float(lam), pose=T,
                        aff=np.array([float(ab[0]), float(ab[1])]), rs=rs, inc=np.array(inc, np.float64)))
        return rs, state

    with np.errstate(all="ignore"):
        while lvl >= 0:
            repeat = f32(1)
            cutoff = f32(p["coarse_cutoff_th"]) * repeat
            res_old, state = evaluate(cur, aff_cur, cutoff, -1, 0.0, [0.0] * 8)
            while res_old[5] > 0.6 and repeat < 50:
                repeat = repeat * f32(2)
                cutoff = f32(p["coarse_cutoff_th"]) * repeat
                res_old, state = evaluate(cur, aff_cur, cutoff, -1, 0.0, [0.0] * 8)
            lam = f32(0.01)
            H, b = calc_gs(lvl, state, (float(aff_cur[0]), float(aff_cur[1])))
            for iteration in range(int(p["max_iterations"][lvl])):
                inc, new_pose, new_aff = lm_step(H, b, lam, cur, aff_cur, p)
                res_new, state = evaluate(new_pose, new_aff, cutoff, iteration, lam, inc)
                accept = bool((res_new[0] / res_new[1] + 0.0) < (res_old[0] / res_old[1] + 0.0))
                log[-1]["accepted"] = int(accept)
                if accept:
                    H, b = calc_gs(lvl, state, (float(new_aff[0]), float(new_aff[1])))
                    res_old, aff_cur, cur = res_new, new_aff, new_pose
                    lam = f32(float(lam) * p["lambda_decrease"])
                else:
                    lam = f32(float(lam) * p["lambda_increase"])
                    if lam < LIMIT:
                        lam = LIMIT
                res["iterations"][lvl] += 1
                if not (math.sqrt(sum(v * v for v in inc)) > 1e-3):
                    break
            last = float(np.sqrt(f32(res_old[0] / res_old[1] + 0.0)))
            res["last_residuals"][lvl] = last
            res["flow"] = res_old[2:5].copy()
            if last > 1.5 * float(min_res_for_abort[lvl]):
                res.update(ok=0, reason=1, abort_level=lvl)
                return res, log
            if repeat > 1 and not have_repeated:
                have_repeated = True
                res["repeated_level"] = lvl
            else:
                lvl -= 1
        res["ref_to_new"] = pose_matrix(cur)
        a, b_ = aff_cur
        res["aff"] = np.array([float(a), float(b_)])
        if (mA != 0 and float(abs(a)) > 1.2) or (mB != 0 and float(abs(b_)) > 200):
            res.update(ok=0, reason=2)
            return res, log
        ra, rb = from_to_vec_exposure(ref_frame[0], ref_frame[1], ref_frame[2], ref_frame[3], a, b_)
        if (mA == 0 and float(abs(np.log(f32(ra)))) > 1.5) or (mB == 0 and float(abs(rb)) > 200):
            res.update(ok=0, reason=3)
            return res, log
        if mA < 0:
            res["aff"][0] = 0
        if mB < 0:
            res["aff"][1] = 0
        res["ok"] = 1
    return res, log


def ulps(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return int(np.abs(ia - ib).max()) if a.size else 0


def pose_ulps(A, B):
    """The largest element-wise distance of two poses [3][4] in ulps, every entry in its own ulps
    (test_sophus_kat's measure)."""
    return ulps(np.asarray(A, np.float64).reshape(12), np.asarray(B, np.float64).reshape(12))
