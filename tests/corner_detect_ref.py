"""A numpy-float32 restatement of FeatureDetector::DetectCorners (reference
src/frontend/FeatureDetector.cc:34-130) with ShiTomasiScore and IC_Angle
(include/frontend/FeatureDetector.h:49-114), ComputeDescriptor (FeatureDetector.cc:132-189) and
FullSystem::makeNewTraces' loop for setting_pointSelection == 1 (src/frontend/FullSystem.cc:1428-1438):
the expected value of ldso_ct_detect_corners.  A helper, not a test file.

The float chains whose order matters -- ShiTomasiScore's three sums over the 8 x 8 box, IC_Angle's
m_10, v_sum and m_01 -- run tap by tap in the reference's order; numpy only carries many features
through the same step at once (float32 element-wise, no contraction).  The cells are a Python loop in
the reference's order (gx outer, gy inner), the candidates of a cell x outer, y inner.

Rules that are this project's and not the reference's (include/ldso_ct.h states them):
  * the sort of a cell's candidates is stable, and a score that is not finite sorts after every
    number, in candidate order (std::sort leaves ties open; its comparator is undefined with NaN);
  * float -> int of a value that is not finite or outside int's range is INT_MIN (x86's truncating
    conversion; undefined in C++);
  * a descriptor tap outside the 31 x 31 patch (only with an angle that is not finite, where the
    reference reads outside the image) reads INT_MIN;
  * the angle is atan2 in double rounded once (the reference: atan2f), the descriptor's rotation
    cos / sin in double rounded once (the reference: cosf / sinf).
"""
import math

import numpy as np

import oracle
import pixel_select_ref as PS

F = np.float32
HALF_PATCH = 15  # FeatureDetector.h:20
INT_MIN = -2 ** 31
STATS = ("gridsize", "k", "candidates", "features", "corners", "max_score_bits")
FEATURE_DTYPE = np.dtype([("score", "<f4"), ("angle", "<f4"), ("is_corner", "<i4"), ("level", "<i4"),
                          ("descriptor", "u1", (32,))])


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def umax_table():
    """FeatureDetector::FeatureDetector (FeatureDetector.cc:10-28)."""
    H = HALF_PATCH
    umax = [0] * (H + 1)
    half_diag = F(F(H) * np.sqrt(F(2))) / F(2)
    vmax = int(math.floor(half_diag + F(1)))
    vmin = int(math.ceil(half_diag))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(float(H * H) - v * v)))
    v0 = 0
    for v in range(H, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


UMAX = umax_table()


class Frame:
    """Level 0 of a frame as makeImages leaves it (pixel_select_ref.Frame without its three-level rule)."""

    def __init__(self, img):
        self.h, self.w = img.shape
        dI0, ag0 = oracle.make_images(img, self.w, self.h)[0]
        self.dI0 = dI0
        self.I = dI0[:, 0].reshape(self.h, self.w)
        self.dx = dI0[:, 1].reshape(self.h, self.w)
        self.dy = dI0[:, 2].reshape(self.h, self.w)
        self.ag = ag0.reshape(self.h, self.w)


def grid(w, h, n):
    """FeatureDetector.cc:37-42 -> dict(gridsize, gridX, gridY, nfeat, k, skip)."""
    gridsize = int(float(np.sqrt(F(w * h // n))) + 0.5)  # integer division, sqrtf, + 0.5 in double
    if gridsize < 1:
        return dict(gridsize=gridsize)
    nfeat = F(F(F(n) / F(w * h)) * F(gridsize * gridsize))
    return dict(gridsize=gridsize, gridX=w // gridsize + 1, gridY=h // gridsize + 1, nfeat=nfeat,
                k=int(math.floor(float(nfeat))) + 1,  # picked++, then `picked > nfeatInGrid` ends the cell
                skip=(HALF_PATCH * 2 // gridsize) + 1)


def shi_tomasi(fr, xs, ys):
    """ShiTomasiScore at integer pixels (xs, ys), halfbox 4, level 0."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    x_min, x_max, y_min, y_max = xs - 4, xs + 4, ys - 4, ys + 4
    border = (x_min < 1) | (x_max >= fr.w - 1) | (y_min < 1) | (y_max >= fr.h - 1)
    cx, cy = np.where(border, 8, xs), np.where(border, 8, ys)  # anywhere inside; the result is replaced
    dXX, dYY, dXY = (np.zeros(xs.shape, F) for _ in range(3))
    with np.errstate(all="ignore"):
        for oy in range(-4, 4):
            for ox in range(-4, 4):
                dx, dy = fr.dx[cy + oy, cx + ox], fr.dy[cy + oy, cx + ox]
                dXX = dXX + dx * dx
                dYY = dYY + dy * dy
                dXY = dXY + dx * dy
        dXX, dYY, dXY = ((a.astype(np.float64) / (2.0 * 64)).astype(F) for a in (dXX, dYY, dXY))
        r = dXX + dYY - np.sqrt((dXX + dYY) * (dXX + dYY) - F(4) * (dXX * dYY - dXY * dXY))
        s = (0.5 * r.astype(np.float64)).astype(F)
    assert s.dtype == F
    return np.where(border, F(0), s)


def sort_key(s):
    return (0, -float(s)) if math.isfinite(s) else (1, 0.0)


def picks_by_sort(scores, k):
    """Indices into the candidate list: a stable descending sort's first min(len, k)."""
    order = sorted(range(len(scores)), key=lambda i: sort_key(scores[i]))
    return order[:k]


def picks_by_rank(scores, k):
    """The parallel form: candidate i is picked iff fewer than k candidates precede it under (score
    descending, candidate index ascending); the picks ordered by that count."""
    keys = [sort_key(s) for s in scores]
    rank = [sum(1 for j in range(len(keys)) if keys[j] < keys[i] or (keys[j] == keys[i] and j < i))
            for i in range(len(keys))]
    return [i for _, i in sorted((r, i) for i, r in enumerate(rank) if r < k)]


def suppress_literal(xs, ys, score, cand):
    """FeatureDetector.cc:99-118, the double loop as written -> is_corner."""
    flag = np.array(cand, bool)
    corners = np.flatnonzero(cand)
    for a in range(corners.size):
        i = corners[a]
        for b in range(a + 1, corners.size):
            j = corners[b]
            ddx, ddy = int(xs[i]) - int(xs[j]), int(ys[i]) - int(ys[j])
            if ddx * ddx + ddy * ddy < 25:  # (uv1 - uv2).norm() < 5 on integer coordinates
                if score[i] > score[j]:
                    flag[j] = False
                else:
                    flag[i] = False
    return flag


def suppress_parallel(xs, ys, score, cand):
    """The order-free form: candidate i survives iff for every other candidate j within the radius
    s_i > s_j when i < j, and not s_j > s_i when j < i."""
    flag = np.array(cand, bool)
    corners = np.flatnonzero(cand)
    X, Y, S = xs[corners].astype(np.int64), ys[corners].astype(np.int64), score[corners]
    for a in range(corners.size):
        near = ((X - X[a]) ** 2 + (Y - Y[a]) ** 2 < 25)
        near[a] = False
        later = np.arange(corners.size) > a
        lost = (near & later & ~(S[a] > S)) | (near & ~later & (S > S[a]))
        if lost.any():
            flag[corners[a]] = False
    return flag


def ic_angle(fr, xs, ys):
    """IC_Angle on level 0 -> (angle float32, m_01, m_10): the chains in the reference's order."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    m_01, m_10 = np.zeros(xs.shape, F), np.zeros(xs.shape, F)
    H = HALF_PATCH
    with np.errstate(all="ignore"):
        for u in range(-H, H + 1):
            m_10 = m_10 + F(u) * fr.I[ys, xs + u]
        for v in range(1, H + 1):
            v_sum = np.zeros(xs.shape, F)
            d = UMAX[v]
            for u in range(-d, d + 1):
                val_plus, val_minus = fr.I[ys + v, xs + u], fr.I[ys - v, xs + u]
                v_sum = v_sum + (val_plus - val_minus)
                m_10 = m_10 + F(u) * (val_plus + val_minus)
            m_01 = m_01 + F(v) * v_sum
        angle = np.arctan2(m_01.astype(np.float64), m_10.astype(np.float64)).astype(F)
    return angle, m_01, m_10


def to_int(a):
    """float32 -> int as x86's truncating conversion: INT_MIN when not finite or out of range."""
    a = np.asarray(a, F)
    ok = np.isfinite(a) & (a >= F(-2 ** 31)) & (a < F(2 ** 31))
    return np.where(ok, np.trunc(np.where(ok, a, 0)).astype(np.int64), INT_MIN)


def descriptor(fr, x, y, angle, pattern):
    """ComputeDescriptor of the feature at (x, y) with the given angle (float32) -> 32 bytes."""
    factor_pi = F(np.pi / float(F(180)))
    with np.errstate(all="ignore"):
        theta = F(F(angle) * factor_pi)  # radians taken for degrees, as the reference has it
        a = F(math.cos(float(theta))) if math.isfinite(theta) else F(np.nan)
        b = F(math.sin(float(theta))) if math.isfinite(theta) else F(np.nan)
        P = np.asarray(pattern, np.int32).reshape(512, 2).astype(F)  # tap t: comparison t // 2, side t % 2
        row = to_int(P[:, 0] * b + P[:, 1] * a)
        col = to_int(P[:, 0] * a - P[:, 1] * b)
    H = HALF_PATCH
    inside = (np.abs(row) <= H) & (np.abs(col) <= H)
    val = fr.I[np.where(inside, y + row, y), np.where(inside, x + col, x)]
    t = np.where(inside, to_int(val), INT_MIN).reshape(256, 2)
    return np.packbits(t[:, 0] < t[:, 1], bitorder="little")  # byte i, bit j: comparison 8 i + j


def detect_corners(fr, n, pattern, host=0):
    """-> dict(xy [n][2] int, feat (FEATURE_DTYPE), rec (immature records), stats (over STATS), info).
    info: per cell the candidates' scores in candidate order and the picks, maxScore, the corner
    candidates."""
    G = grid(fr.w, fr.h, n)
    g = G["gridsize"]
    assert 1 <= g <= 2 * HALF_PATCH, "refused by the library"
    skip, k = G["skip"], G["k"]
    cells = []
    for gx in range(skip, G["gridX"] - skip):
        for gy in range(skip, G["gridY"] - skip):
            x0, y0 = gx * g, gy * g
            block = fr.ag[y0:y0 + g, x0:x0 + g]
            with np.errstate(all="ignore"):
                pos = block[block > 0]  # only `>` from 0: a NaN never wins
                max_grad = pos.max() if pos.size else F(0)
                grad_th = F(0.5 * float(max_grad)) if 0.5 * float(max_grad) > 5 else F(5)
                e = np.flatnonzero(block.T.reshape(-1) > grad_th)  # x outer, y inner
            cells.append(dict(gx=gx, gy=gy, xs=x0 + e // g, ys=y0 + e % g, grad_th=grad_th))
    all_x = np.concatenate([c["xs"] for c in cells]) if cells else np.zeros(0, np.int64)
    all_y = np.concatenate([c["ys"] for c in cells]) if cells else np.zeros(0, np.int64)
    all_s = shi_tomasi(fr, all_x, all_y)
    with np.errstate(all="ignore"):
        pos = all_s[all_s > 0]
    max_score = pos.max() if pos.size else F(0)
    fx, fy, fs, off = [], [], [], 0
    for c in cells:
        m = c["xs"].size
        c["scores"] = all_s[off:off + m]
        off += m
        c["picks"] = picks_by_sort(c["scores"].tolist(), k)
        for i in c["picks"]:
            fx.append(int(c["xs"][i]))
            fy.append(int(c["ys"][i]))
            fs.append(c["scores"][i])
    xs, ys, score = np.array(fx, np.int64), np.array(fy, np.int64), np.array(fs, F)
    score_th = F(0.01 * float(max_score))
    with np.errstate(all="ignore"):
        cand = score > score_th
    is_corner = suppress_parallel(xs, ys, score, cand)
    feat = np.zeros(xs.size, FEATURE_DTYPE)
    feat["score"] = score
    feat["is_corner"] = is_corner
    ci = np.flatnonzero(is_corner)
    angle, _, _ = ic_angle(fr, xs[ci], ys[ci])
    feat["angle"][ci] = angle
    for j, i in enumerate(ci):
        feat["descriptor"][i] = descriptor(fr, xs[i], ys[i], angle[j], pattern)
    uv = np.stack([xs, ys], 1).astype(F).reshape(-1, 2)
    rec = oracle.ip_make(fr.dI0, fr.w, fr.h, uv, 1.0, host)  # every feature: mode 1 drops none
    stats = dict(gridsize=g, k=k, candidates=int(all_x.size), features=int(xs.size), corners=int(ci.size),
                 max_score_bits=int(bits(max_score).reshape(-1)[0]))
    return dict(xy=np.stack([xs, ys], 1).reshape(-1, 2), feat=feat, rec=rec, stats=stats,
                info=dict(grid=G, cells=cells, max_score=max_score, score_th=score_th, cand=cand))


# ---- the inputs both test files use -----------------------------------------------------------
# (w, h, n) -> the (gridsize, k) the tests assert; 192 x 128 is the select tests' aligned size
CASES = {(200, 136, 300): (9, 1), (200, 136, 340): (9, 2), (203, 139, 300): (10, 2), (192, 128, 300): None}
WIDE = (1232, 368, 1500)  # gridsize 17, k 1
KINDS = ("blobs", "tiles", "nan")
TILE = 4  # the period of `tiles`: below half of every gridsize of CASES


def bit_pattern(seed=5):
    """A seeded stand-in for the ORB sampling table: 256 * 4 ints in [-13, 13]."""
    return np.random.default_rng(seed).integers(-13, 14, 1024).astype(np.int32)


def image(kind, w, h, seed=1):
    """blobs: pixel_select_ref's.  tiles: a random TILE x TILE texture repeated in x and y, so that
    the pixels of a cell that differ by a period have bit-equal scores.  nan: pixel_select_ref's nan
    image (noise, 40 NaN pixels: NaN intensities inside orientation patches; makeImages zeroes the
    gradients there, so they make no score non-finite) whose middle third is the isotropic texture
    A (c[x % 4] + c[y % 4]): there dXX and dYY agree to rounding and dXY vanishes, the discriminant
    (dXX + dYY)^2 - 4 (dXX dYY - dXY^2) is rounding noise of either sign, and its square root is NaN
    where it came out negative."""
    if kind == "tiles":
        tile = np.random.default_rng(seed + 200).uniform(40, 200, (TILE, TILE)).astype(F)
        return np.tile(tile, (h // TILE + 1, w // TILE + 1))[:h, :w].copy()
    if kind == "nan":
        img = PS.image("nan", w, h, seed).copy()
        c = np.cos(2 * np.pi * (np.arange(max(w, h)) % TILE + 0.3) / TILE)
        iso = (120.0 + 37.3 * (c[None, :w] + c[:h, None])).astype(F)
        img[:, w // 3:2 * w // 3] = iso[:, w // 3:2 * w // 3]
        return img
    return PS.image(kind, w, h, seed)
