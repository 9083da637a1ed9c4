"""Plain-Python / numpy restatement of the loop closer's matching, written from the reference text with
its sequential loops in its order (paths relative to n-lalanne/LDSO):

  FeatureMatcher::DescriptorDistance / SearchBruteForce / SearchByBoW   src/frontend/FeatureMatcher.cc:16-124
  LoopClosing::ComputeOptimizedPose, map and correspondence search      src/frontend/LoopClosing.cc:264-398
  Frame::SetFeatureGrid / GetFeatureInGrid                              src/Frame.cc:63-108
  RxSO3 / Sim3 point action                                             Sophus rxso3.hpp:259-267, sim3.hpp:228-231

and the seeded generators of the cases the GPU tests (test_loop_match.py, test_loop_projection.py) compare
on.  float is np.float32 and double np.float64 throughout, one operation at a time (no contraction).

Where the reference is undefined the library's rules (include/ldso_lc.h) apply: to_int gives INT_MIN for a
value that is not finite or does not fit; a centre outside the image writes nothing into the map; a map
lookup outside the image reads 0."""
import bisect

import numpy as np

F = np.float32
D = np.float64
GRID = 20  # Frame::gridSize, include/Frame.h:185
INT_MIN = -(2 ** 31)

FEATURE_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("angle", "<f4"), ("inv_d", "<f4"), ("is_corner", "<i4"),
                          ("usable", "<i4"), ("descriptor", "u1", (32,))])
MATCH_DTYPE = np.dtype([("index1", "<i4"), ("index2", "<i4"), ("dist", "<i4")])
PROJECTION_DTYPE = np.dtype([("index_cand", "<i4"), ("index_cur", "<i4"), ("dist", "<i4"), ("reserved_", "<i4"),
                             ("p_ref", "<f8", (3,)), ("p_curr", "<f8", (3,)), ("pixel", "<f8", (2,))])


# ---- DescriptorDistance -----------------------------------------------------------------------
def descriptor_distance(d1, d2):
    """FeatureMatcher.cc:16-33, the portable branch: eight 32-bit words, the bit-twiddling popcount."""
    pa = np.ascontiguousarray(d1, np.uint8).view("<u4")
    pb = np.ascontiguousarray(d2, np.uint8).view("<u4")
    dist = 0
    for i in range(8):
        v = int(pa[i]) ^ int(pb[i])
        v = v - ((v >> 1) & 0x55555555)
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
        dist += ((((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) & 0xFFFFFFFF) >> 24
    return dist


def as_ints(frame):
    """every descriptor as one 256-bit Python int: distance() below is descriptor_distance on them
    (test_loop_ref.py pins the two against each other), fast enough for the searches' double loops"""
    return [int.from_bytes(d.tobytes(), "little") for d in frame["descriptor"]]


def distance(a, b):
    return bin(a ^ b).count("1")


# ---- SearchBruteForce -------------------------------------------------------------------------
def search_brute_force(frame1, frame2, th_low=50, details=None):
    """FeatureMatcher.cc:35-64.  details (a list, optional) receives (i, min_dist_index, min_dist) of every
    corner of frame1, matched or not."""
    d1, d2 = as_ints(frame1), as_ints(frame2)
    matches = []
    for i in range(len(frame1)):
        if not frame1["is_corner"][i]:
            continue
        min_dist = 9999
        min_dist_index = -1
        for j in range(len(frame2)):
            if not frame2["is_corner"][j]:
                continue
            dist = distance(d1[i], d2[j])
            if dist < min_dist:
                min_dist = dist
                min_dist_index = j
        if details is not None:
            details.append((i, min_dist_index, min_dist))
        if min_dist < th_low:
            matches.append((i, min_dist_index, min_dist))
    return np.array(matches, MATCH_DTYPE).reshape(-1)


# ---- SearchByBoW ------------------------------------------------------------------------------
def search_by_bow(frame1, bow1, frame2, bow2, th_low=50, nn_ratio=0.6, details=None):
    """FeatureMatcher.cc:66-124.  bow = (node_ids ascending, [feature indices per node]): the featVec map
    with bowIdx already applied.  details receives (index1, best1, best2) per visited feature."""
    d1, d2 = as_ints(frame1), as_ints(frame2)
    ids1, lists1 = bow1
    ids2, lists2 = bow2
    nn_ratio = F(nn_ratio)
    matches = []
    f1, f2 = 0, 0
    while f1 != len(ids1) and f2 != len(ids2):
        if ids1[f1] == ids2[f2]:
            for idx1 in lists1[f1]:
                best_dist1 = 256
                best_idx2 = -1
                best_dist2 = 256
                for idx2 in lists2[f2]:
                    dist = distance(d1[idx1], d2[idx2])
                    if dist < best_dist1:
                        best_dist2 = best_dist1
                        best_dist1 = dist
                        best_idx2 = idx2
                    elif dist < best_dist2:
                        best_dist2 = dist
                if details is not None:
                    details.append((idx1, best_dist1, best_dist2))
                if best_dist1 <= th_low:
                    if F(best_dist1) < nn_ratio * F(best_dist2):
                        matches.append((idx1, best_idx2, best_dist1))
            f1 += 1
            f2 += 1
        elif ids1[f1] < ids2[f2]:
            f1 = bisect.bisect_left(ids1, ids2[f2])  # featVec.lower_bound
        else:
            f2 = bisect.bisect_left(ids2, ids1[f1])
    return np.array(matches, MATCH_DTYPE).reshape(-1)


def bow_arrays(bow):
    """(node_id, node_begin, feat_idx) as ldso_lc_keyframe_set_bow takes them"""
    ids, lists = bow
    begin = np.zeros(len(ids) + 1, np.int32)
    for k, l in enumerate(lists):
        begin[k + 1] = begin[k] + len(l)
    flat = np.array([i for l in lists for i in l], np.int32)
    return np.array(ids, np.int32), begin, flat


# ---- the inverse-depth map --------------------------------------------------------------------
def to_int(f):
    """x86's truncating float -> int conversion; INT_MIN for what is not finite or does not fit"""
    f = float(f)
    if not np.isfinite(f) or f >= 2147483648.0 or f < -2147483648.0:
        return INT_MIN
    return int(f)


def make_idepth_map(w, h, centers):
    """LoopClosing.cc:266-295 over the contributions in traversal order; the dilation loop (:297-310) runs
    over an empty vector and is not restated."""
    idepth_map = np.zeros((h, w), F)
    for c in np.asarray(centers, F).reshape(-1, 3):
        tu, tv = F(c[0] + F(0.5)), F(c[1] + F(0.5))
        if not (tu > F(-1) and tu < F(w) and tv > F(-1) and tv < F(h)):
            continue  # the reference would write outside its array (or the centre is a NaN / a hole)
        u, v = int(tu), int(tv)
        idepth_map[v, u] = c[2]
    return idepth_map


# ---- SetFeatureGrid / GetFeatureInGrid --------------------------------------------------------
def set_feature_grid(frame, w, h):
    """Frame.cc:63-74; None if a corner would index outside the grid (the library refuses the put)"""
    gw, gh = w // GRID, h // GRID
    grid = [[] for _ in range(gw * gh)]
    for i in range(len(frame)):
        if frame["is_corner"][i]:
            u, v = F(frame["u"][i]), F(frame["v"][i])
            if not (u >= 0 and v >= 0):
                return None
            grid_x, grid_y = to_int(u / F(GRID)), to_int(v / F(GRID))
            if grid_x < 0 or grid_y < 0 or grid_x >= gw or grid_y >= gh:
                return None
            grid[grid_y * gw + grid_x].append(i)
    return grid


def _cdiv(a, b):
    """C's integer division: truncating toward zero"""
    q = abs(a) // b
    return q if a >= 0 else -q


def get_feature_in_grid(frame, grid, w, h, x, y, radius):
    """Frame.cc:76-108 -> (indices with their (ix, iy), the early return taken or None)"""
    x, y, radius = F(x), F(y), F(radius)
    gw, gh = w // GRID, h // GRID
    with np.errstate(all="ignore"):
        grid_x_min = max(0, _cdiv(to_int(x - radius), GRID))
        if grid_x_min >= gw:
            return [], "xmin"
        grid_x_max = min(gw - 1, _cdiv(to_int(x + radius), GRID))
        if grid_x_max < 0:
            return [], "xmax"
        grid_y_min = max(0, _cdiv(to_int(y - radius), GRID))
        if grid_y_min >= gh:
            return [], "ymin"
        grid_y_max = min(gh - 1, _cdiv(to_int(y + radius), GRID))
        if grid_y_max < 0:
            return [], "ymax"
        r2 = radius * radius
        indices = []
        for ix in range(grid_x_min, grid_x_max + 1):
            for iy in range(grid_y_min, grid_y_max + 1):
                for k in grid[iy * gw + ix]:
                    u, v = F(frame["u"][k]), F(frame["v"][k])
                    if ((u - x) * (u - x) + (v - y) * (v - y)) < r2:
                        indices.append((k, ix, iy))
    return indices, None


# ---- the projection search --------------------------------------------------------------------
def project_candidate(p, calib, scr):
    """LoopClosing.cc:337-347 -> (pRef [3] double, u, v float)"""
    fxl, fyl, cxl, cyl, fxli, fyli, cxli, cyli = (F(c) for c in calib)
    qx, qy, qz, qw, tx, ty, tz = (D(c) for c in scr)
    with np.errstate(all="ignore"):
        s = D(1.0) / D(F(p["inv_d"]))
        ax = fxli * (F(p["u"]) - cxl)
        ay = fyli * (F(p["v"]) - cyl)
        r = [s * D(ax), s * D(ay), s * D(1.0)]
        # RxSO3::operator* (rxso3.hpp:259-267); squaredNorm as Eigen's packet reduction adds four doubles
        scale = (qx * qx + qz * qz) + (qy * qy + qw * qw)
        t = [qy * r[2] - qz * r[1], qz * r[0] - qx * r[2], qx * r[1] - qy * r[0]]
        t = [a + a for a in t]
        c = [qy * t[2] - qz * t[1], qz * t[0] - qx * t[2], qx * t[1] - qy * t[0]]
        q = [scale * r[k] + (qw * t[k] + c[k]) for k in range(3)]
        pc = [q[0] + tx, q[1] + ty, q[2] + tz]  # Sim3::operator* (sim3.hpp:228-231)
        x = F(pc[0] / pc[2])
        y = F(pc[1] / pc[2])
        u = fxl * x + cxl
        v = fyl * y + cyl
    return r, u, v, pc


def map_at(idepth_map, fu, fv):
    h, w = idepth_map.shape
    with np.errstate(all="ignore"):
        ui, vi = to_int(F(fu) + F(0.5)), to_int(F(fv) + F(0.5))
    if ui < 0 or vi < 0 or ui >= w or vi >= h:
        return F(0)
    return idepth_map[vi, ui]


def search_by_projection(cur, cand, idepth_map, calib, scr, window_size=5.0, th_high=50, stats=None):
    """LoopClosing.cc:313-398.  stats (a dict, optional) counts the case families met."""
    h, w = idepth_map.shape
    grid = set_feature_grid(cur, w, h)
    assert grid is not None
    dc, dp = as_ints(cur), as_ints(cand)
    fxli, fyli, cxli, cyli = (D(F(c)) for c in calib[4:8])
    st = stats if stats is not None else {}
    for key in ("xmin", "xmax", "ymin", "ymax", "hole", "angle_in", "angle_out", "multi_cell_tie", "behind", "pc2_zero",
                "candidates"):
        st.setdefault(key, 0)
    out = []
    for i in range(len(cand)):
        p = cand[i]
        if not p["usable"]:
            continue
        st["candidates"] += 1
        p_ref, u, v, pc = project_candidate(p, calib, scr)
        st["behind"] += int(pc[2] < 0)
        st["pc2_zero"] += int(pc[2] == 0)
        best_dist = 256
        best_dist2 = 256
        best_idx = -1
        indices, early = get_feature_in_grid(cur, grid, w, h, u, v, window_size)
        if early:
            st[early] += 1
        seen = []
        for k, ix, iy in indices:
            feat = cur[k]
            with np.errstate(all="ignore"):
                gate = float(np.abs(F(feat["angle"]) - F(p["angle"]))) < 0.2
            st["angle_in" if gate else "angle_out"] += 1
            if gate:
                dist = distance(dc[k], dp[i])
                if map_at(idepth_map, feat["u"], feat["v"]) == 0:
                    st["hole"] += 1
                    continue
                seen.append((dist, ix, iy))
                if dist < best_dist:
                    best_dist2 = best_dist
                    best_dist = dist
                    best_idx = k
                elif dist < best_dist2:
                    best_dist2 = dist
        if len({(ix, iy) for d, ix, iy in seen if d == best_dist}) >= 2:
            st["multi_cell_tie"] += 1
        if best_dist <= th_high and best_idx >= 0:
            best = cur[best_idx]
            idepth = map_at(idepth_map, best["u"], best["v"])
            with np.errstate(all="ignore"):
                inv = D(F(1.0) / idepth)
            bu, bv = D(F(best["u"])), D(F(best["v"]))
            k0 = (fxli * bu + D(0) * bv) + cxli * D(1)
            k1 = (D(0) * bu + fyli * bv) + cyli * D(1)
            k2 = (D(0) * bu + D(0) * bv) + D(1) * D(1)
            out.append((i, best_idx, best_dist, 0, tuple(p_ref), (inv * k0, inv * k1, inv * k2), (bu, bv)))
    return np.array(out, PROJECTION_DTYPE).reshape(-1)


# ---- seeded case generators -------------------------------------------------------------------
def flip_bits(desc, n, rng):
    """a copy of the 32-byte descriptor with exactly n bits flipped"""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    pos = rng.choice(256, n, replace=False)
    bits[pos] ^= 1
    return np.packbits(bits)


def make_frame(rng, w, h, n_corners, n_other=0, usable_fraction=1.0):
    """n_corners corners on integer pixels inside the grid mixed with n_other plain features (descriptor 0,
    angle 0, as Feature's defaults), in random feature order"""
    n = n_corners + n_other
    fr = np.zeros(n, FEATURE_DTYPE)
    is_corner = np.zeros(n, bool)
    is_corner[rng.permutation(n)[:n_corners]] = True
    gw, gh = w // GRID, h // GRID
    fr["u"] = rng.integers(0, gw * GRID, n).astype(F)
    fr["v"] = rng.integers(0, gh * GRID, n).astype(F)
    fr["is_corner"] = is_corner
    fr["angle"] = np.where(is_corner, rng.uniform(-np.pi, np.pi, n), 0).astype(F)
    fr["descriptor"] = np.where(is_corner[:, None], rng.integers(0, 256, (n, 32)), 0).astype(np.uint8)
    fr["inv_d"] = F(-1)
    fr["usable"] = rng.random(n) < usable_fraction
    return fr


BRUTE_SIZES = [(1, 1), (63, 65), (64, 64), (200, 333), (333, 0)]
TH_LOW = 50


def brute_case(n1, n2, seed=11):
    """Two frames of n1 / n2 corners mixed with plain features.  Where the sizes allow: corners 0, 1, 2 of
    frame1 get a partner in frame2 at distance TH_LOW - 1, TH_LOW, TH_LOW + 1; corner 0's partner is held
    twice (a tie between two j); corner 3's descriptor is held by two corners of frame2 (a tie at 0)."""
    rng = np.random.default_rng(seed + 1000 * n1 + n2)
    f1 = make_frame(rng, 160, 120, n1, n1 // 3 + 1)
    f2 = make_frame(rng, 160, 120, n2, n2 // 4 + 2)
    c1, c2 = np.flatnonzero(f1["is_corner"]), np.flatnonzero(f2["is_corner"])
    if n1 >= 4 and n2 >= 8:
        js = rng.permutation(n2)[:6]
        for k, d in enumerate((TH_LOW - 1, TH_LOW, TH_LOW + 1)):
            f2["descriptor"][c2[js[k]]] = flip_bits(f1["descriptor"][c1[k]], d, rng)
        f2["descriptor"][c2[js[3]]] = f2["descriptor"][c2[js[0]]]
        f2["descriptor"][c2[js[4]]] = f1["descriptor"][c1[3]]
        f2["descriptor"][c2[js[5]]] = f1["descriptor"][c1[3]]
    return f1, f2


def many_case(seed=5):
    """kf1 (id 0) and four others (ids 1..4), one of them without a corner: _many over [1, 2, 0, 3, 4]"""
    rng = np.random.default_rng(seed)
    frames = {0: make_frame(rng, 160, 120, 130, 40)}
    for kf, (n, other) in zip((1, 2, 3, 4), ((90, 10), (0, 7), (257, 0), (64, 64))):
        frames[kf] = make_frame(rng, 160, 120, n, other)
    c0 = np.flatnonzero(frames[0]["is_corner"])
    for kf in (1, 3, 4):  # near partners, so that every non-empty row has matches
        ck = np.flatnonzero(frames[kf]["is_corner"])
        for t in range(20):
            frames[kf]["descriptor"][ck[(7 * t + kf) % ck.size]] = flip_bits(frames[0]["descriptor"][c0[t + 10 * kf]],
                                                                               int(rng.integers(0, 60)), rng)
    return frames, [1, 2, 0, 3, 4]


NN_RATIO = 0.75


def bow_case(seed=3, disjoint=False):
    """Two frames with a featVec each.  Node ids 10 k + 3; frame1 holds nodes the other lacks and the other
    way round; node 53 has more than 64 features in frame2.  In node 23 frame1's first feature has
    (best, second) = (45, 60) and its second one (3, 4): NN_RATIO * second equals best, both rejected; its
    third one (44, 60), accepted; its fourth one two partners at the same distance 10 (second = best)."""
    rng = np.random.default_rng(seed)
    f1 = make_frame(rng, 160, 120, 220, 30)
    f2 = make_frame(rng, 160, 120, 300, 25)
    c1, c2 = list(np.flatnonzero(f1["is_corner"])), list(np.flatnonzero(f2["is_corner"]))
    rng.shuffle(c1)
    rng.shuffle(c2)

    def take(c, n):
        out = [int(i) for i in c[:n]]
        del c[:n]
        return out

    if disjoint:
        n1 = {3: take(c1, 40), 23: take(c1, 50), 63: take(c1, 30)}
        n2 = {13: take(c2, 60), 33: take(c2, 70), 73: take(c2, 20)}
        return f1, (sorted(n1), [n1[k] for k in sorted(n1)]), f2, (sorted(n2), [n2[k] for k in sorted(n2)])
    n1 = {3: take(c1, 20), 13: take(c1, 30), 23: take(c1, 12), 43: take(c1, 25), 53: take(c1, 40), 93: take(c1, 15)}
    n2 = {13: take(c2, 35), 23: take(c2, 20), 33: take(c2, 18), 53: take(c2, 90), 63: take(c2, 10), 93: take(c2, 30),
          103: take(c2, 5)}
    a, b = n1[23], n2[23]
    for (ia, pairs) in ((a[0], ((b[3], 45), (b[7], 60))), (a[1], ((b[1], 3), (b[11], 4))),
                        (a[2], ((b[5], 44), (b[9], 60))), (a[3], ((b[13], 10), (b[2], 10)))):
        for ib, d in pairs:
            f2["descriptor"][ib] = flip_bits(f1["descriptor"][ia], d, rng)
    # near partners in the shared nodes, at every distance around TH_LOW
    for node in (13, 53, 93):
        for t, ia in enumerate(n1[node][:12]):
            ib = n2[node][(3 * t + 1) % len(n2[node])]
            f2["descriptor"][ib] = flip_bits(f1["descriptor"][ia], 40 + t, rng)
    return f1, (sorted(n1), [n1[k] for k in sorted(n1)]), f2, (sorted(n2), [n2[k] for k in sorted(n2)])


def calib_of(w, h):
    """fxl, fyl, cxl, cyl and the float inverses as CalibHessian::setValueScaled leaves them"""
    fx, fy, cx, cy = F(0.9 * w), F(1.1 * h), F(0.5 * w - 0.5), F(0.5 * h - 0.5)
    return np.array([fx, fy, cx, cy, F(1) / fx, F(1) / fy, -cx / fx, -cy / fy], F)


def sim3_of(scale, rotvec, t):
    """Sophus' storage: quaternion (x, y, z, w) with squared norm = scale, then the translation"""
    rotvec = np.asarray(rotvec, D)
    th = np.linalg.norm(rotvec)
    q = np.array([0, 0, 0, 1.0]) if th == 0 else np.concatenate([np.sin(th / 2) * rotvec / th, [np.cos(th / 2)]])
    return np.concatenate([np.sqrt(scale) * q, np.asarray(t, D)])


def sim3_apply(scr, p):
    q, t = scr[:4], scr[4:]
    s = q @ q
    x, y, z, w = q / np.sqrt(s)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return s * (R @ p) + t, s, R


SIMILARITIES = {
    "identity": sim3_of(1.0, [0, 0, 0], [0, 0, 0]),
    "half": sim3_of(0.5, [0.02, -0.03, 0.05], [0.1, -0.05, 0.2]),
    "double": sim3_of(2.0, [-0.04, 0.01, -0.06], [-0.2, 0.1, 0.3]),
    "to_zero": sim3_of(1.0, [0, 0, 0], [0, 0, -2.0]),  # candidates of inv_d 0.5 land on pc[2] == 0, deeper ones behind
}
PROJECTION_SIZES = [(160, 120), (170, 130)]


def projection_case(w, h, sim, seed=21):
    """(cur, cand, centers, calib, scr): the current keyframe with about 150 corners, the contributions of
    its inverse-depth map (several on one pixel, some corners left as holes) and a candidate keyframe whose
    features are the current one's corners seen through the inverse similarity -- jittered, with bit-flipped
    descriptors and angles on both sides of the 0.2 gate -- plus candidates that project outside the image
    on each side, and a pair of equal corners in two neighbouring cells with one candidate between them."""
    rng = np.random.default_rng(seed + w)
    calib, scr = calib_of(w, h), SIMILARITIES[sim]
    fx, fy, cx, cy = (float(c) for c in calib[:4])
    cur = make_frame(rng, w, h, 150, 20)
    cc = np.flatnonzero(cur["is_corner"])
    # two equal corners either side of the border between cells ix = 1 and ix = 2
    ta, tb = cc[0], cc[1]
    for k, u in ((ta, 38), (tb, 42)):
        cur["u"][k], cur["v"][k] = u, 50
        cur["angle"][k] = F(0.3)
        cur["descriptor"][k] = cur["descriptor"][ta]
    # the map: a contribution on most corners, two on some (the later one wins), a few far from any corner
    centers, depth_of = [], {}
    for k in cc:
        if rng.random() < 0.2 and k not in (ta, tb):
            continue  # a hole
        idepth = F(rng.uniform(0.2, 2.0))
        jit = rng.uniform(-0.45, 0.45, 2)
        if rng.random() < 0.3:
            centers.append((cur["u"][k] - jit[0], cur["v"][k] - jit[1], F(rng.uniform(0.2, 2.0))))
        centers.append((cur["u"][k] + jit[0], cur["v"][k] + jit[1], idepth))
        depth_of[int(cur["v"][k]), int(cur["u"][k])] = idepth
    centers += [(-0.7, 3.2, 0.9), (w - 0.6, 5.0, 0.8), (float("nan"), 4.0, 0.7), (7.0, h + 3.0, 0.6), (-2.0, 8.0, 0.5)]
    centers = np.array(centers, F)
    # the candidates
    inv_s, s, R = None, None, None
    _, s, R = sim3_apply(scr, np.zeros(3))
    t = scr[4:]
    cand = []

    def add(u_cur, v_cur, idepth, desc, angle, is_corner=1, usable=1):
        pc = np.array([(u_cur - cx) / fx, (v_cur - cy) / fy, 1.0]) / idepth
        p_ref = R.T @ (pc - t) / s
        cand.append((fx * p_ref[0] / p_ref[2] + cx, fy * p_ref[1] / p_ref[2] + cy, angle, 1.0 / p_ref[2], is_corner,
                     usable, desc))

    for n, k in enumerate(cc):
        pix = (int(cur["v"][k]), int(cur["u"][k]))
        idepth = depth_of.get(pix, F(1.0))
        jit = rng.uniform(-3, 3, 2)
        d_angle = (0.05, -0.15, 0.19, 0.21, -0.3)[n % 5]
        desc = flip_bits(cur["descriptor"][k], int(rng.integers(0, 70)), rng)
        add(cur["u"][k] + jit[0], cur["v"][k] + jit[1], idepth, desc, cur["angle"][k] + d_angle, usable=n % 11 != 0)
    add(40.0, 50.0, 1.0, flip_bits(cur["descriptor"][ta], 7, rng), 0.3)  # between the two equal corners
    for (u_out, v_out) in ((w + 60.0, 40.0), (-70.0, 40.0), (30.0, h + 60.0), (30.0, -70.0)):
        add(u_out, v_out, 1.0, cur["descriptor"][cc[5]], cur["angle"][cc[5]])
    for n in range(6):  # plain usable features: descriptor 0, angle 0
        add(float(rng.uniform(10, w - 10)), float(rng.uniform(10, h - 10)), 1.0, np.zeros(32, np.uint8), 0.0, is_corner=0)
    cand = np.array(cand, FEATURE_DTYPE)
    if sim == "to_zero":
        cand["inv_d"][::3] = F(0.5)  # pRef[2] = 2 exactly: pc[2] = 0
        cand["inv_d"][1::3] = F(0.25)  # pRef[2] = 4: ... and these stay in front; the rest lies behind
        cand["inv_d"][2::3] = F(0.75)
    cand["inv_d"][-1] = F(0)  # 1.0 / 0: nothing is finite
    cand["inv_d"][-2] = F(-1)  # Feature's default: a point behind the candidate's camera
    # a candidate outside its own keyframe's grid cannot be a corner there (the store refuses such a put)
    gw, gh = w // GRID, h // GRID
    inside = (cand["u"] >= 0) & (cand["v"] >= 0) & (cand["u"] < gw * GRID) & (cand["v"] < gh * GRID)
    cand["is_corner"] &= inside
    return cur, cand, centers, calib, scr
