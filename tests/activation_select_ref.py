"""CoarseDistanceMap (CoarseTracker.cc:795-932) and the walk of FullSystem::activatePointsMT
(FullSystem.cc:1220-1298), restated literally from the reference text: numpy float32 scalars, one
operation per expression (no contraction can happen), Python lists for the two BFS lists, the walk in
order with a real stamp (addIntoDistFinal) for every accept.  Also the order-free model of the stamped
map that DESIGN.md §9e states, so that test_activation_select_ref.py can pin it against the stamps.

Rule that is the library's: `int u = float` of a value that is not finite or does not fit is INT_MIN
(x86's truncating conversion), which fails `u > 0`."""
import numpy as np

F = np.float32
INT_MIN = -(1 << 31)
KEEP, DELETE, OPTIMIZE = 0, 1, 2
IPS_GOOD, IPS_OOB, IPS_OUTLIER, IPS_SKIPPED, IPS_BADCONDITION, IPS_UNINITIALIZED = range(6)


def to_int(f):
    f = F(f)
    if not np.isfinite(f) or f >= F(2147483648.0) or f < F(-2147483648.0):
        return INT_MIN
    return int(f)  # truncation toward zero


def project(krki, kt, u, v, d):
    """ptp = KRKi * Vec3f(u, v, 1) + Kt * d (Eigen: per row three products summed left to right) and
    int u = ptp[0] / ptp[2] + 0.5f."""
    with np.errstate(all="ignore"):
        krki = np.asarray(krki, F).reshape(3, 3)
        kt = np.asarray(kt, F).reshape(3)
        u, v, d = F(u), F(v), F(d)
        ptp = []
        for i in range(3):
            s = F(F(krki[i, 0] * u) + F(krki[i, 1] * v))
            s = F(s + F(krki[i, 2] * F(1)))
            ptp.append(F(s + F(kt[i] * d)))
        x = to_int(F(F(ptp[0] / ptp[2]) + F(0.5)))
        y = to_int(F(F(ptp[1] / ptp[2]) + F(0.5)))
    return x, y, ptp[0]


class DistanceMap:
    """fwdWarpedIDDistFinal of level 1 with growDistBFS and addIntoDistFinal."""

    def __init__(self, w1, h1):
        self.w1, self.h1 = int(w1), int(h1)
        self.m = [F(1000)] * (self.w1 * self.h1)

    def grow(self, lst):
        w1, h1, m = self.w1, self.h1, self.m
        for k in range(1, 40):
            prev, lst = lst, []
            for x, y in prev:
                if x == 0 or y == 0 or x == w1 - 1 or y == h1 - 1:
                    continue
                idx = x + y * w1
                nb = [(1, 0), (-1, 0), (0, 1), (0, -1)]
                if k % 2 == 1:
                    nb += [(1, 1), (-1, 1), (-1, -1), (1, -1)]
                for dx, dy in nb:
                    j = idx + dx + dy * w1
                    if m[j] > k:
                        m[j] = F(k)
                        lst.append((x + dx, y + dy))

    def make(self, seeds):
        """seeds: the kept projections (u, v) in order, duplicates included."""
        self.m = [F(1000)] * (self.w1 * self.h1)
        lst = []
        for x, y in seeds:
            self.m[x + self.w1 * y] = F(0)
            lst.append((x, y))
        self.grow(lst)

    def add(self, x, y):
        self.m[x + self.w1 * y] = F(0)
        self.grow([(x, y)])

    def array(self):
        return np.array(self.m, F).reshape(self.h1, self.w1)


def make_distance_map(w1, h1, krki1, kt1, uvd, host):
    """makeDistanceMap over active points uvd [n][3] with host [n] -> DistanceMap."""
    seeds = []
    for (u, v, d), h in zip(np.asarray(uvd, F).reshape(-1, 3), np.asarray(host).reshape(-1)):
        x, y, _ = project(krki1[h], kt1[h], u, v, d)
        if x > 0 and y > 0 and x < w1 and y < h1:
            seeds.append((x, y))
    dm = DistanceMap(w1, h1)
    dm.make(seeds)
    return dm


def classify(p, flagged, min_quality=3.0):
    """One record before the distance test -> DELETE, KEEP or None (canActivate)."""
    st = int(p["last_status"])
    if not np.isfinite(p["idepth_max"]) or st == IPS_OUTLIER:
        return DELETE
    with np.errstate(all="ignore"):
        can = (st in (IPS_GOOD, IPS_SKIPPED, IPS_BADCONDITION, IPS_OOB) and F(p["last_interval"]) < 8
               and F(p["quality"]) > F(min_quality) and F(F(p["idepth_max"]) + F(p["idepth_min"])) > 0)
    if not can:
        return DELETE if (flagged or st == IPS_OOB) else KEEP
    return None


def walk(dm, pts, krki1, kt1, current_min_act_dist, newest_host, flagged=None, min_quality=3.0):
    """The walk over records `pts` (IMMATURE_DTYPE) on DistanceMap dm, which it stamps.  Hosts ascending,
    newest_host skipped, each host's records in the order they have in pts.
    -> (dispositions [n], selected indices in walk order, counts [kept, deleted, selected, by distance])."""
    n = len(pts)
    disp = np.zeros(n, np.int32)
    sel = []
    by_dist = 0
    w1, h1 = dm.w1, dm.h1
    hosts = np.asarray(pts["host"])
    for h in sorted(set(hosts.tolist())):
        if h == newest_host:
            continue
        for i in np.nonzero(hosts == h)[0]:
            p = pts[i]
            c = classify(p, bool(flagged[h]) if flagged is not None else False, min_quality)
            if c is not None:
                disp[i] = c
                continue
            d = F(F(0.5) * F(F(p["idepth_max"]) + F(p["idepth_min"])))
            x, y, ptp0 = project(krki1[h], kt1[h], p["u"], p["v"], d)
            if not (x > 0 and y > 0 and x < w1 and y < h1):
                disp[i] = DELETE
                continue
            dist = F(dm.m[x + w1 * y] + F(ptp0 - np.floor(ptp0)))
            if dist >= F(F(current_min_act_dist) * F(p["type"])):
                dm.add(x, y)
                disp[i] = OPTIMIZE
                sel.append(int(i))
            else:
                by_dist += 1
    counts = [int((disp == KEEP).sum()), int((disp == DELETE).sum()), len(sel), by_dist]
    return disp, np.array(sel, np.int32), counts


# ---- the order-free model ------------------------------------------------------
def steps(dx, dy):
    """Steps of the alternating 8 / 4 growth between two pixels in free space: the smallest k < 40 with
    max(|dx|, |dy|) <= k and |dx| + |dy| <= k + ceil(k / 2); 1000 if there is none."""
    dx, dy = abs(dx), abs(dy)
    k = max(dx, dy)
    while dx + dy > k + (k + 1) // 2:
        k += 1
    return k if k < 40 else 1000


def model_value(w1, h1, m0, sources, x, y):
    """The map at (x, y) after the stamps `sources` (in order) on the initial map m0 [h1][w1], without
    running a stamp.  Pixels with x == 0 or y == 0 are never read by the walk and are not modelled."""
    def border(px, py):
        return px == 0 or py == 0 or px == w1 - 1 or py == h1 - 1

    def interior_value(px, py):
        v = int(m0[py][px])
        for sx, sy in sources:
            if not border(sx, sy):
                v = min(v, steps(sx - px, sy - py))
        return v

    assert x > 0 and y > 0
    if not border(x, y):
        return interior_value(x, y)
    v = int(m0[y][x])
    if (x, y) in sources:
        v = 0
    if x == w1 - 1 and y == h1 - 1:
        qx, qy = w1 - 2, h1 - 2
        if border(qx, qy):
            return v
        run = int(m0[qy][qx])  # the running minimum of the diagonal neighbour
        for sx, sy in sources:
            if border(sx, sy):
                continue
            t = steps(sx - qx, sy - qy)
            if t < run:
                run = t
                if t % 2 == 0 and t + 1 < 40:
                    v = min(v, t + 1)
        return v
    if x == w1 - 1:
        four, diag = [(x - 1, y)], [(x - 1, y - 1), (x - 1, y + 1)]
    else:
        four, diag = [(x, y - 1)], [(x - 1, y - 1), (x + 1, y - 1)]
    for px, py in four:
        if not border(px, py):
            t = interior_value(px, py)
            if t + 1 < 40:
                v = min(v, t + 1)
    for px, py in diag:
        if not border(px, py):
            t = interior_value(px, py)
            if t % 2 == 0 and t + 1 < 40:
                v = min(v, t + 1)
    return v


def corner_by_levels(w1, h1, m0, sources):
    """The corner's value as k_ct_as_round_corner finds it, without a running minimum: the source that
    lowers (w1-2, h1-2) to T is the earliest of those within T steps of it, if it is at T exactly; the
    smallest even T with such a source gives T + 1."""
    def border(px, py):
        return px == 0 or py == 0 or px == w1 - 1 or py == h1 - 1

    v = int(m0[h1 - 1][w1 - 1])
    if (w1 - 1, h1 - 1) in sources:
        v = 0
    qx, qy = w1 - 2, h1 - 2
    if border(qx, qy):
        return v
    T = 0
    while T < 39 and T < int(m0[qy][qx]) and T + 1 < v:
        near = [steps(sx - qx, sy - qy) for sx, sy in sources if not border(sx, sy)]
        near = [t for t in near if t <= T]
        if near and near[0] == T:
            v = T + 1
        T += 2
    return v
