"""Scenes for the activation selection (tests/test_activation_select*.py): level-1 host tables, active
points as seeds and hand-made immature records, all from seeds.  A scene is a dict: w, h (frame), krki1
[n_hosts][9], kt1 [n_hosts][3], uvd [n][3], seed_host [n], pts (IMMATURE_DTYPE, hosts ascending), cmad,
newest (= n_hosts - 1), flagged [n_hosts]."""
import numpy as np

from ldso_amd import _lib as L

# K[1] Ki[0] for any pinhole: level-1 pixel x1 = 0.5 u - 0.25, so u = 2 x1 + 0.5 lands on x1 exactly
PLAIN = np.array([0.5, 0, -0.25, 0, 0.5, -0.25, 0, 0, 1], np.float32)


def tables(rng, w, h, n_hosts, wild=True):
    """Host 0 plain; the others a small rotation and translation about it; with `wild` the last but one
    host looks away (ptp[2] <= 0 for most depths) and its neighbour throws projections out of the image."""
    krki, kt = [PLAIN.copy()], [np.zeros(3, np.float32)]
    for i in range(1, n_hosts):
        f = 0.8 * w
        K0 = np.array([[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1.0]])
        K1 = np.array([[f / 2, 0, (K0[0, 2] + 0.5) / 2 - 0.5], [0, f / 2, (K0[1, 2] + 0.5) / 2 - 0.5], [0, 0, 1.0]])
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        ang = float(rng.uniform(0, 0.1))
        A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * A @ A
        t = rng.standard_normal(3) * np.array([0.05, 0.05, 0.02])
        if wild and i == n_hosts - 2:
            t = np.array([0.0, 0.0, -2.0])  # ptp[2] = 1 - 2 d
        if wild and i == n_hosts - 3:
            t = np.array([3.0, -2.0, 0.1])
        krki.append((K1 @ R @ np.linalg.inv(K0)).astype(np.float32).reshape(9))
        kt.append((K1 @ t).astype(np.float32))
    return np.stack(krki), np.stack(kt)


def records(n, host, u, v, type_=1.0, idepth=(0.4, 0.6), status=0, interval=1.0, quality=10.0):
    p = np.zeros(n, L.IMMATURE_DTYPE)
    p["u"], p["v"], p["host"], p["type"] = u, v, host, type_
    p["idepth_min"], p["idepth_max"] = idepth
    p["last_status"], p["last_interval"], p["quality"] = status, interval, quality
    p["energy_th"] = 8 * 144
    return p


def scene(w, h, krki1, kt1, uvd, seed_host, pts, cmad, flagged=None):
    n_hosts = len(krki1)
    pts = np.ascontiguousarray(pts[np.argsort(pts["host"], kind="stable")])
    return dict(w=w, h=h, krki1=np.asarray(krki1, np.float32), kt1=np.asarray(kt1, np.float32),
                uvd=np.asarray(uvd, np.float32).reshape(-1, 3), seed_host=np.asarray(seed_host, np.int32).reshape(-1),
                pts=pts, cmad=float(cmad), newest=n_hosts - 1,
                flagged=np.zeros(n_hosts, np.uint8) if flagged is None else np.asarray(flagged, np.uint8))


def random_scene(seed, w, h, hosts, n_seeds, n_recs, cmad):
    """`hosts` hosts and the newest; records of every kind, types 1, 2 and 4 mixed."""
    rng = np.random.default_rng(77000 + seed)
    n_hosts = hosts + 1
    krki1, kt1 = tables(rng, w, h, n_hosts, wild=hosts >= 4)
    uvd = np.stack([rng.uniform(0, w, n_seeds), rng.uniform(0, h, n_seeds), rng.uniform(0.1, 1.0, n_seeds)], 1)
    seed_host = rng.integers(0, hosts, n_seeds)
    p = records(n_recs, rng.integers(0, n_hosts, n_recs), rng.uniform(-2, w + 2, n_recs), rng.uniform(-2, h + 2, n_recs),
                rng.choice([1.0, 2.0, 4.0], n_recs))
    lo = rng.uniform(-0.2, 1.0, n_recs).astype(np.float32)
    p["idepth_min"], p["idepth_max"] = lo, lo + rng.uniform(0, 0.5, n_recs).astype(np.float32)
    k = rng.random(n_recs)
    p["idepth_max"][k < 0.05] = np.nan
    p["idepth_max"][(k >= 0.05) & (k < 0.07)] = np.inf
    p["idepth_min"][(k >= 0.07) & (k < 0.10)] = -p["idepth_max"][(k >= 0.07) & (k < 0.10)]  # sum exactly 0
    p["last_status"] = rng.choice([0, 0, 0, 0, 1, 2, 3, 4, 5], n_recs)
    p["last_interval"] = rng.choice([0.5, 2.0, 7.9, 8.0, 12.0], n_recs, p=[0.4, 0.3, 0.1, 0.1, 0.1])
    p["quality"] = rng.choice([1.0, 3.0, 3.0001, 5.0, 10000.0], n_recs, p=[0.05, 0.1, 0.15, 0.4, 0.3])
    flagged = (rng.random(n_hosts) < 0.4).astype(np.uint8)
    return scene(w, h, krki1, kt1, uvd, seed_host, p, cmad, flagged)


def at_pixels(w, h, xy, types, cmad, seeds_xy=(), fracs=None, hosts=2):
    """Candidates at the level-1 pixels xy (in walk order, all on host 0 unless `hosts` spreads them in
    blocks) through the plain table; fracs: the fraction each adds (u = 2 (x + frac) + 0.5 keeps the
    pixel for frac < 0.5)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    fr = np.zeros(n) if fracs is None else np.asarray(fracs, np.float64)
    n_hosts = hosts + 1
    krki1 = np.tile(PLAIN, (n_hosts, 1))
    kt1 = np.zeros((n_hosts, 3), np.float32)
    host = (np.arange(n) * hosts) // max(n, 1)
    p = records(n, host, 2 * (xy[:, 0] + fr) + 0.5, 2 * xy[:, 1] + 0.5, types)
    s = np.asarray(seeds_xy, np.float64).reshape(-1, 2)
    uvd = np.stack([2 * s[:, 0] + 0.5, 2 * s[:, 1] + 0.5, np.full(len(s), 0.5)], 1)
    return scene(w, h, krki1, kt1, uvd, np.zeros(len(s), np.int32), p, cmad)


def snake(w1, h1, reverse=False):
    """Every pixel the walk can accept, one pixel apart from the previous one."""
    xy = []
    for y in range(1, h1):
        xs = range(1, w1) if y % 2 else range(w1 - 1, 0, -1)
        xy += [(x, y) for x in xs]
    return xy[::-1] if reverse else xy


def border_scene(w, h, first, cmad=2.0):
    """The 10 x 10 example moved into the frame's bottom right corner: stamps (7, 3) and (4, 3) of a
    10 x 10 grid in the order `first` says, then candidates of type 4 on the corner, on (w1-2, h1-2), on
    the last row and the last column; seeds on the last row and column too."""
    w1, h1 = w >> 1, h >> 1
    ox, oy = w1 - 10, h1 - 10
    a, b = (ox + 7, oy + 3), (ox + 4, oy + 3)
    xy = [a, b] if first == 0 else [b, a]
    xy += [(w1 - 1, h1 - 1), (w1 - 2, h1 - 2), (w1 - 1, h1 - 1), (w1 - 5, h1 - 1), (w1 - 1, h1 - 6), (w1 - 1, 3),
           (3, h1 - 1), (w1 - 1, h1 - 2), (w1 - 2, h1 - 1), (w1 - 1, h1 - 1)]
    types = [1, 1] + [4, 4, 4, 2, 2, 1, 1, 1, 1, 1]
    seeds = [(2, h1 - 1), (w1 - 1, 2), (5, 5)]
    return at_pixels(w, h, xy, np.array(types, np.float32), cmad, seeds, hosts=1)


def all_scenes():
    """name -> scene, built on demand."""
    S = {}
    k = 0
    # random: both frames, 2 and 5 hosts, 0 / 1 / ~300 seeds, 1 / ~1200 records, every threshold
    for (w, h), hosts, n_seeds, n_recs, cmad in [
            ((64, 48), 2, 0, 1200, 2.0), ((64, 48), 5, 300, 1200, 0.0), ((64, 48), 5, 300, 1200, 0.7),
            ((64, 48), 2, 300, 1200, 2.0), ((64, 48), 5, 1, 1200, 4.0), ((64, 48), 2, 1, 1, 2.0),
            ((70, 50), 5, 0, 1200, 4.0), ((70, 50), 2, 300, 1200, 0.0), ((70, 50), 2, 1, 1200, 0.7),
            ((70, 50), 5, 300, 1200, 2.0), ((70, 50), 5, 300, 1200, 4.0), ((70, 50), 2, 0, 1, 0.0)]:
        S[f"random-{w}x{h}-{hosts}h-{n_seeds}s-{n_recs}r-{cmad}"] = (random_scene, (k, w, h, hosts, n_seeds, n_recs, cmad))
        k += 1
    rng = np.random.default_rng(5)
    ty = rng.choice([1.0, 2.0, 4.0], 1200).astype(np.float32)
    fr = rng.uniform(0, 0.49, 1200)
    for cmad in (0.0, 0.7, 2.0):
        S[f"one-pixel-{cmad}"] = (at_pixels, (64, 48, [(11, 7)] * 1200, ty, cmad, (), fr))
    S["one-pixel-corner-0.7"] = (at_pixels, (70, 50, [(34, 24)] * 1200, ty, 0.7, (), fr))
    for (w, h) in ((64, 48), (70, 50)):
        for rev in (False, True):
            xy = snake(w >> 1, h >> 1, rev)
            S[f"snake-{w}x{h}-{'rev' if rev else 'fwd'}-2.0"] = (at_pixels, (w, h, xy, np.ones(len(xy), np.float32), 2.0))
    xy = snake(32, 24)
    S["snake-type4-4.0"] = (at_pixels, (64, 48, xy, np.full(len(xy), 4, np.float32), 4.0))
    S["snake-mixed-0.7"] = (at_pixels, (64, 48, xy, ty[:len(xy)], 0.7, [(9, 9)], fr[:len(xy)]))
    for (w, h) in ((64, 48), (70, 50)):
        for first in (0, 1):
            S[f"border-{w}x{h}-{first}"] = (border_scene, (w, h, first))
    return S


def build(entry):
    fn, args = entry
    return fn(*args)
