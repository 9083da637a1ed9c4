"""Scenes for the coarse initializer's tests: a first frame (synth.make_tracker_scene's image), new frames
derived from it, and point lists with brute-force neighbour / parent tables (init_ref.knn_tables).

New frames:
  same     the first image again: with t ~ 0 the alpha energy stays under the cap, so the run never snaps
  shift    the first image resampled bilinearly by the horizontal shift fx * 0.03 of a plane at inverse depth
           1 under t = (0.03, 0, 0); |t| is above sqrt(alphaK / alphaW) = 1 / 60, so the cap engages and the
           run snaps
  expo     as shift, the intensities and the exposure scaled by 1.3, fix_affine 0
"border" shifts the other way (t = (-0.03, 0, 0)), so that its strip of points 3 pixels from the left border
leaves the image pixel by pixel as the steps grow.
Point lists: integer pixel positions + 0.1 as setFirst makes them, row-major, at least 3 pixels from the
border (the walk's range), the strongest gradients among random candidates.
"""
import functools

import numpy as np

import init_ref as IR
import oracle
from ldso_amd import synth

f32 = np.float32
T_TRUE = np.array([0.03, 0.0, 0.0])


def shifted(img, s):
    """I_new(x, y) = I(x - s, y), bilinear, the border columns repeated."""
    h, w = img.shape
    x = np.clip(np.arange(w, dtype=np.float64) - s, 0, w - 1)
    x0 = np.minimum(np.floor(x).astype(np.int64), w - 2)
    fx = x - x0
    return ((1 - fx) * img[:, x0] + fx * img[:, x0 + 1]).astype(f32)


def pick_points(ag, wl, hl, n, rng, border=3):
    """n distinct pixels of [border, wl - border - 2) x [border, hl - border - 2), row-major: the strongest
    absSquaredGrad among 4 n random candidates."""
    xs, ys = np.arange(border, wl - border - 2), np.arange(border, hl - border - 2)
    cand = rng.choice(xs.size * ys.size, size=min(4 * n, xs.size * ys.size), replace=False)
    cx, cy = xs[cand % xs.size], ys[cand // xs.size]
    keep = np.argsort(-ag[cy * wl + cx], kind="stable")[:n]
    idx = np.sort(cy[keep] * wl + cx[keep])
    return np.stack([idx % wl + 0.1, idx // wl + 0.1], axis=1).astype(f32)


class Scene:
    def __init__(self, name, width, height, counts, kind, seed, *, no_nbrs=False, border=False, direction=1.0):
        self.name, self.width, self.height, self.kind = name, width, height, kind
        self.levels = oracle.ct_levels(width, height)
        assert self.levels == len(counts)
        self.calib = np.array([0.87 * width, 0.87 * width, 0.5 * width - 0.5, 0.5 * height - 0.5], f32)
        self.first, _ = synth.make_tracker_scene(width, height, n_points=(1,), seed=seed)
        self.first_exposure = 1.0
        self.first_dI = oracle.make_images(self.first, width, height)
        rng = np.random.default_rng(1000 + seed)
        uv = []
        for l, n in enumerate(counts):
            wl, hl = width >> l, height >> l
            p = pick_points(self.first_dI[l][1], wl, hl, n, rng)
            if border and l == 0:  # a strip of points 3 pixels from each border
                ys = np.arange(3, hl - 5, 7, dtype=f32) + f32(0.1)
                edge = np.concatenate([np.stack([np.full_like(ys, x0 + 0.1), ys], 1) for x0 in (3, wl - 6)])
                p = np.unique(np.concatenate([p, edge.astype(f32)]), axis=0)
                p = p[np.lexsort((p[:, 0], p[:, 1]))]
            uv.append(p)
        nbrs, parents = IR.knn_tables(uv)
        if no_nbrs:
            for nb in nbrs:
                nb[::7] = -1
        self.points = IR.make_points(uv, nbrs, parents)
        self.params = dict(fix_affine=0) if kind == "expo" else {}
        self.direction = direction

    def frame(self, k=1):
        """(image, exposure) of new frame k: shift scenes move on by t = 0.03 k."""
        if self.kind == "same":
            return self.first, 1.0
        img = shifted(self.first, self.direction * float(self.calib[0]) * T_TRUE[0] * k)
        return (img * f32(1.3), 1.3) if self.kind == "expo" else (img, 1.0)

    def frame_dI(self, k=1):
        img, e = self.frame(k)
        return [d for d, _ in oracle.make_images(img, self.width, self.height)], e

    def reference(self, **params):
        return IR.Initializer(self.width, self.height, self.calib, [d for d, _ in self.first_dI], self.first_exposure,
                              self.points, **dict(self.params, **params))


CASES = {
    "same": dict(width=320, height=240, counts=(600, 150, 40), kind="same", seed=1),
    "shift": dict(width=320, height=240, counts=(600, 150, 40), kind="shift", seed=1),
    "expo": dict(width=320, height=240, counts=(600, 150, 40), kind="expo", seed=5),
    "wide5": dict(width=1232, height=368, counts=(300, 200, 150, 80, 40), kind="shift", seed=29),
    "one_point_level": dict(width=320, height=240, counts=(600, 150, 1), kind="shift", seed=4),
    "no_neighbours": dict(width=320, height=240, counts=(600, 150, 40), kind="shift", seed=5, no_nbrs=True),
    "border": dict(width=320, height=240, counts=(300, 150, 40), kind="shift", seed=6, border=True, direction=-1.0),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(name, **CASES[name])
