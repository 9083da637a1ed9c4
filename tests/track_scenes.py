"""The scenes and cases of the trackNewestCoarse tests (test_track_ref.py on the CPU, test_track.py on
the GPU): synth.make_tracker_scene's image as reference keyframe and new frame at once, so the truth
is the identity pose with the reference's own (a, b), and the oracle's calcRes / calcGSSSE as the
callables of track_ref.track."""
import functools

import numpy as np

import oracle
import track_ref
from ldso_amd import synth

REF_AB = (0.02, 3.0)  # lastRef_aff_g2l; both exposures 1
SIZES = {"qvga": ((320, 240), (1500, 300, 100)),   # level 0: five chunks of 256 and 220 more, level 2 under one
         "vga": ((640, 480), (700, 256, 64, 10)),
         "kitti": ((1232, 368), (300, 200, 120, 60, 30))}
MODES = {"ab": (1e12, 1e8), "fix_ab": (-1.0, -1.0), "fix_b": (0.0, -1.0), "fix_a": (-1.0, 0.0)}


class Scene:
    def __init__(self, name, seed=0, far_level=None):
        (w, h), n_points = SIZES[name]
        self.w, self.h = w, h
        self.color, make_pc = synth.make_tracker_scene(w, h, n_points=n_points, seed=seed)
        self.levels = oracle.make_images(self.color, w, h)
        self.pcs = make_pc([dI[:, 0] for dI, _ in self.levels])
        if far_level is not None:  # a level none of whose points lands in the image
            self.pcs[far_level] = dict(u=np.full(5, 1e4, np.float32), v=np.full(5, 1e4, np.float32),
                                       idepth=np.ones(5, np.float32), color=np.ones(5, np.float32))
        self.calib = np.array([384.0, 432.0, 319.5, 239.5], np.float32) * np.float32(w / 640)
        self.calib[2], self.calib[3] = (w - 1) / 2, (h - 1) / 2
        self.K = oracle.ct_make_k(self.calib, w, h)
        self.n_levels = len(self.levels)
        self.coarsest = min(self.n_levels, 5) - 1

    def pc(self, l):
        p = self.pcs[l]
        return (p["u"], p["v"], p["idepth"], p["color"])

    def aff6(self, ab):
        return (1.0, 1.0, REF_AB[0], REF_AB[1], float(ab[0]), float(ab[1]))

    # the oracle as track_ref.track's callables; noise: relative noise on E, H and b (a Generator, sigma)
    def calc_res(self, lvl, T, ab, cutoff, noise=None):
        rs, warped = oracle.ct_calc_res(lvl, self.w >> lvl, self.h >> lvl, self.K[lvl], self.levels[lvl][0],
                                        self.pc(lvl), T, self.aff6(ab), cutoff)
        if noise:
            rs[0] *= 1 + noise[1] * noise[0].standard_normal()
        return rs, warped

    def calc_gs(self, lvl, warped, ab, noise=None):
        H, b = oracle.ct_calc_gs(warped, self.K[lvl, 0], self.K[lvl, 1], self.aff6(ab))
        if noise:
            H = H * (1 + noise[1] * noise[0].standard_normal(H.shape))
            b = b * (1 + noise[1] * noise[0].standard_normal(b.shape))
        return H, b

    def track(self, T, ab, min_res, noise=None, **params):
        """The oracle-driven restatement."""
        return track_ref.track(functools.partial(self.calc_res, noise=noise), functools.partial(self.calc_gs, noise=noise),
                               T, ab, self.coarsest, min_res, ref_frame=(1.0, 1.0) + REF_AB, **params)

    def tracker(self):
        """The scene on the device."""
        from ldso_amd.tracker import CoarseTracker

        ct = CoarseTracker(self.w, self.h)
        ct.make_k(self.calib)
        ct.set_new_frame(self.color, 1.0)
        ct.set_reference([self.pc(l) for l in range(self.n_levels)], 1.0, REF_AB)
        return ct


@functools.lru_cache(maxsize=None)
def scene(name, seed=0, far_level=None):
    return Scene(name, seed, far_level)


def pose(i=0, scale=1.0):
    rng = np.random.default_rng(100 + i)
    return synth.se3_matrix(rng.normal(0, 2e-3, 3) * scale, rng.normal(0, 1e-2, 3) * scale)


NEVER = (np.nan,) * 5  # no residual is above 1.5 NaN
# name -> (scene arguments, start pose, start (a, b), min_res_for_abort, params): each produces, on the oracle
# alone, the event test_track_ref.test_cases_produce_their_events asserts for it
CASES = {
    "reject": (("vga", 3), pose(3, 3.0), REF_AB, NEVER, {}),
    "extrapolate": (("vga", 1), pose(1, 6.0), (0.3, 20.0), NEVER, {}),
    "cutoff_repeat": (("qvga", 2), pose(2, 1.0), (REF_AB[0], REF_AB[1] + 60.0), NEVER, {}),
    "abort_coarsest": (("vga", 3), pose(3, 3.0), REF_AB, (0.01,) * 5, {}),
    "abort_level0": (("qvga", 4), pose(4, 1.0), REF_AB, (1e-6, 1e9, 1e9, 1e9, 1e9), {}),
    "affine_too_big": (("qvga", 5), pose(5, 1.0), (REF_AB[0], 250.0), NEVER,
                       dict(affine_opt_mode_a=-1.0, affine_opt_mode_b=-1.0)),
    # exp(8) times the reference's colours saturates nearly every residual under every cutoff: a stays far off
    "rel_affine_too_big": (("qvga", 6), pose(6, 1.0), (REF_AB[0] + 8.0, REF_AB[1]), NEVER,
                           dict(affine_opt_mode_a=0.0, affine_opt_mode_b=0.0)),
    "empty_level": (("kitti", 7, 2), pose(7, 1.0), REF_AB, NEVER, {}),
}
CONVERGENCE = [("qvga", 10, 1.0), ("vga", 11, 2.0), ("kitti", 12, 1.0)]  # scene, pose(i), scale


def params_of(case_params, mode=None, solve=None):
    p = dict(case_params)
    if mode is not None:
        p["affine_opt_mode_a"], p["affine_opt_mode_b"] = MODES[mode]
    if solve is not None:
        p["solve"] = solve
    return p
