#!/usr/bin/env python3
"""Host-clock timing of trackNewestCoarse's LM loop, two routes alternated:

  before  the loop on the host, one ldso_ct_calc_res_gs round trip per evaluation and ldso_ct_lm_step
          per step (the only route before ldso_ct_track; the loop's own logic is a few Python
          statements per evaluation, on the host clock like everything else);
  after   ldso_ct_track, the whole loop in one launch,

for one start and for eight (the host route runs its eight loops one after another), on bench.py's
640x480 tracker scene and a KITTI-sized one.  Median of --reps; one JSON document on stdout.

    python tools/time_track.py [--reps 50] [--out FILE]
    python tools/time_track.py --probe [--out FILE]

--probe: where one workgroup's time goes.  ldso_ct_track alone, one start, from every coarsest level, on the
bench scene, on 256 points per level (one sweep per evaluation) and on a 32,000-point level 0; with the
evaluations each run made.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldso_amd import _lib as L  # noqa: E402
from ldso_amd import synth  # noqa: E402
from ldso_amd.tracker import CoarseTracker  # noqa: E402

f32 = np.float32
LIMIT = f32(0.001)
MAX_IT = (10, 20, 50, 50, 50)


class HostLoop:
    """trackNewestCoarse (CoarseTracker.cc:61-310) with the default settings and no abort threshold, over the
    C ABI: buffers and ctypes pointers made once."""

    def __init__(self, ct):
        self.ct, self.lib = ct, L.lib()
        self.T, self.Tn = np.zeros((3, 4)), np.zeros((3, 4))
        self.ab, self.abn = np.zeros(2), np.zeros(2)
        self.rs, self.H, self.b, self.inc = np.zeros(6), np.zeros((8, 8)), np.zeros(8), np.zeros(8)
        self.Ha, self.ba = np.zeros((8, 8)), np.zeros(8)
        self.p = {k: L.ptr(getattr(self, k), L.f64p) for k in ("T", "Tn", "ab", "abn", "rs", "H", "b", "inc", "Ha", "ba")}
        self.params = L.LdsoCtTrackParams()
        self.lib.ldso_ct_track_default_params(C.byref(self.params))

    def evaluate(self, lvl, pT, ab, cutoff):
        L.check(self.lib.ldso_ct_calc_res_gs(self.ct._h, lvl, pT, float(ab[0]), float(ab[1]), float(cutoff), self.p["rs"],
                                             self.p["H"], self.p["b"]))

    def run(self, T0, ab0, coarsest):
        self.T[...] = T0
        self.ab[...] = ab0
        iterations, evaluations, repeated = [0] * 5, 0, False
        lvl = coarsest
        while lvl >= 0:
            repeat = f32(1)
            self.evaluate(lvl, self.p["T"], self.ab, 20 * repeat)
            evaluations += 1
            while self.rs[5] > 0.6 and repeat < 50:
                repeat *= f32(2)
                self.evaluate(lvl, self.p["T"], self.ab, 20 * repeat)
                evaluations += 1
            old = self.rs[0] / self.rs[1]
            self.Ha[...] = self.H
            self.ba[...] = self.b
            lam = f32(0.01)
            for _ in range(MAX_IT[lvl]):
                L.check(self.lib.ldso_ct_lm_step(self.p["Ha"], self.p["ba"], float(lam), self.p["T"], self.p["ab"],
                                                 C.byref(self.params), self.p["inc"], self.p["Tn"], self.p["abn"]))
                self.evaluate(lvl, self.p["Tn"], self.abn, 20 * repeat)
                evaluations += 1
                iterations[lvl] += 1
                new = self.rs[0] / self.rs[1]
                if new < old:
                    old = new
                    self.Ha[...] = self.H
                    self.ba[...] = self.b
                    self.T[...] = self.Tn
                    self.ab[...] = self.abn
                    lam = f32(lam * 0.5)
                else:
                    lam = max(f32(lam * 4.0), LIMIT)
                if not (np.sqrt(self.inc @ self.inc) > 1e-3):
                    break
            if repeat > 1 and not repeated:
                repeated = True
            else:
                lvl -= 1
        return iterations, evaluations


def scene(w, h, n_points):
    calib = np.array([384.0, 432.0, 319.5, 239.5], np.float32) * np.float32(w / 640)
    calib[2], calib[3] = (w - 1) / 2, (h - 1) / 2
    color, make_pc = synth.make_tracker_scene(w, h, n_points=n_points, seed=0)
    ct = CoarseTracker(w, h)
    ct.make_k(calib)
    ct.set_new_frame(color, 1.0)
    pcs = make_pc([ct.frame_level(l)[0][:, 0] for l in range(ct.levels)])
    ct.set_reference([(p["u"], p["v"], p["idepth"], p["color"]) for p in pcs], 1.0, (0.02, 3.0))
    return ct, [int(p["u"].size) for p in pcs]


def probe(reps):
    rows = []
    for name, n_points in (("bench", (8000, 4000, 2000, 1000)), ("256 per level", (256,) * 4), ("32000 at level 0", (32000, 256, 256, 256))):
        ct, n_pc = scene(640, 480, n_points)
        rng = np.random.default_rng(3)
        T = synth.se3_matrix(rng.normal(0, 2e-3, 3) * 3, rng.normal(0, 1e-2, 3) * 3)
        for lvl in range(ct.levels):
            ts = []
            for _ in range(reps + 3):
                t0 = time.perf_counter()
                res, _, n = ct.track(T, (0.05, 1.0), coarsest_lvl=lvl, trace=1)
                ts.append((time.perf_counter() - t0) * 1e6)
            rows.append(dict(scene=name, points_per_level=n_pc, coarsest_lvl=lvl, evaluations=n,
                             iterations=res["iterations"].tolist(), track_us=float(np.median(ts[3:]))))
        ct.close()
    return rows


TIMED_SCENES = (("bench 640x480", 640, 480, (8000, 4000, 2000, 1000, 500, 250)),
                ("KITTI 1232x368", 1232, 368, (16000, 6000, 2000, 800, 300)))


def timed(name, w, h, n_points, reps):
    rows = []
    ct, n_pc = scene(w, h, n_points)
    coarsest = min(ct.levels, 5) - 1
    host = HostLoop(ct)
    rng = np.random.default_rng(3)
    Ts = np.stack([synth.se3_matrix(rng.normal(0, 2e-3, 3) * 3, rng.normal(0, 1e-2, 3) * 3) for _ in range(8)])
    ab = np.tile([0.05, 1.0], (8, 1))
    for n in (1, 8):
        before, after = [], []
        for r in range(reps + 3):  # the two routes alternate, the first three rounds warm up
            t0 = time.perf_counter()
            counts = [host.run(Ts[k], ab[k], coarsest) for k in range(n)]
            t1 = time.perf_counter()
            res = ct.track(Ts[:n], ab[:n])
            t2 = time.perf_counter()
            before.append((t1 - t0) * 1e3)
            after.append((t2 - t1) * 1e3)
        rows.append(dict(scene=name, points_per_level=n_pc, starts=n,
                         host_loop_ms=float(np.median(before[3:])), track_ms=float(np.median(after[3:])),
                         host_iterations=[c[0] for c in counts], host_evaluations=[c[1] for c in counts],
                         track_iterations=res["iterations"].tolist(), track_ok=res["ok"].tolist()))
    ct.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.probe:
        rows = probe(a.reps)
    else:
        rows = [r for sc in TIMED_SCENES for r in timed(*sc, a.reps)]
    doc = dict(reps=a.reps, clock="host perf_counter around each route, median" + ("" if a.probe else ", routes alternated"),
               rows=rows)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
