#!/usr/bin/env python3
"""Host-clock timing of the coarse initializer on the device against what a host initializer on this
library pays per frame today.

  track_frame    ldso_ct_init_track_frame, one launch: a frame that does not snap (the first image again) and
                 a frame on a snapped state (the second frame of a shifted sequence)
  readback       ldso_ct_get_frame_level of every level (dI and absSquaredGrad): the images a host
                 CoarseInitializer::trackFrame needs.  The host loop itself is NOT run: its time comes on top.

640x480, 0.03 w h points on level 0 and the reference's densities 0.05 / 0.15 / 0.5 / 1 of w h above, capped by
the level's interior pixels; positions random, neighbour and parent tables as makeNN's (k nearest).  The state is put
back (untimed) before each call; --warmup calls are dropped, then the median [min, max] of --reps.  One JSON
document on stdout.

    python tools/time_init.py [--reps 20] [--warmup 3] [--out FILE]

--profile runs only track_frame (for a kernel trace of its own, rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldso_amd import _lib as L  # noqa: E402
from ldso_amd import synth  # noqa: E402
from ldso_amd.tracker import CoarseInitializer, CoarseTracker  # noqa: E402

DENSITIES = (0.03, 0.05, 0.15, 0.5, 1.0)  # CoarseInitializer.cc:669


def nearest(q, pts, k, chunk=512):
    """Indices of the k nearest pts to each q: scipy's kd-tree where there is one, else brute force in
    chunks.  Any valid table will do: the tables are the caller's input."""
    try:
        from scipy.spatial import cKDTree
        return cKDTree(pts).query(q, k=[*range(1, k + 1)])[1].astype(np.int32)
    except ImportError:
        pass
    out = np.zeros((q.shape[0], k), np.int32)
    for s in range(0, q.shape[0], chunk):
        d = ((q[s:s + chunk, None, :] - pts[None, :, :]) ** 2).sum(-1)
        kk = min(k, d.shape[1] - 1)
        part = np.sort(np.argpartition(d, kk, axis=1)[:, :k], axis=1)
        order = np.argsort(np.take_along_axis(d, part, axis=1), axis=1, kind="stable")
        out[s:s + chunk] = np.take_along_axis(part, order, axis=1)
    return out


def make_points(width, height, levels, rng):
    uv = []
    for l in range(levels):
        wl, hl = width >> l, height >> l
        xs, ys = np.arange(3, wl - 5), np.arange(3, hl - 5)
        n = min(int(DENSITIES[l] * width * height), xs.size * ys.size)
        idx = np.sort(rng.choice(xs.size * ys.size, size=n, replace=False))
        uv.append(np.stack([xs[idx % xs.size] + 0.1, ys[idx // xs.size] + 0.1], axis=1).astype(np.float32))
    out = []
    for l, p in enumerate(uv):
        rec = np.zeros(p.shape[0], L.INIT_POINT_DTYPE)
        rec["u"], rec["v"] = p[:, 0], p[:, 1]
        rec["idepth"] = rec["ir"] = 1
        rec["is_good"] = 1
        rec["my_type"] = 1
        rec["outlier_th"] = 8 * 12 * 12
        rec["neighbours"] = nearest(p.astype(np.float64), p.astype(np.float64), 10)
        rec["parent"] = nearest(p * 0.5 - 0.25, uv[l + 1].astype(np.float64), 1)[:, 0] if l + 1 < levels else -1
        out.append(rec)
    return out


def shifted(img, s):
    h, w = img.shape
    x = np.clip(np.arange(w, dtype=np.float64) - s, 0, w - 1)
    x0 = np.minimum(np.floor(x).astype(np.int64), w - 2)
    fx = x - x0
    return ((1 - fx) * img[:, x0] + fx * img[:, x0 + 1]).astype(np.float32)


def summary(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    width, height = 640, 480
    first, _ = synth.make_tracker_scene(width, height, n_points=(1,), seed=1)
    calib = np.array([0.87 * width, 0.87 * width, 0.5 * width - 0.5, 0.5 * height - 0.5], np.float32)
    frames = [shifted(first, float(calib[0]) * 0.03 * k) for k in (1, 2)]
    tr = CoarseTracker(width, height)
    tr.make_k(calib)
    pts = make_points(width, height, tr.levels, np.random.default_rng(2))
    init = CoarseInitializer(tr)

    def put_back(snapped):
        tr.set_new_frame(first, 1.0)
        init.set_first(pts)
        if snapped:
            tr.set_new_frame(frames[0], 1.0)
            r = init.track_frame()
            assert r["snapped"], "the first shifted frame did not snap"
            tr.set_new_frame(frames[1], 1.0)

    results = {}
    times = {"not_snapped": [], "snapped": [], "readback": []}
    for i in range(a.warmup + a.reps):
        for name in ("not_snapped", "snapped"):
            put_back(name == "snapped")
            t0 = time.perf_counter()
            r = init.track_frame()
            dt = (time.perf_counter() - t0) * 1e3
            results[name] = dict(snapped=int(r["snapped"]), iterations=r["iterations"][:tr.levels].tolist(),
                                 phase_us=dict(zip(L.INIT_PHASES, [float(v) for v in r["phase_us"]])))
            if i >= a.warmup:
                times[name].append(dt)
        if not a.profile:
            t0 = time.perf_counter()
            for l in range(tr.levels):
                tr.frame_level(l)
            if i >= a.warmup:
                times["readback"].append((time.perf_counter() - t0) * 1e3)
    if a.profile:
        times["readback"] = [0.0]
    assert not results["not_snapped"]["snapped"] and results["snapped"]["snapped"]
    doc = dict(width=width, height=height, levels=tr.levels, points=[int(p.size) for p in pts],
               ranks=init.rank_counts().tolist(), reps=a.reps, warmup=a.warmup,
               clock="host perf_counter around the C ABI call; median [min, max]",
               note="readback leaves out the host initializer's own loop",
               runs=results, track_frame_not_snapped=summary(times["not_snapped"]),
               track_frame_snapped=summary(times["snapped"]), readback_all_levels=summary(times["readback"]))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    tr.close()


if __name__ == "__main__":
    main()
