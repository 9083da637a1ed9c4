#!/usr/bin/env python3
"""Host-clock timing of ldso_ct_detect_corners against the route to the same records without it:
ldso_ct_get_frame_level for level 0 (dIp and absSquaredGrad, what a host detector needs), then the uv
upload and ldso_ct_make_immature.  The host detector itself is not run: its time comes on
top of the second column.  The two routes alternate call by call in one process; --warmup calls of each
are dropped, then the median [min, max] of --reps calls.  One JSON document on stdout.

    python tools/time_corners.py [--reps 50] [--warmup 10] [--out FILE]

--profile runs only the detection (for a kernel trace of its own, rocprofv3 --kernel-trace --stats).
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
from ldso_amd.tracker import CoarseTracker  # noqa: E402

F = np.float32
N_FEATURES = 1500  # setting_desiredImmatureDensity


def blob_image(w, h, seed, sigma=(2.0, 8.0)):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 90.0)
    for _ in range(int(w * h / 2000)):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        s = rng.uniform(*sigma)
        A = rng.uniform(20, 80) * rng.choice([-1, 1])
        img += A * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return img


def frame(w, h):
    return (blob_image(w, h, 1) + np.random.default_rng(7).normal(0, 3.0, (h, w))).astype(F)


def summary(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = L.lib()
    pattern = np.random.default_rng(5).integers(-13, 14, 1024).astype(np.int32)  # a stand-in for the ORB table
    rows = []
    for w, h in ((640, 480), (1232, 368)):
        t = CoarseTracker(w, h)
        t.corners_init(pattern)
        t.set_new_frame(frame(w, h))
        cap = 4 * N_FEATURES
        rec = np.zeros(cap, L.IMMATURE_DTYPE)
        feat = np.zeros(cap, L.FEATURE_DTYPE)
        n = C.c_int32()
        st = np.zeros(len(L.CORNER_STATS), np.int32)

        def detect():
            L.check(lib.ldso_ct_detect_corners(t._h, N_FEATURES, 0, cap, rec.ctypes.data, feat.ctypes.data,
                                               C.byref(n), L.ptr(st, L.i32p)))

        detect()
        uv = np.ascontiguousarray(np.stack([rec["u"][:n.value], rec["v"][:n.value]], 1))
        dI, ag = np.zeros((w * h, 3), F), np.zeros(w * h, F)
        recs = np.zeros(n.value, L.IMMATURE_DTYPE)

        def readback():
            L.check(lib.ldso_ct_get_frame_level(t._h, 0, L.ptr(dI, L.f32p), L.ptr(ag, L.f32p)))

        def make():
            L.check(lib.ldso_ct_make_immature(t._h, int(n.value), L.ptr(uv, L.f32p), 1.0, 0, recs.ctypes.data))

        times = {"detect_corners": [], "readback_level_0": [], "upload_make_immature": []}
        routes = (("detect_corners", detect),) if a.profile else (
            ("detect_corners", detect), ("readback_level_0", readback), ("upload_make_immature", make))
        for i in range(a.warmup + a.reps):
            for name, fn in routes:
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        row = dict(width=w, height=h, n_features=N_FEATURES, stats=dict(zip(L.CORNER_STATS, st.tolist())))
        for name, _ in routes:
            row[name] = summary(times[name])
        if not a.profile:
            row["without_median_ms"] = row["readback_level_0"]["median_ms"] + row["upload_make_immature"]["median_ms"]
            assert recs.tobytes() == rec[:n.value].tobytes()  # the same records either way
        rows.append(row)
        t.close()
    doc = dict(reps=a.reps, warmup=a.warmup,
               clock="host perf_counter around the C ABI calls, the routes alternating; median [min, max]", rows=rows)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
