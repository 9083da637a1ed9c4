#!/usr/bin/env python3
"""Host-clock timing of the activation selection on the device against the route without it.

  new route      ldso_ct_make_distance_map_ba + ldso_ct_select_activation (compact) +
                 ldso_ba_activate_points_tracker: no record leaves the device
  without it     ldso_ct_immature_download of the whole set + ldso_ba_activate_points with host records of
                 the same selection + ldso_ct_immature_upload of the survivors.  The host's own distance
                 map and walk are NOT run: their time comes on top of this column.

Both routes run on this build, alternating call by call in one process; the resident set is put back
(untimed) before each call; --warmup calls of each are dropped, then the median [min, max] of --reps.
One JSON document on stdout.

    python tools/time_actsel.py [--reps 50] [--warmup 10] [--out FILE]

--profile runs only the new route (for a kernel trace of its own, rocprofv3 --kernel-trace --stats).
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

from ldso_amd import BAContext, synth  # noqa: E402
from ldso_amd import _lib as L  # noqa: E402
from ldso_amd.tracker import CoarseTracker  # noqa: E402


def level1_tables(w):
    """K[1] R Ki[0] and K[1] t, host -> newest frame, in float as activatePointsMT builds them."""
    fx, fy, cx, cy = [float(v) for v in w.calib]
    K0 = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    K1 = np.array([[fx / 2, 0, (cx + 0.5) / 2 - 0.5], [0, fy / 2, (cy + 0.5) / 2 - 0.5], [0, 0, 1.0]])

    def pose(f):
        T = np.eye(4)
        T[:3, :3] = w.frames["world_to_cam_evalpt"][f][:9].reshape(3, 3)
        T[:3, 3] = w.frames["world_to_cam_evalpt"][f][9:]
        return T

    new = pose(w.n_frames - 1)
    krki, kt = [], []
    for f in range(w.n_frames):
        T = new @ np.linalg.inv(pose(f))
        krki.append((K1.astype(np.float32) @ T[:3, :3].astype(np.float32) @ np.linalg.inv(K0).astype(np.float32)).reshape(9))
        kt.append(K1.astype(np.float32) @ T[:3, 3].astype(np.float32))
    return np.stack(krki).astype(np.float32), np.stack(kt).astype(np.float32)


def summary(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for width, height, n_active, n_records, cmad in ((640, 480, 2000, 9000, 2.0), (640, 480, 2000, 9000, 0.7)):
        w = synth.make_window(n_frames=7, n_points=n_active, width=width, height=height, seed=1)
        src = synth.make_window(n_frames=7, n_points=n_records, width=width, height=height, seed=1)
        pts = synth.immature_from_window(src)
        pts["type"] = np.random.default_rng(3).choice([1.0, 2.0, 4.0], len(pts), p=[0.7, 0.2, 0.1])
        pts["last_interval"] = 1.0
        pts = np.ascontiguousarray(pts[np.argsort(pts["host"], kind="stable")])
        ctx = BAContext(0).load([w])
        ctx.optimize(1)
        krki1, kt1 = level1_tables(w)
        ct = CoarseTracker(width, height)
        # every array the timed calls touch exists before the clock starts: the clock is around the C ABI
        lib, n = L.lib(), len(pts)
        p = L.LdsoCtActselParams(cmad, 3.0, -2)
        disp, idx, cnt = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(len(L.ACTSEL_COUNTS), np.int32)
        ns = C.c_int32()
        act, act_host, down = (np.zeros(n, L.ACTIVATION_DTYPE), np.zeros(n, L.ACTIVATION_DTYPE),
                               np.zeros(n, L.IMMATURE_DTYPE))
        pk, pt, pd, pi, pc = (L.ptr(krki1, L.f32p), L.ptr(kt1, L.f32p), L.ptr(disp, L.i32p), L.ptr(idx, L.i32p),
                              L.ptr(cnt, L.i32p))

        def new_route():
            L.check(lib.ldso_ct_make_distance_map_ba(ct._h, ctx._h, 0, -1, pk, pt, None))
            L.check(lib.ldso_ct_select_activation(ct._h, C.byref(p), None, 1, pd, pi, C.byref(ns), pc))
            L.check(lib.ldso_ba_activate_points_tracker(ctx._h, 0, ct._h, 1, act.ctypes.data))

        def put_back():
            L.check(lib.ldso_ct_immature_upload(ct._h, n, pts.ctypes.data))

        put_back()
        new_route()
        n_sel = int(ns.value)
        counts = dict(zip(L.ACTSEL_COUNTS, cnt.tolist()))
        act_new = act[:n_sel].copy()
        chosen = np.ascontiguousarray(pts[idx[:n_sel]])
        survivors = np.ascontiguousarray(pts[disp == L.ACT_KEEP])

        def without():
            L.check(lib.ldso_ct_immature_download(ct._h, n, down.ctypes.data))
            L.check(lib.ldso_ba_activate_points(ctx._h, 0, n_sel, chosen.ctypes.data, 1, act_host.ctypes.data))
            L.check(lib.ldso_ct_immature_upload(ct._h, len(survivors), survivors.ctypes.data))

        times = {"new_route": [], "without": []}
        for i in range(a.warmup + a.reps):
            for name, fn in ((("new_route", new_route),) if a.profile else (("new_route", new_route), ("without", without))):
                put_back()  # the set as it was, untimed
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        if a.profile:
            times["without"] = [0.0]
        else:
            assert act[:n_sel].tobytes() == act_new.tobytes() == act_host[:n_sel].tobytes()  # the same points either way
        rows.append(dict(width=width, height=height, active_points=n_active, records=len(pts), current_min_act_dist=cmad,
                         counts=counts, new_route=summary(times["new_route"]), without=summary(times["without"])))
        ct.close()
        ctx.close()
    doc = dict(reps=a.reps, warmup=a.warmup,
               clock="host perf_counter around the C ABI calls, the routes alternating; median [min, max]",
               note="the 'without' route leaves out the host's distance map and walk", rows=rows)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
