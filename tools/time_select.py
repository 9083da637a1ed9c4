#!/usr/bin/env python3
"""Host-clock timing of ldso_ct_make_new_traces against the route to the same records without it:
ldso_ct_get_frame_level for levels 0-2 (what a host selector needs), the uv upload and
ldso_ct_make_immature.  The host selector itself is not run: its time comes on top of
the second column.  Median of --reps calls per frame; one JSON document on stdout.

    python tools/time_select.py [--reps 50] [--out FILE]
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


def frame(kind, w, h):
    img = blob_image(w, h, 1)
    if kind == "blobs+noise":
        img = img + np.random.default_rng(7).normal(0, 3.0, img.shape)
    else:  # mixed: vertical bars on the left third, horizontal bars on the top half of the middle third
        yy, xx = np.mgrid[0:h, 0:w]
        img[:, :w // 3] = (90.0 + 60.0 * np.sign(np.sin(2 * np.pi * (xx + 0.5) / 7.0)))[:, :w // 3]
        img[:h // 2, w // 3:2 * w // 3] = (90.0 + 60.0 * np.sign(np.sin(2 * np.pi * (yy + 0.5) / 7.0)))[:h // 2,
                                                                                                       w // 3:2 * w // 3]
    return img.astype(F)


def median_ms(fn, reps, before=None):
    ts = []
    for _ in range(reps + 3):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[3:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = L.lib()
    rows = []
    for w, h in ((640, 480), (1232, 368)):
        t = CoarseTracker(w, h)
        pat = np.random.default_rng(11).integers(0, 256, w * h, dtype=np.uint8)
        p = L.LdsoCtSelectParams()
        lib.ldso_ct_select_default_params(C.byref(p))
        for kind in ("blobs+noise", "mixed"):
            t.set_new_frame(frame(kind, w, h))
            cap = 4 * int(p.density)
            out = np.zeros(cap, L.IMMATURE_DTYPE)
            n = C.c_int32()
            st = np.zeros(len(L.SELECT_STATS), np.int32)

            def new_call():
                L.check(lib.ldso_ct_make_new_traces(t._h, C.byref(p), 0, cap, out.ctypes.data, C.byref(n),
                                                    L.ptr(st, L.i32p)))

            new_ms = median_ms(new_call, a.reps, before=lambda: t.select_init(pat, 3))
            stats = dict(zip(L.SELECT_STATS, st.tolist()))
            # the same records without the call: three levels back, uv up, the records made
            uv = np.ascontiguousarray(np.stack([out["u"][:n.value], out["v"][:n.value]], 1))
            lv = [(np.zeros(((w >> l) * (h >> l), 3), F), np.zeros((w >> l) * (h >> l), F)) for l in range(3)]
            recs = np.zeros(n.value, L.IMMATURE_DTYPE)

            def readback():
                for l in range(3):
                    L.check(lib.ldso_ct_get_frame_level(t._h, l, L.ptr(lv[l][0], L.f32p), L.ptr(lv[l][1], L.f32p)))

            def make():
                L.check(lib.ldso_ct_make_immature(t._h, int(n.value), L.ptr(uv, L.f32p), 1.0, 0, recs.ctypes.data))

            rb_ms, mk_ms = median_ms(readback, a.reps), median_ms(make, a.reps)
            rows.append(dict(width=w, height=h, frame=kind, records=int(n.value), stats=stats,
                             make_new_traces_ms=new_ms, readback_levels_0_2_ms=rb_ms, upload_make_immature_ms=mk_ms,
                             without_ms=rb_ms + mk_ms))
        t.close()
    doc = dict(reps=a.reps, clock="host perf_counter around the C ABI calls, median", rows=rows)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
