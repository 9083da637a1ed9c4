"""Wall time per keyframe of the tracker's reference cloud (CoarseTracker::makeCoarseDepthL0), two routes
from the same bundle-adjustment pass of one window (S7: 7 frames, 2,000 points, 640x480; KITTI's
1232x368, synth.KITTI00):

  (a) host    ldso_ba_get_residuals (state, centre) + ldso_ba_get_points (HdiF), the restatement of
              tests/coarse_depth_ref.py vectorised on the CPU (np.add.at sums in index order, which is
              the reference's sequential chain), ldso_ct_set_reference
  (b) device  ldso_ct_make_reference_ba

Both end in the synchronisation the caller waits for.  The two routes alternate in one process after
a warm-up; the median, the extremes and the quartiles of the repeated calls are reported, with the
host <-> device bytes each route moves (computed from the shapes) and a check that the two clouds are
the same bytes.  A GPU tool: it fails without a device.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (its HIP runtime initialises first, as in the tests)
import numpy as np  # noqa: E402

import coarse_depth_ref as R  # noqa: E402
from ldso_amd import BAContext, synth  # noqa: E402
from ldso_amd import _lib as L  # noqa: E402
from ldso_amd.tracker import CoarseTracker  # noqa: E402

F = np.float32


def host_cloud(w, h, center, hdi, colors):
    """R.make_coarse_depth with the scatter vectorised: np.add.at adds in index order, unbuffered."""
    with np.errstate(all="ignore"):
        tu, tv = center[:, 0] + F(0.5), center[:, 1] + F(0.5)
        ok = (tu > -1) & (tu < w) & (tv > -1) & (tv < h)
        pix = tu[ok].astype(np.int64) + w * tv[ok].astype(np.int64)
        wt = np.sqrt((1e-3 / (hdi[ok].astype(np.float64) + 1e-12)).astype(F))
        I, W = np.zeros(w * h, F), np.zeros(w * h, F)
        np.add.at(I, pix, center[ok, 2] * wt)
        np.add.at(W, pix, wt)
        I, W = I.reshape(h, w), W.reshape(h, w)
        out = []
        for lvl in range(len(colors)):
            if lvl > 0:
                I, W = R._down(I), R._down(W)
            out.append(R._emit_level(lvl, I, W, colors[lvl]))
    return out


def run(name, cfg, reps, warmup):
    win = synth.make_window(**cfg, seed=1)
    w, h = win.width, win.height
    ctx = BAContext(0).load([win])
    ctx.optimize(3, nullspaces=[win.nullspaces()])
    color, _ = synth.make_tracker_scene(w, h, seed=2)
    ct_a, ct_b = CoarseTracker(w, h), CoarseTracker(w, h)
    for ct in (ct_a, ct_b):
        ct.set_new_frame(color, 1.0)
    colors = [np.ascontiguousarray(ct_a.frame_level(l)[0][:, 0]) for l in range(ct_a.levels)]
    # the structure of the traversal is the caller's own bookkeeping: per point (in traversal order) the
    # index of its residual to the newest frame, made once
    ref = win.n_frames - 1
    begin, tgt = np.asarray(win.point_res_begin), np.asarray(win.res_target)
    order = R.window_traversal(win)
    k_of, p_of = [], []
    for p in order:
        ks = [k for k in range(begin[p], begin[p + 1]) if tgt[k] == ref]
        if ks:
            k_of.append(ks[0])
            p_of.append(p)
    k_of, p_of = np.asarray(k_of), np.asarray(p_of)
    Rn, Pn = win.n_residuals, win.n_points
    state, center, hdi = np.zeros(Rn, np.int8), np.zeros((Rn, 3), F), np.zeros(Pn, F)
    lib = L.lib()
    nf, ni8 = L.ptr(None, L.f32p), L.ptr(None, L.i8p)
    last = {}

    def route_a():
        L.check(lib.ldso_ba_get_residuals(ctx._h, 0, ni8, L.ptr(state, L.i8p), nf, nf, L.ptr(center, L.f32p),
                                          L.ptr(None, L.u8p), nf, nf))
        L.check(lib.ldso_ba_get_points(ctx._h, 0, L.ptr(hdi, L.f32p), nf, nf, nf, nf, nf))
        m = state[k_of] == 0
        pcs = host_cloud(w, h, center[k_of[m]], hdi[p_of[m]], colors)
        ct_a.set_reference([tuple(np.ascontiguousarray(p[:, j]) for j in range(4)) for p in pcs], 1.0, (0.0, 0.0))
        last["a"] = pcs

    def route_b():
        last["n"] = ct_b.make_reference_from(ctx, 0, -1, None, 1.0, (0.0, 0.0))

    for _ in range(warmup):
        route_a()
        route_b()
    ta, tb = [], []
    for _ in range(reps):  # alternating, so that both see the same machine
        t0 = time.perf_counter()
        route_a()
        t1 = time.perf_counter()
        route_b()
        t2 = time.perf_counter()
        ta.append(1e3 * (t1 - t0))
        tb.append(1e3 * (t2 - t1))
    same = all(ct_b.reference(l).tobytes() == last["a"][l].tobytes() for l in range(ct_b.levels))

    def stats(t):
        q = np.percentile(t, [0, 25, 50, 75, 100])
        return dict(median_ms=round(float(q[2]), 4), min_ms=round(float(q[0]), 4), q25_ms=round(float(q[1]), 4),
                    q75_ms=round(float(q[3]), 4), max_ms=round(float(q[4]), 4))

    n_pc = int(sum(int(x) for x in last["n"]))
    out = dict(shape=name, width=w, height=h, levels=ct_b.levels, points=Pn, residuals=Rn,
               contributions=int((state[k_of] == 0).sum()), cloud_points=n_pc, reps=reps, warmup=warmup,
               host=stats(ta), device=stats(tb), clouds_identical=bool(same),
               # (a): state 1 B + centre 12 B per residual and the 12 floats ldso_ba_get_points reads per point
               # down, the clouds up; (b): the per-level counts
               host_bytes=dict(d2h=Rn * 13 + Pn * 48, h2d=n_pc * 16),
               device_bytes=dict(d2h=4 * ct_b.levels, h2d=0))
    print(json.dumps(out), flush=True)
    for c in (ct_a, ct_b, ctx):
        c.close()
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    ok = run("S7", synth.S7, a.reps, a.warmup)
    ok = run("KITTI00", synth.KITTI00, a.reps, a.warmup) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
