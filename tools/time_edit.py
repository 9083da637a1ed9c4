"""Host-clock cost of one structural change of a loaded S7-sized window at the C ABI: ldso_ba_edit_window
against ldso_ba_load_frames of the same window, alternated in one process.

The window rotates as the keyframe cycle does: the frame at position 0 leaves with its points and the
residuals into it (every later frame shifts down), then the same frame comes back as the newest, with
one new residual on every surviving point and its own points as new ones.  Two contexts follow the
rotation, one by edits, one by reloads from the host arrays.  Timed per call: the call alone (host work: planning or layout, staging,
launches) and the call plus ldso_ba_sync (the device has finished).  The first cycles are not timed.

    python tools/time_edit.py [--cycles 40] [--warmup 5] [--out FILE]
prints one JSON line: medians with [min, max] in milliseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edit_cases as ec  # noqa: E402
import ragged  # noqa: E402
from ldso_amd import BAContext, synth  # noqa: E402


def stat(v):
    v = np.asarray(v) * 1e3
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    cfg = dict(synth.S7)
    pool = ragged.frontend_window(synth.make_window(n_frames=cfg["n_frames"], n_points=cfg["n_points"], width=cfg["width"],
                                                    height=cfg["height"], seed=1), np.random.default_rng(1001))
    ctxs = {}
    for name in ("edit", "reload"):
        c = BAContext(0)
        c.frames_reserve(pool.n_frames, pool.width, pool.height)
        for f in range(pool.n_frames):
            c.frame_put(ec.FRAME_ID0 + f, pool.dI[f])
        ctxs[name] = c
    sel = ec.full_sel(pool, range(7))
    for c in ctxs.values():
        c.load(ec.window_of(pool, sel), frame_ids=sel.frame_ids())
        c.linearize(False, True)
        c.sync()
    t = {k: [] for k in ("edit_call", "edit_done", "reload_call", "reload_done")}
    shape = None
    for cyc in range(a.warmup + a.cycles):
        oldest = sel.frames[0]
        s6 = ec.edit_remove_frame(pool, sel, oldest)
        s7 = ec.edit_append(pool, s6, oldest)
        # ... and hosts the points it hosted before, as new points with their residuals (the window keeps its size)
        s7 = ec.Sel(s7.frames, s7.pts + [(p, ec.pool_items(pool, p, s7.frames)) for p in range(pool.n_points)
                                         if int(pool.point_host[p]) == oldest])
        acc = dict.fromkeys(t, 0.0)
        for before, after in ((sel, s6), (s6, s7)):
            w_edit, src = ec.window_of(pool, after, before)
            w_load = ec.window_of(pool, after)
            ids = after.frame_ids()
            for name in (("edit", "reload") if cyc % 2 == 0 else ("reload", "edit")):  # alternate who goes first
                c = ctxs[name]
                t0 = time.perf_counter()
                if name == "edit":
                    c.edit(w_edit, ids, *src)
                else:
                    c.load(w_load, frame_ids=ids)
                t1 = time.perf_counter()
                c.sync()
                t2 = time.perf_counter()
                acc[name + "_call"] += t1 - t0
                acc[name + "_done"] += t2 - t0
                c.linearize(False, True)  # the pass the cycle runs next, untimed
                c.sync()
        if cyc >= a.warmup:
            for k in t:
                t[k].append(acc[k])
        sel = s7
        shape = (len(s7.pts), sum(len(i) for _, i in s7.pts))
    out = dict(tool="time_edit", window="S7-sized (7 KF, 640x480)", points=shape[0], residuals=shape[1], cycles=a.cycles,
               warmup=a.warmup, unit="ms per cycle (remove the oldest frame + append a frame), host clock, Python caller",
               **{k: stat(v) for k, v in t.items()}, transfer_edit=ctxs["edit"].transfer_stats(),
               transfer_reload=ctxs["reload"].transfer_stats())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
