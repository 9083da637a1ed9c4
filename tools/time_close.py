"""Host-clock cost of closing a keyframe's points on an S7-sized ragged window at the C ABI: the device
path (ldso_ba_flag_points + ldso_ba_load_marginalization_device) against the host path (the residual and
point read-backs, the classification on the host, ldso_ba_load_marginalization from a host-built window),
each followed by ldso_ba_marginalize_points, alternated in one process on one parent context.

The parent runs the fix pass once; neither path changes it, so every cycle sees the same state.  The
bookkeeping (num_good, last_res, last_state; frame 0 flagged) is flag_cases', the idepth_hessian
threshold the median of the inlier candidates, so about half of them are marginalised.  The host
classification is the decision tree vectorised in numpy (checked against tests/flag_ref.py before
anything is timed).  The first cycles are not timed.

    python tools/time_close.py [--cycles 40] [--warmup 5] [--out FILE]
prints one JSON line: medians with [min, max] in milliseconds, per path the split read-back /
classification / second-context load / the pass and their sum."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flag_cases as fc  # noqa: E402
import flag_ref  # noqa: E402
import ragged  # noqa: E402
import test_marginalization as tm  # noqa: E402
from ldso_amd import BAContext, synth  # noqa: E402
from ldso_amd import _lib as L  # noqa: E402
from ldso_amd.window import Window  # noqa: E402


def stat(v):
    v = np.asarray(v) * 1e3
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def classify(w, pt_of_res, state, flags, idepth, ih, book, A, G, th):
    """flag_ref.flag_points' status and res_live, vectorised."""
    ff, num_good, lr, lst = book
    P = w.n_points
    live = (flags & L.FLAG_ACTIVE) != 0
    n_live = np.bincount(pt_of_res[live], minlength=P)
    vis = np.bincount(pt_of_res[live & (state == L.RES_IN) & (ff[w.res_target] != 0)], minlength=P)
    ls = np.where(lr >= 0, state[np.maximum(lr, 0)], lst)
    ng = num_good + n_live
    oob = ((n_live >= A) & (ng > G + 10) & (n_live - vis < A)) | (ls[:, 0] == L.RES_OOB) | \
          ((n_live >= 2) & (ls[:, 0] == L.RES_OUTLIER) & (ls[:, 1] == L.RES_OUTLIER))
    inl = (n_live >= A) & (ng >= G) & (ih > np.float32(th))
    status = np.where((idepth < 0) | (n_live == 0), flag_ref.OUTLIER,
                      np.where(oob | (ff[w.point_host] != 0), np.where(inl, flag_ref.MARGINALIZED, flag_ref.OUT), flag_ref.ACTIVE))
    return status.astype(np.int8), live.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    cfg = dict(synth.S7)
    w = ragged.frontend_window(synth.make_window(n_frames=cfg["n_frames"], n_points=cfg["n_points"], width=cfg["width"],
                                                 height=cfg["height"], seed=1), np.random.default_rng(1001))
    P, R, A, G = w.n_points, w.n_residuals, 3, 4
    lib = L.lib()
    parent = BAContext(0).load(ragged.clone(w))
    parent.linearize(True, True)
    parent.sync()
    r0, p0 = parent.residuals(0), parent.points(0)
    book = fc.bookkeeping(w, r0["state"], r0["flags"], A, G)
    idepth0 = parent.point_data(0)[:, 2]
    _, d = fc.reference(w, r0["state"], r0["flags"], idepth0, p0["idepth_hessian"], book, A, G, 0.0)
    cand = ~(idepth0 < 0) & (d["n_live"] > 0) & (d["e1"] | d["e2"] | d["e3"] | d["host_flagged"]) & d["inl_a"] & d["inl_g"]
    th = float(np.float32(np.median(p0["idepth_hessian"][cand])))
    ref, _ = fc.reference(w, r0["state"], r0["flags"], idepth0, p0["idepth_hessian"], book, A, G, th)
    pt_of_res = np.repeat(np.arange(P), np.diff(w.point_res_begin))
    st, lv = classify(w, pt_of_res, r0["state"], r0["flags"], idepth0, p0["idepth_hessian"], book, A, G, th)
    assert np.array_equal(st, ref["status"]) and np.array_equal(lv, ref["res_live"])
    params = L.FlagParams.default(min_good_active_res_for_marg=A, min_good_res_for_marg=G, min_idepth_h_marg=th)
    adh = tm.ad_ht_delta(w)
    marg = {k: BAContext(0) for k in ("device", "host")}
    state, flags, energy = np.zeros(R, np.int8), np.zeros(R, np.uint8), np.zeros(R, np.float32)
    ih, pd = np.zeros(P, np.float32), np.zeros((P, L.POINT_STRIDE), np.float32)
    keys = ("readback", "classify", "load", "pass", "total")
    t = {f"{p}_{k}": [] for p in ("device", "host") for k in keys}
    first = {}
    # no collector pause inside a timed close: the device path's wrappers allocate more Python objects
    # than the host path's ctypes calls, and a generation-2 collection is tens of milliseconds here
    gc.collect()
    gc.disable()
    for cyc in range(a.warmup + a.cycles):
        for path in (("device", "host") if cyc % 2 == 0 else ("host", "device")):  # alternate who goes first
            m = marg[path]
            t0 = time.perf_counter()
            if path == "device":
                t1 = t0
                o = parent.flag_points(*book, params=params)
                t2 = time.perf_counter()
                pts = np.flatnonzero(o["status"] == flag_ref.MARGINALIZED).astype(np.int32)
                m.load_marginalization_device(parent, 0, w, pts, o["res_live"])
            else:
                L.check(lib.ldso_ba_get_residuals(parent._h, 0, None, L.ptr(state, L.i8p), L.ptr(energy, L.f32p), None, None,
                                                  L.ptr(flags, L.u8p), None, None))
                L.check(lib.ldso_ba_get_points(parent._h, 0, None, None, L.ptr(ih, L.f32p), None, None, None))
                L.check(lib.ldso_ba_get_point_data(parent._h, 0, L.ptr(pd, L.f32p)))
                t1 = time.perf_counter()
                status, live = classify(w, pt_of_res, state, flags, pd[:, 2], ih, book, A, G, th)
                t2 = time.perf_counter()
                pts = np.flatnonzero(status == flag_ref.MARGINALIZED)
                ks = np.flatnonzero((live != 0) & (status[pt_of_res] == flag_ref.MARGINALIZED))
                begin = np.concatenate([[0], np.cumsum(np.bincount(pt_of_res[ks], minlength=P)[pts])]).astype(np.int32)
                sub = Window(n_frames=w.n_frames, width=w.width, height=w.height, calib=w.calib, frames=w.frames, dI=None,
                             frame_energy_th=w.frame_energy_th, point_host=w.point_host[pts], point_data=pd[pts],
                             point_res_begin=begin, res_target=w.res_target[ks], res_state=state[ks], res_energy=energy[ks],
                             res_flags=flags[ks], precalc=w.precalc, ad_host=w.ad_host, ad_target=w.ad_target,
                             c_prior=w.c_prior, c_delta=w.c_delta, frame_prior=w.frame_prior, frame_delta=w.frame_delta,
                             frame_delta_prior=w.frame_delta_prior, settings=w.settings)
                m.load_marginalization(parent, 0, sub)
            m.sync()
            t3 = time.perf_counter()
            H, b = m.marginalize_points(adh)
            t4 = time.perf_counter()
            if cyc == 0:
                first[path] = (H, b, pts.size)
            if cyc >= a.warmup:
                for k, v in zip(keys, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                    t[f"{path}_{k}"].append(v)
    gc.enable()
    assert np.array_equal(first["device"][0], first["host"][0]) and np.array_equal(first["device"][1], first["host"][1])
    out = dict(tool="time_close", window="S7-sized ragged (7 KF, 640x480)", points=P, residuals=R, marginalized=int(first["device"][2]),
               status_counts=[int(x) for x in ref["counts"]], cycles=a.cycles, warmup=a.warmup,
               unit="ms per close, host clock, Python caller; device_readback is 0 by construction and device_classify is "
                    "ldso_ba_flag_points; slowest_cycle: the timed cycle with the largest total; the Python collector is "
                    "off during the timed loop",
               slowest_cycle={p: int(np.argmax(t[f"{p}_total"])) for p in ("device", "host")},
               **{k: stat(v) for k, v in t.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
