"""The coarse initializer on the device (ldso_ct_init_*) against tests/init_ref.py, the numpy restatement of
CoarseInitializer::trackFrame (multiThreading == false), on the scenes of tests/init_scenes.py.

1. Evaluation.  ldso_ct_init_eval at poses from the scenes: every per-point field bit for bit; every sum
   within the any-order bound |device - exact| <= (n - 1) 2^-24 sum|term|, with n, the exact sum and
   sum|term| in float64 from the restatement's bit-exact float32 terms (H's diagonal and b also count the
   term calcResAndGS adds after the sum; the alpha energy's final product with alphaW adds one rounding);
   the restatement's own reference-order sums satisfy the same bound.  At these sizes (at most 600 points)
   the bound is far below one point's share of a sum, so a dropped or doubled point cannot hide under it.
2. Lock-step.  ldso_ct_init_track_frame with a trace; every logged evaluation replayed through
   ldso_ct_init_eval on a second context (res bitwise), every step through ldso_ct_init_lm_step (increment
   bitwise, pose within 4 ulp per entry: tests/test_track.py's bar, for the same reason); the restatement
   replayed over the log with the logged increments takes the same alpha-cap, accept, snap and exit
   decisions from its own sums (tests/test_init_ref.py shows that this is a fair demand) and ends with every
   point record of every level bit for bit the device's, and the same snapped / frameID / snappedAt / return.
3. optReg on constructed lists, repeatability, and the first frame's hand-off to the BA frame store.
"""
import math

import numpy as np
import pytest

import init_ref as IR
import init_scenes as S
import track_ref as TR
from ldso_amd import _lib as L
from ldso_amd import tracker as T
from ldso_amd.tracker import CoarseInitializer, CoarseTracker

pytestmark = pytest.mark.gpu
f32 = np.float32
TRACE = 512


def context(sc, new_frame=1):
    tr = CoarseTracker(sc.width, sc.height)
    assert tr.levels == sc.levels
    tr.make_k(sc.calib)
    tr.set_new_frame(sc.first, sc.first_exposure)
    init = CoarseInitializer(tr)
    init.set_first(sc.points)
    if new_frame is not None:
        img, e = sc.frame(new_frame)
        tr.set_new_frame(img, e)
    return tr, init


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def differing_fields(dev, ref):
    return [f for f in dev.dtype.names if not same_bytes(dev[f], ref[f])]


def full45(v):
    M = np.zeros((9, 9), np.float64)
    M[IR.TRI_R, IR.TRI_C] = v
    M[IR.TRI_C, IR.TRI_R] = v
    return M


def check_sums(out, n_points, H, b, Hsc, bsc, res, params):
    """The bound of the module docstring for every entry of one evaluation; `out` is the restatement's."""
    def bounded(name, dev, exact, bound, ref):
        dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
        err, rerr = np.abs(dev - exact), np.abs(ref - exact)
        assert (err <= bound).all(), (name, float(err.max()), float(np.max(bound)))
        assert (rerr <= bound).all(), (name + " (reference order)", float(rerr.max()), float(np.max(bound)))

    # H's first three diagonal entries and b's first three get one more term after the sum (:332-339)
    extra = np.zeros(45, f32)
    for k in range(3):
        extra[IR.TRI.index((k, k))] = out["diag_term"]
        extra[IR.TRI.index((k, 8))] = out["tlog_terms"][k]
    ex9, bd9 = IR.sum_bound(out["acc9_terms"])
    ex9a, bd9a = IR.sum_bound(np.concatenate([out["acc9_terms"], extra[None, :]]))
    exact, bound = full45(np.where(extra != 0, ex9a, ex9)), full45(np.where(extra != 0, bd9a, bd9))
    bounded("H", H, exact[:8, :8], bound[:8, :8], out["H"])
    bounded("b", b, exact[:8, 8], bound[:8, 8], out["b"])
    exsc, bdsc = IR.sum_bound(out["sc_terms"])
    bounded("Hsc", Hsc, full45(exsc)[:8, :8], full45(bdsc)[:8, :8], out["Hsc"])
    bounded("bsc", bsc, full45(exsc)[:8, 8], full45(bdsc)[:8, 8], out["bsc"])
    exe, bde = IR.sum_bound(out["e_terms"])
    bounded("E", res[0], exe, bde, out["res"][0])
    assert res[2] == n_points
    if out["capped"]:
        assert res[1] == f32(params["alpha_k"]) * f32(n_points) == out["res"][1]
    else:
        tsq_term = np.asarray(out["tsq_term"], f32).reshape(1)
        exa, bda = IR.sum_bound(np.concatenate([out["ea_terms"], tsq_term]))
        aw = float(params["alpha_w"])
        bounded("alphaEnergy", res[1], exa * aw, bda * aw + 2.0 ** -23 * abs(exa * aw), out["res"][1])


# ---- 1. evaluation ------------------------------------------------------------------------------------
EVAL_POSES = {
    "rest": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0)),
    "moved": ((0.002, -0.001, 0.003), (0.02, 0.001, -0.002), (0.02, 1.5)),
    "left": ((0.0, 0.0, 0.0), (-0.006, 0.0, 0.0), (0.0, 0.0)),  # 1.7 pixels towards the left border at level 0
}


@pytest.mark.parametrize("pose", list(EVAL_POSES))
@pytest.mark.parametrize("name", ["shift", "expo", "border", "one_point_level", "no_neighbours", "wide5"])
def test_evaluation_matches_restatement(built, name, pose):
    sc = S.scene(name)
    tr, init = context(sc)
    ref = sc.reference()
    dI, _ = sc.frame_dI(1)
    om, t, aff = EVAL_POSES[pose]
    Tm = TR.pose_matrix(TR.se3_exp(tuple(t) + tuple(om)))
    rng = np.random.default_rng(5)
    partial = 0
    for lvl in range(sc.levels):
        pts = ref.pts[lvl]
        pts["idepth_new"] = pts["idepth"]
        if pose != "rest":  # a state in mid-run: spread depths, a few points out
            pts["idepth"] = pts["idepth_new"] = (1 + 0.3 * rng.standard_normal(pts.size)).clip(0.2, 3).astype(f32)
            pts["ir"] = (1 + 0.1 * rng.standard_normal(pts.size)).astype(f32)
            pts["is_good"][::11] = 0
            pts["energy"] = rng.uniform(0, 50, (pts.size, 2)).astype(f32)
        init.set_points(lvl, pts)
        before = pts.copy()
        out = ref.calc_res_and_gs(lvl, Tm, (f32(aff[0]), f32(aff[1])), dI[lvl])
        H, b, Hsc, bsc, res, capped = init.eval(lvl, Tm, aff, **sc.params)
        dev = init.points(lvl)
        assert differing_fields(dev, pts) == []
        assert capped == out["capped"]
        check_sums(out, pts.size, H, b, Hsc, bsc, res, ref.p)
        lost = (before["is_good"] != 0) & (pts["is_good_new"] == 0)
        partial += int((lost & (pts["maxstep"] < 1e9)).sum())
        # JbBuffer_new through what doStep exposes: a second evaluation leaves it as the first did
        H2, b2, Hsc2, bsc2, res2, _ = init.eval(lvl, Tm, aff, **sc.params)
        assert all(same_bytes(x, y) for x, y in ((H, H2), (b, b2), (Hsc, Hsc2), (bsc, bsc2), (res, res2)))
    if name == "border" and pose == "left":
        # the maxstep trap: points that left the image at a pattern pixel k > 0 keep the minimum over 0 .. k-1
        assert partial > 0
    tr.close()


# ---- 2. lock-step ---------------------------------------------------------------------------------------
def lock_step(sc, tr, init, rep, ref, frame, params):
    """One frame on the device context (tr, init) and on the restatement ref, the evaluations replayed on the
    replay context rep; returns the restatement's log."""
    img, e = sc.frame(frame)
    dI, _ = sc.frame_dI(frame)
    tr.set_new_frame(img, e)
    rep[0].set_new_frame(img, e)
    res, steps, n = init.track_frame(trace=TRACE, **params)
    assert n == len(steps) <= TRACE
    replays = {}

    def on_eval(k, lvl, Tm, aff, out, pre):
        rep[1].set_points(lvl, pre)
        H, b, Hsc, bsc, r, capped = rep[1].eval(lvl, Tm, (float(aff[0]), float(aff[1])), **params)
        assert same_bytes(r, steps[k]["res"]), (k, r, steps[k]["res"])
        assert int(capped) == steps[k]["alpha_capped"]
        replays[k] = (H, b, Hsc, bsc)
        post = rep[1].points(lvl)
        assert differing_fields(post, ref.pts[lvl]) == [], k

    rres, rlog = ref.track_frame(dI, e, forced=steps, on_eval=on_eval)
    assert len(rlog) == n
    for key in ("lvl", "iteration", "accepted", "alpha_capped", "snapped"):
        assert [int(l[key]) for l in rlog] == steps[key].tolist(), key
    # the exposure-ratio guess (:71-73)
    if e > 0:
        assert steps[0]["aff"][0] == float(f32(math.log(float(f32(e) / f32(sc.first_exposure))))) and steps[0]["aff"][1] == 0
    # every step through ldso_ct_init_lm_step, from the system of the last accepted (or first) evaluation
    cur = None
    for k in range(n):
        s = steps[k]
        if s["iteration"] >= 0:
            lvl = int(s["lvl"])
            inc, To, abo = T.init_lm_step(*replays[cur], s["lambda"], sc.width >> lvl, sc.height >> lvl,
                                          steps[cur]["pose"].reshape(3, 4), steps[cur]["aff"], **params)
            assert same_bytes(inc, s["inc"]), (k, inc, s["inc"])
            assert TR.pose_ulps(To, s["pose"].reshape(3, 4)) <= 4
            assert same_bytes(abo, s["aff"])
            # calcEC's pair: exact while not snapped, else within the bound of its terms
            terms = rlog[k]["reg_terms"]
            assert s["reg_energy"][2] == rlog[k]["reg_energy"][2]
            if terms.shape[0] == 0:
                assert same_bytes(s["reg_energy"], rlog[k]["reg_energy"])
            else:
                cw = float(ref.p["coupling_weight"])
                exact, bound = IR.sum_bound(terms)
                for got in (s["reg_energy"][:2], rlog[k]["reg_energy"][:2]):
                    assert (np.abs(got.astype(np.float64) - cw * exact) <= cw * bound + 2.0 ** -24 * cw * exact).all()
        if s["iteration"] < 0 or s["accepted"]:
            cur = k
    for lvl in range(sc.levels):
        assert differing_fields(init.points(lvl), ref.pts[lvl]) == [], lvl
    for key in ("snapped", "frame_id", "snapped_at", "ret"):
        assert int(res[key]) == int(rres[key]), key
    assert res["iterations"].tolist() == rres["iterations"].tolist()
    assert same_bytes(res["this_to_next"].reshape(3, 4), rres["this_to_next"])
    assert same_bytes(res["this_to_next_aff"], rres["this_to_next_aff"])
    assert same_bytes(res["latest_res"], steps[cur]["res"])
    return res, rlog, steps


LOCK = [(name, None) for name in S.CASES] + [("shift", (1, 1, 1, 1, 1)), ("shift", (0, 0, 0, 0, 0))]


@pytest.mark.parametrize("name,iters", LOCK)
def test_lock_step_through_the_trace(built, name, iters):
    sc = S.scene(name)
    params = dict(sc.params, **({} if iters is None else dict(max_iterations=iters)))
    tr, init = context(sc, None)
    rep = context(sc, None)
    ref = sc.reference(**params)
    res, rlog, steps = lock_step(sc, tr, init, rep, ref, 1, params)
    if name == "same":
        assert not res["snapped"] and not steps["alpha_capped"].any()
    elif iters is None:
        assert res["snapped"] and steps["alpha_capped"].any()
    if iters is not None:  # `iteration >= maxIterations[lvl]` is tested after a step: iters + 1 steps at most
        assert (res["iterations"][:sc.levels] <= np.array(iters[:sc.levels]) + 1).all()
    if name == "wide5":
        assert set(steps["lvl"].tolist()) == {0, 1, 2, 3, 4}
    tr.close()
    rep[0].close()


def test_sequence_carries_state_and_returns(built):
    """Frames 1 .. 8 of the shifted sequence on one context: thisToNext, snapped, frameID and snappedAt carried
    from call to call, and the `frameID > snappedAt + 5` return."""
    sc = S.scene("shift")
    tr, init = context(sc, None)
    rep = context(sc, None)
    ref = sc.reference()
    rets = []
    for k in range(1, 9):
        res, _, _ = lock_step(sc, tr, init, rep, ref, k, {})
        assert res["frame_id"] == k and res["snapped_at"] == 1
        rets.append(int(res["ret"]))
    assert rets == [0, 0, 0, 0, 0, 0, 1, 1]
    tr.close()
    rep[0].close()


def test_rejected_step_leaves_its_maxstep(built):
    """The maxstep trap in the loop: frame 1, then frame 8 of the "border" scene.  An evaluation is rejected
    after one of its points left the image at a pattern pixel k > 0; there is no applyStep, the point stays
    good, and the level's next doStep reads the maxstep that evaluation left: the minimum over 0 .. k-1."""
    sc = S.scene("border")
    tr, init = context(sc, None)
    rep = context(sc, None)
    ref = sc.reference()
    lock_step(sc, tr, init, rep, ref, 1, {})
    seen = []
    orig = ref.calc_res_and_gs

    def spy(lvl, Tm, aff, dI):
        before = ref.pts[lvl].copy()
        out = orig(lvl, Tm, aff, dI)
        lost = (before["is_good"] != 0) & (ref.pts[lvl]["is_good_new"] == 0)
        seen.append(int((lost & (ref.pts[lvl]["maxstep"] < 1e9)).sum()))
        return out

    ref.calc_res_and_gs = spy
    _, rlog, _ = lock_step(sc, tr, init, rep, ref, 8, {})
    hits = [k for k, l in enumerate(rlog) if l["iteration"] >= 0 and not l["accepted"] and seen[k] > 0 and
            k + 1 < len(rlog) and rlog[k + 1]["lvl"] == l["lvl"]]
    assert hits, "the scene no longer produces the case"
    tr.close()
    rep[0].close()


# ---- 3. other checks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chain_before", "chain_after", "mixed"])
def test_opt_reg_equals_the_sequential_sweep(built, kind):
    """optReg on constructed lists: every neighbour precedes the point (each sweep step reads updated values:
    as many ranks as points), every neighbour follows it (all read old values), and a random table with
    self-references, -1 entries and bad points."""
    sc = S.scene("one_point_level")
    n = 300
    rng = np.random.default_rng(9)
    idx = np.arange(n)
    if kind == "chain_before":
        nb = np.stack([idx - 1 - j for j in range(10)], axis=1)
    elif kind == "chain_after":
        nb = np.stack([idx + 1 + j for j in range(10)], axis=1)
    else:
        nb = rng.integers(-1, n, (n, 10))
        nb[::5, 0] = idx[::5]
    nb = np.where((nb < 0) | (nb >= n), -1, nb).astype(np.int32)
    pts = [p.copy() for p in sc.points]
    p0 = pts[0][:n].copy()
    p0["neighbours"] = nb
    p0["idepth"] = rng.uniform(0.2, 3, n).astype(f32)
    p0["ir"] = rng.uniform(0.2, 3, n).astype(f32)
    p0["is_good"] = rng.uniform(size=n) > 0.15
    pts[0] = p0
    tr = CoarseTracker(sc.width, sc.height)
    tr.make_k(sc.calib)
    tr.set_new_frame(sc.first, 1.0)
    init = CoarseInitializer(tr)
    init.set_first(pts)
    ranks = init.rank_counts()
    assert ranks[0] == IR.sweep_ranks(nb) and (kind != "chain_before" or ranks[0] == n)
    ref = IR.Initializer(sc.width, sc.height, sc.calib, [d for d, _ in sc.first_dI], 1.0, pts)
    ref.snapped = True
    ref.opt_reg(0)
    init.opt_reg(0, 0.8, True)
    dev = init.points(0)
    assert differing_fields(dev, ref.pts[0]) == []
    assert not same_bytes(dev["ir"], p0["ir"])
    ref.snapped = False
    ref.opt_reg(0)
    init.opt_reg(0, 0.8, False)
    assert differing_fields(init.points(0), ref.pts[0]) == [] and (ref.pts[0]["ir"] == 1).all()
    tr.close()


def test_same_call_twice_gives_identical_bytes(built):
    sc = S.scene("expo")
    runs = []
    for _ in range(2):
        tr, init = context(sc)
        res, steps, n = init.track_frame(trace=TRACE, **sc.params)
        assert (res["phase_us"] > 0).all()
        res["phase_us"] = 0  # the launch's clock readings are no part of the result
        runs.append((res.tobytes(), steps.tobytes(), n, [init.points(l).tobytes() for l in range(sc.levels)]))
        tr.close()
    assert runs[0] == runs[1]


def test_refusals_on_a_context(built):
    sc = S.scene("one_point_level")
    tr = CoarseTracker(sc.width, sc.height)
    init = CoarseInitializer(tr)
    with pytest.raises(L.LdsoError, match="make_k"):
        init.set_first(sc.points)
    tr.make_k(sc.calib)
    with pytest.raises(L.LdsoError, match="set_new_frame"):
        init.set_first(sc.points)
    tr.set_new_frame(sc.first, 1.0)
    with pytest.raises(L.LdsoError, match="set_first"):
        init.track_frame()
    bad = [p.copy() for p in sc.points]
    bad[0]["neighbours"][3, 2] = bad[0].size
    with pytest.raises(L.LdsoError, match="neighbour"):
        init.set_first(bad)
    init.set_first(sc.points)
    with pytest.raises(L.LdsoError, match="trace_capacity"):
        L.check(L.lib().ldso_ct_init_track_frame(tr._h, None, np.zeros(1, L.INIT_RESULT_DTYPE).ctypes.data,
                                                 np.zeros(1, L.INIT_STEP_DTYPE).ctypes.data, 0, None))
    with pytest.raises(L.LdsoError, match="resident"):
        init.set_points(0, np.roll(sc.points[0], 1))
    res, steps, n = init.track_frame(trace=3)  # a short trace keeps the count
    assert len(steps) == 3 and n > 3
    tr.close()


@pytest.mark.parametrize("layout", [3, 1])
def test_first_frame_hand_off_to_the_frame_store(built, layout):
    """ldso_ba_frame_put_initializer, then ldso_ba_load_frames: the slot's image equals that of
    ldso_ba_frame_put of the host dI, and a pass over the window loaded by id matches the oracle."""
    import oracle
    from test_frame_store import check_pass, make_ctx, window, without_images

    name = "N3P64_160x120"
    w = window(name)
    c = make_ctx(layout, w.n_frames + 1, w)
    tr = CoarseTracker(w.width, w.height)
    tr.make_k(w.calib)
    tr.set_new_frame(w.dI[0, :, 0])
    init = CoarseInitializer(tr)
    uv = [np.array([[20.1, 20.1], [40.1, 30.1], [60.1, 50.1]], f32) / (1 << l) + f32(3) for l in range(tr.levels)]
    nb, par = IR.knn_tables(uv)
    init.set_first(IR.make_points(uv, nb, par))
    tr.set_new_frame(w.dI[1, :, 0])  # the snapshot, not the tracker's current frame, is handed over
    s0 = c.transfer_stats()
    c.frame_put_initializer(0, init)
    assert c.transfer_stats()["h2d_bytes"] == s0["h2d_bytes"]
    c.frame_put(99, w.dI[0])
    a, b = c.frame_get(0, with_grad=layout == 1), c.frame_get(99, with_grad=layout == 1)
    if layout == 1:
        assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    else:
        assert same_bytes(a, b)
    for f in range(1, w.n_frames):
        c.frame_put(f, w.dI[f])
    c.load([without_images(w)], frame_ids=list(range(w.n_frames)))
    check_pass(c, name)
    c.close()
    tr.close()
