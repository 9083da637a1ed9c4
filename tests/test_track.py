"""ldso_ct_track -- trackNewestCoarse's LM loop on the device in one call -- on the GPU, against

  1. itself, step by step: every evaluation the device logged is repeated through
     ldso_ct_calc_res_gs (the Vec6 bit for bit: the kernel's sum tree is that entry point's) and
     ldso_ct_lm_step (the increment bit for bit; the next pose within 4 ulp, every entry in its own
     ulps: host and device run the same statements, SE3::exp's sine and cosine included), and the restatement
     (track_ref.py) replayed over the log must take the same decisions: accepts, lambdas, iteration
     counts, exits;
  2. the oracle-driven restatement, free-running: the same exits, and on the convergence scenes a
     final pose and residuals within four times the spread of two oracle loops whose E, H and b
     carry 1e-7 relative noise (the bar of test_fuzz_optimize.py);
  3. itself, batched: eight starts in one call are the eight single calls bit for bit.
The cases are those test_track_ref.py shows to be well posed on the CPU."""

import numpy as np
import pytest

import track_ref as R
import track_scenes as S
from ldso_amd import _lib as L

pytestmark = pytest.mark.gpu
TRACE = 600  # above the evaluations of any case: 5 levels and a repeat, each 7 cutoffs + 50 iterations at most


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _assert_records_equal(a, b):
    for f in L.TRACK_RESULT_DTYPE.names:
        assert _same_bits(a[f], b[f]), f


def _lock_step(sc, ct, T, ab, mr, params):
    """One device run with its trace, checked step by step; returns (result, evaluations, worst pose ulp)."""
    from ldso_amd import tracker

    res, log, n = ct.track(T, ab, mr, trace=TRACE, **params)
    assert n == len(log) <= TRACE
    Hs, worst, where = [], 0.0, None
    cur = None  # the accepted evaluation: pose, aff, H, b, rs
    for e in log:
        rs, H, b = ct.calc_res_gs(int(e["lvl"]), e["pose"].reshape(3, 4), e["aff"], float(e["cutoff_th"]))
        assert _same_bits(rs, e["rs"]), (int(e["lvl"]), int(e["iteration"]), rs, e["rs"])
        Hs.append((H, b))
        if e["iteration"] < 0:
            # a level starts, and a cutoff doubles, at the pose and (a, b) accepted last
            assert cur is None or (_same_bits(e["pose"], cur[0]) and _same_bits(e["aff"], cur[1]))
            cur = (e["pose"].copy(), e["aff"].copy(), H, b, rs)
            continue
        inc, To, abo = tracker.lm_step(cur[2], cur[3], float(e["lambda"]), cur[0].reshape(3, 4), cur[1], **params)
        assert _same_bits(inc, e["inc"]), (int(e["lvl"]), int(e["iteration"]), inc, e["inc"])
        assert _same_bits(abo, e["aff"])
        d = R.pose_ulps(To, e["pose"])
        if d > worst:
            worst, where = d, (int(e["lvl"]), int(e["iteration"]), To - e["pose"].reshape(3, 4), e["pose"])
        with np.errstate(invalid="ignore"):  # 0 / 0 on a level without a point: NaN rejects
            accept = bool(rs[0] / rs[1] < cur[4][0] / cur[4][1])
        assert accept == bool(e["accepted"])
        if accept:
            cur = (e["pose"].copy(), e["aff"].copy(), H, b, rs)
    print(f"    worst next-pose distance {worst} ulp at (lvl, iteration) {where[:2] if where else None}")
    if worst > 4:
        print("    host - device:\n", where[2], "\n    device pose:\n", where[3].reshape(3, 4))
    assert worst <= 4, (worst, where)
    # the restatement over the logged evaluations: same decisions, same exits
    it = iter(range(len(log)))

    def calc_res(lvl, Tm, ab_, cutoff):
        k = next(it)
        e = log[k]
        assert (lvl, cutoff) == (int(e["lvl"]), float(e["cutoff_th"])) and tuple(ab_) == tuple(e["aff"])
        assert np.abs(Tm - e["pose"].reshape(3, 4)).max() < 1e-12
        return e["rs"], k

    res_r, log_r = R.track(calc_res, lambda lvl, k, ab_: Hs[k], T, ab, sc.coarsest, mr, ref_frame=(1.0, 1.0) + S.REF_AB,
                           **params)
    assert len(log_r) == len(log)
    for e, r in zip(log, log_r):
        assert (int(e["iteration"]), int(e["accepted"]), float(e["lambda"])) == (r["iteration"], r["accepted"], r["lam"])
        # (the increments are pinned above, bit for bit against ldso_ct_lm_step, which test_track_ref.py holds
        # to the restatement at 1e-13 on well-conditioned systems; two backward-stable solves differ by about
        # 8 eps cond(Hl), and cond(Hl) stays below 1e6 on these scenes)
        assert np.abs(e["inc"] - r["inc"]).max() <= 1e-9 * np.abs(r["inc"]).max() + 1e-300
    for f in ("ok", "reason", "abort_level", "repeated_level"):
        assert int(res[f]) == int(res_r[f]), f
    np.testing.assert_array_equal(res["iterations"], res_r["iterations"])
    assert _same_bits(res["last_residuals"], res_r["last_residuals"]) and _same_bits(res["flow"], res_r["flow"])
    assert _same_bits(res["aff"], res_r["aff"])
    assert np.abs(res["ref_to_new"].reshape(3, 4) - res_r["ref_to_new"]).max() < 1e-12
    return res, len(log), worst


@pytest.mark.parametrize("name", list(S.CASES))
def test_lock_step_through_the_trace(built, name):
    sa, T, ab, mr, case_params = S.CASES[name]
    sc = S.scene(*sa)
    ct = sc.tracker()
    worst, total = 0.0, 0
    for mode in S.MODES:
        for solve in (R.SOLVE_FULL, R.SOLVE_REFERENCE):
            params = S.params_of(case_params, mode, solve)
            res, n, w = _lock_step(sc, ct, T, ab, mr, params)
            worst, total = max(worst, w), total + n
    print(f"{name}: {total} evaluations in lock-step, worst next-pose distance {worst} ulp")
    ct.close()


@pytest.mark.parametrize("name", list(S.CASES))
def test_free_running_exits_match_oracle(built, name):
    sa, T, ab, mr, params = S.CASES[name]
    sc = S.scene(*sa)
    ct = sc.tracker()
    res = ct.track(T, ab, mr, **params)
    ref, _ = sc.track(T, ab, mr, **params)
    print(f"{name}: device ok {res['ok']} reason {res['reason']} iterations {res['iterations']}; oracle {ref['iterations']}")
    for f in ("ok", "reason", "repeated_level", "abort_level"):
        assert int(res[f]) == int(ref[f]), f
    np.testing.assert_array_equal(res["iterations"], ref["iterations"])
    np.testing.assert_array_equal(np.isnan(res["last_residuals"]), np.isnan(ref["last_residuals"]))
    ct.close()


@pytest.mark.parametrize("name,i,scale", S.CONVERGENCE)
def test_free_running_converges_within_noise_spread(built, name, i, scale):
    sc = S.scene(name, i)
    ct = sc.tracker()
    T0, ab = S.pose(i, scale), (S.REF_AB[0] + 0.05, S.REF_AB[1] + 2.0)
    res = ct.track(T0, ab, S.NEVER)
    ref, _ = sc.track(T0, ab, S.NEVER)
    noisy = [sc.track(T0, ab, S.NEVER, noise=(np.random.default_rng(50 + k), 1e-7))[0] for k in range(2)]
    spread_T = np.abs(noisy[0]["ref_to_new"] - noisy[1]["ref_to_new"]).max()
    spread_r = np.nanmax(np.abs(noisy[0]["last_residuals"] - noisy[1]["last_residuals"]))
    d_T = np.abs(res["ref_to_new"].reshape(3, 4) - ref["ref_to_new"]).max()
    d_r = np.nanmax(np.abs(res["last_residuals"] - ref["last_residuals"]))
    print(f"{name}: pose distance {d_T:.3g} (noise spread {spread_T:.3g}), residual distance {d_r:.3g} "
          f"(spread {spread_r:.3g}); iterations {res['iterations']} vs {ref['iterations']}")
    assert res["ok"] == 1 == ref["ok"]
    assert d_T <= 4 * spread_T and d_r <= 4 * spread_r


def test_batch_equals_single_calls(built):
    sc = S.scene("qvga", 2)
    ct = sc.tracker()
    far = S.pose(0).copy()
    far[:, 3] = (1e6, 1e6, -1e6)  # every point leaves the image at every level: lastResiduals all NaN
    Ts = np.stack([S.pose(2), S.pose(3, 2.0), S.pose(4, 1.0), far, S.pose(5, 4.0), S.pose(6), S.pose(7, 3.0), S.pose(8)])
    abs_ = np.array([S.REF_AB, (S.REF_AB[0], S.REF_AB[1] + 60.0), S.REF_AB, S.REF_AB, (0.3, 20.0), (-0.1, -5.0), S.REF_AB,
                     (S.REF_AB[0] + 8.0, S.REF_AB[1])])
    mrs = np.full((8, 5), np.nan)
    mrs[2] = 1e-6  # aborts at the coarsest level
    mrs[6] = (1e-6, 1e9, 1e9, 1e9, 1e9)  # aborts at level 0
    batch = ct.track(Ts, abs_, mrs)
    assert batch.shape == (8,)
    for k in range(8):
        _assert_records_equal(batch[k], ct.track(Ts[k], abs_[k], mrs[k]))
    assert batch["reason"][2] == 1 and batch["abort_level"][2] == sc.coarsest and batch["abort_level"][6] == 0
    assert batch["repeated_level"][1] == sc.coarsest and np.all(np.isnan(batch["last_residuals"][3, :sc.n_levels]))
    assert batch["ok"][0] == 1
    ct.close()


def test_calc_res_paths_agree_on_one_pose(built):
    """k_ct_calc_res<false> (ldso_ct_calc_res), <true> (ldso_ct_calc_res_gs) and k_ct_track's sweep are
    instantiations of one per-point function; the lock-step pins the last two to each other, this pins the first
    two, and k_ct_calc_gs over the records the first leaves: the same Vec6, the same warped records, the same
    H and b, bit for bit.  300 points at level 0: two blocks, the second ragged, the shift terms of every 32nd
    point, and points that leave the image, saturate and warp."""
    sc = S.scene("kitti", 7)
    ct = sc.tracker()
    T, ab = S.pose(9, 4.0), (S.REF_AB[0] + 0.05, S.REF_AB[1] + 2.0)
    n = sc.pcs[0]["u"].size
    rs = ct.calc_res(0, T, ab, 20.0)
    warped = ct.warped()
    H, b = ct.calc_gs(0, T, ab)
    rs2, H2, b2 = ct.calc_res_gs(0, T, ab, 20.0)
    warped2 = ct.warped()
    n_sat = round(rs[5] * rs[1])
    print(f"{n} points: {int(rs[1])} in the image, {n_sat} saturated, shift terms {rs[2]:.4g} / {rs[4]:.4g}")
    assert n == 300 and 0 < n_sat < rs[1] < n and rs[2] > 0 and rs[4] > 0
    assert len(warped) == (int(rs[1]) - n_sat + 3) // 4 * 4
    assert _same_bits(rs, rs2) and _same_bits(warped, warped2)
    assert _same_bits(H, H2) and _same_bits(b, b2) and np.all(np.isfinite(H)) and np.abs(b).max() > 0
    ct.close()


def test_refusals_repeatability_and_trace_capacity(built):
    from ldso_amd.tracker import CoarseTracker

    sc = S.scene("qvga", 2)
    T, ab = S.pose(2), S.REF_AB
    raw = CoarseTracker(sc.w, sc.h)
    with pytest.raises(RuntimeError, match="make_k"):
        raw.track(T, ab)
    raw.make_k(sc.calib)
    with pytest.raises(RuntimeError, match="set_new_frame"):
        raw.track(T, ab)
    raw.set_new_frame(sc.color, 1.0)
    with pytest.raises(RuntimeError, match="set_reference"):
        raw.track(T, ab)
    raw.close()
    ct = sc.tracker()
    for lvl in (-1, ct.levels, 5):
        with pytest.raises(RuntimeError, match="coarsest_lvl"):
            ct.track(T, ab, coarsest_lvl=lvl)
    with pytest.raises(RuntimeError, match="n must be"):
        ct.track(np.zeros((0, 3, 4)), np.zeros((0, 2)), np.zeros((0, 5)))
    for bad, match in ((dict(solve=7), "solve"), (dict(coarse_cutoff_th=float("inf")), "cutoff"),
                       (dict(lambda_decrease=0.0), "lambda"), (dict(max_iterations=(10, 20, -1, 50, 50)), "max_iterations")):
        with pytest.raises(RuntimeError, match=match):
            ct.track(T, ab, **bad)
    # a trace with no room is refused
    out = np.zeros(1, L.TRACK_RESULT_DTYPE)
    steps = np.zeros(1, L.TRACK_STEP_DTYPE)
    args = (ct._h, 1, L.ptr(np.ascontiguousarray(T), L.f64p), L.ptr(np.array(ab, np.float64), L.f64p), sc.coarsest,
            L.ptr(np.full(5, np.nan), L.f64p), None, out.ctypes.data, steps.ctypes.data)
    assert L.lib().ldso_ct_track(*args, 0, None) < 0 and "trace_capacity" in L.lib().ldso_ba_last_error().decode()
    # two calls give the same bits; a short trace is the head of the long one and still counts them all
    a, log_a, n_a = ct.track(T, ab, trace=TRACE)
    b, log_b, n_b = ct.track(T, ab, trace=TRACE)
    _assert_records_equal(a, b)
    assert n_a == n_b == len(log_a) > 3 and log_a.tobytes() == log_b.tobytes()
    c, log_c, n_c = ct.track(T, ab, trace=3)
    _assert_records_equal(a, c)
    assert n_c == n_a and len(log_c) == 3 and log_c.tobytes() == log_a[:3].tobytes()
    _assert_records_equal(a, ct.track(T, ab))  # no trace at all
    # a finer start level, and the warped buffers left invalid
    d = ct.track(T, ab, coarsest_lvl=0)
    assert np.all(np.isnan(d["last_residuals"][1:])) and d["iterations"][1:].sum() == 0
    with pytest.raises(RuntimeError, match="calcRes"):
        ct.calc_gs(0, T, ab)
    ct.close()
