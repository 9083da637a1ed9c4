"""ldso_ba_optimize's device loop pinned step by step (k_step_resub: the frame and calibration
step, FrameFramePrecalc::Set for every pair, the solver's prior vector, the point step, canbreak).

test_optimize.py and test_fuzz_optimize.py compare the finished loop with a free-running host loop;
both loops amplify the float reassociation of H, so their bars are wide (5 % of the accumulated
step).  Here the oracle walks beside the device and is put back onto the DEVICE's own state after
every step: optimize(k) for k = 0 ... K gives S_k = (frames, calibration, idepths) and, through
ldso_ba_get_loop_state, the x of the last solve, the precalc rows and the prior vector.  Each step
S_{k-1} -> S_k is then checked by itself, with the device's own x_{k-1}, so nothing accumulates:

  1. energy rows 0 ... k-1 of optimize(k) equal optimize(k-1)'s bit for bit; the call that replays
     the captured graph equals the direct one bit for bit in every output;
  2. x_{k-1} against the oracle's solve of the oracle's system of pass k-1 (test_gpu_parity's
     envelope bar);
  3. frame states against the host helper ldso_ba_frame_step (same se3.h statements; the device
     library's sincos / atan against glibc's), a, b and the calibration bit-equal, every other
     field of the frame record untouched;
  4. the precalc rows against ldso_ba_frame_precalc of the device's stepped states: 1 float ulp,
     at most 0.1 % of the entries not bit-equal, b = bT - a bF within |bF| ulp(a) + ulp(b);
  5. the prior vector: HL diagonal bit-equal to takeData's prior / cPrior under the same settings,
     bL = prior * delta_prior (cPrior * cDeltaF) within item 3's bar;
  6. the point step against the oracle's resubstitution with x_{k-1};
  7. the pass after the step against the oracle's pass from S_k with the device's precalc rows:
     per-residual states, energies and centre projections bit-equal, frameEnergyTH bit-equal, #IN
     equal, E within 1e-12;
  8. iterations and status against ldso_ba_step_canbreak on x_{k-1}; a stopped window keeps S,
     precalc and priors bit for bit and repeats its last energy row.

Measured on an MI355X (worst over all cases and steps; the test prints them):
  item 3: |device - helper| / max(1, |state_f|_inf) = 0: on these windows the device library's
          sincos / atan give glibc's bits.  The bar is 4x the measurement (never above 1e-12), hence 0:
          the stepped states, and item 5's bL, are asserted bit-equal to the host helper's;
  item 4: 0 of 55,584 precalc entries not bit-equal (a and b included, once the device takes the
          float exp as the double exp rounded once: with the device library's expf a was an ulp
          off in some pairs and b, through the rounded product a bF, four of its own ulps --
          more than |bF| ulp(a) + ulp(b), which leaves out ulp(a bF));
  item 6: |step_dev - step_oracle| / |step_oracle| <= 5.96e-6 (N5_fwd_aff, iteration 2); the bar is
          4x that, 2.4e-5, instead of test_gpu_parity's 1e-3.
The zero bars are not vacuous: a build whose device code alone sums the quaternion norm in another
order (a change of an ulp) fails item 3 in every case at the first step (differences of 1e-20),
and one that leaves cPrior * cDeltaF out of bL fails item 5.  Reusing squaredNorm for V's theta_sq
in the device's exp alone is NOT seen here: at these windows' rotation angles (1e-3) it changes no
bit of a step; tests/test_sophus_kat.py::test_exp_theta_sq_known_answers pins it in the shared source.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from ldso_amd import _lib as L
from ldso_amd import synth

K = 4  # iterations 0, 1 solve without the nullspace projection, 2, 3 with it
LIBM_BAR = 0.0     # item 3 (and item 5's bL): 4x the measured 0; never to be raised above 1e-12
POINT_BAR = 2.4e-5  # item 6: 4x the worst measured ratio (test_gpu_parity's bar is 1e-3)

# windows of one context; mode: setting_affineOptModeA / B; exact: LDSO_BA_TUNE_SOLVE_EXACT;
# k_max: the steps walked (batch goes one past K: its first window stops after iteration 3, and the
# step after that shows it standing still while the others run on).  A context takes windows of one
# image size only, so the 11-frame window shares the S7 window's 640 x 480.
CASES = {
    "N2": dict(cfgs=[dict(n_frames=2, n_points=100, width=160, height=120, seed=21)], mode=(1e12, 1e8), exact=False,
               k_max=K),
    "N5_fwd_aff": dict(cfgs=[dict(n_frames=5, n_points=400, motion="forward", outlier_frac=0.1, seed=31)],
                       mode=(-1.0, 5.0), exact=False, k_max=K),
    "batch": dict(cfgs=[dict(synth.S7, seed=62), dict(n_frames=11, n_points=700, seed=41),
                        dict(n_frames=3, n_points=150, seed=51)], mode=(1e12, 1e8), exact=False, k_max=K + 1),
    "S7_exact": dict(cfgs=[dict(synth.S7, seed=63)], mode=(1e12, 1e8), exact=True, k_max=K),
}
STOPPING = {"batch": 0}  # the window of the case that leaves the loop on canbreak


def settings_of(case):
    a, b = case["mode"]
    return L.OptSettings.default(affine_opt_mode_a=a, affine_opt_mode_b=b)


def window(cfg, s):
    w = synth.make_window(**cfg)
    w.settings = s
    return w.refresh_frame_terms()


def ulp32(a, b):
    """distance in float32 representation steps, elementwise"""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(2 ** 31) - ia, ia)
    ib = np.where(ib < 0, -(2 ** 31) - ib, ib)
    return np.abs(ia - ib)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sum_nid(w, idepth):
    """doStepFromBackup's float sumNID (FullSystem.cc:1899-1909): hosts in turn, each host's points in
    the caller's order (the device's point order without ranks), a float chain."""
    s = np.float32(0)
    for f in range(w.n_frames):
        for q in np.flatnonzero(w.point_host == f):
            s = np.float32(s + np.float32(abs(idepth[q])))
    return s


# ------------------------------------------------------------------------------------------
# CPU: the cases are well posed (host loop alone)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_lockstep_cases_are_well_posed(built, name):
    """Each window runs its iterations with a finite x on the host loop, keeps at least 20 % of its
    residuals active at every pass, and the window that stops does so with its canbreak ratios at
    least 5 % away from 1 at every iteration (seeds are chosen for this, not the bars)."""
    from test_optimize import host_optimize

    case = CASES[name]
    s = settings_of(case)
    with oracle.affine_opt_modes(*case["mode"]):
        for i, cfg in enumerate(case["cfgs"]):
            w = window(cfg, s)
            n_res = w.n_residuals
            e, fr, cv, idep, its, st, ratios = host_optimize(w, case["k_max"], w.nullspaces())
            worst = ratios.max(axis=1)
            print(f"{name}[{i}]: its {its} status {st}, #IN/R {[round(float(r[2]) / n_res, 3) for r in e]}, "
                  f"max canbreak ratios {np.round(worst, 3)}")
            assert st != L.OPT_LOST and np.isfinite(fr["state"]).all() and np.isfinite(idep).all()
            assert all(float(r[2]) >= 0.2 * n_res for r in e)
            if STOPPING.get(name) == i:
                assert st == L.OPT_CONVERGED and its == K, "the stopping window leaves after iteration K - 1"
                assert np.all(np.abs(worst - 1.0) >= 0.05)
            else:
                assert its == case["k_max"] and st == L.OPT_RAN_ALL


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
def device_run(case, k):
    """optimize(k) on a fresh context, then the same windows loaded again and optimize(k) replayed
    from the captured graph: every output equal bit for bit; returns the replayed outputs per window."""
    from ldso_amd import BAContext

    s = settings_of(case)
    ctx = BAContext(0)
    if case["exact"]:
        ctx.set_tuning(12, 1)  # LDSO_BA_TUNE_SOLVE_EXACT
    ctx.set_settings(s)
    calls = []
    for call in range(2):
        ws = [window(cfg, s) for cfg in case["cfgs"]]
        nss = [w.nullspaces() for w in ws]
        ctx.load(ws)
        e, fr, cv, idep, its, st = ctx.optimize(k, nullspaces=nss, settings=s)
        outs, off = [], 0
        for i, w in enumerate(ws):
            ls = ctx.loop_state(i)
            outs.append(dict(e=e[:, i].copy(), frames=fr[off:off + w.n_frames].copy(), calib=cv[i].copy(),
                             idepth=idep[i].copy(), its=int(its[i]), status=int(st[i]), res=ctx.residuals(i),
                             th=ctx.frame_energy_th(i), x=ls["x"], precalc=ls["precalc"], prior=ls["prior"]))
            off += w.n_frames
        calls.append(outs)
    ctx.close()
    for i, (a, b) in enumerate(zip(*calls)):
        for key in a:
            if key == "x" and k == 0:
                continue  # no solve has run: x is whatever the buffer held
            if key == "res":
                for rk in a["res"]:
                    assert same_bits(a["res"][rk], b["res"][rk]), ("replay", k, i, rk)
            elif key in ("its", "status"):
                assert a[key] == b[key], ("replay", k, i, key)
            else:
                assert same_bits(a[key], b[key]), ("replay", k, i, key)
    return calls[1]


def host_frame_step(frames, x, cval, czero):
    out = np.zeros_like(frames)
    sf, cd = np.zeros(4, np.float32), np.zeros(4, np.float32)
    cv = np.ascontiguousarray(cval, np.float64).copy()
    L.check(L.lib().ldso_ba_frame_step(len(frames), np.ascontiguousarray(frames).ctypes.data,
                                       L.ptr(np.ascontiguousarray(x, np.float64), L.f64p), out.ctypes.data,
                                       L.ptr(cv, L.f64p), L.ptr(np.ascontiguousarray(czero, np.float64), L.f64p),
                                       L.ptr(sf, L.f32p), L.ptr(cd, L.f32p)))
    return out, cv, sf, cd


def host_precalc(frames, calib_f32):
    N = len(frames)
    pre = np.zeros((N * N, L.PRECALC_STRIDE), np.float32)
    L.check(L.lib().ldso_ba_frame_precalc(N, np.ascontiguousarray(frames).ctypes.data,
                                          L.ptr(np.ascontiguousarray(calib_f32, np.float32), L.f32p), L.ptr(pre, L.f32p)))
    return pre


def host_take_data(frames, s):
    N = len(frames)
    prior, delta, dprior = (np.zeros((N, 8)) for _ in range(3))
    L.check(L.lib().ldso_ba_frame_take_data(N, np.ascontiguousarray(frames).ctypes.data, C.byref(s),
                                            L.ptr(prior, L.f64p), L.ptr(delta, L.f64p), L.ptr(dprior, L.f64p)))
    return prior, dprior


def check_residuals(dev, ow, e_cpu, e_row, tag):
    """the per-residual half of test_gpu_parity.compare_pass on optimize's own outputs"""
    rc = ow.residuals()
    for key in ("new_state", "state", "flags", "state_energy", "new_energy_wo", "center"):
        assert same_bits(dev["res"][key], rc[key]), (tag, key, int((dev["res"][key] != rc[key]).sum()))
    assert same_bits(dev["th"], ow.frame_energy_th()), (tag, "frame_energy_th", dev["th"], ow.frame_energy_th())
    assert e_row[2] == e_cpu[2], (tag, "#IN", e_row, e_cpu)
    assert abs(e_row[0] - e_cpu[0]) <= 1e-12 * abs(e_cpu[0]), (tag, "E", e_row, e_cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_loop_in_lockstep_with_the_oracle(built, name):
    from test_gpu_parity import sensitivity
    from test_optimize import canbreak_numpy

    case = CASES[name]
    s = settings_of(case)
    th_opt, min_its = 1.2, 1
    lib = L.lib()
    worst_libm, worst_bl, worst_point, n_pre_diff, n_pre = 0.0, 0.0, 0.0, 0, 0
    runs = [device_run(case, k) for k in range(case["k_max"] + 1)]
    with oracle.affine_opt_modes(*case["mode"]):
        for i, cfg in enumerate(case["cfgs"]):
            w = window(cfg, s)
            N, ns = w.n_frames, w.nullspaces()
            czero = w.calib.astype(np.float64) * (1.0 / 50.0)
            loaded = dict(frames=np.ascontiguousarray(w.frames).copy(), idepth=w.point_data[:, 2].copy(),
                          precalc=w.precalc.copy())
            ow = oracle.OracleWindow(w, threads=0)
            ow.reset_oob()
            e_cpu, sysm = ow.iteration()
            # ---- S_0: optimize(0) is the initial pass alone and returns the loaded window ----
            d0 = runs[0][i]
            tag = (name, i, 0)
            assert (d0["its"], d0["status"]) == (0, L.OPT_RAN_ALL), tag
            assert same_bits(d0["frames"], loaded["frames"]) and same_bits(d0["calib"], czero), tag
            assert same_bits(d0["idepth"], loaded["idepth"]) and same_bits(d0["precalc"], loaded["precalc"]), tag
            t = oracle.frame_terms(w)
            hl = np.concatenate([t["c_prior"], t["frame_prior"].ravel()])
            assert same_bits(d0["prior"][:, 0], hl), tag
            bl = np.concatenate([w.c_prior * w.c_delta.astype(np.float64), (w.frame_prior * w.frame_delta_prior).ravel()])
            assert same_bits(d0["prior"][:, 1], bl), tag  # the loaded terms, multiplied on the host
            check_residuals(d0, ow, e_cpu, d0["e"][0], tag)
            stop_at = None
            for k in range(1, case["k_max"] + 1):
                prev, dev = runs[k - 1][i], runs[k][i]
                tag = (name, i, k)
                # ---- 1. repeatability -----------------------------------------------------
                assert same_bits(dev["e"][:k], prev["e"][:k]), tag
                assert dev["idepth"].dtype == np.float32 and np.isfinite(dev["idepth"]).all(), tag
                # ---- 8. a stopped window keeps its state ------------------------------------
                if stop_at is not None:
                    at = runs[stop_at][i]
                    assert (dev["its"], dev["status"]) == (stop_at, L.OPT_CONVERGED), tag
                    for key in ("frames", "calib", "idepth", "precalc", "prior", "th"):
                        assert same_bits(dev[key], at[key]), (tag, key)
                    for rk in ("new_state", "state", "flags", "state_energy", "new_energy_wo", "center"):
                        assert same_bits(dev["res"][rk], at["res"][rk]), (tag, rk)
                    for row in range(stop_at + 1, k + 1):
                        assert same_bits(dev["e"][row], dev["e"][stop_at]), (tag, row)
                    continue
                x = dev["x"]
                assert np.isfinite(x).all(), tag
                # ---- 2. the solve -----------------------------------------------------------
                xo = oracle.solve_system(N, k - 1, 1e-5, sysm, nullspaces=ns)
                env = sensitivity(N, k - 1, sysm, ns, xo)
                rel = np.linalg.norm(x - xo) / np.linalg.norm(xo)
                bar = max(1e-6, 20 * env)
                if case["exact"] and 20 * env <= 1e-9:  # the envelope allows the solver's own bar
                    bar = 1e-9
                print(f"{tag} solve: |x_dev - x_oracle| / |x| = {rel:.3e}, envelope {env:.3e}, bar {bar:.3e}")
                assert rel <= bar, tag
                # ---- 3. the frame and calibration step --------------------------------------
                h_fr, h_cv, h_sf, h_cd = host_frame_step(prev["frames"], x, prev["calib"], czero)
                for f in range(N):
                    d = np.abs(dev["frames"]["state"][f, :6] - h_fr["state"][f, :6]).max()
                    worst_libm = max(worst_libm, d / max(1.0, np.abs(h_fr["state"][f]).max()))
                    assert d <= LIBM_BAR * max(1.0, np.abs(h_fr["state"][f]).max()), (tag, f, d)
                assert same_bits(dev["frames"]["state"][:, 6:], h_fr["state"][:, 6:]), tag
                assert same_bits(dev["calib"], h_cv), tag
                for key in ("state_zero", "world_to_cam_evalpt", "ab_exposure", "is_first_frame", "pad_"):
                    assert same_bits(dev["frames"][key], prev["frames"][key]), (tag, key)
                # ---- 4. FrameFramePrecalc::Set of the device's stepped states ---------------
                h_pre = host_precalc(dev["frames"], h_sf)
                u = ulp32(dev["precalc"], h_pre)
                plain = np.ones(L.PRECALC_STRIDE, bool)
                plain[[24, 25]] = False
                assert u[:, plain].max() <= 1, (tag, "precalc", int(u[:, plain].max()))
                assert u[:, 24].max() <= 1, (tag, "a", int(u[:, 24].max()))
                bF = np.array([np.float32(1000.0 * dev["frames"]["state"][e % N, 7]) for e in range(N * N)], np.float64)
                tol_b = np.abs(bF) * np.spacing(np.abs(h_pre[:, 24])).astype(np.float64) + \
                    np.spacing(np.abs(h_pre[:, 25])).astype(np.float64)
                assert np.all(np.abs(dev["precalc"][:, 25].astype(np.float64) - h_pre[:, 25]) <= tol_b), (tag, "b")
                assert same_bits(dev["precalc"][:, 26:27], h_pre[:, 26:27]), tag
                assert same_bits(dev["precalc"][:, 39:], h_pre[:, 39:]) and not dev["precalc"][:, 39:].any(), tag
                n_pre_diff += int((u != 0).sum())
                n_pre += u.size
                # ---- 5. the prior vector ------------------------------------------------------
                w.frames = dev["frames"]
                w.calib, w.c_delta = h_sf.copy(), h_cd.copy()
                t = oracle.frame_terms(w)
                hl = np.concatenate([t["c_prior"], t["frame_prior"].ravel()])
                p_prior, p_dprior = host_take_data(dev["frames"], s)
                assert same_bits(t["frame_prior"], p_prior), tag
                assert same_bits(dev["prior"][:, 0], hl), (tag, "HL")
                want = np.concatenate([t["c_prior"] * h_cd.astype(np.float64), (p_prior * p_dprior).ravel()])
                scale = np.concatenate([np.maximum(1, np.abs(t["c_prior"])) * np.maximum(1, np.abs(h_cd)),
                                        (np.maximum(1, np.abs(p_prior)) * np.maximum(1, np.abs(p_dprior))).ravel()])
                worst_bl = max(worst_bl, float((np.abs(dev["prior"][:, 1] - want) / scale).max()))
                assert np.all(np.abs(dev["prior"][:, 1] - want) <= LIBM_BAR * scale), (tag, "bL", worst_bl)
                assert same_bits(dev["prior"][:4, 1], want[:4]), (tag, "cPrior cDeltaF")
                # ---- 6. the point step ------------------------------------------------------
                step_o = ow.resubstitute(x, 1e-5).astype(np.float64)
                step_d = dev["idepth"].astype(np.float64) - prev["idepth"].astype(np.float64)
                ratio = np.linalg.norm(step_d - step_o) / max(np.linalg.norm(step_o), 1e-300)
                worst_point = max(worst_point, ratio)
                print(f"{tag} point step: |d_dev - d_oracle| / |d_oracle| = {ratio:.3e} (|d| = {np.linalg.norm(step_o):.3e})")
                assert np.linalg.norm(step_d - step_o) <= POINT_BAR * np.linalg.norm(step_o) + 1e-12, tag
                # ---- 8. the exits -------------------------------------------------------------
                cb = C.c_int32(0)
                L.check(lib.ldso_ba_step_canbreak(N, L.ptr(np.ascontiguousarray(x), L.f64p), float(sum_nid(w, prev["idepth"])),
                                                  float(np.float32(w.n_points)), th_opt, C.byref(cb)))
                r = canbreak_numpy(N, x, prev["idepth"], th_opt)
                print(f"{tag} canbreak ratios {np.round(r, 4)} -> {bool(cb.value)}; device its {dev['its']} status {dev['status']}")
                stops = bool(cb.value) and k - 1 >= min_its
                if abs(r.max() - 1.0) >= 0.01:
                    assert (dev["its"], dev["status"]) == (k, L.OPT_CONVERGED if stops else L.OPT_RAN_ALL), tag
                else:
                    stops = dev["status"] == L.OPT_CONVERGED  # undecidable within rounding: follow the device
                if stops:
                    stop_at = k
                # ---- 7. the pass after the step, from the device's S_k ------------------------
                w.point_data = w.point_data.copy()
                w.point_data[:, 2] = dev["idepth"]
                w.point_data[:, 3] = dev["idepth"]
                w.point_data[:, 5] = 0
                for key in ("ad_host", "ad_target", "c_prior", "frame_prior", "frame_delta", "frame_delta_prior"):
                    setattr(w, key, t[key])
                w.precalc = dev["precalc"].copy()  # the device's rows: the pass comparison stays free of libm
                w.frame_energy_th = ow.frame_energy_th().copy()
                ow.update(w)
                e_cpu, sysm = ow.iteration()
                check_residuals(dev, ow, e_cpu, dev["e"][k], tag)
            ow.close()
    if STOPPING.get(name) is not None:
        last = runs[case["k_max"]][STOPPING[name]]
        assert last["status"] == L.OPT_CONVERGED and last["its"] < case["k_max"], "no window stopped while others ran on"
    print(f"{name}: item 3 worst |device - helper| / max(1, |state|_inf) = {worst_libm:.3e}; "
          f"item 4 precalc entries not bit-equal {n_pre_diff} of {n_pre}; item 5 worst bL difference {worst_bl:.3e}; item 6 worst point-step ratio {worst_point:.3e}")
    assert n_pre_diff <= 1e-3 * n_pre


# ------------------------------------------------------------------------------------------
# ldso_ba_get_loop_state's error convention
# ------------------------------------------------------------------------------------------
def test_loop_state_without_a_context(built):
    lib = L.lib()
    assert lib.ldso_ba_get_loop_state(None, 0, L.ptr(None, L.f64p), L.ptr(None, L.f32p), L.ptr(None, L.f64p)) < 0
    assert b"null ctx" in lib.ldso_ba_last_error()


@pytest.mark.gpu
def test_loop_state_errors_and_null_outputs(built):
    """No windows and a bad window index are refused with a message; any output may be NULL; after
    a load the view is the loaded precalc rows and the uploaded prior vector."""
    from ldso_amd import BAContext

    ctx = BAContext(0)
    with pytest.raises(RuntimeError, match="no windows loaded"):
        ctx.loop_state(0)
    ws = [synth.make_window(n_frames=3, n_points=40, width=160, height=120, seed=5),
          synth.make_window(n_frames=2, n_points=30, width=160, height=120, seed=6)]
    pre = [w.precalc.copy() for w in ws]
    hl = [np.concatenate([w.c_prior, w.frame_prior.ravel()]) for w in ws]
    ctx.load(ws)
    lib = L.lib()
    for bad in (-1, 2):
        assert lib.ldso_ba_get_loop_state(ctx._h, bad, L.ptr(None, L.f64p), L.ptr(None, L.f32p), L.ptr(None, L.f64p)) < 0
        assert b"bad window index" in lib.ldso_ba_last_error()
    L.check(lib.ldso_ba_get_loop_state(ctx._h, 1, L.ptr(None, L.f64p), L.ptr(None, L.f32p), L.ptr(None, L.f64p)))
    for i in range(2):
        ls = ctx.loop_state(i)
        assert same_bits(ls["precalc"], pre[i]) and same_bits(ls["prior"][:, 0], hl[i]), i
    ctx.close()
