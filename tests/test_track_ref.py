"""trackNewestCoarse's LM loop (CoarseTracker.cc:61-310) without a GPU: the Python restatement
(track_ref.py) against answers that do not share its code, the library's host step
(ldso_ct_lm_step) against the restatement, the refusals that need no device, and the well-posedness
of the cases test_track.py runs on the GPU -- each must show its event on the oracle alone.
Parity unpinned by the reference binary itself (Eigen is absent here): the solve decision rests on
the reference text and Eigen's documented LDLT<., Lower> contract."""
import ctypes as C

import numpy as np
import pytest

import track_ref as R
import track_scenes as S
from ldso_amd import _lib as L


@pytest.mark.parametrize("n", [6, 7, 8])
def test_ldlt_matches_numpy(n):
    rng = np.random.default_rng(n)
    for k in range(20):
        M = rng.standard_normal((n, n + 3))
        A = M @ M.T + n * np.eye(n)  # SPD, condition number of a few tens
        b = rng.standard_normal(n)
        lower = np.tril(A) + np.triu(rng.standard_normal((n, n)), 1)  # the upper triangle is never read
        x = np.array(R.ldlt_solve(lower, b))
        ref = np.linalg.solve(A, b)
        assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max(), k


def test_diagonal_mode_known_answer():
    """REFERENCE: inc_i = -b_i / (H_ii (1 + lambda)), whatever stands off the diagonal."""
    H = np.diag([2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0]) + 0.5
    H[np.diag_indices(8)] -= 0.5
    b = -np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    lam = np.float32(0.25)  # 1 + lambda exact in float
    for mode, keep in (("ab", range(8)), ("fix_ab", range(6)), ("fix_b", range(7)), ("fix_a", (0, 1, 2, 3, 4, 5, 7))):
        p = S.params_of(R.DEFAULTS, mode, R.SOLVE_REFERENCE)
        inc = R.lm_increment(H, b, lam, p)
        want = np.zeros(8)
        for i in keep:
            want[i] = (i + 1) / (2.0 ** (i + 1) * 1.25)
        np.testing.assert_array_equal(inc, want)
    # FULL on the same system is numpy's answer
    inc = R.lm_increment(H, b, lam, S.params_of(R.DEFAULTS, "ab", R.SOLVE_FULL))
    np.testing.assert_allclose(inc, np.linalg.solve(H + np.diag(np.diag(H)) * 0.25, -b), rtol=1e-12)
    # a zero pivot gives a zero increment (LDLT::_solve_impl's tolerance), not a division by zero
    H0 = H.copy()
    H0[3, 3] = 0
    assert R.lm_increment(H0, b, lam, S.params_of(R.DEFAULTS, "ab", R.SOLVE_REFERENCE))[3] == 0


def _lib_step(H, b, lam, T, ab, params):
    p = L.LdsoCtTrackParams()
    L.lib().ldso_ct_track_default_params(C.byref(p))
    for k, v in params.items():
        setattr(p, k, (C.c_int32 * 5)(*v) if k == "max_iterations" else v)
    inc, To, abo = np.zeros(8), np.zeros((3, 4)), np.zeros(2)
    rc = L.lib().ldso_ct_lm_step(L.ptr(np.ascontiguousarray(H, np.float64).reshape(64), L.f64p),
                                 L.ptr(np.ascontiguousarray(b, np.float64), L.f64p), float(lam),
                                 L.ptr(np.ascontiguousarray(T, np.float64), L.f64p),
                                 L.ptr(np.ascontiguousarray(ab, np.float64), L.f64p), C.byref(p), L.ptr(inc, L.f64p),
                                 L.ptr(To, L.f64p), L.ptr(abo, L.f64p))
    return rc, inc, To, abo


def _system(rng):
    M = rng.standard_normal((8, 12))
    D = np.array([30, 30, 30, 300, 300, 300, 50, 1]) * 10.0 ** rng.uniform(-0.5, 0.5, 8)
    return D[:, None] * (M @ M.T) * D[None, :], rng.standard_normal(8) * D * 0.01


@pytest.mark.parametrize("solve", [R.SOLVE_FULL, R.SOLVE_REFERENCE])
@pytest.mark.parametrize("mode", list(S.MODES))
def test_lm_step_matches_restatement(built, mode, solve):
    rng = np.random.default_rng(7)
    params = S.params_of({}, mode, solve)
    worst_inc, worst_pose = 0.0, 0.0
    for k in range(12):
        H, b = _system(rng)
        lam = np.float32([0.01, 0.005, 0.000625, 7.8125e-05, 5.12, 0.001][k % 6])  # both sides of the extrapolation limit
        T = S.pose(k, 5.0)
        ab = (0.02 + 0.1 * k, 3.0 - k)
        rc, inc, To, abo = _lib_step(H, b, lam, T, ab, params)
        assert rc == 0
        inc_r, pose_r, aff_r = R.lm_step(H, b, lam, R.pose_from_matrix(T), (np.float32(ab[0]), np.float32(ab[1])),
                                         dict(R.DEFAULTS, **params))
        inc_r = np.array(inc_r)
        worst_inc = max(worst_inc, float(np.abs(inc - inc_r).max() / np.abs(inc_r).max()))
        worst_pose = max(worst_pose, R.pose_ulps(To, R.pose_matrix(pose_r)))
        np.testing.assert_array_equal(abo, np.array(aff_r, np.float64))
        assert np.all((inc_r == 0) == (inc == 0))  # the fixed parameters' zeros
    print(f"lm_step vs restatement ({mode}, solve {solve}): inc {worst_inc:.3g} relative, pose {worst_pose} ulp")
    assert worst_inc <= 1e-13 and worst_pose <= 4


def test_lm_step_non_finite_guard(built):
    """A non-finite increment is zeroed (CoarseTracker.cc:197-206): the pose and (a, b) stay."""
    rng = np.random.default_rng(3)
    H, b = _system(rng)
    T = S.pose(1, 3.0)
    for poison in ("H", "b", "huge"):
        H2, b2 = H.copy(), b.copy()
        if poison == "H":
            H2[:] = np.nan  # a level with no warped point: 0 * (1 / 0)
        elif poison == "b":
            b2[2] = np.inf
        else:
            b2[:] = 1e300
            H2 = np.eye(8) * 1e-300
        for solve in (R.SOLVE_FULL, R.SOLVE_REFERENCE):
            rc, inc, To, abo = _lib_step(H2, b2, 0.01, T, (0.5, 2.0), dict(solve=solve))
            assert rc == 0
            np.testing.assert_array_equal(inc, np.zeros(8))
            assert np.abs(To - T).max() < 1e-15  # exp(0) * T, through the quaternion and back
            np.testing.assert_array_equal(abo, [0.5, 2.0])
            inc_r, pose_r, aff_r = R.lm_step(H2, b2, 0.01, R.pose_from_matrix(T), (np.float32(0.5), np.float32(2.0)),
                                        dict(R.DEFAULTS, solve=solve))
            assert inc_r == [0.0] * 8 and tuple(aff_r) == (0.5, 2.0)
            assert R.pose_ulps(To, R.pose_matrix(pose_r)) <= 4


def test_refusals_without_a_device(built):
    lib = L.lib()
    for name in ("ldso_ct_track", "ldso_ct_lm_step", "ldso_ct_track_default_params"):
        assert hasattr(lib, name)
    assert lib.ldso_ct_num_kernels() == 7 and lib.ldso_ba_abi_version() == 7
    p = L.LdsoCtTrackParams()
    lib.ldso_ct_track_default_params(C.byref(p))
    assert (p.coarse_cutoff_th, p.lambda_increase, p.lambda_decrease, list(p.max_iterations), p.solve) == \
        (20.0, 4.0, 0.5, [10, 20, 50, 50, 50], L.TRACK_SOLVE_FULL)
    assert p.affine_opt_mode_a == np.float32(1e12) and p.affine_opt_mode_b == np.float32(1e8)
    H, b = _system(np.random.default_rng(0))
    T = S.pose(0)
    for bad, match in ((dict(solve=2), "solve"), (dict(coarse_cutoff_th=0.0), "cutoff"),
                       (dict(lambda_increase=float("nan")), "lambda"), (dict(lambda_decrease=-1.0), "lambda"),
                       (dict(affine_opt_mode_a=float("inf")), "affine"), (dict(max_iterations=(10, 0, 50, 50, 50)), "max_iterations")):
        rc, *_ = _lib_step(H, b, 0.01, T, (0, 0), bad)
        assert rc < 0 and match in lib.ldso_ba_last_error().decode(), bad
    # a null context is refused before any device call
    out = np.zeros(1, L.TRACK_RESULT_DTYPE)
    rc = lib.ldso_ct_track(None, 1, L.ptr(np.ascontiguousarray(T), L.f64p), L.ptr(np.zeros(2), L.f64p), 0,
                           L.ptr(np.zeros(5), L.f64p), None, out.ctypes.data, None, 0, None)
    assert rc < 0 and "null context" in lib.ldso_ba_last_error().decode()


def _run(name):
    sa, T, ab, mr, params = S.CASES[name]
    return S.scene(*sa).track(T, ab, mr, **params)


def test_cases_produce_their_events(built):
    """Each case of test_track.py shows, on the oracle-driven restatement alone, the event it is there for."""
    res, log = _run("reject")
    assert any(e["iteration"] >= 0 and not e["accepted"] for e in log) and res["ok"] == 1
    res, log = _run("extrapolate")
    run = best = 0
    for e in log:
        run = run + 1 if e["iteration"] >= 0 and e["accepted"] else 0
        best = max(best, run)
    assert best >= 4 and any(e["iteration"] >= 0 and 0 < e["lam"] < 1e-3 for e in log)
    res, log = _run("cutoff_repeat")
    doubled = [e for e in log if e["iteration"] == -1 and e["cutoff_th"] > 20]
    assert log[0]["rs"][5] > 0.6 and doubled  # more than 60 % saturated under the first cutoff
    assert res["repeated_level"] == S.scene(*S.CASES["cutoff_repeat"][0]).coarsest
    assert sum(1 for e in log if e["lvl"] == res["repeated_level"] and e["iteration"] == -1 and e["cutoff_th"] == 20) == 2
    res, log = _run("abort_coarsest")
    sc = S.scene(*S.CASES["abort_coarsest"][0])
    assert (res["ok"], res["reason"], res["abort_level"]) == (0, 1, sc.coarsest)
    np.testing.assert_array_equal(res["ref_to_new"], S.CASES["abort_coarsest"][1])
    res, log = _run("abort_level0")
    assert (res["ok"], res["reason"], res["abort_level"]) == (0, 1, 0) and np.all(np.isfinite(res["last_residuals"][:3]))
    res, log = _run("affine_too_big")
    assert (res["ok"], res["reason"]) == (0, 2) and res["aff"][1] == 250.0
    res, log = _run("rel_affine_too_big")
    assert (res["ok"], res["reason"]) == (0, 3) and abs(res["aff"][0]) > 1.2  # |a| itself is not tested when mode A is 0
    res, log = _run("empty_level")
    assert res["ok"] == 1 and np.isnan(res["last_residuals"][2]) and np.all(np.isfinite(res["last_residuals"][[0, 1, 3, 4]]))
    e = [e for e in log if e["lvl"] == 2]
    assert e[0]["rs"][1] == 0 and np.isnan(e[0]["rs"][5]) and np.all(e[1]["inc"] == 0) and res["iterations"][2] == 1


@pytest.mark.parametrize("name,i,scale", S.CONVERGENCE)
def test_full_loop_converges_to_the_truth(built, name, i, scale):
    sc = S.scene(name, i)
    T0 = S.pose(i, scale)
    res, log = sc.track(T0, (S.REF_AB[0] + 0.05, S.REF_AB[1] + 2.0), S.NEVER)
    eye = np.eye(3, 4)
    d0, d1 = np.abs(T0 - eye).max(), np.abs(res["ref_to_new"] - eye).max()
    print(f"{name}: |T - I| {d0:.3g} -> {d1:.3g}, (a, b) -> {res['aff']}, iterations {res['iterations']}")
    assert res["ok"] == 1 and d1 < 0.01 * d0
    assert abs(res["aff"][0] - S.REF_AB[0]) < 1e-3 and abs(res["aff"][1] - S.REF_AB[1]) < 0.05


def test_lm_step_large_rotations(built):
    """SE3::exp's sine and cosine in the step are the library's own text (one for host and device),
    not libm's: steps of up to several radians, through every quadrant of the reduction, against the
    restatement on math.sin / math.cos.  The two may round a sine differently in the last bit (glibc is not
    correctly rounded everywhere), which R(q) carries as a few 2^-53: the bar is 1e-14, absolute on the
    rotation and relative on the translation, a hundred times that and 1e-3 of what a wrong quadrant or a
    lost term of the series would show."""
    rng = np.random.default_rng(11)
    params = dict(solve=R.SOLVE_REFERENCE)
    T = S.pose(3, 5.0)
    worst = 0.0
    for k in range(200):
        target = np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 1, 3) * rng.choice([0.01, 1.0, 4.0]), [0, 0]])
        b = -1.25 * target / np.array(R.SCALE)  # H = I and lambda = 0.25: inc = target / SCALE exactly, then scaled back
        rc, inc, To, abo = _lib_step(np.eye(8), b, 0.25, T, (0.0, 0.0), params)
        assert rc == 0
        _, pose_r, _ = R.lm_step(np.eye(8), b, 0.25, R.pose_from_matrix(T), (np.float32(0), np.float32(0)),
                                 dict(R.DEFAULTS, **params))
        Tr = R.pose_matrix(pose_r)
        worst = max(worst, np.abs(To[:, :3] - Tr[:, :3]).max(), np.abs(To[:, 3] - Tr[:, 3]).max() / np.abs(Tr[:, 3]).max())
    print(f"large rotations: worst distance {worst:.3g}")
    assert worst <= 1e-14
