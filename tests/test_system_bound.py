"""tests/system_bound.py on the CPU: the oracle's own float-accumulated system sits within a few
units of rounding of the float64 rebuild, elementwise; defects that the per-block bar
(test_gpu_parity.BLOCK_TOL) lets pass are caught; the vectorised rebuild equals a plain loop."""
import numpy as np
import pytest

import oracle
import system_bound as sb
from ldso_amd import synth

SMALL = dict(width=160, height=120)
WINDOWS = {
    "N4P70": dict(n_frames=4, n_points=70, seed=3, **SMALL),
    "N7P300": dict(n_frames=7, n_points=300, seed=5, **SMALL),
    "kitti00_N5P300": dict(synth.KITTI00, n_frames=5, n_points=300, seed=13),
}


def oracle_pass(cfg, prior=False):
    w = synth.make_window(**cfg)
    if prior:  # an inverse-depth prior on every third point, its delta of either sign
        k = np.arange(w.n_points)
        w.point_data[:, 4] = np.where(k % 3 == 0, 50.0 + k, 0.0)
        w.point_data[:, 5] = np.where(k % 2 == 0, 0.01, -0.02)
    ow = oracle.OracleWindow(w, threads=0)
    _, O = ow.iteration()
    out = dict(w=ow.window, O=O, J=ow.jacobians(), res=ow.residuals(), hdi=ow.points()["HdiF"])
    ow.close()
    return out


@pytest.fixture(scope="module")
def n7(built):
    return oracle_pass(WINDOWS["N7P300"])


@pytest.mark.parametrize("name", list(WINDOWS) + ["N4P70-prior"])
def test_oracle_is_within_its_bound(built, name):
    """Tier 1 holds for the oracle's system, its four ratios are at most 8 (measured: at most 5.43)
    and an element no addend reaches is exactly 0; also with inverse-depth priors on the points
    (scAddPoint adds them to H_dd and, shifted to zero, to b_d)."""
    p = oracle_pass(WINDOWS[name.split("-")[0]], prior=name.endswith("-prior"))
    if name.endswith("-prior"):
        plain = oracle_pass(WINDOWS["N4P70"])
        assert not np.array_equal(plain["O"]["bsc"], p["O"]["bsc"]) and not np.array_equal(plain["hdi"], p["hdi"])
    D, B, cnt = sb.dense_bound(p["w"], p["J"], p["res"], p["hdi"])
    r = sb.ratios(p["O"], D, B)
    t1 = sb.tier1_violations(p["O"], D, B, cnt)
    print(name, "active residuals", int((p["res"]["flags"] & 1).sum()), {k: f"{r[k][0]:.2f}" for k in sb.KEYS})
    for k in sb.KEYS:
        assert t1[k][0] == 0, (k, t1[k])
        assert r[k][0] <= 8.0, (k, r[k])
        assert r[k][1] == 0.0, (k, r[k])
        assert np.count_nonzero(B[k]) > 0.5 * B[k].size  # the window reaches most of the system
    sym = {k: (np.triu(v) + np.triu(v, 1).T if v.ndim == 2 else v) for k, v in p["O"].items()}
    sb.assert_elementwise(sym, p["O"], D, B, cnt, name)


def _fails(G, O, D, B, cnt, what):
    with pytest.raises(AssertionError):
        sb.assert_elementwise(G, O, D, B, cnt, what)


def test_planted_defects(n7):
    """Five defects planted into the oracle's own system on N7 P300: each fails assert_elementwise,
    and the first two pass the per-block bar (measured 6.1e-5 and 2.6e-5 below BLOCK_TOL = 1e-4),
    which is why the elementwise bound exists."""
    from test_gpu_parity import BLOCK_TOL, block_errors

    w, O, J, res, hdi = (n7[k] for k in ("w", "O", "J", "res", "hdi"))
    N = w.n_frames
    D, B, cnt = sb.dense_bound(w, J, res, hdi)
    O = {k: (np.triu(v) + np.triu(v, 1).T if v.ndim == 2 else v) for k, v in O.items()}  # as the device returns one
    sb.assert_elementwise(O, O, D, B, cnt, "unplanted")

    # 1. a uniform low-order error: all of HA scaled by 1 + 2^-14
    G = dict(O, HA=O["HA"] * (1 + 2.0 ** -14))
    err = block_errors(G["HA"], O["HA"], N)
    print(f"HA (1 + 2^-14): block error {err:.2e}, ratio {sb.ratios(G, D, B)['HA'][0]:.3g}")
    assert 0 < err < BLOCK_TOL
    _fails(G, O, D, B, cnt, "scaled HA")

    # 2. the smallest nonzero element of frame block (0, 1) sign-flipped, with its mirror
    blk = np.abs(O["HA"][4:12, 12:20])
    i, j = np.unravel_index(np.argmin(np.where(blk > 0, blk, np.inf)), blk.shape)
    G = dict(O, HA=O["HA"].copy())
    G["HA"][4 + i, 12 + j] *= -1
    G["HA"][12 + j, 4 + i] *= -1
    err = block_errors(G["HA"], O["HA"], N)
    print(f"sign flip of HA[{4 + i}, {12 + j}]: block error {err:.2e}, ratio {sb.ratios(G, D, B)['HA'][0]:.3g}")
    assert 0 < err < BLOCK_TOL
    _fails(G, O, D, B, cnt, "sign flip")

    # 3. one active residual left out of the rebuild
    k = int(np.flatnonzero(res["flags"] & 1)[37])
    _fails(O, O, *sb.dense_bound(w, J, res, hdi, skip=[k]), "residual left out")

    # 4. one point's Schur term scaled by 1 + 2^-12
    p = int(np.flatnonzero(hdi > 0)[11])
    without = hdi.copy()
    without[p] = 0
    Dp = sb.dense_bound(w, J, res, without)[0]
    term = np.triu(D["Hsc"] - Dp["Hsc"])
    G = dict(O, Hsc=O["Hsc"] + 2.0 ** -12 * (term + np.triu(term, 1).T), bsc=O["bsc"] + 2.0 ** -12 * (D["bsc"] - Dp["bsc"]))
    assert 0 < block_errors(G["Hsc"], O["Hsc"], N)
    _fails(G, O, D, B, cnt, "scaled Schur term")

    # 5. the affine-b row and column of block (0, 1) zeroed
    G = dict(O, HA=O["HA"].copy())
    G["HA"][4 + 7, 12:20] = 0
    G["HA"][4:12, 12 + 7] = 0
    G["HA"][12:20, 4 + 7] = 0
    G["HA"][12 + 7, 4:12] = 0
    _fails(G, O, D, B, cnt, "zeroed affine-b")

    # a lower triangle that is no mirror of the upper one
    G = dict(O, HA=O["HA"].copy())
    G["HA"][20, 5] += 1.0
    _fails(G, O, D, B, cnt, "asymmetric")


def loop_bound(w, J, res):
    """test_oracle_kat.dense_system with the absolute sums and the addend counts beside it."""
    N, Dn = w.n_frames, w.dim
    B = dict(HA=np.zeros((Dn, Dn)), bA=np.zeros(Dn), Hsc=np.zeros((Dn, Dn)), bsc=np.zeros(Dn))
    cnt = dict(HA=np.zeros((Dn, Dn)), bA=np.zeros(Dn), Hsc=np.zeros((Dn, Dn)), bsc=np.zeros(Dn))
    adH, adT = np.abs(w.ad_host.reshape(-1, 8, 8)), np.abs(w.ad_target.reshape(-1, 8, 8))
    for p in range(w.n_points):
        hpd, c, hdd, bd, cb = np.zeros(Dn), np.zeros(Dn), 0.0, 0.0, 0
        for k in range(w.point_res_begin[p], w.point_res_begin[p + 1]):
            if not res["flags"][k] & 1:
                continue
            h, t = w.point_host[p], w.res_target[k]
            Js = sb.unpack_J(J[k])
            Jk = {n: np.abs(v) for n, v in Js.items()}
            for i in range(8):
                hdd += (Js["JIdx"][:, i] @ Js["Jpdd"]) ** 2  # the weight 1 / H_dd is the signed sum's
                g = Jk["JIdx"][:, i]
                jrel = np.concatenate([g @ Jk["Jpdxi"], [Jk["JabF"][0, i], Jk["JabF"][1, i]]])
                row = np.zeros(Dn)
                row[:4] = g @ Jk["Jpdc"]
                row[4 + 8 * h:12 + 8 * h] += adH[h + N * t] @ jrel
                row[4 + 8 * t:12 + 8 * t] += adT[h + N * t] @ jrel
                jd, r = g @ Jk["Jpdd"], Jk["resF"][i]
                z = (row > 0).astype(float)
                B["HA"] += np.outer(row, row)
                cnt["HA"] += np.outer(z, z)
                B["bA"] += row * r
                cnt["bA"] += z * (r > 0)
                hpd += row * jd
                c += z * (jd > 0)
                bd += jd * r
                cb += jd * r > 0
        if hdd > 0:
            z = (hpd > 0).astype(float)
            B["Hsc"] += np.outer(hpd, hpd) / hdd
            cnt["Hsc"] += np.outer(c, z) + np.outer(z, c)
            B["bsc"] += hpd * bd / hdd
            cnt["bsc"] += (c + cb * z) * (bd > 0)
    return B, cnt


def test_vectorised_rebuild_equals_the_loop(built):
    from test_oracle_kat import dense_system

    p = oracle_pass(WINDOWS["N4P70"])
    w, J, res = p["w"], p["J"].astype(np.float64), p["res"]
    D, B, cnt = sb.dense_bound(w, p["J"], res)
    pts = []
    Dl = dict(zip(sb.KEYS, dense_system(w, J, res, pts)))
    Bl, cl = loop_bound(w, J, res)
    for k in sb.KEYS:
        assert np.linalg.norm(D[k] - Dl[k]) <= 1e-13 * np.linalg.norm(Dl[k]), k
        assert np.linalg.norm(B[k] - Bl[k]) <= 1e-13 * np.linalg.norm(Bl[k]), k
        np.testing.assert_array_equal(cnt[k], cl[k], err_msg=k)
        assert np.all(np.abs(D[k]) <= B[k] * (1 + 1e-12))
        assert np.array_equal(B[k] > 0, cnt[k] > 0)
    hpd, hdd, bd = sb.point_terms(w, p["J"], res)
    for q, (a, b, c) in enumerate(pts):
        np.testing.assert_allclose(hpd[q], a, rtol=1e-12, atol=1e-12 * np.abs(a).max() if a.any() else 0)
        np.testing.assert_allclose([hdd[q], bd[q]], [b, c], rtol=1e-12)
    # with the per-point HdiF the Schur terms change only by HdiF's own float rounding (no prior here)
    Dh = sb.dense_bound(w, p["J"], res, p["hdi"])[0]
    assert np.array_equal(Dh["HA"], D["HA"]) and np.linalg.norm(Dh["Hsc"] - D["Hsc"]) <= 1e-5 * np.linalg.norm(D["Hsc"])


@pytest.mark.parametrize("mode", ["fixed", "fix_a"])
def test_fixed_affine_modes_zero_bA_rows_only(built, mode):
    """With setting_affineOptModeA / B < 0 linearize zeroes JabF after JabJIdx and Jab2 were summed from
    it: HA and Hsc keep their affine terms, bA's a / b rows are exactly 0.  The rebuild follows with
    jabf_lin(); from the zeroed JabF alone it would call HA's affine terms unreachable (B == 0)."""
    import test_settings as ts

    s = ts.settings(mode)
    a, b = ts.MODES[mode]
    with oracle.affine_opt_modes(a, b):
        ow = oracle.OracleWindow(ts.window(WINDOWS["N4P70"], s), threads=0)
        _, O = ow.iteration()
    J, lin, res, hdi = ow.jacobians(), ow.jabf_lin(), ow.residuals(), ow.points()["HdiF"]
    assert not np.array_equal(J[:, 46:62], lin)
    D, B, cnt = sb.dense_bound(ow.window, J, res, hdi, jab_lin=lin)
    r, t1 = sb.ratios(O, D, B), sb.tier1_violations(O, D, B, cnt)
    for k in sb.KEYS:
        assert t1[k][0] == 0 and r[k][0] <= 8.0 and r[k][1] == 0.0, (k, r[k], t1[k])
    rows = ts.ab_rows(ow.window.n_frames)
    zero = rows if mode == "fixed" else rows[0::2]
    assert not B["bA"][zero].any() and np.all(B["bA"][np.setdiff1d(np.arange(B["bA"].size), zero)] > 0)
    assert np.all(np.diag(B["HA"])[rows] > 0)
    Dz, Bz, _ = sb.dense_bound(ow.window, J, res, hdi)
    assert sb.ratios(O, Dz, Bz)["HA"][1] > 0
    ow.close()
