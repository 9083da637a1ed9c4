"""Randomised optimize sweep: seeded random windows (2-11 keyframes, 100-700
points, the fuzz frame sizes, random pinhole models, forward or sideways motion, 0-20 % outliers,
all four affine-mode settings), one or two per batch, through ldso_ba_optimize's device loop against
the same loop driven from the host by the oracle (tests/test_optimize.py's host_optimize).

Bars, as test_optimize's: the initial pass bit-exact in #IN and 1e-12 in energy, later passes
within the north star's 1e-4 relative in energy and 0.2 % in #IN, the accumulated frame / point
steps within 5 % (norm) of the host loop's -- or, where larger, four times the spread of two host
loops whose stitched HA / Hsc and bA / bsc have every entry scaled by 1 + 1e-7 N(0, 1) before each
solve (about one float ulp: the size of the GPU's reassociated partial sums).  A window whose steps
stay 30-100x the convergence thresholds (most random draws here) passes such differences into x
along its near-gauge directions and its later passes follow them (test_optimize's note): one
two-keyframe draw differs from the host loop by 6.5e-5 at pass 1 and 1.3e-4 at pass 2, the
perturbed host loops from each other by 7.8e-5 and 2.6e-4.  The loop runs three iterations.
Iteration count and exit status are compared only when the canbreak ratios of the host loop stay
5 % away from the threshold at every iteration (the ratios and the decision are printed);
otherwise the float reassociation of x may flip it, and that draw checks the passes both loops
ran."""
import numpy as np
import pytest

import oracle
from ldso_amd import _lib as L
from ldso_amd import dist as ldist  # noqa: F401  (imports torch before the HIP library loads)
from ldso_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [(160, 120), (317, 203), (640, 480), (1242, 375)]
AFFINE = [(1e12, 1e8), (0.0, 0.0), (-1.0, -1.0), (-1.0, 5.0)]
N_ITS = 3


def draw(case):
    rng = np.random.default_rng(11000 + case)
    W, H = SIZES[rng.integers(len(SIZES))]
    cfgs = []
    for _ in range(int(rng.integers(1, 3))):
        N = int(rng.integers(2, 12))
        calib = None
        if rng.random() < 0.5:
            f = float(rng.uniform(0.4, 1.2)) * W
            calib = [f, f * float(rng.uniform(0.95, 1.05)), W / 2 + float(rng.uniform(-0.1, 0.1)) * W,
                     H / 2 + float(rng.uniform(-0.1, 0.1)) * H]
        cfgs.append(dict(n_frames=N, n_points=int(rng.integers(100, 700)), width=W, height=H,
                         seed=int(rng.integers(1 << 30)), outlier_frac=float(rng.uniform(0.0, 0.2)),
                         motion=str(rng.choice(["sideways", "forward"])), calib=calib,
                         plane_depth=max(25.0, 2.5 * (N - 1))))
    return cfgs, AFFINE[rng.integers(len(AFFINE))]


def perturbed_solve(rng, rel=1e-7):
    """oracle.solve_system with every entry of HA / Hsc and bA / bsc scaled by 1 + rel N(0, 1)
    (H kept symmetric); the priors HL / bL are exact on the device and stay untouched."""
    solve = oracle.solve_system

    def f(n_frames, it, lam, sysm, *a, **k):
        s2 = dict(sysm)
        for hk, bk in (("HA", "bA"), ("Hsc", "bsc")):
            H, b = np.array(sysm[hk]), np.array(sysm[bk])
            E = rel * H * rng.standard_normal(H.shape)
            s2[hk] = H + np.triu(E) + np.triu(E, 1).T
            s2[bk] = b * (1 + rel * rng.standard_normal(b.shape))
        return solve(n_frames, it, lam, s2, *a, **k)

    return f


def window(cfg, s):
    w = synth.make_window(**cfg)
    w.settings = s
    return w.refresh_frame_terms()


@pytest.mark.parametrize("case", range(10))
def test_random_optimize_matches_host_loop(built, case, monkeypatch):
    cfgs, aff = draw(case)
    print(f"case {case}: affine {aff}")
    check_optimize_against_host_loop([(lambda s, c=c: window(c, s)) for c in cfgs], cfgs, aff, case, monkeypatch)


def check_optimize_against_host_loop(factories, labels, aff, case, monkeypatch):
    """factories: one per window of the batch, each f(settings) -> a fresh copy of that window;
    labels: what to print for each; case: seeds the perturbed host loops."""
    from ldso_amd import BAContext
    from test_optimize import host_optimize

    s = L.OptSettings.default(affine_opt_mode_a=aff[0], affine_opt_mode_b=aff[1])
    ws = [f(s) for f in factories]
    nss = [w.nullspaces() for w in ws]
    ctx = BAContext(0).set_settings(s).load(ws)
    e_dev, fr_dev, c_dev, idep_dev, its_dev, st_dev = ctx.optimize(N_ITS, nullspaces=nss)
    ctx.close()
    off = 0
    with oracle.affine_opt_modes(*aff):
        for i, (make, cfg, ns) in enumerate(zip(factories, labels, nss)):
            n = ws[i].n_frames
            e_h, fr_h, c_h, idep_h, its_h, st_h, ratios = host_optimize(make(s), N_ITS, ns)
            spread_e, spread_fr, spread_id = np.zeros(len(e_h)), 0.0, 0.0
            with monkeypatch.context() as m:
                for k in range(2):
                    m.setattr(oracle, "solve_system", perturbed_solve(np.random.default_rng(100 * case + k)))
                    e_p, fr_p, _, idep_p, its_p, _, _ = host_optimize(make(s), N_ITS, ns)
                    if its_p == its_h:
                        spread_e = np.maximum(spread_e, np.abs(np.array(e_p)[:, 0] - np.array(e_h)[:, 0]))
                        spread_fr = max(spread_fr, float(np.linalg.norm(fr_p["state"] - fr_h["state"])))
                        spread_id = max(spread_id, float(np.linalg.norm(idep_p - idep_h)))
            edge = bool(len(ratios)) and bool(np.any(np.abs(ratios.max(axis=1) - 1.0) < 0.05))
            print(f"  {cfg}\n  host {its_h} its status {st_h}, device {its_dev[i]} status {st_dev[i]}, "
                  f"max ratios {ratios.max(axis=1) if len(ratios) else []}, near threshold {edge}")
            e = e_dev[:, i]
            assert e[0, 2] == e_h[0][2] and abs(e[0, 0] - e_h[0][0]) <= 1e-12 * abs(e_h[0][0])
            if not edge:
                assert (int(its_dev[i]), int(st_dev[i])) == (its_h, st_h)
            passes = min(len(e_h), int(its_dev[i]) + 1)
            for p in range(1, passes):
                print(f"  pass {p}: device {e[p]}, host {e_h[p]}, rel {abs(e[p, 0] / e_h[p][0] - 1):.3g}, "
                      f"perturbed-host spread {spread_e[p] / abs(e_h[p][0]):.3g}")
                assert abs(e[p, 0] - e_h[p][0]) <= max(1e-4 * abs(e_h[p][0]), 4 * spread_e[p]), p
                assert abs(e[p, 2] - e_h[p][2]) <= 2e-3 * e_h[p][2], p
            if (int(its_dev[i]), int(st_dev[i])) == (its_h, st_h) and st_h != L.OPT_LOST:
                w0 = make(s)
                fd = fr_dev["state"][off:off + n]
                assert np.linalg.norm(fd - fr_h["state"]) <= max(0.05 * np.linalg.norm(fr_h["state"] - w0.frames["state"]),
                                                                4 * spread_fr)
                assert np.linalg.norm(c_dev[i] - c_h) <= 0.05 * np.linalg.norm(c_h - w0.calib / 50.0) + 1e-12
                di = idep_h - w0.point_data[:, 2]
                assert np.linalg.norm(idep_dev[i][:len(di)] - idep_h) <= max(0.05 * np.linalg.norm(di), 4 * spread_id) + 1e-12
            off += n
