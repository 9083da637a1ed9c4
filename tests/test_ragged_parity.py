"""GPU parity on ragged, mixed-state windows (tests/ragged.py): windows as LDSO's frontend leaves
them -- points with 0 to N-1 residuals in shuffled target order, residuals loaded OOB (with stale
energies) / OUTLIER / IN with mixed isNew and isActiveAndIsGoodNEW, no point on the newest frame, a
frame nobody targets -- against the oracle, at test_gpu_parity.compare_pass's bars unchanged (per
residual and per point bit-exact, the energy to 1e-12, the stitched 8x8 blocks within 1e-4, the
priors exact).  tests/test_ragged_cases.py shows on the CPU that every window used here is well posed.

What each part is there to break:
  * k_point_sc's record gather clamped with nres, the pt_tgt nibble decode, the zero fill of unfilled
    row slots and the sum in residual order (k_point_sc.h) -- points with 1 ... N-1 residuals in
    shuffled order, at N = 16 all 15 nibbles and target 15; hosts with 1, 17 and 65 points (one past
    a block of 16 / of 64);
  * k_linearize's target-bucket chunks and both stitches on uneven and empty (host, target) pairs,
    the geometry snapshot written by a pair's first chunk -- empty_newest, untargeted, N = 2;
  * the OOB early return giving back the loaded state_energy, and the records of residuals that
    are not active -- the second accumulating pass and the fix pass;
  * item_base / res_base after an empty range -- the batch with an R = 0 window in the middle;
  * k_resubstitute's per-point target list, zero-residual points (step 0 exactly);
  * point marginalisation and the device optimize loop on such parents."""
import numpy as np
import pytest

import oracle
import ragged
from ldso_amd import BAContext
from ldso_amd import _lib as L

pytestmark = pytest.mark.gpu


def two_passes_and_the_fix_pass(ctx, ws):
    """linearize(fix=False, accumulate=True) twice beside oracle.iteration() twice (the second pass
    sees the persisted OOB states and the inactive records), compare_pass after each; then
    reset_oob and the fix pass, rel_bs included, as test_fuzz_parity does.  The caller holds the
    oracle's affine modes.  Returns the oracle windows (after the fix pass)."""
    from test_gpu_parity import compare_pass

    ows = [oracle.OracleWindow(ragged.clone(w), threads=0) for w in ws]
    for _ in range(2):
        ctx.linearize(fix=False, accumulate=True)
        for i, ow in enumerate(ows):
            e_cpu, s_cpu = ow.iteration()
            compare_pass(ctx, ow, i, e_cpu, s_cpu)
    ctx.reset_oob()
    ctx.linearize(fix=True, accumulate=False)
    for i, ow in enumerate(ows):
        ow.reset_oob()
        e_cpu = ow.linearize_all(True)
        compare_pass(ctx, ow, i, e_cpu, None, check_system=False)
        np.testing.assert_array_equal(ctx.residuals(i)["rel_bs"], ow.residuals()["rel_bs"])
    return ows


# ---- a. deterministic edge windows ------------------------------------------------------------
@pytest.mark.parametrize("name", list(ragged.EDGE_CASES))
def test_edge_windows_match_oracle(built, name):
    w = ragged.edge_window(name)
    ctx = BAContext(0).load([ragged.clone(w)])
    for ow in two_passes_and_the_fix_pass(ctx, [w]):
        ow.close()
    ctx.close()


def test_batch_with_an_empty_window_in_the_middle(built):
    """[N=5 ragged, N=7 with 60 points and no residual, N=3 ragged] in one context: the windows
    after the empty range match the oracle, and the empty one gives energy (0, 0, 0), HA = Hsc = 0
    and HL, bL equal to its priors exactly."""
    ws = ragged.batch_windows()
    assert ws[1].n_points > 0 and ws[1].n_residuals == 0
    ctx = BAContext(0).load([ragged.clone(w) for w in ws])
    ows = two_passes_and_the_fix_pass(ctx, ws)
    ctx.linearize(fix=False, accumulate=True)
    e, s = ctx.energy(1), ctx.system(1)
    assert tuple(e) == (0.0, 0.0, 0.0)
    for k in ("HA", "Hsc", "bA", "bsc"):
        assert not s[k].any(), k
    w = ws[1]
    e_o, s_o = ows[1].iteration()
    hl = np.concatenate([w.c_prior, w.frame_prior.ravel()])
    np.testing.assert_array_equal(np.diag(s["HL"]), hl)
    assert not (s["HL"] - np.diag(np.diag(s["HL"]))).any()
    np.testing.assert_array_equal(s["HL"], s_o["HL"])
    np.testing.assert_array_equal(s["bL"], s_o["bL"])
    for ow in ows:
        ow.close()
    ctx.close()


# ---- b. randomised sweep ----------------------------------------------------------------------
@pytest.mark.parametrize("case", range(ragged.N_FUZZ))
def test_random_ragged_windows_match_oracle(built, case):
    wins, opts, chunk, layout, aff = ragged.fuzz_draw(case)
    print(f"case {case}: chunk {chunk}, layout {layout}, affine {aff}")
    for c, o in zip(wins, opts):
        print("  ", c, o)
    s = L.OptSettings.default(affine_opt_mode_a=aff[0], affine_opt_mode_b=aff[1])
    ws = ragged.fuzz_windows(case, s)
    ctx = BAContext(0)
    ctx.set_tuning(6, chunk)   # LDSO_BA_TUNE_TOP_CHUNK
    ctx.set_tuning(2, layout)  # LDSO_BA_TUNE_TILED_IMAGES
    ctx.set_settings(s).load([ragged.clone(w) for w in ws])
    with oracle.affine_opt_modes(*aff):
        for ow in two_passes_and_the_fix_pass(ctx, ws):
            ow.close()
    ctx.close()


# ---- c. solve and resubstitution ----------------------------------------------------------------
@pytest.mark.parametrize("name", ragged.SOLVE_CASES)
def test_device_solve_and_resubstitution_on_ragged_windows(built, name):
    from test_gpu_parity import sensitivity

    w = ragged.edge_window(name)
    N, ns = w.n_frames, w.nullspaces()
    ow = oracle.OracleWindow(ragged.clone(w), threads=0)
    e_cpu, s_cpu = ow.iteration()
    # exact mode: bit-identical to the host solver on the same stitched system, as ldso_ba.h promises
    c = BAContext(0)
    c.set_tuning(12, 1)  # LDSO_BA_TUNE_SOLVE_EXACT
    c.load([ragged.clone(w)])
    c.linearize()
    for it in (0, 2):
        xd = c.solve_device(it, 1e-5, [ns])[0]
        np.testing.assert_array_equal(xd, c.solve(0, it, 1e-5, ns))
        # and the device resubstitution equals the host-staged one from the same x, bit for bit
        np.testing.assert_array_equal(c.resubstitute_device(1e-5)[0], c.resubstitute(0, xd, 1e-5))
    c.close()
    # default mode against the oracle: test_single_pass_parity's envelope bar, its 1e-3 on the steps
    c = BAContext(0).load([ragged.clone(w)])
    c.linearize()
    empty = np.diff(w.point_res_begin) == 0
    assert empty.any() or name == "N3_one_each"
    for it in (0, 2):
        xd = c.solve_device(it, 1e-5, [ns])[0]
        xc = oracle.solve_system(N, it, 1e-5, s_cpu, nullspaces=ns)
        env = sensitivity(N, it, s_cpu, ns, xc)
        rel = np.linalg.norm(xd - xc) / np.linalg.norm(xc)
        print(f"{name} it={it}: |xd-xc|/|xc|={rel:.3e} envelope={env:.3e}")
        assert rel <= max(1e-6, 20 * env)
        stg = c.resubstitute_device(1e-5)[0]
        stc = ow.resubstitute(xd, 1e-5)
        assert np.linalg.norm(stg - stc) <= 1e-3 * np.linalg.norm(stc) + 1e-12
        assert np.linalg.norm(stc) > 0
        assert not stg[empty].any() and not stc[empty].any()  # zero-residual points: step 0 exactly
    c.close()
    ow.close()


# ---- d. point marginalisation on ragged parents -------------------------------------------------
@pytest.mark.parametrize("case", range(6))
def test_point_marginalisation_on_ragged_parents(built, case):
    """test_fuzz_parity's marginalisation check with a ragged parent: host 0's points and a random
    fraction of the rest, without the zero-residual points (flagPointsForRemoval drops those and
    never marginalises them)."""
    from ldso_amd import synth
    from test_fuzz_parity import check_point_marginalisation

    rng = np.random.default_rng(7100 + case)
    N = [2, 3, 5, 7, 8, 11][case]
    cfg = dict(n_frames=N, n_points=int(rng.integers(80, 300)), width=160, height=120,
               seed=int(rng.integers(1 << 30)), motion=str(rng.choice(["sideways", "forward"])),
               outlier_frac=float(rng.uniform(0.0, 0.2)))
    opts = dict(untargeted=0) if case == 3 else dict(rank=True) if case == 4 else {}
    frac, scale = float(rng.uniform(0.05, 0.5)), float(rng.choice([0.0, 1.0, 3.0]))
    print(f"case {case}: {cfg} {opts}, fraction {frac:.2f}, delta scale {scale}")
    w = ragged.frontend_window(synth.make_window(**cfg), np.random.default_rng(7200 + case), **opts)
    S = np.array(sorted(set(np.flatnonzero(w.point_host == 0)) |
                        set(np.flatnonzero(rng.random(w.n_points) < frac))), np.int64)
    S = S[np.diff(w.point_res_begin)[S] > 0]
    n_res = np.diff(w.point_res_begin)[S]
    assert len(S) >= 10 and (N == 2 or n_res.min() < n_res.max())
    check_point_marginalisation(ragged.clone(w), ragged.clone(w), S, scale)


# ---- f. the device optimize loop on ragged windows ------------------------------------------------
@pytest.mark.parametrize("n_frames,opts", [(3, {}), (7, dict(rank=True, empty_newest=True)), (11, dict(untargeted=0))],
                         ids=["N3", "N7_rank", "N11"])
def test_optimize_on_ragged_windows_matches_host_loop(built, n_frames, opts, monkeypatch):
    from ldso_amd import synth
    from test_fuzz_optimize import check_optimize_against_host_loop

    cfg = dict(n_frames=n_frames, n_points=250, width=160, height=120, seed=400 + n_frames)

    def make(s):
        w = synth.make_window(**cfg)
        w.settings = s
        return ragged.frontend_window(w, np.random.default_rng(14000 + n_frames), **opts)

    check_optimize_against_host_loop([make], [(cfg, opts)], (1e12, 1e8), 50 + n_frames, monkeypatch)
