"""GPU parity of SHARDED contexts on the ragged, mixed-state windows of tests/ragged.py: `world`
contexts on device 0, each holding its run of the host-frame partition, with the exchange done by the
test through the library's documented calls (tests/sharded.py), beside the oracle on the WHOLE
window.  Bars are the project's own: per residual and per point bit for bit, the reduced system
within test_gpu_parity.BLOCK_TOL per 8x8 block and elementwise within tests/system_bound.py's rounding
bound of the whole window's float64 rebuild, the priors exact, #IN equal, the energy to 1e-9
(test_s11_split_over_four_contexts' bar), the threshold bit for bit on every rank.
tests/test_sharded_cases.py shows on the CPU that every case is well posed.

What each part is there to break:
  * pt_orig / rs_orig of a shard -- a rank's read or update landing in another rank's caller slots
    (union_* assert that every slot outside the rank's run keeps its zero bytes), with a point_rank
    permutation, zero-residual points and shuffled residual lists;
  * ranks with points but no residual into the newest frame, ranks without residuals, ranks without
    points: their pass, export (pads only), partial system (zeros), solve and resubstitution;
  * the three-call threshold route on a window nobody's residual targets the newest frame of;
  * more than one pass -- the exchanged threshold and the persisted OOB states feed the second pass
    and the fix pass; ldso_ba_update through pt_orig on every shard between GN iterations;
  * the automatic chunk of a shard (from r_est / shard_count) beside forced chunks of 8 and 64;
  * k_stitch's records path (16 keyframes) and the per-window slots of a batch on shards."""
import numpy as np
import pytest

import oracle
import ragged
import sharded
import system_bound
from ldso_amd import _lib as L

pytestmark = pytest.mark.gpu


def compare_sharded_pass(sh, ows, results, check_system=True, tag=""):
    """test_gpu_parity.compare_pass for the ranks of `sh` beside the whole-window oracles `ows` after
    a pass and its exchange; results[i] = (energy, system or None) of oracle i.  Returns the worst
    block error of the reduced systems (0 without check_system)."""
    from test_gpu_parity import BLOCK_TOL, block_errors, vec_block_errors

    worst = 0.0
    for i, ow in enumerate(ows):
        N = ow.window.n_frames
        e_cpu, s_cpu = results[i]
        rg, rc = sh.union_residuals(i), ow.residuals()
        for k in sharded.RESIDUAL_KEYS:
            np.testing.assert_array_equal(rg[k], rc[k], err_msg=f"{tag} window {i} {k}")
        act = (rc["flags"] & 1).astype(bool)
        np.testing.assert_array_equal(rg["jpjdf"][act], rc["jpjdf"][act], err_msg=f"{tag} window {i} jpjdf")
        e = sh.energy[i]
        assert e[2] == e_cpu[2], (tag, i, e, e_cpu)
        assert abs(e[0] - e_cpu[0]) <= 1e-9 * abs(e_cpu[0]), (tag, i, e, e_cpu)
        th = ow.frame_energy_th()
        for r, c in enumerate(sh.ctxs):
            np.testing.assert_array_equal(c.frame_energy_th(i), th, err_msg=f"{tag} window {i} rank {r}")
        if not check_system:
            continue
        pg, pc = sh.union_points(i), ow.points()
        for k in sharded.POINT_KEYS:
            np.testing.assert_array_equal(pg[k], pc[k], err_msg=f"{tag} window {i} {k}")
        systems = [c.system(i) for c in sh.ctxs]
        for r, s in enumerate(systems):
            errs = {k: block_errors(s[k], s_cpu[k], N) for k in ("HA", "Hsc")}
            errs.update({k: vec_block_errors(s[k], s_cpu[k], N) for k in ("bA", "bsc")})
            if r == 0:
                print(f"{tag} window {i}: reduced-system block errors", {k: f"{v:.2e}" for k, v in errs.items()})
            worst = max(worst, max(errs.values()))
            assert max(errs.values()) < BLOCK_TOL, (tag, i, r, errs)
            if r == 0:  # the other ranks hold the same reduced system, bit for bit (below)
                system_bound.check_system(s, ow, s_cpu, f"{tag} window {i}")
            np.testing.assert_array_equal(s["HL"], s_cpu["HL"])
            np.testing.assert_array_equal(s["bL"], s_cpu["bL"])
            for k in ("HA", "bA", "Hsc", "bsc"):  # one reduced system, on every rank
                np.testing.assert_array_equal(s[k], systems[0][k], err_msg=f"{tag} window {i} rank {r} {k}")
    return worst


def two_sharded_passes_and_the_fix_pass(sh, ws, tag):
    """test_ragged_parity.two_passes_and_the_fix_pass on shards: two accumulating passes, each with
    its exchange (the second sees the exchanged threshold and the persisted OOB states), then
    reset_oob and the fix pass, rel_bs included."""
    ows = [oracle.OracleWindow(ragged.clone(w), threads=0) for w in ws]
    worst = 0.0
    for p in range(2):
        sh.pass_and_exchange(fix=False, accumulate=True)
        worst = max(worst, compare_sharded_pass(sh, ows, [ow.iteration() for ow in ows], tag=f"{tag} pass {p}"))
    for c in sh.ctxs:
        c.reset_oob()
    sh.pass_and_exchange(fix=True, accumulate=False)
    results = []
    for ow in ows:
        ow.reset_oob()
        results.append((ow.linearize_all(True), None))
    compare_sharded_pass(sh, ows, results, check_system=False, tag=f"{tag} fix pass")
    for i, ow in enumerate(ows):
        np.testing.assert_array_equal(sh.union_residuals(i)["rel_bs"], ow.residuals()["rel_bs"])
        ow.close()
    print(f"{tag}: worst reduced-system block error {worst:.2e}")


# ---- a. two passes and the fix pass, per case ---------------------------------------------------
# the automatic chunk on every case; forced chunks of 8 and of 64 on two of them
PASS_PARAMS = [(name, 0) for name in sharded.SHARD_CASES] + [("N11P200", 8), ("host1_17", 64)]


@pytest.mark.parametrize("name,chunk", PASS_PARAMS, ids=[f"{n}-chunk{c}" if c else n for n, c in PASS_PARAMS])
def test_sharded_passes_match_oracle(built, name, chunk):
    case = sharded.SHARD_CASES[name]
    ws = sharded.case_windows(name)
    sharded.check_case_properties(name, ws)
    sh = sharded.Shards(ws, case["world"], tuning=((sharded.TUNE_TOP_CHUNK, chunk),) if chunk else ())
    try:
        assert sum(c.stats()["points"] for c in sh.ctxs) == sum(w.n_points for w in ws)
        assert sum(c.stats()["residuals"] for c in sh.ctxs) == sum(w.n_residuals for w in ws)
        two_sharded_passes_and_the_fix_pass(sh, ws, f"{name}/{case['world']}")
    finally:
        sh.close()


# ---- b. GN lock-step ------------------------------------------------------------------------------
LOCKSTEP_PARAMS = [(name, False) for name in sharded.SOLVE_CASES] + [("N7_holes_rank", True)]


@pytest.mark.parametrize("name,exact", LOCKSTEP_PARAMS, ids=[f"{n}-exact" if x else n for n, x in LOCKSTEP_PARAMS])
def test_sharded_gn_lockstep(built, name, exact):
    """Three GN iterations with the ranks and the whole-window oracle in lock-step: pass + exchange
    (the checks of a), the redundant device solve (bitwise the same x on every rank, inside the
    oracle's rounding envelope), the shard-local resubstitution (union of the ranks' steps against
    the oracle's from the same x), then the host steps as test_optimize.host_optimize does --
    doStepFromBackup with that x and those steps, the frame terms, the oracle's threshold -- and
    hands the SAME stepped window to the oracle and to every rank's update.  Both sides are fed
    identical x and steps, so every pass is again bit for bit per residual and per point."""
    from test_gpu_parity import sensitivity

    case = sharded.SHARD_CASES[name]
    world = case["world"]
    w0 = sharded.case_windows(name)[0]
    sharded.check_case_properties(name, [w0])
    N, ns = w0.n_frames, w0.nullspaces()
    empty = np.diff(w0.point_res_begin) == 0
    assert empty.any() or name == "N3_one_each"
    sh = sharded.Shards([w0], world, tuning=((sharded.TUNE_SOLVE_EXACT, 1),) if exact else ())
    ow = oracle.OracleWindow(ragged.clone(w0), threads=0)
    w = ragged.clone(w0)  # the host's window, stepped after every iteration
    cval = w.calib.astype(np.float64) * (1.0 / 50.0)
    czero = cval.copy()
    frames = np.ascontiguousarray(w.frames).copy()
    worst = 0.0
    try:
        for it in range(3):
            tag = f"{name}/{world} it {it}"
            sh.pass_and_exchange(fix=False, accumulate=True)
            e_cpu, s_cpu = ow.iteration()
            worst = max(worst, compare_sharded_pass(sh, [ow], [(e_cpu, s_cpu)], tag=tag))
            xs = [c.solve_device(it, 1e-5, [ns])[0] for c in sh.ctxs]
            for r in range(1, world):
                np.testing.assert_array_equal(xs[r], xs[0], err_msg=f"{tag}: x of rank {r}")
            x = xs[0]
            if exact:  # the exact mode is the host solver on the same reduced system, bit for bit (ldso_ba.h)
                np.testing.assert_array_equal(x, sh.ctxs[world - 1].solve(0, it, 1e-5, ns))
            xc = oracle.solve_system(N, it, 1e-5, s_cpu, nullspaces=ns)
            env = sensitivity(N, it, s_cpu, ns, xc)
            rel = np.linalg.norm(x - xc) / np.linalg.norm(xc)
            print(f"{tag}: |x-xc|/|xc|={rel:.3e} envelope={env:.3e}")
            assert rel <= max(1e-6, 20 * env)
            stg = sh.union_steps()[0]
            stc = ow.resubstitute(x, 1e-5)
            assert np.linalg.norm(stc) > 0
            assert np.linalg.norm(stg - stc) <= 1e-3 * np.linalg.norm(stc) + 1e-12
            assert not stg[empty].any() and not stc[empty].any()  # zero-residual points: step 0 exactly
            # the host step (FullSystem.cc:1826-1931, 1667-1675), every statement the oracle's
            frames, cval, sf, cd, idepth, _ = oracle.do_step_from_backup(
                frames, x, cval, czero, w.point_host, w.point_data[:, 2], stg)
            w.frames = frames
            w.calib = sf.copy()
            w.c_delta = cd.copy()
            w.point_data = w.point_data.copy()
            w.point_data[:, 2] = idepth
            w.point_data[:, 3] = idepth
            w.point_data[:, 5] = idepth - idepth
            t = oracle.frame_terms(w)
            for k in ("precalc", "ad_host", "ad_target", "c_prior", "frame_prior", "frame_delta", "frame_delta_prior"):
                setattr(w, k, t[k])
            w.frame_energy_th = ow.frame_energy_th().copy()  # the newest frame's carries into the next pass
            ow.update(w)
            for c in sh.ctxs:
                c.update(0, w)
        # the pass after the third step: the updates reached every shard
        sh.pass_and_exchange(fix=False, accumulate=True)
        worst = max(worst, compare_sharded_pass(sh, [ow], [ow.iteration()], tag=f"{name}/{world} after it 2"))
        print(f"{name}/{world}{' exact' if exact else ''}: worst reduced-system block error {worst:.2e}")
    finally:
        ow.close()
        sh.close()


# ---- c. empty ranks and no_newest -------------------------------------------------------------------
def test_empty_ranks_pass_export_solve_and_resubstitute(built):
    """N2P6 over 8 ranks: two ranks hold no point.  They load, pass, export, solve and resubstitute
    without error; their partial system is all zeros, their energy (0, 0, 0), their export pads
    only; on the reduced system their solve equals the other ranks' bit for bit."""
    case = sharded.SHARD_CASES["N2P6"]
    w = sharded.case_windows("N2P6")[0]
    pr = sharded.check_case_properties("N2P6", [w])[0]
    idle = [r for r, p in enumerate(pr["P"]) if p == 0]
    assert len(idle) >= 2
    ns = w.nullspaces()
    sh = sharded.Shards([w], case["world"])
    try:
        sh.pass_and_exchange()
        for r in idle:
            c = sh.ctxs[r]
            assert c.stats()["points"] == 0 and c.stats()["residuals"] == 0
            assert not sh.partials[r].any()
            assert tuple(c.energy(0)) == (0.0, 0.0, 0.0)
            assert np.all(sh.gathered[r] == -1.0)
        assert sh.stride == max(max(pr["newest"]), 1)
        ow = oracle.OracleWindow(ragged.clone(w), threads=0)
        compare_sharded_pass(sh, [ow], [ow.iteration()], tag="N2P6/8")
        for it in (0, 2):
            xs = [c.solve_device(it, 1e-5, [ns])[0] for c in sh.ctxs]
            assert np.isfinite(xs[0]).all() and xs[0].any()
            for r in range(1, sh.world):
                np.testing.assert_array_equal(xs[r], xs[0], err_msg=f"it {it} rank {r}")
            stg = sh.union_steps()[0]
            stc = ow.resubstitute(xs[0], 1e-5)
            assert np.linalg.norm(stg - stc) <= 1e-3 * np.linalg.norm(stc) + 1e-12
        w1 = ragged.clone(w)  # the same window with the exchanged threshold: update() on every rank,
        w1.frame_energy_th = ow.frame_energy_th().copy()  # the ones without points included
        for c in sh.ctxs:
            c.update(0, w1)
        sh.pass_and_exchange()
        compare_sharded_pass(sh, [ow], [ow.iteration()], tag="N2P6/8 pass 1")
        ow.close()
    finally:
        sh.close()


def test_no_newest_three_call_route(built):
    """No residual of the window targets the newest frame: ldso_ba_newest_stride gives 1 on every
    rank (never 0, which export_newest and frame_threshold_gathered refuse), every rank exports one
    pad, and the gathered selection leaves the reference's default 1152 on every rank.  The pass
    itself already selects 1152 from a rank's own (empty) segment, so the route is also run alone
    over a threshold that update() set to 777: the three calls are seen to write it."""
    import ctypes as C

    case = sharded.SHARD_CASES["no_newest"]
    w = sharded.case_windows("no_newest")[0]
    sharded.check_case_properties("no_newest", [w])
    N = w.n_frames
    sh = sharded.Shards([w], case["world"])
    try:
        for c in sh.ctxs:
            st = C.c_int64(-1)
            L.check(L.lib().ldso_ba_newest_stride(c._h, C.byref(st)))
            assert st.value == 1
        sh.pass_and_exchange()
        assert sh.stride == 1 and np.all(sh.gathered == -1.0)
        ow = oracle.OracleWindow(ragged.clone(w), threads=0)
        compare_sharded_pass(sh, [ow], [ow.iteration()], tag="no_newest/3")
        assert ow.frame_energy_th()[-1] == sharded.DEFAULT_TH
        w1 = ragged.clone(w)
        w1.frame_energy_th = ow.frame_energy_th().copy()
        w1.frame_energy_th[-1] = 777.0
        for c in sh.ctxs:
            c.update(0, w1)
            np.testing.assert_array_equal(c.frame_energy_th(0), w1.frame_energy_th)
        sh.exchange_threshold()
        assert sh.stride == 1 and np.all(sh.gathered == -1.0)
        for c in sh.ctxs:
            np.testing.assert_array_equal(c.frame_energy_th(0), ow.frame_energy_th())
            assert c.frame_energy_th(0)[N - 1] == sharded.DEFAULT_TH
        ow.close()
    finally:
        sh.close()


# ---- d. refusals that exist stay pinned on a ragged shard -------------------------------------------
def test_refusals_on_a_ragged_shard(built):
    """ldso_ba_linearize_residuals on a sharded window and ldso_ct_make_reference_ba from a sharded
    context are refused (both need every caller slot of the window), on the first and the last rank,
    before a pass and after one."""
    from ldso_amd import BAContext, synth
    from ldso_amd.tracker import CoarseTracker

    w = ragged.edge_window("N7_holes_rank")
    tr = CoarseTracker(w.width, w.height)
    tr.make_k(w.calib)
    tr.set_new_frame(synth.make_tracker_scene(w.width, w.height, seed=4)[0], 1.0)
    for rank, world in ((0, 3), (2, 3)):
        c = BAContext(0).load([ragged.clone(w)], shard_rank=rank, shard_count=world)
        for _ in range(2):
            with pytest.raises(L.LdsoError, match="sharded") as ei:
                c.linearize_residuals(0)
            assert ei.value.code == -1
            with pytest.raises(L.LdsoError, match="shard of its points") as ei:
                tr.make_reference_from(c, 0)
            assert ei.value.code == -1
            c.linearize()
        c.close()
    tr.close()
