"""The sharded cases of tests/sharded.py are well posed, on the oracle alone (no GPU): the shard rule
cuts every case window into contiguous runs of the device order at every world size, each case has
the ranks it is named for (empty, without residuals, without a newest-frame residual, a cut inside
a host), and the ranks' oracle passes sum to the whole window's far inside the GPU's block
tolerance, with the gathered threshold equal to the whole window's.  These are conditions on the
inputs of test_sharded_parity.py, not bars on a kernel: a draw that misses one is replaced, never the
condition."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ragged
import sharded
from ldso_amd import _lib as L
from ldso_amd import dist as ldist

# The GPU's bar per 8x8 block (test_gpu_parity.BLOCK_TOL) must not be spent on the reassociation of
# the ranks' float64 partial sums alone: a tenth of it is the condition on the inputs.
SUM_TOL = 1e-5


@pytest.mark.parametrize("name", list(sharded.SHARD_CASES))
def test_shard_rule_on_case_windows(built, name):
    """ldso_ba_shard_points at worlds 1, 2, 3, 4, 7 and 16: every point exactly once; every non-empty
    run contiguous in the device order (host, then point_rank or the caller's order); the runs
    concatenated in rank order ARE the device order (what the sharded sumNID chain rests on); loads
    within two points' residuals of each other when the window has residuals, and within one point
    when it has none (equal point counts)."""
    for i, w in enumerate(sharded.case_windows(name)):
        s = w.c_struct()
        assert L.lib().ldso_ba_validate_window(C.byref(s)) == 0, L.lib().ldso_ba_last_error()
        w._keep = []
        order = sharded.device_order(w)
        pos = np.empty(w.n_points, np.int64)
        pos[order] = np.arange(w.n_points)
        nres = np.diff(w.point_res_begin)
        for world in sharded.WORLDS:
            parts = [ldist.shard_points(w, r, world) for r in range(world)]
            tag = (name, i, world)
            np.testing.assert_array_equal(np.sort(np.concatenate(parts)), np.arange(w.n_points), err_msg=str(tag))
            for p in parts:
                if len(p):
                    q = pos[p]
                    assert np.all(np.diff(q) == 1), (tag, "a run is not contiguous in the device order")
            np.testing.assert_array_equal(np.concatenate(parts), order, err_msg=str(tag))
            if w.n_residuals > 0:
                loads = [int(nres[p].sum()) for p in parts]
                assert max(loads) - min(loads) <= 2 * nres.max(), (tag, loads)
            else:
                assert max(map(len, parts)) - min(map(len, parts)) <= 1, (tag, [len(p) for p in parts])


@pytest.mark.parametrize("name", list(sharded.SHARD_CASES))
def test_case_has_what_it_is_named_for(built, name):
    ws = sharded.case_windows(name)
    props = sharded.check_case_properties(name, ws)
    for w, pr in zip(ws, props):
        print(name, {k: v for k, v in pr.items() if k != "hosts"})
    if isinstance(sharded.SHARD_CASES[name]["windows"], str):  # and still what ragged.py names it for
        case = ragged.EDGE_CASES[name]
        ragged.check_properties(ws[0], case["opts"], case["want"])


@pytest.mark.parametrize("name", list(sharded.SHARD_CASES))
def test_shard_sums_on_the_oracle(built, name):
    """The oracle on each rank's ldist.subset_window: {HA, bA, Hsc, bsc} summed in rank order within
    SUM_TOL per block of the whole window's pass, the energy to 1e-9, #IN equal, and
    ldist.frame_threshold over the ranks' newest-frame NewEnergyWithOutlier values bit-equal to the
    whole window's setNewFrameEnergyTH (1152 where nothing targets the newest frame)."""
    from test_gpu_parity import block_errors, vec_block_errors

    world = sharded.SHARD_CASES[name]["world"]
    worst = 0.0
    for i, w in enumerate(sharded.case_windows(name)):
        N = w.n_frames
        full = oracle.OracleWindow(ragged.clone(w), threads=0)
        e_full, s_full = full.iteration()
        total = {k: np.zeros_like(s_full[k]) for k in ("HA", "bA", "Hsc", "bsc")}
        e_sum, newest = np.zeros(3), []
        for r in range(world):
            sub = ldist.subset_window(ragged.clone(w), ldist.shard_points(w, r, world))
            ow = oracle.OracleWindow(sub, threads=0)
            e, s = ow.iteration()
            for k in total:
                total[k] += s[k]
            e_sum += e
            newest.append(ow.residuals()["new_energy_wo"][sub.res_target == N - 1])
            np.testing.assert_array_equal(s["HL"], s_full["HL"])  # every rank keeps the priors
            np.testing.assert_array_equal(s["bL"], s_full["bL"])
            ow.close()
        errs = {k: block_errors(total[k], s_full[k], N) for k in ("HA", "Hsc")}
        errs.update({k: vec_block_errors(total[k], s_full[k], N) for k in ("bA", "bsc")})
        print(f"{name}[{i}] world {world}: shard-sum block errors", {k: f"{v:.2e}" for k, v in errs.items()})
        worst = max(worst, max(errs.values()))
        assert max(errs.values()) < SUM_TOL, errs
        assert e_sum[2] == e_full[2]
        assert abs(e_sum[0] - e_full[0]) <= 1e-9 * abs(e_full[0])
        th = ldist.frame_threshold(np.concatenate(newest))
        assert th == full.frame_energy_th()[-1], (th, full.frame_energy_th())
        if name == "no_newest" or w.n_residuals == 0:
            assert sum(map(len, newest)) == 0 and th == sharded.DEFAULT_TH
        full.close()
    print(f"{name}: worst shard-sum block error {worst:.2e}")
