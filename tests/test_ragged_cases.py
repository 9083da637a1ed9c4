"""The ragged windows of tests/ragged.py are well posed, on the oracle alone (no GPU): the library's
validator accepts each, each really has the irregularities its case is named for, the reference
pass keeps enough residuals IN, and the stitched system and its solves are finite.  These are
conditions on the inputs of test_ragged_parity.py / test_relinearize.py, not bars on a kernel: a draw
that misses one is replaced, never the condition."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ragged
from ldso_amd import _lib as L

IN_FLOOR = 0.2  # test_optimize_lockstep's floor on #IN / R


def check_well_posed(w, opts, want, aff=(1e12, 1e8), tag=""):
    s = w.c_struct()
    assert L.lib().ldso_ba_validate_window(C.byref(s)) == 0, L.lib().ldso_ba_last_error()
    w._keep = []
    pr = ragged.check_properties(w, opts, want)
    N, R = w.n_frames, w.n_residuals
    with oracle.affine_opt_modes(*aff):
        ow = oracle.OracleWindow(ragged.clone(w), threads=0)
        e, sysm = ow.iteration()
        res = ow.residuals()
        n_in = int(np.sum(res["state"] == L.RES_IN))
        print(f"{tag}: N {N} P {w.n_points} R {R} IN after one pass {n_in} ({n_in / max(R, 1):.0%}), "
              f"{ {k: v for k, v in pr.items() if not k.endswith('counts')} }")
        assert n_in >= IN_FLOOR * R
        assert np.isfinite(e).all()
        for k, v in sysm.items():
            assert np.isfinite(v).all(), k
        ns = w.nullspaces()
        for it in (0, 2):
            assert np.isfinite(oracle.solve_system(N, it, 1e-5, sysm, nullspaces=ns)).all(), it
        if R == 0:  # nothing but the priors
            assert tuple(e) == (0.0, 0.0, 0.0) and not sysm["HA"].any() and not sysm["Hsc"].any()
        ow.close()


@pytest.mark.parametrize("name", list(ragged.EDGE_CASES))
def test_edge_windows_are_well_posed(built, name):
    case = ragged.EDGE_CASES[name]
    check_well_posed(ragged.edge_window(name), case["opts"], case["want"], tag=name)


def test_batch_windows_are_well_posed(built):
    for i, (w, c) in enumerate(zip(ragged.batch_windows(), ragged.BATCH)):
        want = {} if c["opts"].get("all_empty") else dict(zero_res_points=1, shuffled_points=5, stale_oob=1)
        check_well_posed(w, c["opts"], want, tag=f"batch[{i}]")


@pytest.mark.parametrize("case", range(ragged.N_FUZZ))
def test_fuzz_draws_are_well_posed(built, case):
    wins, opts, chunk, layout, aff = ragged.fuzz_draw(case)
    s = L.OptSettings.default(affine_opt_mode_a=aff[0], affine_opt_mode_b=aff[1])
    for i, (w, o) in enumerate(zip(ragged.fuzz_windows(case, s), opts)):
        check_well_posed(w, o, ragged.expected_properties(w, o), aff, tag=f"case {case}[{i}] {o}")


def test_transform_is_deterministic_and_keeps_the_regular_window(built):
    """The same rng seed gives the same window; every kept residual is one of the regular window's
    (same host, a target other than the host, no duplicate)."""
    a, b = ragged.edge_window("N7_holes_rank"), ragged.edge_window("N7_holes_rank")
    for k in ("point_host", "point_data", "point_res_begin", "res_target", "res_state", "res_energy", "res_flags",
              "point_rank"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for p in range(a.n_points):
        t = a.res_target[a.point_res_begin[p]:a.point_res_begin[p + 1]]
        assert len(set(t.tolist())) == len(t) and a.point_host[p] not in t
