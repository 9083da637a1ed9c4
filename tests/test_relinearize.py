"""ldso_ba_linearize_residuals and ldso_ba_update_residuals, the two entry points the C++ face
(ldso_amd/cpp/energy_functional.cpp) relies on, through BAContext.linearize_residuals /
update_residuals.

linearize_residuals runs k_linearize on scratch copies for ONE window of a batch (its item_base and
res_base, the planes' stride R_tot, a second geometry snapshot) and must leave the context as it
was; update_residuals scatters caller-order arrays through rs_orig.  Against the oracle everything
is bit-exact: a fresh OracleWindow of the same window with the context's current frameEnergyTH runs
resetOOB + linearizeAll(false) (state_NewState, state_NewEnergyWithOutlier, centerProjectedTo) and
then applyRes (state_energy = state_NewEnergy, which resetOOB left 0 where the residual came out
OOB; JpJdF where IN).  A fresh oracle's centerProjectedTo stays (0, 0, 0) where the centre
projection fails, so the expected center_ok is "any component non-zero".

What each part is there to break: win 0's res_base / item_base used for another window (the batch
queried at 0, 1, 2 and then 2, 0: scratch reused across windows of different size); the planes'
stride; outputs that are NULL; the scratch pass writing into the live states, records, snapshot or
thresholds (byte-identical reads around the call, and a following pass equal to a twin context's);
update_residuals scattering in device order instead of through rs_orig, or into another window."""
import numpy as np
import pytest

import oracle
import ragged
from ldso_amd import _lib as L
from ldso_amd import synth

_S = dict(width=160, height=120)
BATCH = [dict(cfg=dict(n_frames=3, n_points=80, seed=321, edge_frac=0.2, **_S), opts={}),
         dict(cfg=dict(n_frames=7, n_points=150, seed=322, motion="forward", edge_frac=0.2, **_S), opts=dict(untargeted=0)),
         dict(cfg=dict(n_frames=13, n_points=100, seed=323, plane_depth=30.0, **_S), opts=dict(rank=True))]
REGULAR = dict(n_frames=5, n_points=150, seed=324, motion="forward", edge_frac=0.2, **_S)
OUTPUTS = ("new_state", "new_energy", "new_energy_wo", "center", "center_ok", "jpjdf")


def batch_windows(s=None):
    out = []
    for i, c in enumerate(BATCH):
        w = synth.make_window(**c["cfg"])
        w.settings = s
        out.append(ragged.frontend_window(w, np.random.default_rng(15000 + i), **c["opts"]))
    return out


def regular_window(s=None):
    w = synth.make_window(**REGULAR)
    w.settings = s
    return w.refresh_frame_terms()


def expected_relinearisation(w, frame_energy_th):
    """The oracle's resetOOB + linearizeAll(false) + applyRes of window w under the thresholds given."""
    wo = ragged.clone(w)
    wo.frame_energy_th = np.ascontiguousarray(frame_energy_th, np.float32).copy()
    ow = oracle.OracleWindow(wo, threads=0)
    ow.reset_oob()
    ow.linearize_all(False)
    r = ow.residuals()
    o = dict(new_state=r["new_state"].copy(), new_energy_wo=r["new_energy_wo"].copy(), center=r["center"].copy())
    ow.apply_res()
    r = ow.residuals()
    o["new_energy"] = r["state_energy"].copy()
    o["jpjdf"] = np.where((o["new_state"] == L.RES_IN)[:, None], r["jpjdf"], np.float32(0))
    o["center_ok"] = np.any(o["center"] != 0, axis=1).astype(np.uint8)
    ow.close()
    return o


def pushed_state(w, rng):
    """Random reachable residual states for window w: (state, state_energy, flags)."""
    R = w.n_residuals
    u = rng.random(R)
    state = np.where(u < 0.15, L.RES_OOB, np.where(u < 0.3, L.RES_OUTLIER, L.RES_IN)).astype(np.int8)
    energy = rng.uniform(1.0, 400.0, R).astype(np.float32)
    flags = (np.where(rng.random(R) < 0.5, L.FLAG_NEW, 0) |
             np.where((rng.random(R) < 0.5) & (state == L.RES_IN), L.FLAG_ACTIVE, 0)).astype(np.uint8)
    return state, energy, flags


# ------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------
def test_null_context_is_refused(built):
    lib = L.lib()
    assert lib.ldso_ba_linearize_residuals(None, 0, None, None, None, None, None, None) < 0
    assert b"bad arguments" in lib.ldso_ba_last_error()
    z8, zf, zu = np.zeros(1, np.int8), np.zeros(1, np.float32), np.zeros(1, np.uint8)
    assert lib.ldso_ba_update_residuals(None, 0, L.ptr(z8, L.i8p), L.ptr(zf, L.f32p), L.ptr(zf, L.f32p),
                                        L.ptr(zu, L.u8p)) < 0
    assert b"bad arguments" in lib.ldso_ba_last_error()


def test_relinearize_cases_are_well_posed(built):
    """On the oracle alone: the windows are accepted, keep most residuals IN, hold residuals whose
    centre projection fails (center_ok == 0) and, under the pushed states of the update_residuals
    tests, residuals that go from not-OOB to OOB in one pass (the applyRes copy is observable)."""
    import ctypes as C

    ws = batch_windows() + [regular_window()]
    n_bad_center = 0
    for i, w in enumerate(ws):
        s = w.c_struct()
        assert L.lib().ldso_ba_validate_window(C.byref(s)) == 0
        w._keep = []
        e = expected_relinearisation(w, w.frame_energy_th)
        frac = np.mean(e["new_state"] == L.RES_IN)
        bad = int(np.sum(e["center_ok"] == 0))
        print(f"window {i}: R {w.n_residuals}, IN {frac:.0%}, center_ok == 0 on {bad}")
        assert frac >= 0.2 and np.isfinite(e["new_energy"]).all()
        n_bad_center += bad
    assert n_bad_center > 0
    w = ws[1]
    state, energy, flags = pushed_state(w, np.random.default_rng(16001))
    wp = ragged.clone(w)
    wp.res_state, wp.res_energy, wp.res_flags = state, energy, flags
    ow = oracle.OracleWindow(wp, threads=0)
    ow.iteration()
    went_oob = (state != L.RES_OOB) & (ow.residuals()["state"] == L.RES_OOB)
    print(f"pushed window: {int(went_oob.sum())} residuals go from not-OOB to OOB")
    assert went_oob.sum() >= 3
    ow.close()


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
def snapshot(ctx):
    """Everything readable of every window, as bytes."""
    out = []
    for i in range(len(ctx.windows)):
        for d in (ctx.residuals(i), ctx.points(i), ctx.system(i)):
            out += [(i, k, np.ascontiguousarray(v).tobytes()) for k, v in d.items()]
        out.append((i, "energy", ctx.energy(i).tobytes()))
        out.append((i, "frame_energy_th", ctx.frame_energy_th(i).tobytes()))
    return out


def assert_same_snapshot(a, b):
    assert len(a) == len(b)
    for (i, k, x), (_, _, y) in zip(a, b):
        assert x == y, (i, k)


def check_relinearisation(ctx, ws, win, alone=False):
    """ctx.linearize_residuals(win) bit-equal to the oracle's, nothing else of the context moved."""
    before = snapshot(ctx)
    got = ctx.linearize_residuals(win)
    assert_same_snapshot(before, snapshot(ctx))
    want = expected_relinearisation(ws[win], ctx.frame_energy_th(win))
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (win, k, int(np.sum(got[k] != want[k])))
    if alone:  # each output requested alone, the others NULL: the same bits
        for k in OUTPUTS:
            one = ctx.linearize_residuals(win, only=(k,))
            assert list(one) == [k] and one[k].tobytes() == got[k].tobytes(), k
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["regular", "ragged"])
def test_linearize_residuals_single_window(built, kind):
    """Before any pass and after two accumulating passes (moved thresholds, persisted OOB states), on
    a regular and a ragged window; each output also requested alone; a following pass equals that of
    a twin context that never made the call."""
    from ldso_amd import BAContext

    make = regular_window if kind == "regular" else (lambda: ragged.edge_window("N7_holes_rank"))
    w = make()
    ctx, twin = BAContext(0).load([ragged.clone(w)]), BAContext(0).load([ragged.clone(w)])
    got = check_relinearisation(ctx, [w], 0, alone=True)
    if kind == "regular":
        assert (got["center_ok"] == 0).any()  # forward motion, points near the border
    for c in (ctx, twin):
        c.linearize(fix=False, accumulate=True)
        c.linearize(fix=False, accumulate=True)
    th = ctx.frame_energy_th(0)
    assert not np.array_equal(th, w.frame_energy_th) and (ctx.residuals(0)["state"] == L.RES_OOB).any()
    check_relinearisation(ctx, [w], 0)
    for c in (ctx, twin):
        c.linearize(fix=False, accumulate=True)
    for a, b in ((ctx.system(0), twin.system(0)), (ctx.residuals(0), twin.residuals(0))):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    ctx.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,layout,aff", [(0, 1, (1e12, 1e8)), (8, 3, (-1.0, -1.0)), (64, 1, (-1.0, -1.0)),
                                              (64, 3, (1e12, 1e8)), (8, 1, (1e12, 1e8))])
def test_linearize_residuals_in_a_batch(built, chunk, layout, aff):
    """[N=3, N=7, N=13] in one context queried at win 0, 1, 2 and again at 2, 0 (scratch reused
    across windows of different size), before a pass and after two; chunk 8 / 64 / automatic, both
    image layouts, a and b fixed and the default.  (Fixed a, b zero JabF only, Residuals.cc:186-187;
    JpJdF[6:8] = JabJIdx Jpdd, Residuals.h:128, is formed from sums the modes do not touch, so it is
    compared like the rest, not expected to vanish.)"""
    from ldso_amd import BAContext

    s = L.OptSettings.default(affine_opt_mode_a=aff[0], affine_opt_mode_b=aff[1])
    ws = batch_windows(s)
    ctx, twin = BAContext(0), BAContext(0)
    for c in (ctx, twin):
        c.set_tuning(6, chunk)   # LDSO_BA_TUNE_TOP_CHUNK
        c.set_tuning(2, layout)  # LDSO_BA_TUNE_TILED_IMAGES
        c.set_settings(s).load([ragged.clone(w) for w in ws])
    with oracle.affine_opt_modes(*aff):
        for win in (0, 1, 2, 2, 0):
            check_relinearisation(ctx, ws, win)
        for c in (ctx, twin):
            c.linearize(fix=False, accumulate=True)
            c.linearize(fix=False, accumulate=True)
        for win in (1, 2, 0):
            check_relinearisation(ctx, ws, win)
    for c in (ctx, twin):
        c.linearize(fix=False, accumulate=True)
    for i in range(3):
        for a, b in ((ctx.system(i), twin.system(i)), (ctx.residuals(i), twin.residuals(i))):
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (i, k)
    ctx.close()
    twin.close()


@pytest.mark.gpu
def test_linearize_residuals_refusals(built):
    from ldso_amd import BAContext
    from ldso_amd import dist as ldist

    ws = batch_windows()
    ctx = BAContext(0).load([ragged.clone(w) for w in ws])
    for bad in (-1, 3):
        with pytest.raises(L.LdsoError, match="bad arguments") as ei:
            ctx.linearize_residuals(bad)
        assert ei.value.code == -1
        with pytest.raises(L.LdsoError, match="bad arguments") as ei:
            ctx.update_residuals(bad, *[np.zeros(1)] * 4)
        assert ei.value.code == -1
    ctx.linearize()
    some = np.flatnonzero(np.diff(ws[0].point_res_begin) > 0)[::3]
    marg = BAContext(0).load_marginalization(ctx, 0, ldist.subset_window(ws[0], some))
    with pytest.raises(L.LdsoError, match="marginalisation") as ei:
        marg.linearize_residuals(0)
    assert ei.value.code == -1
    marg.close()
    shard = BAContext(0).load([ragged.clone(ws[1])], 0, 2)
    with pytest.raises(L.LdsoError, match="sharded") as ei:
        shard.linearize_residuals(0)
    assert ei.value.code == -1
    shard.close()
    ctx.close()


@pytest.mark.gpu
def test_update_residuals_reaches_one_window_in_caller_order(built):
    """Random reachable states pushed into window 1 of the batch: residuals(1) returns exactly those
    in the caller's order (a ragged window: rs_orig is far from the identity), windows 0 and 2 keep
    every byte."""
    from ldso_amd import BAContext

    ws = batch_windows()
    ctx = BAContext(0).load([ragged.clone(w) for w in ws])
    ctx.linearize(fix=False, accumulate=True)
    before = snapshot(ctx)
    state, energy, flags = pushed_state(ws[1], np.random.default_rng(16001))
    ctx.update_residuals(1, state, energy, np.zeros_like(energy), flags)
    r = ctx.residuals(1)
    np.testing.assert_array_equal(r["state"], state)
    np.testing.assert_array_equal(r["state_energy"], energy)
    np.testing.assert_array_equal(r["flags"], flags)
    after = snapshot(ctx)
    for (i, k, x), (_, _, y) in zip(before, after):
        if i != 1:
            assert x == y, (i, k)
    ctx.close()


@pytest.mark.gpu
def test_update_residuals_then_a_pass_matches_the_oracle(built):
    """new_energy = 0 pushed with the states: the next pass equals the oracle's pass over a window that
    carries the pushed states (and the pushed state_NewEnergy: a window alone implies state_NewEnergy
    == state_energy), at compare_pass's full bar, for every window of the batch."""
    from ldso_amd import BAContext
    from test_gpu_parity import compare_pass

    ws = batch_windows()
    ctx = BAContext(0).load([ragged.clone(w) for w in ws])
    state, energy, flags = pushed_state(ws[1], np.random.default_rng(16001))
    ctx.update_residuals(1, state, energy, np.zeros_like(energy), flags)
    ws[1].res_state, ws[1].res_energy, ws[1].res_flags = state, energy, flags
    ctx.linearize(fix=False, accumulate=True)
    for i, w in enumerate(ws):
        ow = oracle.OracleWindow(ragged.clone(w), threads=0)
        if i == 1:
            ow.set_residuals(new_energy=np.zeros_like(energy))
        e_cpu, s_cpu = ow.iteration()
        compare_pass(ctx, ow, i, e_cpu, s_cpu)
        ow.close()
    ctx.close()


@pytest.mark.gpu
def test_update_residuals_new_energy_is_what_apply_res_copies(built):
    """A recognisable state_NewEnergy (1000 + k) pushed: after one pass every residual pushed not-OOB
    that came out OOB holds exactly that as state_energy (linearize returns before it writes
    state_NewEnergy, applyRes copies it), and every residual pushed OOB keeps the pushed state_energy."""
    from ldso_amd import BAContext

    ws = batch_windows()
    ctx = BAContext(0).load([ragged.clone(w) for w in ws])
    state, energy, flags = pushed_state(ws[1], np.random.default_rng(16001))
    new_energy = (1000 + np.arange(state.size)).astype(np.float32)
    ctx.update_residuals(1, state, energy, new_energy, flags)
    ctx.linearize(fix=False, accumulate=True)
    r = ctx.residuals(1)
    was_oob = state == L.RES_OOB
    went_oob = ~was_oob & (r["state"] == L.RES_OOB)
    assert went_oob.sum() >= 3 and was_oob.sum() >= 3
    np.testing.assert_array_equal(r["state_energy"][went_oob], new_energy[went_oob])
    np.testing.assert_array_equal(r["state_energy"][was_oob], energy[was_oob])
    assert (r["state"][was_oob] == L.RES_OOB).all()
    # and the whole pass against the oracle carrying the same four arrays
    from test_gpu_parity import compare_pass

    wp = ragged.clone(ws[1])
    wp.res_state, wp.res_energy, wp.res_flags = state, energy, flags
    ow = oracle.OracleWindow(wp, threads=0)
    ow.set_residuals(new_energy=new_energy)
    e_cpu, s_cpu = ow.iteration()
    compare_pass(ctx, ow, 1, e_cpu, s_cpu)
    ow.close()
    ctx.close()
