"""ldso_ba_edit_window against a fresh load, bit for bit.

Two contexts load the same window (edit_cases.base_sel: N = 4, 70 points, buckets of exactly 16, 17
and 1 residuals, hosts of exactly 16 and 17 points, states mixed by ragged.frontend_window) by frame
id and run a pass.  Context A is edited; the `after` it is handed holds NaN / OUTLIER / all flag bits
at every carried entry, so anything read from it there shows.  Context B's residuals and point
records are read back, after' is built on the host and loaded fresh.  Both then run a pass and
ldso_ba_iterate, and every result -- energy, the six blocks of the system, every per-residual and
per-point output, the frame thresholds, x and the point steps -- is compared as bytes."""
import numpy as np
import pytest

import edit_cases as ec
from ldso_amd import BAContext
from ldso_amd import _lib as L

pytestmark = pytest.mark.gpu
ITEM_ORDER = 10  # LDSO_BA_TUNE_ITEM_ORDER


def make_ctx(pool, tuning=()):
    c = BAContext(0)
    for k, v in tuning:
        c.set_tuning(k, v)
    c.frames_reserve(pool.n_frames, pool.width, pool.height)
    for f in range(pool.n_frames):
        c.frame_put(ec.FRAME_ID0 + f, pool.dI[f])
    return c


def same(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def compare(A, B, what):
    same(A.energy(0), B.energy(0), f"{what}: energy")
    sa, sb = A.system(0), B.system(0)
    for k in sa:
        same(sa[k], sb[k], f"{what}: {k}")
    ra, rb = A.residuals(0), B.residuals(0)
    for k in ra:
        same(ra[k], rb[k], f"{what}: residual {k}")
    pa, pb = A.points(0), B.points(0)
    for k in pa:
        same(pa[k], pb[k], f"{what}: point {k}")
    same(A.point_data(0), B.point_data(0), f"{what}: point records")
    same(A.frame_energy_th(0), B.frame_energy_th(0), f"{what}: frame thresholds")


def pass_and_iterate(A, B, what):
    for c in (A, B):
        c.linearize(fix=False, accumulate=True)
    compare(A, B, f"{what}, pass")
    out = [c.iterate(0, 1e-5) for c in (A, B)]
    for (ea, xa, sa), (eb, xb, sb) in [out]:
        same(ea, eb, f"{what}: iterate energy")
        same(xa[0], xb[0], f"{what}: x")
        same(sa[0], sb[0], f"{what}: point steps")
    compare(A, B, f"{what}, iterate")


def read_back(B):
    r = B.residuals(0)
    return r["state"], r["state_energy"], r["flags"], B.point_data(0)


def loaded_pair(pool, sel, tuning=(), before_edit=None):
    """Two contexts that loaded `sel`, ran a pass and then before_edit(ctx, window)."""
    ctxs = []
    for _ in range(2):
        c = make_ctx(pool, tuning)
        w = ec.window_of(pool, sel)
        c.load(w, frame_ids=sel.frame_ids())
        c.linearize(fix=False, accumulate=True)
        if before_edit:
            before_edit(c, w)
        ctxs.append(c)
    return ctxs


def edit_and_reload(pool, A, B, sel, after_sel, new_energy=None):
    """A is edited into after_sel; B reloads after' built from its own read-back.  new_energy: the
    loaded window's state_NewEnergy where the test set it apart (caller order), carried by A on the
    device and restated on B with ldso_ba_update_residuals."""
    after, srcs = ec.window_of(pool, after_sel, sel)
    A.edit(after, after_sel.frame_ids(), *srcs)
    st, en, fl, pd = read_back(B)
    full = ec.filled(after, srcs, st, en, fl, pd)
    B.load(full, frame_ids=after_sel.frame_ids())
    if new_energy is not None:
        ne = full.res_energy.copy()
        cr = srcs[2] >= 0
        ne[cr] = new_energy[srcs[2][cr]]
        B.update_residuals(0, full.res_state, full.res_energy, ne, full.res_flags)


def run(name_or_edit, tuning=(), before_edit=None, new_energy=None):
    pool = ec.make_pool()
    sel = ec.base_sel(pool)
    A, B = loaded_pair(pool, sel, tuning, before_edit)
    edit = ec.EDITS[name_or_edit] if isinstance(name_or_edit, str) else name_or_edit
    ne = new_energy(B) if new_energy else None
    edit_and_reload(pool, A, B, sel, edit(pool, sel), ne)
    pass_and_iterate(A, B, str(name_or_edit))
    A.close()
    B.close()


@pytest.mark.parametrize("name", list(ec.EDITS))
def test_edit_equals_fresh_load(built, name):
    """(a) - (g)"""
    run(name)


def test_edit_host_major_item_order(built):
    run("e_cycle", tuning=((ITEM_ORDER, 1),))


def test_edit_after_optimize(built):
    """(h) the carried inverse depths are the ones the device loop stepped, which no host array holds."""
    stepped = []

    def optimize(c, w):
        before = c.point_data(0)
        c.optimize(2, nullspaces=[w.nullspaces()])
        stepped.append(not np.array_equal(before[:, 2], c.point_data(0)[:, 2]))

    run("e_cycle", before_edit=optimize)
    assert all(stepped)


def test_edit_carries_new_energy(built):
    """(i) state_NewEnergy set apart from state_energy on every OOB residual (and every third other
    one): the edit carries it; after a resetOOB-free pass an IN residual that projects out of bounds
    takes it back as its state_energy."""
    def set_apart(c, w):
        r = c.residuals(0)
        ne = r["state_energy"].copy()
        assert np.any(r["state"] == L.RES_OOB)
        ne[(r["state"] == L.RES_OOB) | (np.arange(ne.size) % 3 == 0)] += np.float32(7.0)
        c.update_residuals(0, r["state"], r["state_energy"], ne, r["flags"])
        c.new_energy_set = ne

    run("a_drop", before_edit=set_apart, new_energy=lambda B: B.new_energy_set)


def test_two_edits_in_a_row(built):
    """(j) two edits against one fresh load of the final window."""
    pool = ec.make_pool()
    s0 = ec.base_sel(pool)
    s1 = ec.edit_drop(pool, s0)
    s2 = ec.edit_insert_points(pool, s1)
    A, B = loaded_pair(pool, s0)
    w1, src1 = ec.window_of(pool, s1, s0)
    A.edit(w1, s1.frame_ids(), *src1)
    w2, src2 = ec.window_of(pool, s2, s1)
    A.edit(w2, s2.frame_ids(), *src2)
    # s2's carried entries seen from s0
    w2b, src_b = ec.window_of(pool, s2, s0)
    st, en, fl, pd = read_back(B)
    B.load(ec.filled(w2b, src_b, st, en, fl, pd), frame_ids=s2.frame_ids())
    pass_and_iterate(A, B, "two edits")
    A.close()
    B.close()


@pytest.mark.parametrize("name", list(ec.DEGENERATE))
def test_edit_to_a_window_without_residuals_and_back(built, name):
    """(l), (m) a zero through every part of the edit and of the load: counts of 0, uploads of 0 bytes,
    fills of 0 words, then growth from the one-element minimum.  The base window is edited to one
    with no residuals (and, in (l), no points) and a pass runs -- compared after the pass only, since
    ldso_ba_iterate has nothing to solve for there; then it is edited back to the base selection,
    where every residual (in (l) every point too) is new.  B follows by reloads."""
    pool = ec.make_pool()
    s0 = ec.base_sel(pool)
    s1 = ec.DEGENERATE[name](pool, s0)
    assert sum(len(items) for _, items in s1.pts) == 0 and (len(s1.pts) == 0) == (name == "l_no_points")
    A, B = loaded_pair(pool, s0)
    edit_and_reload(pool, A, B, s0, s1)
    for c in (A, B):
        c.linearize(fix=False, accumulate=True)
    compare(A, B, f"{name}, pass")
    edit_and_reload(pool, A, B, s1, s0)
    pass_and_iterate(A, B, f"{name} and back")
    A.close()
    B.close()


def test_keyframe_cycle_moves_no_image_and_stops_allocating(built):
    """(k) N = 7 -> 6 -> 7 at an S7 window's point count, twice.  The first cycle drops the oldest frame
    and appends a new one (image positions shift: device-to-device copies only); the second drops the
    newest and appends it again, so its windows have the structure of the first cycle's and every
    buffer's capacity has been seen.  No image byte crosses from the host in either; the second
    allocates nothing.  The result is the fresh load's."""
    pool = ec.make_pool(n_frames=8, n_points=2300, seed=43)
    s7 = ec.full_sel(pool, range(7))
    s6 = ec.edit_remove_frame(pool, s7, 0)
    s7b = ec.edit_append(pool, s6, 7)
    A, B = loaded_pair(pool, s7)
    t0 = A.transfer_stats()
    steps = [(s7, s6), (s6, s7b), (s7b, s6), (s6, s7b)]
    stats = []
    for a, b in steps:
        w, src = ec.window_of(pool, b, a)
        A.edit(w, b.frame_ids(), *src)
        A.linearize(fix=False, accumulate=True)
        stats.append(A.transfer_stats())
    assert stats[-1]["h2d_bytes"] == t0["h2d_bytes"]
    assert stats[1]["d2d_bytes"] > t0["d2d_bytes"]
    assert stats[3]["allocs"] == stats[1]["allocs"]
    # B: one fresh load of the final window, with what it would hold after the same passes -- the
    # passes change the carried state, so B follows A's sequence by reloading at every step
    for a, b in steps:
        w, src = ec.window_of(pool, b, a)
        st, en, fl, pd = read_back(B)
        B.load(ec.filled(w, src, st, en, fl, pd), frame_ids=b.frame_ids())
        B.linearize(fix=False, accumulate=True)
    compare(A, B, "cycle")
    A.close()
    B.close()


def test_refused_edit_leaves_the_context_alone(built):
    pool = ec.make_pool()
    sel = ec.base_sel(pool)
    A, B = loaded_pair(pool, sel)
    after, srcs = ec.window_of(pool, ec.edit_drop(pool, sel), sel)
    bad = [s.copy() for s in srcs]
    bad[2][1] = bad[2][0]
    with pytest.raises(L.LdsoError, match="twice"):
        A.edit(after, sel.frame_ids(), *bad)
    ids = sel.frame_ids()
    ids[1] = 9999
    with pytest.raises(L.LdsoError, match="not resident") as ei:
        A.edit(after, ids, *srcs)
    assert ei.value.code == L.ERR_FRAME_STORE
    assert A.windows[0].n_residuals == B.windows[0].n_residuals
    pass_and_iterate(A, B, "refused")
    A.close()
    B.close()


def test_contexts_that_cannot_be_edited(built):
    pool = ec.make_pool()
    sel = ec.base_sel(pool)
    after, srcs = ec.window_of(pool, ec.edit_identity(pool, sel), sel)
    ids = sel.frame_ids()
    c = make_ctx(pool)
    c.load(ec.window_of(pool, sel))  # images from the host
    with pytest.raises(L.LdsoError, match="ldso_ba_load_frames"):
        c.edit(after, ids, *srcs)
    c.load(ec.window_of(pool, sel), 0, 2, frame_ids=ids)
    with pytest.raises(L.LdsoError, match="sharded"):
        c.edit(after, ids, *srcs)
    c.load([ec.window_of(pool, sel), ec.window_of(pool, sel)], frame_ids=np.concatenate([ids, ids]))
    with pytest.raises(L.LdsoError, match="one window"):
        c.edit(after, ids, *srcs)
    c.load(ec.window_of(pool, sel), frame_ids=ids)
    m = BAContext(0)
    m.load_marginalization(c, 0, ec.window_of(pool, sel))
    with pytest.raises(L.LdsoError, match="marginalisation"):
        m.edit(after, ids, *srcs)
    m.close()
    c.close()
    c = make_ctx(pool, ((ITEM_ORDER, 2),))
    c.load(ec.window_of(pool, sel), frame_ids=ids)
    with pytest.raises(L.LdsoError, match="ITEM_ORDER 2"):
        c.edit(after, ids, *srcs)
    c.close()
