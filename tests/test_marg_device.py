"""ldso_ba_load_marginalization_device against ldso_ba_load_marginalization fed from read-backs, exactly.

The parent loads a ragged window (flag_cases / edit_cases' pool, 160 x 120) and runs the fix pass.
The host-window side reads the parent back (ldso_ba_get_point_data, ldso_ba_get_residuals), cuts the
selected points and residuals out on the host and loads them with ldso_ba_load_marginalization; the
device side hands the same selection to ldso_ba_load_marginalization_device.  Both then run
ldso_ba_marginalize_points.  The gathered context runs the same kernels on the same layout and the
same values, so H, b, every per-residual and per-point output and the point records are equal bit
for bit."""
import numpy as np
import pytest

import edit_cases as ec
import flag_cases as fc
import ragged
import test_marginalization as tm
from ldso_amd import BAContext
from ldso_amd import _lib as L
from ldso_amd.window import Window

pytestmark = pytest.mark.gpu


def make_parent(name="pool5", optimize=False):
    w = ragged.clone(fc.window(name))
    c = BAContext(0).load(w)
    if optimize:
        before = c.point_data(0)[:, 2].copy()
        c.optimize(2, nullspaces=[w.nullspaces()])
        assert not np.array_equal(before, c.point_data(0)[:, 2])
    c.linearize(fix=True, accumulate=True)
    return c, w


def sub_window(parent, w, pts, live):
    """The selection cut out of the parent's read-backs on the host."""
    r, pd = parent.residuals(0), parent.point_data(0)
    ks, begin = [], [0]
    for p in pts:
        ks += [k for k in range(int(w.point_res_begin[p]), int(w.point_res_begin[p + 1])) if live is None or live[k]]
        begin.append(len(ks))
    ks = np.array(ks, np.int64)
    pts = np.asarray(pts, np.int64)
    s = Window(n_frames=w.n_frames, width=w.width, height=w.height, calib=w.calib.copy(), frames=w.frames, dI=None,
               frame_energy_th=w.frame_energy_th.copy(), point_host=w.point_host[pts].astype(np.int32),
               point_data=pd[pts].reshape(-1, L.POINT_STRIDE).copy(), point_res_begin=np.array(begin, np.int32),
               res_target=w.res_target[ks].astype(np.int32), res_state=r["state"][ks].copy(),
               res_energy=r["state_energy"][ks].copy(), res_flags=r["flags"][ks].copy(), settings=w.settings)
    for k in ("precalc", "ad_host", "ad_target", "c_prior", "c_delta", "frame_prior", "frame_delta", "frame_delta_prior"):
        setattr(s, k, getattr(w, k))
    return s


def results(m, adh):
    H, b = m.marginalize_points(adh)
    return dict(H=H, b=b, point_data=m.point_data(0), **{f"res_{k}": v for k, v in m.residuals(0).items()},
                **{f"pt_{k}": v for k, v in m.points(0).items()})


def assert_same(dev, host, what):
    assert set(dev) == set(host)
    for k in host:
        d, h = np.ascontiguousarray(dev[k]), np.ascontiguousarray(host[k])
        assert d.shape == h.shape and d.dtype == h.dtype and d.tobytes() == h.tobytes(), f"{what}: {k}"


def both(parent, w, pts, live, what, marg=None):
    """marg: a context to load the device side into (None: a new one).  Returns it."""
    adh = tm.ad_ht_delta(w)
    mh = BAContext(0).load_marginalization(parent, 0, sub_window(parent, w, pts, live))
    host = results(mh, adh)
    mh.close()
    md = (marg or BAContext(0)).load_marginalization_device(parent, 0, w, pts, live)
    dev = results(md, adh)
    assert_same(dev, host, what)
    return md, dev


def edge_selection(w):
    """Buckets 0 -> 1 and 1 -> 0 of exactly 16 and 17 residuals (k_linearize's chunk), hosts 0 and 1 of
    exactly 16 and 17 points (k_point_sc's block), some of host 2's; the hosts interleaved."""
    has = lambda p, t: t in w.res_target[w.point_res_begin[p]:w.point_res_begin[p + 1]]
    h0 = [p for p in range(w.n_points) if w.point_host[p] == 0 and has(p, 1)][:16]
    h1 = [p for p in range(w.n_points) if w.point_host[p] == 1 and has(p, 0)][:17]
    h2 = [p for p in range(w.n_points) if w.point_host[p] == 2][::3]
    pts = sorted(h0 + h1 + h2)
    n01 = sum(1 for p in h0 for k in range(w.point_res_begin[p], w.point_res_begin[p + 1]) if w.res_target[k] == 1)
    n10 = sum(1 for p in h1 for k in range(w.point_res_begin[p], w.point_res_begin[p + 1]) if w.res_target[k] == 0)
    assert (len(h0), len(h1), n01, n10) == (16, 17, 16, 17)
    return np.array(pts, np.int32)


def test_bucket_and_block_edges(built):
    parent, w = make_parent()
    pts = edge_selection(w)
    md, dev = both(parent, w, pts, None, "edges")
    assert np.abs(dev["H"]).max() > 0 and np.any(dev["res_flags"] & L.FLAG_ACTIVE)
    # the marginalisation window's caller order is the list's order
    md2, dev2 = both(parent, w, pts[::-1].copy(), None, "edges reversed")
    assert np.array_equal(dev2["point_data"], dev["point_data"][::-1])
    for c in (md, md2, parent):
        c.close()


def test_res_live_removes_residuals(built):
    """What the keyframe close hands over: the residuals the fix pass left active, of every point that
    keeps one -- among them points with a single live residual."""
    parent, w = make_parent()
    live = (parent.residuals(0)["flags"] & L.FLAG_ACTIVE).astype(np.uint8)
    n_live = np.add.reduceat(np.r_[live, 0], w.point_res_begin[:-1]) * (np.diff(w.point_res_begin) > 0)
    assert 0 < live.sum() < live.size and np.any(n_live == 1)
    pts = np.flatnonzero(n_live > 0).astype(np.int32)
    md, dev = both(parent, w, pts, live, "res_live")
    assert dev["res_state"].size == int(live[np.concatenate([np.arange(w.point_res_begin[p], w.point_res_begin[p + 1])
                                                             for p in pts])].sum())
    # points that keep no residual at all ride along
    md2, _ = both(parent, w, np.arange(w.n_points, dtype=np.int32), live, "res_live, all points")
    for c in (md, md2, parent):
        c.close()


def test_records_stepped_by_optimize(built):
    parent, w = make_parent(optimize=True)
    md, dev = both(parent, w, edge_selection(w), None, "after optimize")
    # the records are the device's, not the loaded ones
    assert not np.array_equal(dev["point_data"][:, 2], w.point_data[edge_selection(w), 2])
    md.close()
    parent.close()


def test_no_points(built):
    parent, w = make_parent("base4")
    md, dev = both(parent, w, np.zeros(0, np.int32), None, "no points")
    assert not dev["H"].any() and not dev["b"].any() and dev["res_state"].size == 0
    md.close()
    parent.close()


def test_second_load_into_the_same_context(built):
    parent, w = make_parent()
    pts = edge_selection(w)
    md, _ = both(parent, w, pts, None, "first load")
    other = np.setdiff1d(np.arange(w.n_points, dtype=np.int32), pts)[::2].copy()
    live = (np.arange(w.n_residuals) % 4 != 1).astype(np.uint8)
    both(parent, w, other, live, "second load", marg=md)
    both(parent, w, np.zeros(0, np.int32), None, "third load, empty", marg=md)
    both(parent, w, pts, None, "fourth load", marg=md)
    # the parent was only read: a twin that never lent its arrays runs the same pass
    twin, _ = make_parent()
    for c in (parent, twin):
        c.linearize(fix=False, accumulate=True)
    import test_edit_parity as tep
    tep.compare(parent, twin, "parent after the loads")
    for c in (md, parent, twin):
        c.close()


def test_refusals(built):
    parent, w = make_parent("base4")
    m = BAContext(0)
    with pytest.raises(L.LdsoError, match="not a point of the parent"):
        m.load_marginalization_device(parent, 0, w, [0, w.n_points])
    with pytest.raises(L.LdsoError, match="twice"):
        m.load_marginalization_device(parent, 0, w, [3, 4, 3])
    other = ec.window_of(ec.make_pool(), ec.edit_remove_frame(ec.make_pool(), ec.base_sel(ec.make_pool()), 0))
    with pytest.raises(L.LdsoError, match="parent"):
        m.load_marginalization_device(parent, 0, other, [0])
    m.set_tuning(10, 2)  # LDSO_BA_TUNE_ITEM_ORDER
    with pytest.raises(L.LdsoError, match="ITEM_ORDER 2"):
        m.load_marginalization_device(parent, 0, w, [0, 1])
    m.close()
    sharded = BAContext(0).load(ragged.clone(w), 0, 2)
    m = BAContext(0)
    with pytest.raises(L.LdsoError, match="sharded"):
        m.load_marginalization_device(sharded, 0, w, [0])
    m.close()
    sharded.close()
    parent.close()
