"""The activation selection on the device (ldso_ct_make_distance_map / _ba, ldso_ct_select_activation,
ldso_ct_immature_append, ldso_ba_activate_points_tracker) against the literal restatement in
tests/activation_select_ref.py: the map, the dispositions, the selected indices, the counts, the selected
records and the compacted resident set, byte for byte.  The scenes are tests/actsel_scenes.py's."""
import numpy as np
import pytest

import activation_select_ref as R
import actsel_scenes as S
from ldso_amd import _lib as L
from ldso_amd import synth

pytestmark = pytest.mark.gpu

SCENES = S.all_scenes()
_cache = {}


def reference(name):
    """(scene, map after makeDistanceMap, dispositions, selected indices, counts), computed once."""
    if name not in _cache:
        sc = S.build(SCENES[name])
        dm = R.make_distance_map(sc["w"] >> 1, sc["h"] >> 1, sc["krki1"], sc["kt1"], sc["uvd"], sc["seed_host"])
        m0 = dm.array().copy()
        disp, sel, counts = R.walk(dm, sc["pts"], sc["krki1"], sc["kt1"], sc["cmad"], sc["newest"], sc["flagged"])
        for a in (m0, disp, sel):
            a.setflags(write=False)
        _cache[name] = (sc, m0, disp, sel, counts)
    return _cache[name]


def select(ct, sc, compact=False):
    return ct.select_activation(sc["cmad"], 3.0, sc["newest"], sc["flagged"], compact)


@pytest.mark.parametrize("name", list(SCENES))
def test_selection_matches_the_walk(built, name):
    from ldso_amd.tracker import CoarseTracker

    sc, m0, disp_ref, sel_ref, counts_ref = reference(name)
    pts = sc["pts"]
    ct = CoarseTracker(sc["w"], sc["h"])
    m = ct.make_distance_map(sc["krki1"], sc["kt1"], sc["uvd"], sc["seed_host"])
    assert m.tobytes() == m0.tobytes()
    ct.immature_upload(pts)
    disp, sel, counts = select(ct, sc)
    print(name, counts)
    assert np.array_equal(disp, disp_ref), np.flatnonzero(disp != disp_ref)[:10]
    assert np.array_equal(sel, sel_ref)
    assert list(counts.values()) == counts_ref
    assert ct.selection_download().tobytes() == pts[sel_ref].tobytes()
    assert ct.immature_download().tobytes() == pts.tobytes()  # compact = 0 leaves the set untouched
    disp2, sel2, counts2 = select(ct, sc)                     # the same call again: the same bytes
    assert disp2.tobytes() == disp.tobytes() and sel2.tobytes() == sel.tobytes() and counts2 == counts
    assert ct.selection_download().tobytes() == pts[sel_ref].tobytes()
    disp3, sel3, counts3 = select(ct, sc, compact=True)
    assert disp3.tobytes() == disp.tobytes() and sel3.tobytes() == sel.tobytes() and counts3 == counts
    assert ct.immature_download().tobytes() == pts[disp_ref == R.KEEP].tobytes()
    ct.close()


def level1_tables(rng, w, n_hosts):
    krki, kt = S.tables(rng, w.width, w.height, n_hosts, wild=False)
    return krki, kt


@pytest.mark.parametrize("cfg", [dict(n_frames=3, n_points=2, seed=3), dict(n_frames=6, n_points=300, seed=4),
                                 dict(n_frames=5, n_points=0, seed=5)])
def test_map_from_a_ba_context(built, cfg):
    """160 x 120 windows (level 1 is 80 x 60: four growth tiles) after one optimize: the seeds read on the
    device give the map of the same seeds through the host entry, and both the restatement's."""
    from ldso_amd import BAContext
    from ldso_amd.tracker import CoarseTracker

    w = synth.make_window(width=160, height=120, **cfg)
    ctx = BAContext(0).load([w])
    idepth = ctx.optimize(1)[3][0] if w.n_points else np.zeros(0, np.float32)
    N = w.n_frames
    krki1, kt1 = level1_tables(np.random.default_rng(cfg["seed"]), w, N)
    ct = CoarseTracker(160, 120)
    got = ct.make_distance_map_ba(ctx, 0, krki1, kt1)
    old = w.point_host != N - 1
    uvd = np.stack([w.point_data[old, 0], w.point_data[old, 1], idepth[old]], 1) if w.n_points else np.zeros((0, 3))
    host = w.point_host[old]
    ref = R.make_distance_map(80, 60, krki1, kt1, uvd, host).array()
    assert got.tobytes() == ref.tobytes()
    assert ct.make_distance_map(krki1, kt1, uvd, host).tobytes() == ref.tobytes()
    if w.n_points > 100:
        assert (ref == 0).sum() > 10 and (ref == 1000).sum() < ref.size
        # another newest: another map
        got1 = ct.make_distance_map_ba(ctx, 0, krki1, kt1, newest=0)
        o1 = w.point_host != 0
        ref1 = R.make_distance_map(80, 60, krki1, kt1, np.stack([w.point_data[o1, 0], w.point_data[o1, 1], idepth[o1]], 1),
                                   w.point_host[o1]).array()
        assert got1.tobytes() == ref1.tobytes() and got1.tobytes() != got.tobytes()
    ct.close()
    ctx.close()


def test_append_then_trace(built):
    """immature_append puts records behind the resident set, and ldso_ct_trace then traces all of them:
    the same bytes as a tracker that uploaded the whole set at once."""
    from ldso_amd.tracker import CoarseTracker
    from test_immature import blob_image

    w, h = 160, 120
    rng = np.random.default_rng(9)
    host_img, new_img = blob_image(w, h, seed=1), blob_image(w, h, shift=3.0, seed=1)
    krki = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (3, 1))
    kt = np.zeros((3, 3), np.float32)
    kt[:, 0] = [6.0, 7.0, 8.0]
    aff = np.tile(np.array([1.0, 0.0], np.float32), (3, 1))
    a, b = CoarseTracker(w, h), CoarseTracker(w, h)
    for ct in (a, b):
        ct.set_new_frame(host_img)
    recs = [a.make_immature(np.stack([rng.uniform(8, w - 9, n), rng.uniform(8, h - 9, n)], 1).astype(np.float32), 1.0, i)
            for i, n in enumerate((300, 1, 700))]
    whole = np.concatenate(recs)
    a.immature_upload(recs[0])
    a.immature_append(recs[1])
    a.immature_append(recs[2])  # grows the buffer: the resident records move on the device
    a.immature_append(recs[2][:0])
    assert a.immature_download().tobytes() == whole.tobytes()
    b.immature_upload(whole)
    for ct in (a, b):
        ct.set_new_frame(new_img)
    ca, cb = a.trace(krki, kt, aff), b.trace(krki, kt, aff)
    assert ca.tolist() == cb.tolist() and ca.sum() == len(whole) and ca[5] < len(whole)
    assert a.immature_download().tobytes() == b.immature_download().tobytes()
    # appending to an empty set is an upload
    c = CoarseTracker(w, h)
    c.immature_append(recs[0])
    assert c.immature_download().tobytes() == recs[0].tobytes()
    for ct in (a, b, c):
        ct.close()


@pytest.mark.parametrize("img_mode", [3, 1])
def test_activate_points_tracker(built, img_mode):
    """k_activate on the resident selection gives the bytes ldso_ba_activate_points gives on the downloaded
    selection."""
    from ldso_amd import BAContext
    from ldso_amd.tracker import CoarseTracker

    w = synth.make_window(n_frames=5, n_points=600, width=160, height=120, seed=11)
    pts = synth.immature_from_window(w)
    rng = np.random.default_rng(2)
    pts["type"] = rng.choice([1.0, 2.0, 4.0], len(pts))
    pts["last_interval"] = 1.0
    pts["idepth_max"][:4] = np.nan
    pts = np.ascontiguousarray(pts[np.argsort(pts["host"], kind="stable")])
    ctx = BAContext(0)
    ctx.set_tuning(2, img_mode)
    ctx.load([w])
    ctx.optimize(1)
    krki1, kt1 = level1_tables(rng, w, w.n_frames)
    ct = CoarseTracker(160, 120)
    ct.make_distance_map_ba(ctx, 0, krki1, kt1, want_map=False)
    ct.immature_upload(pts)
    disp, sel, counts = ct.select_activation(0.0, compact=True)  # every candidate in the image
    assert 50 < counts["selected"] < len(pts) and counts["deleted"] >= 4
    chosen = ct.selection_download()
    assert chosen.tobytes() == pts[sel].tobytes()
    for min_obs in (1, 3):
        got = ctx.activate_points_tracker(0, ct, min_obs)
        ref = ctx.activate_points(0, chosen, min_obs)
        assert got.tobytes() == ref.tobytes()
    assert (got["status"] == 0).sum() > 10
    ct.close()
    ctx.close()


def test_refusals(built):
    from ldso_amd import BAContext
    from ldso_amd.tracker import CoarseTracker

    ct = CoarseTracker(64, 48)
    pts = S.records(3, [0, 1, 2], 20.5, 20.5)
    ct.immature_upload(pts)
    with pytest.raises(L.LdsoError, match="no distance map"):
        ct.select_activation()
    with pytest.raises(L.LdsoError, match="no selection"):
        ct.selection_download()
    t2 = np.tile(S.PLAIN, (2, 1)), np.zeros((2, 3), np.float32)
    t3 = np.tile(S.PLAIN, (3, 1)), np.zeros((3, 3), np.float32)
    with pytest.raises(L.LdsoError, match="host index"):
        ct.make_distance_map(*t2, [[1, 1, 1]], [2])
    with pytest.raises(L.LdsoError, match="n_hosts"):
        ct.make_distance_map(np.tile(S.PLAIN, (17, 1)), np.zeros((17, 3), np.float32), np.zeros((0, 3)), [])
    ct.make_distance_map(*t2, np.zeros((0, 3)), [])
    with pytest.raises(L.LdsoError, match="n_hosts"):  # a record of host 2
        ct.select_activation()
    ct.make_distance_map(*t3, np.zeros((0, 3)), [])
    for bad in (dict(current_min_act_dist=-0.1), dict(current_min_act_dist=4.5), dict(current_min_act_dist=np.nan),
                dict(newest_host=3), dict(newest_host=-3), dict(min_trace_quality=np.nan)):
        with pytest.raises(L.LdsoError):
            ct.select_activation(**bad)
    disp, sel, _ = ct.select_activation(2.0, newest_host=-1)  # no host skipped
    assert disp.tolist() == [R.OPTIMIZE, R.KEEP, R.KEEP] and sel.tolist() == [0]
    with pytest.raises(L.LdsoError):
        ct.immature_append(S.records(1, -1, 1, 1))
    # the bundle-adjustment side
    w = synth.make_window(n_frames=4, n_points=50, width=160, height=120, seed=1)
    ctx = BAContext(0).load([w])
    t4 = np.tile(S.PLAIN, (4, 1)), np.zeros((4, 3), np.float32)
    with pytest.raises(L.LdsoError, match="frame size"):
        ct.make_distance_map_ba(ctx, 0, *t4)
    big = CoarseTracker(160, 120)
    with pytest.raises(L.LdsoError, match="no selection"):
        ctx.activate_points_tracker(0, big)
    with pytest.raises(L.LdsoError):
        big.make_distance_map_ba(ctx, 1, *t4)
    with pytest.raises(L.LdsoError, match="newest"):
        big.make_distance_map_ba(ctx, 0, *t4, newest=4)
    big.make_distance_map(*t3, np.zeros((0, 3)), [])
    big.immature_upload(pts)
    big.select_activation(0.0)
    with pytest.raises(L.LdsoError, match="n_hosts"):  # 3 hosts, a window of 4 frames
        ctx.activate_points_tracker(0, big)
    from ldso_amd import dist as ldist

    ctx.linearize()
    marg = BAContext(0).load_marginalization(ctx, 0, ldist.subset_window(w, np.arange(0, w.n_points, 2)))
    with pytest.raises(L.LdsoError, match="marginalisation"):
        big.make_distance_map_ba(marg, 0, *t4)
    marg.close()
    # a context that holds a shard of the window's points
    shard = BAContext(0).load([synth.make_window(n_frames=4, n_points=50, width=160, height=120, seed=1)], shard_rank=0,
                              shard_count=3)
    with pytest.raises(L.LdsoError, match="shard of its points") as ei:
        big.make_distance_map_ba(shard, 0, *t4)
    assert ei.value.code == -1
    shard.close()
    for c in (ct, big, ctx):
        c.close()
