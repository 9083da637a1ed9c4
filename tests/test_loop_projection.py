"""ComputeOptimizedPose's correspondence search on the device (ldso_lc_make_idepth_map, _ba,
ldso_lc_search_by_projection) against the sequential restatement in tests/loop_ref.py, and the tracker's
corner detection handed to the store on the device (ldso_lc_keyframe_put_tracker).  Every comparison is
exact: the map and the output records byte for byte (the doubles as bit patterns)."""
import ctypes as C
import functools

import numpy as np
import pytest

import loop_ref as R
from ldso_amd import _lib as L

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def matcher_of(built):
    from ldso_amd.loop import LoopMatcher

    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[w, h] = LoopMatcher(w, h, max_keyframes=4, max_features=512)
        return made[w, h]

    yield get
    for m in made.values():
        m.close()


@functools.lru_cache(maxsize=None)
def case(w, h, sim):
    cur, cand, centers, calib, scr = R.projection_case(w, h, sim)
    return cur, cand, centers, calib, scr, R.make_idepth_map(w, h, centers)


@functools.lru_cache(maxsize=None)
def expected(w, h, sim, window):
    """The restatement's result; computed once per case and left unchanged."""
    cur, cand, centers, calib, scr, idm = case(w, h, sim)
    stats = {}
    return R.search_by_projection(cur, cand, idm, calib, scr, window, 50, stats), stats


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("size", R.PROJECTION_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sim", sorted(R.SIMILARITIES))
def test_projection(matcher_of, size, sim):
    w, h = size
    m = matcher_of(w, h)
    cur, cand, centers, calib, scr, idm = case(w, h, sim)
    m.put(10, cur)
    m.put(20, cand)
    got_map = m.make_idepth_map(centers)
    assert same(got_map, idm) and np.count_nonzero(idm) >= 100
    for window in (5.0, 25.0):
        want, stats = expected(w, h, sim, window)
        got = m.search_by_projection(10, 20, calib, scr, window, 50)
        assert got.size == want.size, (got.size, want.size)
        assert same(got, want), [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        assert same(m.search_by_projection(10, 20, calib, scr, window, 50), got)
        if sim == "to_zero":
            assert stats["pc2_zero"] >= 30 and stats["behind"] >= 30
        else:
            assert want.size >= 30 and stats["multi_cell_tie"] >= 1 and stats["hole"] >= 1
            assert min(stats[k] for k in ("xmin", "xmax", "ymin", "ymax")) >= 1
    if sim == "half":  # capacity too small: the needed count, nothing written
        want = expected(w, h, sim, 5.0)[0]
        buf = np.full(80 * want.size, 9, np.uint8)
        n = C.c_int32()
        rc = L.lib().ldso_lc_search_by_projection(m._h, 10, 20, L.ptr(calib, L.f32p), L.ptr(scr, L.f64p), 5.0, 50,
                                                  want.size - 1, buf.ctypes.data, C.byref(n))
        assert rc < 0 and n.value == want.size and (buf == 9).all()
        # the fields the map fills in later, overwritten on the device
        usable = np.zeros(len(cand), np.int32)
        usable[::2] = 1
        m.update(20, cand["inv_d"], usable)
        cand2 = cand.copy()
        cand2["usable"] = usable
        want2 = R.search_by_projection(cur, cand2, idm, calib, scr, 5.0, 50)
        assert 0 < want2.size < want.size and same(m.search_by_projection(10, 20, calib, scr, 5.0, 50), want2)
    m.drop(10)
    m.drop(20)


def test_projection_needs_a_map(built):
    from ldso_amd.loop import LoopMatcher

    m = LoopMatcher(160, 120, 2, 64)
    fr = R.make_frame(np.random.default_rng(0), 160, 120, 10, 2)
    m.put(0, fr)
    with pytest.raises(L.LdsoError, match="map"):
        m.search_by_projection(0, 0, R.calib_of(160, 120), R.SIMILARITIES["identity"])
    with pytest.raises(L.LdsoError, match="map"):
        m.idepth_map()
    assert not m.make_idepth_map(np.zeros((0, 3), F)).any()
    assert m.search_by_projection(0, 0, R.calib_of(160, 120), R.SIMILARITIES["identity"]).size == 0
    m.close()


def test_idepth_map_from_a_ba_pass(built):
    import coarse_depth_ref as CD
    from ldso_amd import BAContext, synth
    from ldso_amd.loop import LoopMatcher

    win = synth.make_window(n_frames=3, n_points=64, width=160, height=120, seed=6)
    win.point_rank = np.random.default_rng(4).permutation(win.n_points).astype(np.int32)
    m = LoopMatcher(160, 120, 2, 64)
    ctx = BAContext(0).load([win])
    with pytest.raises(L.LdsoError, match="pass"):
        m.make_idepth_map_from(ctx, 0)
    ctx.linearize(fix=False, accumulate=True)
    res = ctx.residuals(0)
    for target in (-1, 1):
        frame = win.n_frames - 1 if target < 0 else target
        centers, _ = CD.window_contributions(win, res["state"], res["center"], np.zeros(win.n_points, F), frame)
        assert centers.shape[0] >= 5
        got = m.make_idepth_map_from(ctx, 0, target)
        assert same(got, m.idepth_map())
        host = m.make_idepth_map(centers)  # the same pass's read-back centres in device point order
        assert same(got, host) and same(got, R.make_idepth_map(160, 120, centers))
        assert np.count_nonzero(got) >= 5
    with pytest.raises(L.LdsoError, match="target_frame"):
        m.make_idepth_map_from(ctx, 0, 3)
    with pytest.raises(L.LdsoError, match="window"):
        m.make_idepth_map_from(ctx, 1)
    big = LoopMatcher(320, 240, 2, 64)
    with pytest.raises(L.LdsoError, match="size"):
        big.make_idepth_map_from(ctx, 0)
    big.close()
    ctx.close()
    m.close()


def test_put_tracker_equals_put_of_the_downloaded_features(built):
    import corner_detect_ref as CR
    from ldso_amd.loop import LoopMatcher
    from ldso_amd.tracker import CoarseTracker

    w, h, n = 200, 136, 340  # gridsize 9, two picks per cell (corner_detect_ref.CASES)
    t = CoarseTracker(w, h)
    m = LoopMatcher(w, h, 3, 1024)
    with pytest.raises(L.LdsoError, match="detection"):
        m.put_tracker(1, t)
    t.corners_init(CR.bit_pattern())
    t.set_new_frame(CR.image("blobs", w, h))
    rec, feat, st = t.detect_corners(n)
    print(feat.size, st)
    assert feat.size >= 30 and st["corners"] >= 5 and st["corners"] < feat.size
    want = np.zeros(feat.size, L.LC_FEATURE_DTYPE)
    want["u"], want["v"], want["angle"], want["inv_d"] = rec["u"], rec["v"], feat["angle"], -1
    want["is_corner"], want["descriptor"] = feat["is_corner"], feat["descriptor"]
    m.put_tracker(1, t)
    m.put(2, want)
    got = m.get(1)
    assert same(got, want) and same(m.get(2), want)
    # both keyframes are indexed alike: the same matches either way
    a, b = m.search_brute_force(1, 2), m.search_brute_force(2, 1)
    assert a.size == st["corners"] and same(a, b) and same(a, R.search_brute_force(want, want))
    other = LoopMatcher(160, 120, 2, 1024)
    with pytest.raises(L.LdsoError, match="size"):
        other.put_tracker(1, t)
    small = LoopMatcher(w, h, 2, 8)
    with pytest.raises(L.LdsoError, match="max_features"):
        small.put_tracker(1, t)
    for x in (other, small, m):
        x.close()
    t.close()
