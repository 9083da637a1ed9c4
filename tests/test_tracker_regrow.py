"""The tracker context's grow-only buffers walked up and down on one context (a small input, a
larger one, the small one again), its kernel timer, and contexts created and destroyed in a row.
Every result is compared with what the other tracker tests compare against: the oracle
(test_tracker, test_immature) or tests/coarse_depth_ref.py (test_tracking_ref), with their
tolerances; nothing is compared with a second run of the library.

The frames are 64 x 48, where setGlobalCalib's level rule gives one level (3072 pixels are not
more than 5000); the reference-cloud tests also run at 128 x 96, the smallest such frame with two."""
import numpy as np
import pytest

import coarse_depth_ref as R
import oracle
from ldso_amd import synth
from test_immature import differing
from test_tracker import AFF6, pc_tuple, pose

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
SIZES = [(64, 48), (128, 96)]


def _calib(w, h):
    return np.array([0.6 * w, 0.9 * h, 0.5 * w - 0.5, 0.5 * h - 0.5], F)


def _tracker(w, h, seed=4):
    from ldso_amd.tracker import CoarseTracker

    color, _ = synth.make_tracker_scene(w, h, seed=seed)
    ct = CoarseTracker(w, h)
    ct.make_k(_calib(w, h))
    ct.set_new_frame(color, 1.0)
    return ct, color


@pytest.mark.parametrize("wh", SIZES)
def test_set_reference_grows_and_shrinks(built, wh):
    """40, 400, 40 points per level: the cloud and the warped buffers grow, then keep their
    addresses; the block partials grow from one block to two.  Tolerances of
    test_gpu_calc_res_and_gs_match_oracle."""
    w, h = wh
    ct, color = _tracker(w, h)
    levels = oracle.make_images(color, w, h)
    assert ct.levels == len(levels) == len(R.level_sizes(w, h))
    K = oracle.ct_make_k(_calib(w, h), w, h)
    for step, n in enumerate((40, 400, 40)):
        _, make_pc = synth.make_tracker_scene(w, h, n_points=(n,), seed=10 + step)
        pcs = make_pc([dI[:, 0] for dI, _ in levels])
        assert all(p["u"].size == n for p in pcs)
        ct.set_reference([pc_tuple(p) for p in pcs], 1.0, AFF6[2:4])
        for l in range(ct.levels):
            T = pose(step, 2.0 ** l)
            rs_o, warped_o = oracle.ct_calc_res(l, w >> l, h >> l, K[l], levels[l][0], pc_tuple(pcs[l]), T, AFF6, 20.0)
            Ho, bo = oracle.ct_calc_gs(warped_o, K[l, 0], K[l, 1], AFF6)
            assert rs_o[1] > n // 2  # most points are evaluated
            rs = ct.calc_res(l, T, AFF6[4:6], 20.0)
            np.testing.assert_array_equal(ct.warped(), warped_o)
            rs2, H, b = ct.calc_res_gs(l, T, AFF6[4:6], 20.0)
            np.testing.assert_array_equal(ct.warped(), warped_o)
            for r in (rs, rs2):
                assert r[1] == rs_o[1]
                assert abs(r[0] - rs_o[0]) <= 1e-5 * abs(rs_o[0]) + 1e-6
                np.testing.assert_allclose(r[[2, 4]], rs_o[[2, 4]], rtol=1e-5, atol=1e-9)
                assert r[3] == 0 and abs(r[5] - rs_o[5]) <= 1e-7
            assert np.abs(H - Ho).max() <= 1e-5 * np.abs(Ho).max(), (n, l)
            assert np.abs(b - bo).max() <= 1e-5 * np.abs(bo).max(), (n, l)
    ct.close()


@pytest.mark.parametrize("wh", SIZES)
def test_make_reference_grows_and_shrinks(built, wh):
    """30, 300, 30 host contributions: byte-exact clouds and counts, as test_tracking_ref."""
    w, h = wh
    ct, _ = _tracker(w, h)
    colors = [np.ascontiguousarray(ct.frame_level(l)[0][:, 0]) for l in range(ct.levels)]
    for step, n in enumerate((30, 300, 30)):
        rng = np.random.default_rng(20 + step)
        center = np.stack([rng.uniform(-1, w, n), rng.uniform(-1, h, n), rng.uniform(0.1, 2.0, n)], axis=1).astype(F)
        hdi = (10.0 ** rng.uniform(-6, 4, n)).astype(F)
        pc_n = ct.make_reference(center, hdi, 1.0, AFF6[2:4])
        want = R.make_coarse_depth(w, h, center, hdi, colors)
        assert len(want) == ct.levels and want[0].shape[0] >= n // 2
        for l in range(ct.levels):
            got = ct.reference(l)
            assert pc_n[l] == want[l].shape[0] == got.shape[0], (n, l)
            assert got.tobytes() == want[l].tobytes(), (n, l)
    ct.close()


def _blobs(shift=0.0, a=1.0, b=0.0):
    """A textured 64 x 48 image evaluated at (x - shift, y), with affine brightness a, b."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    xx = xx - shift
    img = np.full((H, W), 90.0)
    for _ in range(40):
        cx, cy, s = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1.5, 5.0)
        img += rng.uniform(20, 80) * rng.choice([-1, 1]) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return (a * img + b).astype(F)


def _features(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(8, W - 14, n), rng.uniform(8, H - 8, n)], 1).astype(F)


def _host_tables():
    """Host 0: a translation along x with 2 px of disparity at inverse depth 0.5; hosts 1-2 rotated."""
    fx, fy = 0.6 * W, 0.9 * H
    K = np.array([[fx, 0, 0.5 * W - 0.5], [0, fy, 0.5 * H - 0.5], [0, 0, 1]])
    krki, kt, aff = [np.eye(3, dtype=F)], [np.array([4.0, 0, 0], F)], [np.array((1.1, -5.0), F)]
    for i, (ang, t) in enumerate([(0.02, (1.5, -0.5, 0.01)), (-0.05, (-2.0, 1.0, -0.02))]):
        c, s = np.cos(ang), np.sin(ang)
        krki.append((K @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.linalg.inv(K)).astype(F))
        kt.append(np.array(t, F))
        aff.append(np.array((1.0 + 0.1 * i, 2.0 * i), F))
    return np.stack(krki), np.stack(kt), np.stack(aff)


def test_make_immature_grows_and_shrinks(built):
    """5, 300, 5 new points: records equal to the oracle's, word for word."""
    from ldso_amd.tracker import CoarseTracker

    img = _blobs()
    dI = oracle.make_images(img, W, H)[0][0]
    ct = CoarseTracker(W, H)
    ct.set_new_frame(img)
    for step, n in enumerate((5, 300, 5)):
        uv = _features(n, 30 + step)
        got = ct.make_immature(uv, 2.0, step)
        assert differing(got, oracle.ip_make(dI, W, H, uv, 2.0, step)).size == 0, n
    ct.close()


def test_trace_grows_and_shrinks(built):
    """3 points on 1 host, 200 on 3 hosts, 3 on 1 host: the resident records and the host tables
    grow and are reused; statuses, intervals and counters equal to the oracle's (test_gpu_trace_parity)."""
    from ldso_amd.tracker import CoarseTracker

    host, new = _blobs(), _blobs(shift=2.0, a=1.1, b=-5.0)
    dH, dN = (oracle.make_images(x, W, H)[0][0] for x in (host, new))
    krki, kt, aff = _host_tables()
    ct = CoarseTracker(W, H)
    ct.set_new_frame(new)
    seen = set()
    for step, (n, n_hosts) in enumerate(((3, 1), (200, 3), (3, 1))):
        pts = np.concatenate([oracle.ip_make(dH, W, H, _features((n + k) // n_hosts, 40 + 3 * step + k), 1.0, k)
                              for k in range(n_hosts)])
        assert pts.size == n
        pts["idepth_min"][1::5], pts["idepth_max"][1::5] = 0.3, 0.8  # finite intervals
        ref = pts.copy()
        ct.immature_upload(pts)
        for _ in range(2):  # two successive traces on the resident records
            c = ct.trace(krki[:n_hosts], kt[:n_hosts], aff[:n_hosts])
            cr = oracle.ip_trace(dN, W, H, krki[:n_hosts], kt[:n_hosts], aff[:n_hosts], ref)
            got = ct.immature_download()
            bad = differing(got, ref)
            assert bad.size == 0, (n, bad[:5])
            np.testing.assert_array_equal(c, cr)
            assert c.sum() == n
        seen.update(ref["last_status"].tolist())
    assert len(seen) >= 3  # the scene drives more than one exit of traceOn
    ct.close()


def _counts(times):
    return {k: v[1] for k, v in times.items()}


def test_kernel_timer_counts(built):
    """One set_new_frame, calc_res and calc_gs with timing on: one launch in each of their four
    slots, none elsewhere; an untimed call adds nothing; turning timing on again zeroes."""
    w, h = W, H
    ct, color = _tracker(w, h)
    levels = oracle.make_images(color, w, h)
    _, make_pc = synth.make_tracker_scene(w, h, n_points=(300,), seed=3)
    ct.set_reference([pc_tuple(p) for p in make_pc([dI[:, 0] for dI, _ in levels])], 1.0, AFF6[2:4])
    names = ["k_ct_pyr_down", "k_ct_pyr_grad", "k_ct_calc_res", "k_ct_calc_gs", "k_ct_make_immature", "k_ct_trace",
             "k_ct_ip_count"]
    want = dict(zip(names, (1, 1, 1, 1, 0, 0, 0)))

    def calls():
        ct.set_new_frame(color, 1.0)
        ct.calc_res(0, pose(0), AFF6[4:6], 20.0)
        ct.calc_gs(0, pose(0), AFF6[4:6])

    ct.set_kernel_timing(True)
    calls()
    t = ct.kernel_times()
    assert list(t) == names and _counts(t) == want
    assert all(np.isfinite(ms) and ms >= 0 for ms, _ in t.values())
    assert all(ms == 0 for ms, n in t.values() if n == 0)
    ct.set_kernel_timing(False)
    calls()
    assert ct.kernel_times() == t  # counts and times left alone
    ct.set_kernel_timing(True)
    assert all(v == (0.0, 0) for v in ct.kernel_times().values())
    calls()
    assert _counts(ct.kernel_times()) == want
    ct.close()


def test_ba_kernel_timer_counts(built):
    """The same on the bundle-adjustment side: one linearize(accumulate=1) is one launch of
    k_linearize, k_point_sc, k_stitch and k_stitch_sum."""
    from ldso_amd import BAContext

    ctx = BAContext(0)
    ctx.load([synth.make_window(n_frames=3, n_points=64, seed=5)])
    launched = {"k_linearize", "k_point_sc", "k_stitch", "k_stitch_sum"}
    ctx.set_kernel_timing(True)
    ctx.linearize(fix=False, accumulate=True)
    t = ctx.kernel_times()
    assert {k: n for k, (ms, n) in t.items()} == {k: int(k in launched) for k in t} and launched <= set(t)
    assert all(np.isfinite(ms) and ms >= 0 for ms, _ in t.values())
    ctx.set_kernel_timing(False)
    off = ctx.kernel_times()
    ctx.linearize(fix=False, accumulate=True)
    assert ctx.kernel_times() == off  # an untimed pass adds nothing
    ctx.set_kernel_timing(True)
    assert all(n == 0 and ms == 0 for ms, n in ctx.kernel_times().values())
    ctx.linearize(fix=False, accumulate=True)
    assert {k: n for k, (ms, n) in ctx.kernel_times().items()} == {k: int(k in launched) for k in t}
    ctx.close()


def test_create_and_close_in_a_row(built):
    """20 contexts, one frame each: every call returns 0 (the wrappers raise otherwise)."""
    from ldso_amd.tracker import CoarseTracker

    color, _ = synth.make_tracker_scene(W, H, seed=1)
    for _ in range(20):
        ct = CoarseTracker(W, H)
        ct.set_new_frame(color, 1.0)
        ct.close()
