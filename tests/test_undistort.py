"""Frame ingestion on the device (ldso_ct_set_new_frame_raw, k_ct_undistort) against the NumPy restatement
of PhotometricUndistorter::processFrame and Undistort::undistort (tests/undistort_ref.py): the image equal
everywhere, NaN where the restatement has NaN (a NaN's sign and payload are not part of the claim), inf
where it has inf; the exposure the reference would return; the entries the footprint rule rejected; the
pyramid and a tracking run behind the raw frame bit-equal to those behind ldso_ct_set_new_frame of the
restatement's image; a torch tensor as the source.  Contexts of one and of two pyramid levels, a source of
83 x 61.  The cases are those test_undistort_ref.py shows to be well posed on the CPU."""
import numpy as np
import pytest

import undistort_ref as R

pytestmark = pytest.mark.gpu

_trackers = {}


@pytest.fixture(scope="module")
def tracker_of(built):
    from ldso_amd.tracker import CoarseTracker

    def get(w, h):
        if (w, h) not in _trackers:
            _trackers[w, h] = CoarseTracker(w, h)
        return _trackers[w, h]

    yield get
    for t in _trackers.values():
        t.close()
    _trackers.clear()


def _set_raw(t, c, raw=None):
    outside = t.undistort_init(**c.init)
    return outside, t.set_new_frame_raw(c.raw if raw is None else raw, c.exposure, c.factor)


def _assert_image(got, want, what):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, (what, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])
    assert np.array_equal(got, want, equal_nan=True)


# cases 1-5: uint8 with a vignette that has zeros, uint16 with 65536 entries, the three ways into the first
# branch with factor 0.5, use_exposure 0, passthrough next to an inf
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(R.CASES))
def test_image(tracker_of, name, size):
    w, h = size
    t = tracker_of(w, h)
    assert t.levels == (1 if size == R.SIZES[0] else 2)
    c = R.case(name, w, h)
    want, want_exposure, want_outside = R.expected(name, w, h)
    outside, exposure = _set_raw(t, c)
    got = t.undistorted()
    print(name, size, "rejected", outside, "exposure", exposure, "nan", int(np.isnan(got).sum()), "inf", int(np.isinf(got).sum()))
    assert outside == want_outside
    assert exposure == want_exposure
    _assert_image(got, want, name)


# case 6: the pyramid behind the raw frame is the pyramid behind the restatement's image
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", R.NAN_FREE)
def test_pyramid_equals_set_new_frame(tracker_of, name, size):
    w, h = size
    t = tracker_of(w, h)
    c = R.case(name, w, h)
    want = R.expected(name, w, h)[0]
    assert np.isfinite(want).all()
    _set_raw(t, c)
    raw_levels = [t.frame_level(l) for l in range(t.levels)]
    t.set_new_frame(np.zeros((h, w), np.float32))  # nothing of the raw frame is left behind
    t.set_new_frame(want, R.expected(name, w, h)[1])
    for l, (dI, ag) in enumerate(raw_levels):
        dI2, ag2 = t.frame_level(l)
        assert dI.tobytes() == dI2.tobytes() and ag.tobytes() == ag2.tobytes(), l
        assert np.abs(dI[:, 1:]).max() > 0


# case 7: a torch tensor on the GPU as the source equals the host path
@pytest.mark.parametrize("name", ["u8_mode2", "u16_mode2", "passthrough_inf"])
def test_torch_tensor_source(tracker_of, name):
    import torch

    w, h = R.SIZES[1]
    t = tracker_of(w, h)
    c = R.case(name, w, h)
    _, exposure = _set_raw(t, c)
    host_img, host_levels = t.undistorted(), [t.frame_level(l) for l in range(t.levels)]
    t.set_new_frame(np.zeros((h, w), np.float32))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = torch.from_numpy(c.raw.copy()).cuda(non_blocking=True)
        assert dev.dtype == (torch.uint8 if c.raw.dtype == np.uint8 else torch.uint16)
        exposure_dev = t.set_new_frame_raw(dev, c.exposure, c.factor)  # the current stream is `side`
    assert exposure_dev == exposure
    _assert_image(t.undistorted(), host_img, name)
    _assert_image(t.undistorted(), R.expected(name, w, h)[0], name)
    for l, (dI, ag) in enumerate(host_levels):
        dI2, ag2 = t.frame_level(l)
        assert np.array_equal(dI, dI2, equal_nan=True) and np.array_equal(ag, ag2, equal_nan=True), l
    side.synchronize()


# case 8: trackNewestCoarse on a reference set beforehand gives the same result after either way
def test_track_after_either_way(tracker_of):
    from ldso_amd import _lib as L

    w, h = R.SIZES[1]
    t = tracker_of(w, h)
    name = "u8_mode1"
    c = R.case(name, w, h)
    want, exposure, _ = R.expected(name, w, h)
    t.make_k((100.0, 100.0, 79.5, 59.5))
    rng = np.random.default_rng(5)
    pc = []
    for l in range(t.levels):
        wl, hl, n = w >> l, h >> l, 600 >> l
        u, v = rng.uniform(3, wl - 4, n).astype(np.float32), rng.uniform(3, hl - 4, n).astype(np.float32)
        lvl_img = want if l == 0 else want.reshape(hl, 2, wl, 2).mean((1, 3))
        color = lvl_img[v.astype(int), u.astype(int)].astype(np.float32)
        pc.append((u, v, rng.uniform(0.5, 1.5, n).astype(np.float32), color))
    t.set_reference(pc, ab_exposure=exposure)
    T0 = np.hstack([np.eye(3), [[0.01], [-0.005], [0.002]]])

    _set_raw(t, c)
    a, steps_a, n_a = t.track(T0, (0.0, 0.0), trace=64)
    t.set_new_frame(np.zeros((h, w), np.float32))
    t.set_new_frame(want, exposure)
    b, steps_b, n_b = t.track(T0, (0.0, 0.0), trace=64)
    assert n_a == n_b and n_a > 2
    for f in L.TRACK_RESULT_DTYPE.names:
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
    for f in L.TRACK_STEP_DTYPE.names:
        assert steps_a[f].tobytes() == steps_b[f].tobytes(), f
    assert np.isfinite(a["last_residuals"]).any() and np.asarray(a["iterations"]).sum() > 0
