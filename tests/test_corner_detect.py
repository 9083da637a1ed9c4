"""Corner detection on the device (ldso_ct_detect_corners) against the numpy restatement of
FeatureDetector::DetectCorners, ComputeDescriptor and makeNewTraces' mode-1 loop
(tests/corner_detect_ref.py): the features' count, order and pixels, score and corner flag bit for
bit, the immature records byte for byte (NaN equals NaN, test_immature.differing), every stats field;
the angle against atan2 in double rounded once; the descriptor in lock-step at the device's own angle
bits -- on sizes whose sides are multiples of 8 and 32 and one where neither is, on images with
suppressed neighbours (blobs), bit-equal scores (tiles) and scores that are not finite (nan)."""
import ctypes as C
import functools

import numpy as np
import pytest

import corner_detect_ref as R
from ldso_amd import _lib as L
from test_immature import differing

pytestmark = pytest.mark.gpu

HOST = 3
CASES = [(kind,) + case for case in sorted(R.CASES) for kind in R.KINDS] + [("blobs",) + R.WIDE]


@functools.lru_cache(maxsize=None)
def image(kind, w, h):
    img = R.image(kind, w, h)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def frame(kind, w, h):
    return R.Frame(image(kind, w, h))


@functools.lru_cache(maxsize=None)
def pattern():
    p = R.bit_pattern()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def expected(kind, w, h, n):
    """The restatement's result; computed once per case and left unchanged."""
    return R.detect_corners(frame(kind, w, h), n, pattern(), HOST)


_trackers = {}


@pytest.fixture(scope="module")
def tracker_of(built):
    from ldso_amd.tracker import CoarseTracker

    def get(w, h):
        if (w, h) not in _trackers:
            _trackers[w, h] = CoarseTracker(w, h)
            _trackers[w, h].corners_init(pattern())
        return _trackers[w, h]

    yield get
    for t in _trackers.values():
        t.close()
    _trackers.clear()


def same_bits_or_both_nan(a, b):
    return (R.bits(a) == R.bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}n{c[3]}")
def test_parity(tracker_of, case):
    kind, w, h, n = case
    ref = expected(*case)
    t = tracker_of(w, h)
    t.set_new_frame(image(kind, w, h))
    rec, feat, st = t.detect_corners(n, host=HOST)
    print(case, st)
    assert st == ref["stats"]
    assert feat.size == rec.size == ref["feat"].size
    assert np.array_equal(np.stack([rec["u"], rec["v"]], 1), ref["xy"].astype(np.float32))
    assert same_bits_or_both_nan(feat["score"], ref["feat"]["score"]).all()
    assert np.array_equal(feat["is_corner"], ref["feat"]["is_corner"])
    assert (feat["level"] == 0).all()
    assert differing(rec, ref["rec"]).size == 0
    assert (rec["type"] == 1).all() and (rec["host"] == HOST).all()

    # the angle: atan2 in double rounded once; at most 1 % of the corners one float ulp off
    ci = np.flatnonzero(feat["is_corner"])
    got, want = feat["angle"][ci], ref["feat"]["angle"][ci]
    off = ~same_bits_or_both_nan(got, want)
    print("corners", ci.size, "angles off:", int(off.sum()), "NaN angles:", int(np.isnan(got).sum()))
    assert off.sum() <= 0.01 * ci.size
    assert (np.abs(R.bits(got[off]).astype(np.int64) - R.bits(want[off]).astype(np.int64)) == 1).all()

    # the descriptor in lock-step: the restatement evaluated at the device's angle bits
    fr = frame(kind, w, h)
    for j, i in enumerate(ci):
        x, y = ref["xy"][i]
        assert np.array_equal(feat["descriptor"][i], R.descriptor(fr, x, y, got[j], pattern())), (i, x, y)
        if not off[j]:
            assert np.array_equal(feat["descriptor"][i], ref["feat"]["descriptor"][i]), (i, x, y)

    # non-corners carry nothing
    nc = feat["is_corner"] == 0
    assert (R.bits(feat["angle"][nc]) == 0).all() and not feat["descriptor"][nc].any()


def test_repeatable(tracker_of):
    w, h, n = 203, 139, 300
    t = tracker_of(w, h)
    t.set_new_frame(image("nan", w, h))
    out = []
    for _ in range(2):
        rec, feat, st = t.detect_corners(n, host=HOST)
        out.append((rec.tobytes(), feat.tobytes(), st))
    assert out[0] == out[1]


def test_capacity_too_small_then_retry(tracker_of):
    kind, w, h, n = "tiles", 200, 136, 340
    ref = expected(kind, w, h, n)
    need = ref["feat"].size
    t = tracker_of(w, h)
    t.set_new_frame(image(kind, w, h))
    with pytest.raises(L.LdsoError, match="capacity"):
        t.detect_corners(n, host=HOST, capacity=need - 1)
    got = C.c_int32()
    rec = np.zeros(need, L.IMMATURE_DTYPE)
    feat = np.zeros(need, L.FEATURE_DTYPE)
    assert L.lib().ldso_ct_detect_corners(t._h, n, HOST, need - 1, rec.ctypes.data, feat.ctypes.data, C.byref(got),
                                          None) < 0
    assert got.value == need
    assert not rec.tobytes().strip(b"\0") and not feat.tobytes().strip(b"\0")  # nothing written
    rec, feat, st = t.detect_corners(n, host=HOST, capacity=got.value)
    assert st == ref["stats"] and differing(rec, ref["rec"]).size == 0
    assert np.array_equal(feat["is_corner"], ref["feat"]["is_corner"])
    # capacity None: starts from twice n and grows by itself
    rec2, feat2, _ = t.detect_corners(n, host=HOST)
    assert rec2.tobytes() == rec.tobytes() and feat2.tobytes() == feat.tobytes()


def test_refusals(built):
    from ldso_amd.tracker import CoarseTracker

    w, h = 200, 136
    t = CoarseTracker(w, h)
    try:
        t.set_new_frame(image("blobs", w, h))
        with pytest.raises(L.LdsoError, match="corners_init"):
            t.detect_corners(300)
        bad = pattern().copy()
        bad[777] = 14
        with pytest.raises(L.LdsoError, match="13"):
            t.corners_init(bad)
        bad[777] = -14
        with pytest.raises(L.LdsoError, match="13"):
            t.corners_init(bad)
        with pytest.raises(L.LdsoError, match="corners_init"):  # a refused table does not count
            t.detect_corners(300)
        t.corners_init(pattern())
        with pytest.raises(L.LdsoError, match="gridsize 37"):
            t.detect_corners(20)
        with pytest.raises(L.LdsoError, match="gridsize 0"):
            t.detect_corners(w * h + 1)
        for n in (0, -5):
            with pytest.raises(L.LdsoError, match="n_features"):
                t.detect_corners(n)
        rec, feat, st = t.detect_corners(300)  # and the context still works
        assert st["features"] == rec.size == feat.size > 0
    finally:
        t.close()
    t = CoarseTracker(w, h)
    try:
        t.corners_init(pattern())
        with pytest.raises(L.LdsoError, match="set_new_frame"):
            t.detect_corners(300)
    finally:
        t.close()


def test_selector_state_untouched(tracker_of):
    """detect_corners after make_new_traces on the same frame: the selector's potential stays, and
    the selection that follows is the one a context without the detection makes."""
    import pixel_select_ref as PS

    w, h = 192, 128
    t = tracker_of(w, h)
    t.set_new_frame(image("blobs", w, h))
    t.select_init(PS.pattern_of(w, h), 3)
    rec_a, st_a = t.make_new_traces(host=HOST, density=300)
    pot = t.select_potential
    rec, feat, st = t.detect_corners(300, host=HOST)
    assert t.select_potential == pot
    assert st == expected("blobs", w, h, 300)["stats"]
    t.select_init(PS.pattern_of(w, h), 3)
    rec_b, st_b = t.make_new_traces(host=HOST, density=300)
    assert st_a == st_b and rec_a.tobytes() == rec_b.tobytes() and t.select_potential == pot
