"""SearchBruteForce and SearchByBoW on the device (ldso_lc_search_brute_force, _many, ldso_lc_search_by_bow)
against the sequential restatement in tests/loop_ref.py.  Every comparison is exact: match lists as integer
triples in the reference's order, the per-corner minima of every keyframe, and the bytes of repeated calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import loop_ref as R
from ldso_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(built):
    from ldso_amd.loop import LoopMatcher

    m = LoopMatcher(160, 120, max_keyframes=6, max_features=512)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def brute_expected(n1, n2):
    """The restatement's result; computed once per case and left unchanged."""
    f1, f2 = R.brute_case(n1, n2)
    details = []
    m = R.search_brute_force(f1, f2, R.TH_LOW, details)
    return f1, f2, m, details


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("sizes", R.BRUTE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_brute_force(matcher, sizes):
    f1, f2, want, details = brute_expected(*sizes)
    matcher.put(1, f1)
    matcher.put(2, f2)
    assert same(matcher.get(1), f1) and same(matcher.get(2), f2)
    got = matcher.search_brute_force(1, 2, R.TH_LOW)
    assert same(got, want), (got, want)
    assert same(matcher.search_brute_force(1, 2, R.TH_LOW), got)  # two identical calls, identical bytes
    # the per-corner minima, matched or not
    counts, idx, dist = matcher.search_brute_force_many(1, [2], sizes[0], R.TH_LOW)
    assert counts[0] == want.size
    assert list(dist[0]) == [d[2] for d in details]
    assert list(idx[0]) == [d[1] if d[2] < R.TH_LOW else -1 for d in details]
    # kf1 == kf2
    self_want = R.search_brute_force(f1, f1, R.TH_LOW)
    assert same(matcher.search_brute_force(1, 1, R.TH_LOW), self_want) and self_want.size == sizes[0]
    if want.size:  # capacity too small: the needed count, nothing written
        buf = np.full(3 * want.size, -5, np.int32)
        n = C.c_int32()
        rc = L.lib().ldso_lc_search_brute_force(matcher._h, 1, 2, R.TH_LOW, want.size - 1, buf.ctypes.data, C.byref(n))
        assert rc < 0 and n.value == want.size and (buf == -5).all()
        assert b"capacity" in L.lib().ldso_ba_last_error()
    matcher.drop(1)
    matcher.drop(2)


def test_brute_force_many_equals_single_calls(matcher):
    frames, order = R.many_case()
    for kf, fr in frames.items():
        matcher.put(kf, fr)
    n1 = int(frames[0]["is_corner"].sum())
    counts, idx, dist = matcher.search_brute_force_many(0, order, n1, R.TH_LOW)
    again = matcher.search_brute_force_many(0, order, n1, R.TH_LOW)
    assert all(same(a, b) for a, b in zip((counts, idx, dist), again))
    c0 = np.flatnonzero(frames[0]["is_corner"])
    for row, kf in enumerate(order):
        single = matcher.search_brute_force(0, kf, R.TH_LOW)
        details = []
        want = R.search_brute_force(frames[0], frames[kf], R.TH_LOW, details)
        assert same(single, want), kf
        assert counts[row] == want.size
        keep = idx[row] >= 0
        assert np.array_equal(c0[keep], single["index1"]) and np.array_equal(idx[row][keep], single["index2"])
        assert np.array_equal(dist[row][keep], single["dist"])
        assert list(dist[row]) == [d[2] for d in details]
    assert counts[order.index(2)] == 0 and counts[order.index(0)] == n1 and (counts[[0, 3, 4]] >= 5).all()
    only_counts = matcher.search_brute_force_many(0, order, n1, R.TH_LOW, details=False)[0]
    assert same(only_counts, counts)
    with pytest.raises(L.LdsoError, match="not in the store"):
        matcher.search_brute_force_many(0, [1, 77], n1)
    for kf in frames:
        matcher.drop(kf)


def test_search_by_bow(matcher):
    f1, b1, f2, b2 = R.bow_case()
    details = []
    want = R.search_by_bow(f1, b1, f2, b2, R.TH_LOW, R.NN_RATIO, details)
    assert want.size >= 20 and (45, 60) in [d[1:] for d in details] and (3, 4) in [d[1:] for d in details]
    matcher.put(1, f1)
    matcher.put(2, f2)
    with pytest.raises(L.LdsoError, match="featVec"):
        matcher.search_by_bow(1, 2)
    matcher.set_bow(1, *R.bow_arrays(b1))
    matcher.set_bow(2, *R.bow_arrays(b2))
    got = matcher.search_by_bow(1, 2, R.TH_LOW, R.NN_RATIO)
    assert same(got, want), (got, want)
    assert same(matcher.search_by_bow(1, 2, R.TH_LOW, R.NN_RATIO), got)
    # the reference's defaults, and the two keyframes swapped
    assert same(matcher.search_by_bow(1, 2), R.search_by_bow(f1, b1, f2, b2))
    assert same(matcher.search_by_bow(2, 1, R.TH_LOW, R.NN_RATIO), R.search_by_bow(f2, b2, f1, b1, R.TH_LOW, R.NN_RATIO))
    assert same(matcher.search_by_bow(1, 1, R.TH_LOW, R.NN_RATIO), R.search_by_bow(f1, b1, f1, b1, R.TH_LOW, R.NN_RATIO))
    buf = np.full(3 * want.size, -5, np.int32)
    n = C.c_int32()
    rc = L.lib().ldso_lc_search_by_bow(matcher._h, 1, 2, R.TH_LOW, R.NN_RATIO, want.size - 1, buf.ctypes.data, C.byref(n))
    assert rc < 0 and n.value == want.size and (buf == -5).all()
    # an empty intersection
    g1, c1, g2, c2 = R.bow_case(disjoint=True)
    matcher.put(3, g1)
    matcher.put(4, g2)
    matcher.set_bow(3, *R.bow_arrays(c1))
    matcher.set_bow(4, *R.bow_arrays(c2))
    assert matcher.search_by_bow(3, 4, R.TH_LOW, R.NN_RATIO).size == 0
    # set_bow's refusals leave the stored vector as it was
    ids, begin, flat = R.bow_arrays(b1)
    with pytest.raises(L.LdsoError, match="ascending"):
        matcher.set_bow(1, ids[::-1].copy(), begin, flat)
    bad = flat.copy()
    bad[3] = int(np.flatnonzero(f1["is_corner"] == 0)[0])
    with pytest.raises(L.LdsoError, match="not a corner"):
        matcher.set_bow(1, ids, begin, bad)
    bad[3] = len(f1)
    with pytest.raises(L.LdsoError, match="out of range"):
        matcher.set_bow(1, ids, begin, bad)
    assert same(matcher.search_by_bow(1, 2, R.TH_LOW, R.NN_RATIO), want)
    for kf in (1, 2, 3, 4):
        matcher.drop(kf)


def test_store_refusals_change_nothing(matcher):
    rng = np.random.default_rng(1)
    fr = R.make_frame(rng, 160, 120, 30, 5)
    for kf in range(6):
        matcher.put(kf, fr)
    with pytest.raises(L.LdsoError, match="full"):
        matcher.put(6, fr)
    other = R.make_frame(rng, 160, 120, 20, 0)
    matcher.put(3, other)  # replacing a stored keyframe needs no free place
    assert same(matcher.get(3), other)
    with pytest.raises(L.LdsoError, match="max_features"):
        matcher.put(2, np.zeros(513, R.FEATURE_DTYPE))
    for u, v in ((160.0, 5.0), (5.0, 120.0), (-0.5, 5.0), (float("nan"), 5.0)):
        bad = other.copy()
        k = int(np.flatnonzero(bad["is_corner"])[4])
        bad["u"][k], bad["v"][k] = u, v
        with pytest.raises(L.LdsoError, match="outside the feature grid"):
            matcher.put(3, bad)
        bad["is_corner"][k] = 0  # a plain feature may lie anywhere
        matcher.put(5, bad)
    assert same(matcher.get(3), other) and same(matcher.get(2), fr)
    with pytest.raises(L.LdsoError, match="not in the store"):
        matcher.get(9)
    with pytest.raises(L.LdsoError, match="count"):
        matcher.update(3, np.zeros(3, np.float32), np.zeros(3, np.int32))
    inv_d = rng.uniform(0.1, 2, len(other)).astype(np.float32)
    usable = (rng.random(len(other)) < 0.5).astype(np.int32)
    matcher.update(3, inv_d, usable)
    want = other.copy()
    want["inv_d"], want["usable"] = inv_d, usable
    assert same(matcher.get(3), want)
    n = C.c_int32()
    buf = np.full(56 * 4, 7, np.uint8)
    assert L.lib().ldso_lc_keyframe_get(matcher._h, 3, 4, buf.ctypes.data, C.byref(n)) < 0
    assert n.value == len(other) and (buf == 7).all()
    for kf in range(6):
        matcher.drop(kf)
    with pytest.raises(L.LdsoError, match="not in the store"):
        matcher.drop(0)
