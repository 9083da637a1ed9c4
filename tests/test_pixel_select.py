"""Pixel selection on the device (ldso_ct_select_pixels, ldso_ct_make_new_traces) against the numpy
restatement of PixelSelector::makeMaps and makeNewTraces' walk (tests/pixel_select_ref.py): the
selection map byte for byte, every stats field, and the immature records byte for byte (NaN equals
NaN, test_immature.differing) in the walk's order -- on a size whose sides are multiples of 32 and
one where neither is, on images with direction-dependent cells (mixed) and with NaN pixels, from
starting points that take each branch of makeMaps."""
import ctypes as C
import functools

import numpy as np
import pytest

import pixel_select_ref as R
from ldso_amd import _lib as L
from test_immature import differing

pytestmark = pytest.mark.gpu

# the four pairs tests/test_pixel_select_ref.py shows to take makeMaps' branches, and a start from a
# coarser potential
PAIRS = R.PAIRS + ((1500, 5),)
KINDS = ("blobs", "mixed", "nan")
HOST = 4


@functools.lru_cache(maxsize=None)
def image(kind, w, h, seed=1):
    img = R.image(kind, w, h, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def frame(kind, w, h, seed=1):
    return R.Frame(image(kind, w, h, seed))


@functools.lru_cache(maxsize=None)
def pattern(w, h):
    return R.pattern_of(w, h)


@functools.lru_cache(maxsize=None)
def expected(kind, w, h, density, potential, extra=()):
    """(map, records, stats, potential left) of the restatement; computed once per case."""
    sel = R.Selector(pattern(w, h), potential)
    m, st, _ = sel.make_maps(frame(kind, w, h), density=density, **dict(extra))
    rec, _ = R.walk(frame(kind, w, h), m, HOST)
    return m, rec, st, sel.potential


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


def check_case(t, kind, w, h, density, potential, extra=()):
    m_ref, rec_ref, st_ref, pot_ref = expected(kind, w, h, density, potential, extra)
    t.set_new_frame(image(kind, w, h))
    t.select_init(pattern(w, h), potential)
    m, st = t.select_pixels(density=density, **dict(extra))
    print(kind, (w, h), (density, potential), st, "differing map pixels:", np.count_nonzero(m != m_ref))
    assert m.dtype == np.float32 and m.astype(np.uint8).tobytes() == m_ref.tobytes()
    assert st == st_ref
    assert t.select_potential == pot_ref
    t.select_init(pattern(w, h), potential)
    rec, st2 = t.make_new_traces(host=HOST, density=density, **dict(extra))
    assert st2 == st_ref and t.select_potential == pot_ref
    assert rec.size == rec_ref.size
    assert differing(rec, rec_ref).size == 0
    return rec, st


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"d{p[0]}p{p[1]}")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity(tracker_of, size, kind, pair):
    w, h = size
    check_case(tracker_of(w, h), kind, w, h, *pair)


def test_without_direction_distribution(tracker_of):
    check_case(tracker_of(200, 136), "blobs", 200, 136, 300, 3, (("select_direction_distribution", 0),))


def test_th_factor_two(tracker_of):
    check_case(tracker_of(200, 136), "blobs", 200, 136, 300, 3, (("th_factor", 2.0),))


def test_repeatable(tracker_of):
    w, h = 200, 136
    t = tracker_of(w, h)
    t.set_new_frame(image("mixed", w, h))
    out = []
    for _ in range(2):
        t.select_init(pattern(w, h), 3)
        m, st = t.select_pixels(density=300)
        t.select_init(pattern(w, h), 3)
        rec, st2 = t.make_new_traces(density=300)
        out.append((m.tobytes(), rec.tobytes(), st, st2))
    assert out[0] == out[1]


def test_potential_carries_over(tracker_of):
    w, h = 192, 128
    t = tracker_of(w, h)
    t.select_init(pattern(w, h), 3)
    sel = R.Selector(pattern(w, h), 3)
    for seed in (1, 2, 3):
        t.set_new_frame(image("blobs", w, h, seed))
        rec, st = t.make_new_traces(host=HOST, density=300)
        rec_ref, st_ref, _, _ = sel.make_new_traces(frame("blobs", w, h, seed), host=HOST, density=300)
        assert st == st_ref and t.select_potential == sel.potential
        assert rec.size == rec_ref.size and differing(rec, rec_ref).size == 0


def test_capacity_too_small_then_retry(tracker_of):
    w, h = 192, 128
    t = tracker_of(w, h)
    _, rec_ref, st_ref, _ = expected("blobs", w, h, 300, 3)
    t.set_new_frame(image("blobs", w, h))
    t.select_init(pattern(w, h), 3)
    with pytest.raises(L.LdsoError, match="capacity"):
        t.make_new_traces(host=HOST, capacity=rec_ref.size - 1, density=300)
    n = C.c_int32()
    p = t._select_params(dict(density=300))
    buf = np.zeros(rec_ref.size, L.IMMATURE_DTYPE)
    assert L.lib().ldso_ct_make_new_traces(t._h, C.byref(p), HOST, rec_ref.size - 1, buf.ctypes.data, C.byref(n),
                                           None) < 0
    assert n.value == rec_ref.size
    assert t.select_potential == 3  # put back: the retry repeats the selection
    rec, st = t.make_new_traces(host=HOST, capacity=n.value, density=300)
    assert st == st_ref and rec.size == rec_ref.size and differing(rec, rec_ref).size == 0


def test_refusals(built):
    from ldso_amd.tracker import CoarseTracker

    w, h = 192, 128
    t = CoarseTracker(w, h)
    try:
        t.select_init(pattern(w, h), 3)
        with pytest.raises(L.LdsoError, match="set_new_frame"):
            t.select_pixels(density=300)
    finally:
        t.close()
    t = CoarseTracker(w, h)
    try:
        t.set_new_frame(image("blobs", w, h))
        with pytest.raises(L.LdsoError, match="select_init"):
            t.select_pixels(density=300)
        with pytest.raises(L.LdsoError, match="select_init"):
            t.make_new_traces(density=300)
        t.select_init(pattern(w, h), 3)
        for bad in (dict(density=0.0), dict(density=float("nan")), dict(density=float("inf")),
                    dict(density=300, recursions=-1)):
            with pytest.raises(L.LdsoError):
                t.select_pixels(**bad)
            with pytest.raises(L.LdsoError):
                t.make_new_traces(**bad)
        assert t.select_potential == 3
    finally:
        t.close()
    small = CoarseTracker(160, 120)  # two pyramid levels
    try:
        assert small.levels == 2
        with pytest.raises(L.LdsoError, match="levels"):
            small.select_init(R.pattern_of(160, 120), 3)
        small.set_new_frame(R.image("blobs", 160, 120))
        with pytest.raises(L.LdsoError, match="levels"):
            small.select_pixels(density=300)
    finally:
        small.close()


def test_wide_unaligned_frame(tracker_of):
    """752 x 480: more cells and more pixels than one workgroup scans, neither side a multiple of 32."""
    check_case(tracker_of(752, 480), "blobs", 752, 480, 1500, 3)
