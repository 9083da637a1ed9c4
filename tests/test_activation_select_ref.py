"""Pins tests/activation_select_ref.py, the literal restatement of CoarseDistanceMap and of
activatePointsMT's walk, with answers that do not share its code, and the order-free model of the
stamped map against the literal stamps.  No GPU."""
import numpy as np
import pytest

import activation_select_ref as R
import actsel_scenes as S
from ldso_amd import _lib as L


def stamped(w1, h1, seeds, stamps):
    dm = R.DistanceMap(w1, h1)
    dm.make(seeds)
    m0 = dm.array().copy()
    for x, y in stamps:
        dm.add(x, y)
    return m0, dm.array()


def test_order_free_model_equals_literal_stamps():
    rng = np.random.default_rng(20261020)
    n_grids = 1200
    corner_lowered = border_checked = 0
    for g in range(n_grids):
        w1, h1 = int(rng.integers(4, 27)), int(rng.integers(4, 19))
        forced = [(w1 - 1, int(rng.integers(1, h1))), (int(rng.integers(1, w1)), h1 - 1), (w1 - 1, h1 - 1),
                  (w1 - 2, h1 - 2)]

        def draw(n):
            pts = [(int(rng.integers(1, w1)), int(rng.integers(1, h1))) for _ in range(n)]
            pts += [forced[i] for i in range(4) if rng.random() < 0.35]
            return [pts[i] for i in rng.permutation(len(pts))]

        seeds, stamps = draw(int(rng.integers(0, 4))), draw(int(rng.integers(1, 7)))
        m0, m = stamped(w1, h1, seeds, stamps)
        for y in range(1, h1):
            for x in range(1, w1):
                assert R.model_value(w1, h1, m0, stamps, x, y) == m[y, x], (g, w1, h1, seeds, stamps, x, y)
        assert R.corner_by_levels(w1, h1, m0, stamps) == m[h1 - 1, w1 - 1], (g, w1, h1, seeds, stamps)
        corner_lowered += m[h1 - 1, w1 - 1] not in (0, 1000)
        border_checked += (m[1:, w1 - 1] < 1000).sum() + (m[h1 - 1, 1:] < 1000).sum()
    assert corner_lowered > 20 and border_checked > 1000  # the hard cases were there


def test_known_examples():
    # a 6 x 8 grid (w1 = 6, h1 = 8): source (1, 2) reaches (0, 4) at 3, not at the free-space 2, because
    # (0, 3) is on the border and does not propagate
    _, m = stamped(6, 8, [(1, 2)], [])
    assert R.steps(1, 2) == 2 and m[4, 0] == 3 and m[3, 0] == 1
    # a 10 x 10 grid: the corner depends on the order of the stamps
    _, m = stamped(10, 10, [], [(7, 3), (4, 3)])
    assert m[9, 9] == 1000 and m[8, 8] == 5
    _, m = stamped(10, 10, [], [(4, 3), (7, 3)])
    assert m[9, 9] == 7 and m[8, 8] == 5
    assert R.model_value(10, 10, np.full((10, 10), 1000), [(7, 3), (4, 3)], 9, 9) == 1000
    assert R.model_value(10, 10, np.full((10, 10), 1000), [(4, 3), (7, 3)], 9, 9) == 7


def test_hand_worked_map_9x7():
    # seeds A = (2, 2) and B = (8, 4) on the last column.  Step 1 takes the 8 neighbours, step 2 the 4
    # neighbours, step 3 the 8 again: from A, offset (2, 1) is reached at 2, (2, 2) at 3 (a diagonal step,
    # a straight step, then no diagonal left at the even step), (3, 3) at 4 (diagonal, straight, diagonal,
    # straight); B is on the border and never spreads.
    _, m = stamped(9, 7, [(2, 2), (8, 4)], [])
    assert m[2, 2] == 0 and m[4, 8] == 0
    assert m[3, 4] == 2 and m[4, 4] == 3 and m[5, 5] == 4
    assert m[2, 3] == 1 and m[3, 3] == 1 and m[2, 4] == 2 and m[2, 5] == 3 and m[2, 7] == 5
    # around B only what A reaches: (7, 4) is A's at max(5, 2) = 5, (8, 3) and (8, 5) come from (7, *)
    assert m[4, 7] == 5 and m[3, 7] == 5
    assert m[3, 8] == 6 and m[5, 8] == 6  # not 1: B did not propagate
    # (1, 1) is set at the odd step 1 and so spreads at the even step 2, without diagonals: the corner
    # (0, 0), whose other neighbours are border pixels, is never reached; neither is (0, 6) from (1, 5)
    assert m[0, 0] == 1000 and m[6, 0] == 1000 and m[1, 0] == 2
    want_row2 = [2, 1, 0, 1, 2, 3, 4, 5, 6]
    assert m[2].tolist() == want_row2


def rec(**kw):
    p = S.records(1, 0, 20.5, 20.5)  # the plain table puts it on (10, 10)
    for k, v in kw.items():
        p[k] = v
    return p


@pytest.mark.parametrize("fields,flagged,want", [
    (dict(), False, R.OPTIMIZE),
    (dict(idepth_max=np.nan), False, R.DELETE),
    (dict(idepth_max=np.inf), False, R.DELETE),
    (dict(last_status=R.IPS_OUTLIER), False, R.DELETE),
    (dict(last_status=R.IPS_UNINITIALIZED), False, R.KEEP),
    (dict(last_status=R.IPS_UNINITIALIZED), True, R.DELETE),
    (dict(last_status=R.IPS_SKIPPED), False, R.OPTIMIZE),
    (dict(last_status=R.IPS_BADCONDITION), False, R.OPTIMIZE),
    (dict(last_status=R.IPS_OOB), False, R.OPTIMIZE),
    (dict(quality=3.0), False, R.KEEP),                       # `>`, not `>=`
    (dict(quality=3.0), True, R.DELETE),
    (dict(quality=np.float32(3.0000002)), False, R.OPTIMIZE),
    (dict(last_interval=8.0), False, R.KEEP),                 # `< 8`
    (dict(last_interval=np.float32(7.9999995)), False, R.OPTIMIZE),
    (dict(idepth_min=-0.6, idepth_max=0.6), False, R.KEEP),   # the sum is 0, not > 0
    (dict(last_status=R.IPS_OOB, quality=1.0), False, R.DELETE),  # OOB that cannot activate, host not flagged
    (dict(last_status=R.IPS_OOB, quality=1.0), True, R.DELETE),
    (dict(u=-40.0), False, R.DELETE),                         # projects left of the image
    (dict(u=0.4), False, R.DELETE),                           # u = 0 fails `u > 0`
])
def test_classification_branches(fields, flagged, want):
    dm = R.DistanceMap(32, 24)
    dm.make([])
    disp, sel, counts = R.walk(dm, rec(**fields), [S.PLAIN], [np.zeros(3, np.float32)], 2.0, newest_host=1,
                               flagged=[flagged])
    assert disp[0] == want
    assert sel.tolist() == ([0] if want == R.OPTIMIZE else [])
    assert counts == [int(want == R.KEEP), int(want == R.DELETE), int(want == R.OPTIMIZE), 0]


def test_distance_test_and_fraction():
    # a seed on (10, 10): a candidate on (12, 10) sees 2; type 1 with currentMinActDist 2 activates at
    # 2 + frac >= 2, type 2 (threshold 4) does not; the fraction comes from ptp[0]
    krki, kt = [S.PLAIN], [np.zeros(3, np.float32)]
    for type_, frac, want in [(1.0, 0.0, R.OPTIMIZE), (2.0, 0.0, R.KEEP), (1.0, 0.25, R.OPTIMIZE)]:
        dm = R.make_distance_map(32, 24, krki, kt, [[20.5, 20.5, 0.5]], [0])
        p = rec(u=2 * (12 + frac) + 0.5, type=type_)
        disp, _, counts = R.walk(dm, p, krki, kt, 2.0, newest_host=1)
        assert disp[0] == want and counts[3] == int(want == R.KEEP)
    # threshold 2.25 (0.75 * 3 is not a reference type, the arithmetic is): 2 + 0.25 >= 2.25, 2 + 0.2 is not
    for frac, want in [(0.25, R.OPTIMIZE), (0.2, R.KEEP)]:
        dm = R.make_distance_map(32, 24, krki, kt, [[20.5, 20.5, 0.5]], [0])
        disp, _, _ = R.walk(dm, rec(u=2 * (12 + frac) + 0.5, type=3.0), krki, kt, 0.75, newest_host=1)
        assert disp[0] == want
    # an accept stamps the map before the next candidate: the second of two neighbours is kept
    dm = R.make_distance_map(32, 24, krki, kt, [], [])
    two = np.concatenate([rec(), rec(u=22.5)])
    disp, sel, counts = R.walk(dm, two, krki, kt, 2.0, newest_host=1)
    assert disp.tolist() == [R.OPTIMIZE, R.KEEP] and sel.tolist() == [0] and counts == [1, 0, 1, 1]
    # the newest host's records are kept untouched
    disp, _, counts = R.walk(R.make_distance_map(32, 24, krki, kt, [], []), rec(idepth_max=np.nan), krki, kt, 2.0,
                             newest_host=0)
    assert disp.tolist() == [R.KEEP] and counts == [1, 0, 0, 0]


def test_conversion_rule():
    assert R.to_int(np.float32(np.nan)) == R.INT_MIN and R.to_int(np.float32(3e9)) == R.INT_MIN
    assert R.to_int(np.float32(-0.7)) == 0 and R.to_int(np.float32(5.9)) == 5
    x, y, _ = R.project(S.PLAIN, [0, 0, -2], 20.5, 20.5, 0.5)  # ptp[2] = 0: division by zero
    assert x == R.INT_MIN


def test_scenes_are_well_posed():
    """What the GPU tests rely on occurs in their scenes: every disposition, a candidate that passes the
    initial map but is rejected because of an earlier accept, an accept on the last row or column."""
    seen = set()
    late_reject = border_accept = outside = behind = 0
    scenes = S.all_scenes()
    for name in ("random-64x48-5h-300s-1200r-0.7", "random-70x50-5h-300s-1200r-2.0", "border-64x48-0", "border-70x50-1",
                 "snake-64x48-fwd-2.0"):
        sc = S.build(scenes[name])
        w1, h1 = sc["w"] >> 1, sc["h"] >> 1
        dm = R.make_distance_map(w1, h1, sc["krki1"], sc["kt1"], sc["uvd"], sc["seed_host"])
        m0 = dm.array().copy()
        pts = sc["pts"]
        disp, sel, counts = R.walk(dm, pts, sc["krki1"], sc["kt1"], sc["cmad"], sc["newest"], sc["flagged"])
        seen |= set(disp.tolist())
        assert counts[0] + counts[1] + counts[2] == len(pts)
        for i in range(len(pts)):
            p = pts[i]
            hst = int(p["host"])
            if hst == sc["newest"] or R.classify(p, sc["flagged"][hst]) is not None:
                continue
            d = np.float32(0.5) * (p["idepth_max"] + p["idepth_min"])
            x, y, ptp0 = R.project(sc["krki1"][hst], sc["kt1"][hst], p["u"], p["v"], d)
            if not (0 < x < w1 and 0 < y < h1):
                outside += 1
                k9 = sc["krki1"][hst]
                behind += bool(k9[6] * p["u"] + k9[7] * p["v"] + k9[8] + sc["kt1"][hst][2] * d <= 0)
                continue
            passes0 = m0[y, x] + (ptp0 - np.floor(ptp0)) >= np.float32(sc["cmad"]) * p["type"]
            late_reject += bool(passes0 and disp[i] == R.KEEP)
            border_accept += bool(disp[i] == R.OPTIMIZE and (x == w1 - 1 or y == h1 - 1))
    assert seen == {R.KEEP, R.DELETE, R.OPTIMIZE}
    # the two orders of the 10 x 10 example decide the first corner candidate (record 2) differently
    first = []
    for name in ("border-64x48-0", "border-64x48-1"):
        sc = S.build(scenes[name])
        dm = R.make_distance_map(32, 24, sc["krki1"], sc["kt1"], sc["uvd"], sc["seed_host"])
        first.append(R.walk(dm, sc["pts"], sc["krki1"], sc["kt1"], sc["cmad"], sc["newest"])[0][2])
    assert first == [R.OPTIMIZE, R.KEEP]
    assert late_reject > 0 and border_accept > 0 and outside > 0 and behind > 0


def test_dtype_is_the_abi_record():
    assert S.records(1, 0, 0, 0).dtype == L.IMMATURE_DTYPE
