"""Pins tests/loop_ref.py, the restatement the GPU tests of the loop closer's matching compare with, against
independent formulations, and shows that every case family the GPU tests rely on really occurs in the
generated inputs (counts asserted, so that no case passes vacuously).  No GPU."""
import functools

import numpy as np

import loop_ref as R

F = np.float32


def popcount_matrix(f1, f2):
    a = np.unpackbits(f1["descriptor"], axis=1).astype(np.int32)
    b = np.unpackbits(f2["descriptor"], axis=1).astype(np.int32)
    return a @ (1 - b).T + (1 - a) @ b.T


def test_descriptor_distance_against_unpackbits():
    rng = np.random.default_rng(0)
    d = rng.integers(0, 256, (40, 32)).astype(np.uint8)
    d[1] = d[0]
    d[2] = 255 - d[0]
    fr = np.zeros(40, R.FEATURE_DTYPE)
    fr["descriptor"] = d
    ints = R.as_ints(fr)
    for i in range(40):
        for j in range(40):
            want = int(np.unpackbits(d[i] ^ d[j]).sum())
            assert R.descriptor_distance(d[i], d[j]) == want == R.distance(ints[i], ints[j])
    assert R.descriptor_distance(d[0], d[1]) == 0 and R.descriptor_distance(d[0], d[2]) == 256
    assert R.descriptor_distance(R.flip_bits(d[5], 49, rng), d[5]) == 49


@functools.lru_cache(maxsize=None)
def brute(n1, n2):
    f1, f2 = R.brute_case(n1, n2)
    details = []
    m = R.search_brute_force(f1, f2, R.TH_LOW, details)
    return f1, f2, m, details


def test_brute_force_against_argmin_of_the_distance_matrix():
    ties = 0
    planted = set()
    for n1, n2 in R.BRUTE_SIZES:
        f1, f2, m, details = brute(n1, n2)
        c1, c2 = np.flatnonzero(f1["is_corner"]), np.flatnonzero(f2["is_corner"])
        assert (c1.size, c2.size) == (n1, n2) and len(f1) > n1 and len(f2) > n2
        assert [d[0] for d in details] == list(c1)
        if n2 == 0:
            assert m.size == 0 and all(d[1:] == (-1, 9999) for d in details)
            continue
        M = popcount_matrix(f1[c1], f2[c2])
        j = M.argmin(axis=1)  # numpy's argmin returns the first index among equal minima
        best = M[np.arange(n1), j]
        assert [(d[1], d[2]) for d in details] == list(zip(c2[j], best))
        keep = best < R.TH_LOW
        assert np.array_equal(m["index1"], c1[keep]) and np.array_equal(m["index2"], c2[j][keep])
        assert np.array_equal(m["dist"], best[keep])
        ties += int(((M == best[:, None]).sum(axis=1) > 1).sum())
        planted |= set(best[:3]) if n1 >= 4 and n2 >= 8 else set()
    assert ties >= 4  # every planted case holds two
    assert {R.TH_LOW - 1, R.TH_LOW, R.TH_LOW + 1} <= planted
    # kf1 == kf2: every corner finds itself at distance 0 (or an equal one before it)
    f1 = brute(200, 333)[0]
    m = R.search_brute_force(f1, f1, R.TH_LOW)
    assert m.size == 200 and (m["dist"] == 0).all() and (m["index2"] <= m["index1"]).all()


def test_bow_against_a_sort_of_each_nodes_distances():
    f1, b1, f2, b2 = R.bow_case()
    details = []
    m = R.search_by_bow(f1, b1, f2, b2, R.TH_LOW, R.NN_RATIO, details)
    shared = sorted(set(b1[0]) & set(b2[0]))
    assert shared == [13, 23, 53, 93] and set(b1[0]) - set(b2[0]) and set(b2[0]) - set(b1[0])
    assert max(len(l) for l in b2[1]) > 64
    want, visited, at_equality, accepted_edges = [], [], 0, set()
    for node in shared:  # the merge walk visits the intersection, ascending
        l1, l2 = b1[1][b1[0].index(node)], b2[1][b2[0].index(node)]
        M = popcount_matrix(f1[l1], f2[l2])
        for r, i1 in enumerate(l1):
            order = np.argsort(M[r], kind="stable")
            best, second = int(M[r][order[0]]), int(M[r][order[1]])
            visited.append((i1, best, second))
            if best <= R.TH_LOW:
                if float(best) == R.NN_RATIO * second:
                    at_equality += 1
                if F(best) < F(R.NN_RATIO) * F(second):
                    want.append((i1, l2[order[0]], best))
                    accepted_edges.add(best)
    assert details == visited
    assert [tuple(x) for x in m] == want and len(want) >= 20
    assert at_equality == 2
    assert (45, 60) in [v[1:] for v in visited] and (3, 4) in [v[1:] for v in visited]
    assert (44, 60) in [v[1:] for v in visited] and (10, 10) in [v[1:] for v in visited]
    assert R.TH_LOW in accepted_edges and R.TH_LOW + 1 in {v[1] for v in visited}
    # an empty intersection: nothing is visited
    g1, c1, g2, c2 = R.bow_case(disjoint=True)
    det = []
    assert R.search_by_bow(g1, c1, g2, c2, R.TH_LOW, R.NN_RATIO, det).size == 0 and det == []


def test_idepth_map_keeps_the_last_writer():
    c = np.array([[3.2, 4.4, 0.5], [2.6, 3.7, 0.7], [-0.7, 0.2, 0.9], [-1.5, 0.2, 1.0], [15.5, 0.2, 1.0],
                  [np.nan, 1.0, 1.0], [3.4, 4.0, 0.0]], F)
    m = R.make_idepth_map(16, 12, c)
    assert m[4, 3] == F(0.0) and m[0, 0] == F(0.9) and np.count_nonzero(m) == 1
    m2 = R.make_idepth_map(16, 12, c[[6, 1, 0]])
    assert m2[4, 3] == F(0.5)


def dense_projection(cur, cand, idepth_map, calib, scr, window_size, th_high):
    """every corner within the radius, then the minimum of (dist, ix, iy, index)"""
    h, w = idepth_map.shape
    gw, gh = w // R.GRID, h // R.GRID
    cc = np.flatnonzero(cur["is_corner"])
    M = popcount_matrix(cand, cur[cc])
    r = F(window_size)
    out = []
    for i in np.flatnonzero(cand["usable"]):
        _, u, v, _ = R.project_candidate(cand[i], calib, scr)
        if not (np.isfinite(u) and np.isfinite(v)):
            continue
        keys = []
        for n, k in enumerate(cc):
            fu, fv = cur["u"][k], cur["v"][k]
            if not ((fu - u) * (fu - u) + (fv - v) * (fv - v)) < r * r:
                continue
            if not float(np.abs(cur["angle"][k] - cand["angle"][i])) < 0.2:
                continue
            if idepth_map[int(fv + F(0.5)), int(fu + F(0.5))] == 0:
                continue
            keys.append((int(M[i, n]), int(fu) // R.GRID, int(fv) // R.GRID, int(k)))
        if keys and min(keys)[0] <= th_high:
            out.append((int(i), min(keys)[3], min(keys)[0]))
    return out


@functools.lru_cache(maxsize=None)
def projection(w, h, sim, window):
    cur, cand, centers, calib, scr = R.projection_case(w, h, sim)
    idm = R.make_idepth_map(w, h, centers)
    stats = {}
    got = R.search_by_projection(cur, cand, idm, calib, scr, window, 50, stats)
    return cur, cand, idm, calib, scr, got, stats


def test_projection_against_a_dense_evaluation_and_the_case_families():
    total = {}
    for w, h in R.PROJECTION_SIZES:
        for sim in R.SIMILARITIES:
            for window in (5.0, 25.0):
                cur, cand, idm, calib, scr, got, stats = projection(w, h, sim, window)
                assert abs(int(cur["is_corner"].sum()) - 150) <= 1
                want = dense_projection(cur, cand, idm, calib, scr, window, 50)
                assert [(g["index_cand"], g["index_cur"], g["dist"]) for g in got] == want, (w, h, sim, window)
                if sim != "to_zero":
                    assert len(want) >= 30
                    assert stats["multi_cell_tie"] >= 1
                    assert min(stats[k] for k in ("xmin", "xmax", "ymin", "ymax")) >= 1, stats
                    assert stats["hole"] >= 1 and stats["angle_in"] >= 30 and stats["angle_out"] >= 30
                else:
                    assert stats["pc2_zero"] >= 30 and stats["behind"] >= 30
                for k, v in stats.items():
                    total[k] = total.get(k, 0) + v
                # the outputs are the reference's expressions of the partner
                for g in got[:5]:
                    f = cur[g["index_cur"]]
                    idepth = idm[int(f["v"] + F(0.5)), int(f["u"] + F(0.5))]
                    assert idepth != 0 and g["pixel"][0] == f["u"] and g["pixel"][1] == f["v"]
                    assert g["p_curr"][2] == np.float64(F(1) / idepth)
                    assert g["p_ref"][2] == 1.0 / np.float64(cand["inv_d"][g["index_cand"]])
    assert all(total[k] >= 1 for k in ("xmin", "xmax", "ymin", "ymax", "hole", "multi_cell_tie", "behind", "pc2_zero"))
    # the angle gate compares a float difference in double: a float just under 0.2f passes, 0.2f itself
    # (above the double 0.2) does not
    assert float(F(0.2)) > 0.2 and float(np.nextafter(F(0.2), F(0))) < 0.2
    # both maps of the several-centres-on-one-pixel kind occur
    _, _, centers, _, _ = R.projection_case(160, 120, "identity")
    pix = [(int(c[0] + F(0.5)), int(c[1] + F(0.5))) for c in centers if np.isfinite(c[0]) and c[0] > 0]
    assert len(pix) - len(set(pix)) >= 10


def test_get_feature_in_grid_truncates_toward_zero():
    fr = np.zeros(2, R.FEATURE_DTYPE)
    fr["u"], fr["v"], fr["is_corner"] = [1, 21], [1, 1], 1
    grid = R.set_feature_grid(fr, 60, 40)
    assert grid[0] == [0] and grid[1] == [1]
    # x - radius = -25: int(-25) / 20 = -1 in C (floor division would give -2); either way max(0, .) = 0
    assert [k for k, _, _ in R.get_feature_in_grid(fr, grid, 60, 40, 0.0, 1.0, 25.0)[0]] == [0, 1]
    # x + radius = -15: int(-15) / 20 = 0 in C, so the search goes on where floor division would return
    assert R.get_feature_in_grid(fr, grid, 60, 40, -20.0, 1.0, 5.0) == ([], None)
    assert R.get_feature_in_grid(fr, grid, 60, 40, -30.0, 1.0, 5.0) == ([], "xmax")
    assert R.get_feature_in_grid(fr, grid, 60, 40, float("nan"), 1.0, 5.0) == ([], "xmax")
    assert R.get_feature_in_grid(fr, grid, 60, 40, 70.0, 1.0, 5.0) == ([], "xmin")
    assert R.to_int(float("inf")) == R.INT_MIN and R.to_int(-3.9) == -3
    bad = fr.copy()
    bad["u"][1] = 60  # w / 20 = 3 cells: int(60 / 20) = 3 is outside
    assert R.set_feature_grid(bad, 60, 40) is None
    bad["u"][1] = -1
    assert R.set_feature_grid(bad, 60, 40) is None
