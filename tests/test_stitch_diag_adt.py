"""The host stitch's two treatments of the target adjoints: ad_target blocks that are all diagonal
(setAdjointsF's) are applied as row / column scalings, any other ad_target as dense 8x8 products
(also forced by LDSO_BA_STITCH_DENSE_ADT=1).

  * On diagonal adjoints the two paths give the same numbers: one context of ragged windows
    (2, 3, 7 and 11 keyframes, hosts without points), each path under both LDSO_BA_HS_SPLIT settings.
  * A non-diagonal ad_target takes the dense products: the system matches the oracle, which reads
    the same array, and differs from that of the array's diagonal alone.
  * The choice follows the data on the device: after ldso_ba_update swaps diagonal adjoints for
    non-diagonal ones, a replayed ldso_ba_optimize graph equals a fresh load of the latter.
  * The host's diagonality test (ldso_ba_adjoints_diagonal) on the CPU: exact zeros only.
"""
import numpy as np
import pytest

from ldso_amd import BAContext, synth
from ldso_amd import _lib as L

SMALL = dict(width=160, height=120)
KEYS = ("HA", "bA", "Hsc", "bsc")


def without_hosts(w, hosts):
    """w without the points (and residuals) hosted by the frames `hosts`"""
    return synth.permute_points(w, np.flatnonzero(~np.isin(w.point_host, hosts)))


def ragged_windows():
    """2, 3, 7 and 11 keyframes, a few dozen points each; frame 1 of the 3-keyframe window, frames 0 and
    4 of the 7-keyframe one and the newest frame of the 11-keyframe one host no points"""
    ws = [synth.make_window(n_frames=n, n_points=p, seed=300 + n, **SMALL) for n, p in ((2, 24), (3, 30), (7, 63), (11, 77))]
    ws[1], ws[2], ws[3] = without_hosts(ws[1], [1]), without_hosts(ws[2], [0, 4]), without_hosts(ws[3], [10])
    for w, empty in zip(ws[1:], ([1], [0, 4], [10])):
        assert w.n_points >= 12 and not np.isin(w.point_host, empty).any()
    return ws


def one_pass(ws):
    c = BAContext(0).load(ws)
    c.linearize(fix=False, accumulate=True)
    out = [dict(c.system(i), energy=c.energy(i)) for i in range(len(ws))]
    c.close()
    return out


@pytest.mark.gpu
def test_dense_and_diagonal_paths_give_the_same_numbers(built, monkeypatch):
    runs = {}
    for dense in ("1", "0"):
        monkeypatch.setenv("LDSO_BA_STITCH_DENSE_ADT", dense)
        for split in ("0", "1"):
            monkeypatch.setenv("LDSO_BA_HS_SPLIT", split)
            runs[dense, split] = one_pass(ragged_windows())
    ref = runs["1", "0"]
    assert all(np.abs(s[k]).max() > 0 for s in ref for k in KEYS)  # a pass ran: nothing compares empty arrays
    for key, run in runs.items():
        for i, (a, b) in enumerate(zip(ref, run)):
            for k in KEYS + ("energy",):
                # numeric equality: +0 and -0 compare equal
                assert np.array_equal(a[k], b[k]), (key, i, k, int((a[k] != b[k]).sum()))


ND_CFG = dict(n_frames=5, n_points=200, seed=311, **SMALL)


def nondiagonal_window(cfg=ND_CFG, entry=1e-3, diagonal_only=False):
    """cfg's window with ad_target[pair (h = 1, t = 3)][0][1] = entry (diagonal_only: left at zero)"""
    w = synth.make_window(**cfg).refresh_frame_terms()
    lib = L.lib()
    assert lib.ldso_ba_adjoints_diagonal(w.n_frames, L.ptr(w.ad_target, L.f64p)) == 1
    if not diagonal_only:
        w.ad_target[1 + w.n_frames * 3, 0 * 8 + 1] = entry
        assert lib.ldso_ba_adjoints_diagonal(w.n_frames, L.ptr(w.ad_target, L.f64p)) == 0
    return w


@pytest.mark.gpu
def test_nondiagonal_adjoints_take_the_dense_products(built):
    import oracle
    import test_gpu_parity as gp

    c = BAContext(0).load([nondiagonal_window()])
    c.linearize(fix=False, accumulate=True)
    ow = oracle.OracleWindow(nondiagonal_window(), threads=0)
    e_cpu, s_cpu = ow.iteration()
    s_nd = gp.compare_pass(c, ow, 0, e_cpu, s_cpu)  # the blocks within gp.BLOCK_TOL of the oracle's
    c.close()
    # what the scalings would give: the system of the diagonal alone.  The off-diagonal entry moved
    # host 1's contribution, so the dense products ran
    c = BAContext(0).load([nondiagonal_window(diagonal_only=True)])
    c.linearize(fix=False, accumulate=True)
    s_d = c.system(0)
    c.close()
    assert not np.array_equal(s_nd["HA"], s_d["HA"]) and not np.array_equal(s_nd["Hsc"], s_d["Hsc"])
    # ... and moved it toward the oracle's: the entry's effect on a block (some 1e-4 of its norm) is
    # far above the two sides' rounding (some 1e-7)
    N = ND_CFG["n_frames"]
    assert gp.block_errors(s_nd["Hsc"], s_cpu["Hsc"], N) < 0.1 * gp.block_errors(s_d["Hsc"], s_cpu["Hsc"], N)


@pytest.mark.gpu
def test_update_to_nondiagonal_adjoints_reaches_a_captured_graph(built):
    w_d, w_nd = nondiagonal_window(diagonal_only=True), nondiagonal_window()
    ns = [w_d.nullspaces()]
    a = BAContext(0).load([w_d])
    first = a.optimize(3, nullspaces=ns)
    a.optimize(3, nullspaces=ns)  # the second call captures the graph, on diagonal adjoints
    # the window as loaded, but for the adjoints: frame terms and point records (update), residual states
    a.update(0, w_nd)
    a.update_residuals(0, w_nd.res_state, w_nd.res_energy, w_nd.res_energy, w_nd.res_flags)
    replayed = a.optimize(3, nullspaces=ns)
    a.close()
    b = BAContext(0).load([nondiagonal_window()])
    fresh = b.optimize(3, nullspaces=ns)
    b.close()
    for x, y in zip(replayed, fresh):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    assert not np.array_equal(np.asarray(first[1]["state"]), np.asarray(fresh[1]["state"]))  # the entry matters


def test_host_diagonality_test_is_exact(built):
    lib = L.lib()
    N = 3
    w = synth.make_window(n_frames=N, n_points=10, seed=1, **SMALL).refresh_frame_terms()

    def diag(ad):
        return lib.ldso_ba_adjoints_diagonal(N, L.ptr(np.ascontiguousarray(ad, np.float64), L.f64p))

    assert diag(w.ad_target) == 1 and diag(w.ad_host) == 0  # setAdjointsF's: AT diagonal, AH -Adj^T
    assert diag(np.zeros((N * N, 64))) == 1
    for block, entry in ((0, 1), (4, 8), (N * N - 1, 62)):  # first and last off-diagonal entries, a middle block
        for value, expect in ((0.0, 1), (-0.0, 1), (5e-324, 0), (-5e-324, 0), (1e-3, 0), (np.nan, 0), (np.inf, 0)):
            ad = w.ad_target.copy()
            ad[block, entry] = value
            assert diag(ad) == expect, (block, entry, value)
    ad = w.ad_target.copy()
    ad[:, ::9] = [0.0, -0.0, 5e-324, np.nan, np.inf, 1.0, -1.0, 2.0]  # the diagonal itself is free
    assert diag(ad) == 1
    assert lib.ldso_ba_adjoints_diagonal(0, L.ptr(w.ad_target, L.f64p)) < 0
    assert lib.ldso_ba_adjoints_diagonal(N, L.ptr(None, L.f64p)) < 0
