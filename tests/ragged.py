"""Windows as LDSO's frontend leaves them, made from synth.make_window's regular ones.

synth.make_window gives every point N-1 residuals in ascending target order, all IN with energy 0
and flag NEW, and lets every frame host points and be a target.  The frontend never hands over such
a window: points hold between 0 and N-1 residuals in the order they were added (a point that lost
all of them stays in the frame until removeOutliers), the newest keyframe hosts no active point, the
oldest is often nobody's target, and the residual states, energies and flags are what the previous
keyframe cycle left.  frontend_window() applies all of that, deterministically from its rng; the
cases the ragged tests share (edge windows, the batch, the randomised sweep) are defined here too,
so the CPU tests that show the cases are well posed and the GPU tests run the same windows.
"""
import numpy as np

from ldso_amd import _lib as L
from ldso_amd import synth

IN, OOB, OUTLIER = L.RES_IN, L.RES_OOB, L.RES_OUTLIER


def _keep_points(w, points):
    """w restricted to `points` (ascending caller indices) with their residual runs."""
    from ldso_amd import dist as ldist

    return ldist.subset_window(w, np.asarray(points, np.int64))


def frontend_window(w, rng, *, empty_newest=False, untargeted=None, rank=False, all_empty=False, one_each=False,
                    host_count=None):
    """A copy of the regular window `w` as the frontend leaves one.

    Residual lists: a point keeps 0 residuals (8 % of the points), 1 (17 %), all N-1 (25 %) or a
    uniform count in [1, N-1] (the rest); the kept ones are a random subset in shuffled target order.
    Initial state, only what the reference can reach: 10 % OOB, 10 % OUTLIER, the rest IN; state_energy
    U[0, 400) on 60 % and 0 on the rest, never 0 on an OOB residual (its stale energy is what
    linearize returns at once); isNew on 40 %; isActiveAndIsGoodNEW on half of the IN residuals only
    (applyRes clears it whenever a residual leaves IN, Residuals.h:70-88).

    empty_newest: no point is hosted by frame N-1; untargeted=f: no residual targets frame f;
    rank: a random permutation as point_rank; all_empty: every point keeps 0 residuals;
    one_each: every point keeps exactly 1; host_count=(h, n): frame h hosts exactly n points."""
    N = w.n_frames
    keep = np.ones(w.n_points, bool)
    if empty_newest:
        keep &= w.point_host != N - 1
    if host_count is not None:
        h, n = host_count
        mine = np.flatnonzero(keep & (w.point_host == h))
        assert len(mine) >= n, f"frame {h} hosts {len(mine)} points, {n} wanted"
        keep[mine[n:]] = False
    o = _keep_points(w, np.flatnonzero(keep))
    P = o.n_points
    begin, tgt = [0], []
    u = rng.random(P)
    for p in range(P):
        cand = o.res_target[o.point_res_begin[p]:o.point_res_begin[p + 1]]
        if untargeted is not None:
            cand = cand[cand != untargeted]
        if all_empty:
            k = 0
        elif one_each:
            k = 1
        elif u[p] < 0.08:
            k = 0
        elif u[p] < 0.25:
            k = 1
        elif u[p] < 0.50:
            k = N - 1
        else:
            k = int(rng.integers(1, N)) if N > 1 else 0
        k = min(k, len(cand))
        tgt.append(rng.permutation(cand)[:k])
        begin.append(begin[-1] + k)
    R = begin[-1]
    o.point_res_begin = np.asarray(begin, np.int32)
    o.res_target = (np.concatenate(tgt) if P else np.zeros(0)).astype(np.int32)
    s = rng.random(R)
    o.res_state = np.where(s < 0.1, OOB, np.where(s < 0.2, OUTLIER, IN)).astype(np.int8)
    e = np.where(rng.random(R) < 0.6, rng.uniform(0.0, 400.0, R), 0.0).astype(np.float32)
    stale = np.maximum(rng.uniform(0.0, 400.0, R).astype(np.float32), np.float32(2.0 ** -10))
    o.res_energy = np.where((o.res_state == OOB) & (e == 0), stale, e).astype(np.float32)
    new = rng.random(R) < 0.4
    active = (rng.random(R) < 0.5) & (o.res_state == IN)
    o.res_flags = (np.where(new, L.FLAG_NEW, 0) | np.where(active, L.FLAG_ACTIVE, 0)).astype(np.uint8)
    o.point_rank = rng.permutation(P).astype(np.int32) if rank else None
    o.frame_energy_th = w.frame_energy_th.copy()
    o.settings = w.settings
    o._keep = []
    return o.refresh_frame_terms()


def clone(w):
    """An independent copy of the window's mutable state (the oracle and the context each take one)."""
    o = w.copy_state()
    for k in ("point_host", "point_res_begin", "res_target"):
        setattr(o, k, getattr(w, k).copy())
    return o


def properties(w):
    """What a ragged case is named for, counted on the window itself."""
    N = w.n_frames
    n_res = np.diff(w.point_res_begin)
    shuffled = sum(1 for p in range(w.n_points)
                   if np.any(np.diff(w.res_target[w.point_res_begin[p]:w.point_res_begin[p + 1]]) < 0))
    full_shuffled = sum(1 for p in range(w.n_points) if n_res[p] == N - 1 and N > 2
                        and np.any(np.diff(w.res_target[w.point_res_begin[p]:w.point_res_begin[p + 1]]) < 0))
    return dict(
        zero_res_points=int(np.sum(n_res == 0)), one_res_points=int(np.sum(n_res == 1)),
        shuffled_points=int(shuffled), full_shuffled_points=int(full_shuffled),
        stale_oob=int(np.sum((w.res_state == OOB) & (w.res_energy != 0))),
        bad_active=int(np.sum((w.res_state != IN) & ((w.res_flags & L.FLAG_ACTIVE) != 0))),
        host_counts=np.bincount(w.point_host, minlength=N).tolist(),
        target_counts=np.bincount(w.res_target, minlength=N).tolist(),
        max_target=int(w.res_target.max()) if w.n_residuals else -1)


# ---- the deterministic edge windows (all 160 x 120) ---------------------------------------------
# cfg: synth.make_window's arguments; opts: frontend_window's; seed: the transform's rng;
# want: properties the case is there for, as lower bounds on properties()'s counts
_S = dict(width=160, height=120)
EDGE_CASES = {
    "N2P40": dict(cfg=dict(n_frames=2, n_points=40, seed=301, **_S), opts={}, seed=1,
                  want=dict(zero_res_points=1, one_res_points=20, stale_oob=1)),
    "N3_one_each": dict(cfg=dict(n_frames=3, n_points=90, seed=302, **_S), opts=dict(one_each=True), seed=2,
                        want=dict(one_res_points=90, stale_oob=1)),
    "N7_holes_rank": dict(cfg=dict(n_frames=7, n_points=150, seed=303, edge_frac=0.2, **_S),
                          opts=dict(empty_newest=True, untargeted=0, rank=True), seed=3,
                          want=dict(zero_res_points=1, shuffled_points=10, stale_oob=1)),
    "N8P200": dict(cfg=dict(n_frames=8, n_points=200, seed=304, motion="forward", **_S), opts={}, seed=4,
                   want=dict(zero_res_points=1, shuffled_points=10, stale_oob=1)),
    "N11P200": dict(cfg=dict(n_frames=11, n_points=200, seed=305, outlier_frac=0.15, **_S), opts={}, seed=5,
                    want=dict(zero_res_points=1, shuffled_points=10, stale_oob=1)),
    "N13P120": dict(cfg=dict(n_frames=13, n_points=120, seed=306, plane_depth=30.0, **_S), opts={}, seed=6,
                    want=dict(zero_res_points=1, one_res_points=10, full_shuffled_points=10, stale_oob=1)),
    "N16P120": dict(cfg=dict(n_frames=16, n_points=120, seed=307, plane_depth=37.5, **_S), opts={}, seed=7,
                    want=dict(zero_res_points=1, one_res_points=10, full_shuffled_points=10, stale_oob=1, max_target=15)),
    # frame 1 hosts one point more than a k_point_sc block of 16 / of 64 holds, and a single point
    "host1_1": dict(cfg=dict(n_frames=4, n_points=320, seed=308, **_S), opts=dict(host_count=(1, 1)), seed=8,
                    want=dict(zero_res_points=1, shuffled_points=10, stale_oob=1)),
    "host1_17": dict(cfg=dict(n_frames=4, n_points=320, seed=308, **_S), opts=dict(host_count=(1, 17)), seed=9,
                     want=dict(zero_res_points=1, shuffled_points=10, stale_oob=1)),
    "host1_65": dict(cfg=dict(n_frames=4, n_points=320, seed=308, **_S), opts=dict(host_count=(1, 65)), seed=10,
                     want=dict(zero_res_points=1, shuffled_points=10, stale_oob=1)),
}
SOLVE_CASES = ["N3_one_each", "N7_holes_rank", "N8P200", "N11P200"]  # windows the device solve takes (<= 11 keyframes)


def edge_window(name, settings=None):
    case = EDGE_CASES[name]
    w = synth.make_window(**case["cfg"])
    w.settings = settings
    return frontend_window(w, np.random.default_rng(12000 + case["seed"]), **case["opts"])


BATCH = [dict(cfg=dict(n_frames=5, n_points=120, seed=311, **_S), opts={}),
         dict(cfg=dict(n_frames=7, n_points=60, seed=312, **_S), opts=dict(all_empty=True)),
         dict(cfg=dict(n_frames=3, n_points=80, seed=313, edge_frac=0.2, **_S), opts={})]


def batch_windows(cases=BATCH, seed=12100):
    """[N=5 ragged, N=7 with P > 0 and R = 0, N=3 ragged]: item_base / res_base after an empty range."""
    return [frontend_window(synth.make_window(**c["cfg"]), np.random.default_rng(seed + i), **c["opts"])
            for i, c in enumerate(cases)]


# ---- the randomised sweep -------------------------------------------------------------------------
N_FUZZ = 16


def fuzz_draw(case):
    """test_fuzz_parity.draw(case) (window count, sizes, N, P, camera, motion, chunk, layout, affine
    modes) plus frontend_window's options per window from a generator of their own."""
    from test_fuzz_parity import draw

    wins, chunk, layout, aff = draw(case)
    rng = np.random.default_rng(13000 + case)
    opts = []
    for c in wins:
        o = dict(empty_newest=bool(rng.random() < 0.4), rank=bool(rng.random() < 0.4))
        if rng.random() < 0.4:
            o["untargeted"] = 0 if rng.random() < 0.7 else int(rng.integers(c["n_frames"]))
        opts.append(o)
    return wins, opts, chunk, layout, aff


def fuzz_windows(case, settings=None):
    wins, opts, chunk, layout, aff = fuzz_draw(case)
    out = []
    for i, (c, o) in enumerate(zip(wins, opts)):
        w = synth.make_window(**c)
        w.settings = settings
        out.append(frontend_window(w, np.random.default_rng([13000 + case, i]), **o))
    return out


def expected_properties(w, opts):
    """Lower bounds that a draw of this size must meet (far below the expected counts: 8 % of the
    points without residuals, about half with a shuffled list, 10 % of the residuals OOB); a draw
    of a few points promises nothing.  check_properties adds the options' own."""
    N, P = w.n_frames, w.n_points
    want = {}
    if P >= 100 and N >= 3 and not opts.get("all_empty") and not opts.get("one_each"):
        want = dict(zero_res_points=1, shuffled_points=max(1, P // 50), stale_oob=1)
    return want


def check_properties(w, opts, want):
    """Assert the window has what its case is named for; returns properties(w)."""
    pr = properties(w)
    N = w.n_frames
    assert pr["bad_active"] == 0, "an OOB or OUTLIER residual with isActiveAndIsGoodNEW is unreachable"
    for k, v in want.items():
        assert pr[k] >= v, (k, pr[k], v)
    if opts.get("empty_newest"):
        assert pr["host_counts"][N - 1] == 0
    if opts.get("untargeted") is not None:
        assert pr["target_counts"][opts["untargeted"]] == 0
    if opts.get("all_empty"):
        assert w.n_points > 0 and w.n_residuals == 0
    if opts.get("one_each"):
        assert pr["one_res_points"] == w.n_points
    if opts.get("host_count"):
        h, n = opts["host_count"]
        assert pr["host_counts"][h] == n
    if opts.get("rank"):
        assert sorted(w.point_rank.tolist()) == list(range(w.n_points))
    return pr
