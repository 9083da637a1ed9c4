"""The windows and edits the ldso_ba_edit_window tests share (test_edit_plan on the CPU,
test_edit_parity on the GPU).

Every window here is a selection from one pool: a regular synthetic window of one frame more than
the loaded one, passed through ragged.frontend_window so that residual lists, states, energies and
flags are mixed.  A selection names pool frames, pool points in the caller's order and, per point,
residual items; an edit is a second selection, and frame_src / point_src / res_src follow from the
identities (an entry the loaded selection does not hold is new).  Residuals the pool does not hold
(one to a newly appended frame on every surviving point) are made as the frontend makes them: IN,
energy 0, isNew.

base_sel is the smallest window at which the layout can go wrong (N = 4, about 70 points): the
(host, target) buckets 0->1, 1->0 and 3->0 hold exactly 16, 17 and 1 residuals (k_linearize's chunk
is 16) and hosts 0 and 1 hold exactly 16 and 17 points (k_point_sc's block is 16)."""
import copy
import functools

import numpy as np

import ragged
from ldso_amd import _lib as L
from ldso_amd import synth
from ldso_amd.window import Window

SIZE = dict(width=160, height=120)  # the smallest frame the parity tests use
FRAME_ID0 = 100                     # frame-store id of pool frame f: FRAME_ID0 + f


class Sel:
    """frames: pool frame indices in window order; pts: [(pool point, [residual item])] in caller
    order, a residual item being (key, pool target frame, state, energy, flags)."""

    def __init__(self, frames, pts):
        self.frames = list(frames)
        self.pts = [(int(p), list(items)) for p, items in pts]

    def frame_ids(self):
        return np.array([FRAME_ID0 + f for f in self.frames], np.int64)

    def buckets(self, pool):
        out = {}
        for p, items in self.pts:
            for it in items:
                key = (int(pool.point_host[p]), it[1])
                out[key] = out.get(key, 0) + 1
        return out

    def host_counts(self, pool):
        out = {}
        for p, _ in self.pts:
            out[int(pool.point_host[p])] = out.get(int(pool.point_host[p]), 0) + 1
        return out


@functools.lru_cache(maxsize=None)
def make_pool(n_frames=5, n_points=400, seed=41):
    w = synth.make_window(n_frames=n_frames, n_points=n_points, seed=seed, **SIZE)
    return ragged.frontend_window(w, np.random.default_rng(seed + 1000))


def pool_items(pool, p, frames):
    """The pool's residuals of point p whose target is one of `frames`, in the pool's order."""
    return [(int(k), int(pool.res_target[k]), int(pool.res_state[k]), float(pool.res_energy[k]), int(pool.res_flags[k]))
            for k in range(int(pool.point_res_begin[p]), int(pool.point_res_begin[p + 1])) if int(pool.res_target[k]) in frames]


def fresh_item(p, t):
    """A residual as FullSystem::activatePointsMT / makeKeyFrame insert it."""
    return (("n", int(p), int(t)), int(t), L.RES_IN, 0.0, L.FLAG_NEW)


def full_sel(pool, frames):
    """Every pool point hosted by one of `frames`, with its residuals into them."""
    frames = list(frames)
    return Sel(frames, [(p, pool_items(pool, p, frames)) for p in range(pool.n_points) if int(pool.point_host[p]) in frames])


def base_sel(pool):
    frames = [0, 1, 2, 3]
    targets = lambda p: {int(t) for t in pool.res_target[pool.point_res_begin[p]:pool.point_res_begin[p + 1]]}
    hosted = lambda h: [p for p in range(pool.n_points) if int(pool.point_host[p]) == h]
    pick = {0: [p for p in hosted(0) if 1 in targets(p)][:16], 1: [p for p in hosted(1) if 0 in targets(p)][:17],
            2: hosted(2)[:25], 3: hosted(3)[:12]}
    pts, seen30 = [], False
    for p in sorted(sum(pick.values(), [])):  # caller order: the pool's, the hosts interleaved
        items = pool_items(pool, p, frames)
        if int(pool.point_host[p]) == 3:  # bucket 3 -> 0 keeps a single residual
            kept = []
            for it in items:
                if it[1] == 0:
                    if seen30:
                        continue
                    seen30 = True
                kept.append(it)
            items = kept
        pts.append((p, items))
    s = Sel(frames, pts)
    b, h = s.buckets(pool), s.host_counts(pool)
    assert (b[(0, 1)], b[(1, 0)], b[(3, 0)]) == (16, 17, 1), b
    assert (h[0], h[1]) == (16, 17) and len(pts) == 70, h
    return s


# ---- the edits: loaded selection -> edited selection ---------------------------------------------
def _drop(sel, pool, pred):
    """Without the residuals for which pred(host, target, n-th of its bucket) holds."""
    seen, pts = {}, []
    for p, items in sel.pts:
        kept = []
        for it in items:
            b = (int(pool.point_host[p]), it[1])
            n = seen[b] = seen.get(b, -1) + 1
            if not pred(b[0], b[1], n):
                kept.append(it)
        pts.append((p, kept))
    return Sel(sel.frames, pts)


def edit_drop(pool, sel):
    """(a) residual drops that empty bucket 3 -> 0 and take bucket 1 -> 0 from 17 to 16."""
    out = _drop(sel, pool, lambda h, t, n: (h, t) == (3, 0) or ((h, t) == (1, 0) and n == 5) or ((h, t) == (2, 1) and n % 3 == 0))
    b = out.buckets(pool)
    assert (3, 0) not in b and b[(1, 0)] == 16
    return out


def edit_remove_host(pool, sel, host=2):
    """(b) every point of one host removed."""
    return Sel(sel.frames, [(p, it) for p, it in sel.pts if int(pool.point_host[p]) != host])


def edit_remove_frame(pool, sel, frame):
    """(c) a frame removed with its points and the residuals into it; the later frames shift down."""
    return Sel([f for f in sel.frames if f != frame],
               [(p, [it for it in items if it[1] != frame]) for p, items in sel.pts if int(pool.point_host[p]) != frame])


def edit_append(pool, sel, frame=4):
    """(d) a frame appended with one new residual on every surviving point; it hosts nothing."""
    return Sel(sel.frames + [frame], [(p, items + [fresh_item(p, frame)]) for p, items in sel.pts])


def edit_cycle(pool, sel):
    """(e) the keyframe cycle in one call: frame 0 out, frame 4 in, residuals dropped."""
    out = edit_append(pool, edit_remove_frame(pool, sel, 0))
    return _drop(out, pool, lambda h, t, n: (t != 4 and n % 4 == 1) or (t == 4 and n % 5 == 2))


def edit_insert_points(pool, sel):
    """(f) new points with their residuals: in the middle of host 1's run (17 -> 22 points: a second
    and a shorter third block), at the front and at the end of the caller order."""
    have = {p for p, _ in sel.pts}
    fresh = lambda h, n: [(p, pool_items(pool, p, sel.frames)) for p in range(pool.n_points)
                          if int(pool.point_host[p]) == h and p not in have][:n]
    pts = list(sel.pts)
    run1 = [i for i, (p, _) in enumerate(pts) if int(pool.point_host[p]) == 1]
    mid = run1[8]
    pts[mid:mid] = fresh(1, 5)
    new3 = fresh(3, 3)
    return Sel(sel.frames, new3[:1] + pts + new3[1:] + fresh(0, 1))


def edit_identity(pool, sel):
    """(g)"""
    return Sel(sel.frames, sel.pts)


def edit_no_points(pool, sel):
    """(l) the frames alone: P = R = 0."""
    return Sel(sel.frames, [])


def edit_no_residuals(pool, sel):
    """(m) every point kept, every residual dropped: P > 0, R = 0."""
    return Sel(sel.frames, [(p, []) for p, _ in sel.pts])


# windows without residuals: a pass runs on them, ldso_ba_iterate has nothing to solve for
DEGENERATE = {
    "l_no_points": edit_no_points,
    "m_no_residuals": edit_no_residuals,
}


EDITS = {
    "a_drop": edit_drop,
    "b_remove_host": edit_remove_host,
    "c_remove_frame0": lambda pool, sel: edit_remove_frame(pool, sel, 0),
    "c_remove_frame2": lambda pool, sel: edit_remove_frame(pool, sel, 2),
    "d_append": edit_append,
    "e_cycle": edit_cycle,
    "f_insert_points": edit_insert_points,
    "g_identity": edit_identity,
}


# ---- selections as windows ------------------------------------------------------------------------
def window_of(pool, sel, before=None, rank=False):
    """The Window of a selection.  With `before` (the loaded selection) also (frame_src, point_src,
    res_src), and the carried entries' point_data / res_state / res_energy / res_flags are poisoned
    (NaN, OUTLIER, all flag bits): the edit must not read them."""
    remap = {f: i for i, f in enumerate(sel.frames)}
    host, data, begin, tgt, st, en, fl, keys = [], [], [0], [], [], [], [], []
    for p, items in sel.pts:
        host.append(remap[int(pool.point_host[p])])
        data.append(pool.point_data[p])
        for key, t, s, e, f in items:
            tgt.append(remap[t])
            st.append(s)
            en.append(e)
            fl.append(f)
            keys.append(key)
        begin.append(len(tgt))
    w = Window(n_frames=len(sel.frames), width=pool.width, height=pool.height, calib=pool.calib.copy(),
               frames=pool.frames[sel.frames].copy(), dI=np.ascontiguousarray(pool.dI[sel.frames]),
               frame_energy_th=pool.frame_energy_th[sel.frames].copy(), point_host=np.array(host, np.int32),
               point_data=np.array(data, np.float32).reshape(-1, L.POINT_STRIDE), point_res_begin=np.array(begin, np.int32),
               res_target=np.array(tgt, np.int32), res_state=np.array(st, np.int8), res_energy=np.array(en, np.float32),
               res_flags=np.array(fl, np.uint8), settings=pool.settings)
    if rank:  # a fixed permutation of the pool's points, restricted: carried points keep their order
        perm = np.random.default_rng(77).permutation(pool.n_points)
        w.point_rank = np.array([perm[p] for p, _ in sel.pts], np.int32)
    w.refresh_frame_terms()
    if before is None:
        return w
    bfr = {f: i for i, f in enumerate(before.frames)}
    bpt = {p: i for i, (p, _) in enumerate(before.pts)}
    bres = {it[0]: i for i, it in enumerate(it for _, items in before.pts for it in items)}
    frame_src = np.array([bfr.get(f, -1) for f in sel.frames], np.int32)
    point_src = np.array([bpt.get(p, -1) for p, _ in sel.pts], np.int32)
    res_src = np.array([bres.get(k, -1) for k in keys], np.int32)
    w.point_data[point_src >= 0] = np.nan
    w.res_state[res_src >= 0] = L.RES_OUTLIER
    w.res_energy[res_src >= 0] = np.nan
    w.res_flags[res_src >= 0] = 0xFF
    return w, (frame_src, point_src, res_src)


def filled(after, srcs, state, energy, flags, point_data):
    """after': `after` with its carried entries filled in from the loaded window's read-back (caller
    order of the loaded window)."""
    _, point_src, res_src = srcs
    w = copy.copy(after)
    w._keep = []
    for k in ("point_data", "res_state", "res_energy", "res_flags"):
        setattr(w, k, getattr(after, k).copy())
    cp, cr = point_src >= 0, res_src >= 0
    w.point_data[cp] = point_data[point_src[cp]]
    w.res_state[cr] = state[res_src[cr]]
    w.res_energy[cr] = energy[res_src[cr]]
    w.res_flags[cr] = flags[res_src[cr]]
    return w
