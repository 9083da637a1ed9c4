"""A numpy-float32 restatement of CoarseTracker::makeCoarseDepthL0 (reference
src/frontend/CoarseTracker.cc:357-538), the expected value of ldso_ct_make_reference and
ldso_ct_make_reference_ba.  A helper, not a test file.

The scatter is a sequential Python loop over the contributions, in the order given (the sums of a
pixel depend on it from three contributions on); everything after it is element-wise float32 in the
reference's statement order:

  scatter     u = int(c[0] + 0.5f), v = int(c[1] + 0.5f); weight = sqrtf(float(1e-3 / (double(HdiF)
              + 1e-12))); idepth[u, v] += c[2] * weight; weightSums[u, v] += weight.  A centre
              outside [0, w) x [0, h) -- undefined behaviour in the reference -- is skipped.
  downsample  levels 1..L-1: ((a + b) + c) + d of the undilated level below.
  dilate      once per level, pixels with weight <= 0 from the neighbours with weight > 0 of the
              backup copy: diagonal (+1+w, -1-w, +w-1, -w+1) on levels 0 and 1, axis (+1, -1, +w,
              -w) above; sum / numn and num / numn with float counters.
  normalise   interior pixels [2, w-2) x [2, h-2) in row-major order: weight > 0 -> idepth /=
              weight, emitted unless the colour is not finite or !(idepth > 0).

Only interior pixels are computed after the downsample: the dilation of a border pixel (and the
reference's flat-index row wrap there) is read by nobody, since a filled pixel reads only
neighbours whose backup weight is > 0, which the dilation leaves alone.
"""
import numpy as np

MAX_LEVELS = 6
F = np.float32


# five contributions on one pixel whose weights span 1e-3 ... 1e3 (HdiF = 1e-3 / weight^2)
FIVE_CENTER = np.array([[57.1, 33.2, 0.731], [56.9, 32.8, 1.37], [57.3, 33.4, 0.211], [56.6, 33.0, 2.93],
                        [57.0, 32.6, 0.517]], F)
FIVE_HDI = np.array([1e3, 1e-9, 1e-1, 1e-5, 1e-3 / 3.0], F)


def level_sizes(w, h):
    """ldso_ct_create's rule (GlobalCalib.cc:20-30)."""
    out = [(w, h)]
    while w % 2 == 0 and h % 2 == 0 and w * h > 5000 and len(out) < MAX_LEVELS:
        w, h = w // 2, h // 2
        out.append((w, h))
    return out


def weight_of(hdi):
    with np.errstate(all="ignore"):
        return np.sqrt(F(1e-3 / (np.float64(F(hdi)) + 1e-12)))


def pixel_of(c0, c1, w, h):
    """(u, v) of a centre, or None where the reference would write outside its arrays."""
    tu, tv = F(c0) + F(0.5), F(c1) + F(0.5)
    if not (tu > -1 and tu < w and tv > -1 and tv < h):  # NaN fails too
        return None
    return int(tu), int(tv)  # truncation, as the reference's float -> int


def scatter(w, h, center, hdi):
    """Level 0 of idepth / weightSums: the sequential sums in contribution order."""
    center = np.asarray(center, F).reshape(-1, 3)
    hdi = np.asarray(hdi, F).reshape(-1)
    idepth = np.zeros((h, w), F)
    wsum = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for c, hd in zip(center, hdi):
            px = pixel_of(c[0], c[1], w, h)
            if px is None:
                continue
            u, v = px
            wt = weight_of(hd)
            idepth[v, u] = idepth[v, u] + F(c[2] * wt)
            wsum[v, u] = wsum[v, u] + wt
    return idepth, wsum


def _down(m):
    return ((m[0::2, 0::2] + m[0::2, 1::2]) + m[1::2, 0::2]) + m[1::2, 1::2]


def _emit_level(lvl, I, W, color):
    h, w = I.shape
    if w <= 4 or h <= 4:
        return np.zeros((0, 4), F)
    ys, xs = slice(2, h - 2), slice(2, w - 2)

    def sh(m, dy, dx):
        return m[2 + dy:h - 2 + dy, 2 + dx:w - 2 + dx]

    offs = [(1, 1), (-1, -1), (1, -1), (-1, 1)] if lvl < 2 else [(0, 1), (0, -1), (1, 0), (-1, 0)]  # (dy, dx)
    idv, wt = I[ys, xs].copy(), W[ys, xs].copy()
    s = np.zeros_like(idv)
    num = np.zeros_like(idv)
    numn = np.zeros_like(idv)
    with np.errstate(all="ignore"):
        for dy, dx in offs:
            wn, idn = sh(W, dy, dx), sh(I, dy, dx)
            m = wn > 0
            s = np.where(m, s + idn, s)
            num = np.where(m, num + wn, num)
            numn = np.where(m, numn + F(1), numn)
        fill = (wt <= 0) & (numn > 0)
        idv = np.where(fill, s / numn, idv)
        wt = np.where(fill, num / numn, wt)
        pos = wt > 0
        idv = np.where(pos, idv / wt, idv)
        col = np.asarray(color, F).reshape(h, w)[ys, xs]
        emit = pos & np.isfinite(col) & (idv > 0)
    yy, xx = np.nonzero(emit)  # row-major
    return np.stack([(xx + 2).astype(F), (yy + 2).astype(F), idv[yy, xx], col[yy, xx]], axis=1).astype(F)


def make_coarse_depth(w, h, center, hdi, colors):
    """The clouds of every level, [n][4] = (u, v, idepth, color) float32.
    colors: per level the flat dIp[lvl][:, 0] of the reference keyframe."""
    sizes = level_sizes(w, h)
    assert len(colors) == len(sizes)
    I, W = scatter(w, h, center, hdi)
    out = []
    with np.errstate(all="ignore"):
        for lvl in range(len(sizes)):
            if lvl > 0:
                I, W = _down(I), _down(W)
            assert I.shape == (sizes[lvl][1], sizes[lvl][0])
            out.append(_emit_level(lvl, I, W, colors[lvl]))
    return out


def window_traversal(win):
    """The reference's point order: frames in window order, each frame's points by rank (stable;
    the caller's order without ranks)."""
    host = np.asarray(win.point_host)
    order = []
    for f in range(win.n_frames):
        idx = np.nonzero(host == f)[0]
        if win.point_rank is not None:
            idx = idx[np.argsort(np.asarray(win.point_rank)[idx], kind="stable")]
        order.extend(idx.tolist())
    return order


def window_contributions(win, state, center, hdi, ref_frame):
    """(center [n][3], hdi [n]) of a window's points whose residual to ref_frame is IN (0)."""
    cs, hs = [], []
    begin, tgt = np.asarray(win.point_res_begin), np.asarray(win.res_target)
    for p in window_traversal(win):
        for k in range(begin[p], begin[p + 1]):
            if tgt[k] == ref_frame and state[k] == 0:
                cs.append(center[k])
                hs.append(hdi[p])
    return np.asarray(cs, F).reshape(-1, 3), np.asarray(hs, F).reshape(-1)
