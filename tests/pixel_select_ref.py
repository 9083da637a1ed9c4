"""A numpy-float32 restatement of PixelSelector::makeHists / select / makeMaps (reference
src/frontend/PixelSelector2.cc:27-316) and of FullSystem::makeNewTraces' walk for
setting_pointSelection == 0 (src/frontend/FullSystem.cc:1439-1461): the expected value of
ldso_ct_select_pixels and ldso_ct_make_new_traces.  A helper, not a test file.

select() is the sequential state machine it is in the reference -- three nested levels of cells
(pot, 2 pot, 4 pot) clipped at the right and bottom edges, one running best value and best index
per level, the -2 sentinels, strict comparisons, the direction drawn from randomPattern[n2] when
a block of any level starts -- as a Python loop over the pixels in that order.  Only what does not
depend on the traversal is computed ahead as float32 arrays in the reference's statement order:
the three threshold tests of a pixel and |dx * d.x + dy * d.y| for the 16 directions.

Rules that are this project's and not the reference's:
  * thsSmoothed is looked up at (x >> 5) + (y >> 5) * (w // 32).  Entries past the (w // 32) x
    (h // 32) grid that makeHists fills are 0 (uninitialised memory in the reference); the strip
    right of the last whole block therefore reads the first block of the next block row, and the
    bottom strip reads 0.
  * a potential above 32767 is 32767 (the reference's float -> int conversion is undefined there).
"""
import numpy as np

import oracle

F = np.float32
MAX_POTENTIAL = 32767
DEFAULTS = dict(density=1500.0, recursions=1, th_factor=1.0, min_grad_hist_cut=0.5, min_grad_hist_add=7.0,
                grad_downweight_per_level=0.75, select_direction_distribution=1)
# PixelSelector2.cc:186-202
DIRECTIONS = np.array([(0, 1.0000), (0.3827, 0.9239), (0.1951, 0.9808), (0.9239, 0.3827), (0.7071, 0.7071),
                       (0.3827, -0.9239), (0.8315, 0.5556), (0.8315, -0.5556), (0.5556, -0.8315), (0.9808, 0.1951),
                       (0.9239, -0.3827), (0.7071, -0.7071), (0.5556, 0.8315), (0.9808, -0.1951), (1.0000, 0.0000),
                       (0.1951, -0.9808)], F)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    return p


class Frame:
    """Levels 0-2 of a frame as makeImages leaves them."""

    def __init__(self, img):
        self.h, self.w = img.shape
        lv = oracle.make_images(img, self.w, self.h)
        assert len(lv) >= 3, "the selector reads three pyramid levels"
        self.dI0 = lv[0][0]
        self.ag = [lv[l][1] for l in range(3)]
        self.wl = [self.w >> l for l in range(3)]


def hist_of_block(ag0, w, h, bx, by):
    """The 50 ints of one 32 x 32 block: [0] the pixels counted, [1 + g] the bins."""
    hist = np.zeros(50, np.int64)
    for j in range(32):
        jt = j + 32 * by
        for i in range(32):
            it = i + 32 * bx
            if it > w - 2 or jt > h - 2 or it < 1 or jt < 1:
                continue
            g = int(np.sqrt(ag0[it + jt * w]))
            g = min(g, 48)
            hist[g + 1] += 1
            hist[0] += 1
    return hist


def hist_quantile(hist, below):
    th = int(F(int(hist[0])) * F(below) + F(0.5))
    for i in range(90):
        th -= int(hist[i + 1]) if i + 1 < len(hist) else 0
        if th < 0:
            return i
    return 90


def make_hists(fr, p):
    """-> (ths [h32][w32], thsSmoothed flat with the zero entries, the histograms)."""
    w, h = fr.w, fr.h
    w32, h32 = w // 32, h // 32
    ths = np.zeros((h32, w32), F)
    hists = {}
    for y in range(h32):
        for x in range(w32):
            hists[x, y] = hist_of_block(fr.ag[0], w, h, x, y)
            ths[y, x] = F(hist_quantile(hists[x, y], p["min_grad_hist_cut"])) + F(p["min_grad_hist_add"])
    n_ths = max(((w - 1) >> 5) + ((h - 1) >> 5) * w32 + 1, w32 * h32)
    sm = np.zeros(n_ths, F)
    for y in range(h32):
        for x in range(w32):
            s, num = F(0), F(0)
            taps = []
            if x > 0:
                if y > 0:
                    taps.append((x - 1, y - 1))
                if y < h32 - 1:
                    taps.append((x - 1, y + 1))
                taps.append((x - 1, y))
            if x < w32 - 1:
                if y > 0:
                    taps.append((x + 1, y - 1))
                if y < h32 - 1:
                    taps.append((x + 1, y + 1))
                taps.append((x + 1, y))
            if y > 0:
                taps.append((x, y - 1))
            if y < h32 - 1:
                taps.append((x, y + 1))
            taps.append((x, y))
            for tx, ty in taps:
                num = F(num + F(1))
                s = F(s + ths[ty, tx])
            sm[x + y * w32] = F(F(s / num) * F(s / num))
    return ths, sm, hists


def pixel_tests(fr, sm, p):
    """Per pixel, ahead of the traversal: border, the threshold in force, the three tests and
    dirNorm under every direction (float32, statement order)."""
    w, h = fr.w, fr.h
    yy, xx = np.mgrid[0:h, 0:w]
    border = (xx < 4) | (xx >= w - 5) | (yy < 4) | (yy > h - 4)
    th0 = sm[(xx >> 5) + (yy >> 5) * (w // 32)].astype(F)
    dw1 = F(p["grad_downweight_per_level"])
    dw2 = F(dw1 * dw1)
    thf = F(p["th_factor"])
    th1 = (th0 * dw1).astype(F)
    th2 = (th1 * dw2).astype(F)
    a0 = fr.ag[0].reshape(h, w)
    a1 = fr.ag[1][(xx >> 1) + (yy >> 1) * fr.wl[1]]
    a2 = fr.ag[2][(xx >> 2) + (yy >> 2) * fr.wl[2]]
    with np.errstate(all="ignore"):
        p0 = a0 > (th0 * thf).astype(F)
        p1 = a1 > (th1 * thf).astype(F)
        p2 = a2 > (th2 * thf).astype(F)
        dx = fr.dI0[:, 1].reshape(h, w)
        dy = fr.dI0[:, 2].reshape(h, w)
        dn = np.stack([np.abs((dx * d[0]).astype(F) + (dy * d[1]).astype(F)).astype(F) for d in DIRECTIONS])
    return dict(border=border, th0=th0, p0=p0, p1=p1, p2=p2, a=(a0, a1, a2), dn=dn)


def select(fr, T, pot, pattern, p):
    """PixelSelector::select -> (map uint8 [h][w], (n2, n3, n4), info).  info["blocked"] counts the
    cells that hold a pixel past the level-0 threshold and make no pick."""
    w, h = fr.w, fr.h
    dist = bool(p["select_direction_distribution"])
    border = T["border"].tolist()
    P0, P1, P2 = T["p0"].tolist(), T["p1"].tolist(), T["p2"].tolist()
    A0, A1, A2 = T["a"]
    dn = T["dn"]
    out = np.zeros((h, w), np.uint8)
    n2 = n3 = n4 = 0
    blocked = 0
    pat = pattern.reshape(-1)
    zero, big = F(0), F(1e10)
    for y4 in range(0, h, 4 * pot):
        for x4 in range(0, w, 4 * pot):
            my3, mx3 = min(4 * pot, h - y4), min(4 * pot, w - x4)
            best4, val4 = -1, zero
            d4 = int(pat[n2]) & 0xF
            for y3 in range(0, my3, 2 * pot):
                for x3 in range(0, mx3, 2 * pot):
                    x34, y34 = x3 + x4, y3 + y4
                    my2, mx2 = min(2 * pot, h - y34), min(2 * pot, w - x34)
                    best3, val3 = -1, zero
                    d3 = int(pat[n2]) & 0xF
                    for y2 in range(0, my2, pot):
                        for x2 in range(0, mx2, pot):
                            x234, y234 = x2 + x34, y2 + y34
                            my1, mx1 = min(pot, h - y234), min(pot, w - x234)
                            best2, val2 = -1, zero
                            d2 = int(pat[n2]) & 0xF
                            past = False
                            for yf in range(y234, y234 + my1):
                                brow, r0, r1, r2 = border[yf], P0[yf], P1[yf], P2[yf]
                                for xf in range(x234, x234 + mx1):
                                    if brow[xf]:
                                        continue
                                    idx = xf + w * yf
                                    if r0[xf]:
                                        past = True
                                        v = dn[d2, yf, xf] if dist else A0[yf, xf]
                                        if v > val2:
                                            val2, best2, best3, best4 = v, idx, -2, -2
                                    if best3 == -2:
                                        continue
                                    if r1[xf]:
                                        v = dn[d3, yf, xf] if dist else A1[yf, xf]
                                        if v > val3:
                                            val3, best3, best4 = v, idx, -2
                                    if best4 == -2:
                                        continue
                                    if r2[xf]:
                                        v = dn[d4, yf, xf] if dist else A2[yf, xf]
                                        if v > val4:
                                            val4, best4 = v, idx
                            if best2 > 0:
                                out.reshape(-1)[best2] = 1
                                val3 = big
                                n2 += 1
                            elif past:
                                blocked += 1
                    if best3 > 0:
                        out.reshape(-1)[best3] = 2
                        val4 = big
                        n3 += 1
            if best4 > 0:
                out.reshape(-1)[best4] = 4
                n4 += 1
    return out, (n2, n3, n4), dict(blocked=blocked)


class Selector:
    """PixelSelector: the pattern and the potential that persists from frame to frame."""

    def __init__(self, pattern, potential=3):
        self.pattern = np.ascontiguousarray(pattern, np.uint8).reshape(-1)
        self.potential = int(potential)

    def make_maps(self, fr, **kw):
        """-> (map uint8 [h][w], stats dict as ldso_ct_select_pixels', trail).  trail: one dict per
        select pass (pot, n, quotia, map before any sub-selection, info) plus the hists."""
        p = params(**kw)
        assert self.pattern.size == fr.w * fr.h
        ths, sm, hists = make_hists(fr, p)
        T = pixel_tests(fr, sm, p)
        want = F(p["density"])
        left = int(p["recursions"])
        trail = []
        while True:
            pot = self.potential
            m, n, info = select(fr, T, min(pot, max(fr.w, fr.h)), self.pattern, p)
            have = F(n[0] + n[1] + n[2])
            with np.errstate(all="ignore"):
                quotia = F(want / have)
                K = F(F(have * F(pot + 1)) * F(pot + 1))
                ideal_f = F(np.sqrt(F(K / want)) - F(1))
            ideal = int(ideal_f) if ideal_f < MAX_POTENTIAL else MAX_POTENTIAL
            ideal = max(ideal, 1)
            trail.append(dict(pot=pot, n=n, quotia=float(quotia), map=m.copy(), info=info))
            if left > 0 and float(quotia) > 1.25 and pot > 1:
                if ideal >= pot:
                    ideal = pot - 1
            elif left > 0 and float(quotia) < 0.25:
                if ideal <= pot:
                    ideal = min(pot + 1, MAX_POTENTIAL)
            else:
                break
            self.potential = ideal
            left -= 1
        num = int(have)
        if float(quotia) < 0.95:
            char_th = int(F(255) * quotia) & 0xFF
            flat = m.reshape(-1)
            nz = np.flatnonzero(flat)
            drop = self.pattern[:nz.size] > char_th
            flat[nz[drop]] = 0
            num -= int(drop.sum())
        self.potential = ideal
        stats = dict(num=num, n2=n[0], n3=n[1], n4=n[2], potential_used=pot, potential_next=ideal, passes=len(trail))
        return m, stats, dict(passes=trail, ths=ths, smoothed=sm, hists=hists, tests=T, params=p)

    def make_new_traces(self, fr, host=0, **kw):
        """-> (records, stats, trail, pixels the walk selected): makeMaps, then walk()."""
        m, stats, trail = self.make_maps(fr, **kw)
        rec, walked = walk(fr, m, host)
        return rec, stats, trail, walked


def walk(fr, m, host=0):
    """makeNewTraces' walk over x in [3, w-4), y in [3, h-4) in row-major order: one record per
    selected pixel, its type the map value; records with a non-finite energy_th dropped.
    -> (records, selected pixels walked)."""
    inner = np.zeros_like(m, bool)
    inner[3:fr.h - 4, 3:fr.w - 4] = True
    ys, xs = np.nonzero((m != 0) & inner)  # row-major
    uv = np.stack([xs, ys], 1).astype(F)
    rec = oracle.ip_make(fr.dI0, fr.w, fr.h, uv, 1.0, host)
    rec["type"] = m[ys, xs].astype(F)
    keep = np.isfinite(rec["energy_th"])
    return rec[keep].copy(), int(ys.size)


# ---- the inputs both test files use -----------------------------------------------------------
SIZES = ((192, 128), (200, 136))  # both sides multiples of 32 / neither (aliased right strip, zero bottom strip)
PAIRS = ((300, 3), (20, 2), (600, 1), (3000, 3))  # (density, starting potential)


def pattern_of(w, h, seed=11):
    return np.random.default_rng(seed).integers(0, 256, w * h, dtype=np.uint8)


def image(kind, w, h, seed=1):
    """blobs: test_immature.blob_image.  mixed: its left third replaced by +-60 vertical bars of
    period ~7 px (dy == 0 cells), the top half of the middle third by horizontal bars (dx == 0).
    nan: blobs plus sigma 3 noise, 40 NaN pixels at least 8 px from the border."""
    from test_immature import blob_image

    img = blob_image(w, h, seed=seed).copy()
    if kind == "mixed":
        yy, xx = np.mgrid[0:h, 0:w]
        bars_v = (90.0 + 60.0 * np.sign(np.sin(2 * np.pi * (xx + 0.5) / 7.0))).astype(F)
        bars_h = (90.0 + 60.0 * np.sign(np.sin(2 * np.pi * (yy + 0.5) / 7.0))).astype(F)
        img[:, :w // 3] = bars_v[:, :w // 3]
        img[:h // 2, w // 3:2 * w // 3] = bars_h[:h // 2, w // 3:2 * w // 3]
    elif kind == "nan":
        rng = np.random.default_rng(seed + 100)
        img = (img + rng.normal(0, 3.0, img.shape)).astype(F)
        ys = rng.integers(8, h - 8, 40)
        xs = rng.integers(8, w - 8, 40)
        img[ys, xs] = np.nan
    else:
        assert kind == "blobs", kind
    return img
