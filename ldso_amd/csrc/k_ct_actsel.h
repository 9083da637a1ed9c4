// k_ct_actsel.h -- which immature points to activate: CoarseDistanceMap::makeDistanceMap / growDistBFS /
// addIntoDistFinal (CoarseTracker.cc:795-932) and the walk of FullSystem::activatePointsMT
// (FullSystem.cc:1220-1298), on level 1.  The walk is sequential in the text, not in its dependencies
// (DESIGN.md §9e): after any sequence of stamps a pixel other than the corner (w1-1, h1-1) holds a value
// that depends on the set of stamps alone, and only map values below a candidate's threshold decide it.
//   k_ct_as_seed      thread per active point: the projection in the reference's operation order, a kept
//                     point stores 0 (every store writes the same value: no atomics)
//   k_ct_as_grow      workgroup per kAsTile^2 tile with a 39 pixel halo in LDS (bytes): 39 synchronous
//                     frontier steps, odd k the 8-neighbourhood, even k the 4-neighbourhood; a pixel on the
//                     image border never propagates.  A step only writes k over values > k and only reads
//                     k - 1, so it runs in place; the halo is as wide as the steps are many, so the tile
//                     itself is exact.  1024 threads, each reading its pixels four to a word
//   k_ct_as_classify  thread per record: DELETE / KEEP / candidate, the candidate's pixel, threshold and
//                     fraction; one that fails against the initial map is KEEP at once (the map only
//                     decreases), the others are live and counted into 8 x 8 pixel bins
//   k_ct_as_scatter   the live candidates into their bins (k_ct_sel_scan gave the offsets); the order inside
//                     a bin is whatever the integer atomics give and no result depends on it
//   k_ct_as_round     thread per live candidate, one launch per round: its map value from the initial map
//                     and the accepted earlier candidates within its radius (ceil(threshold) - 1 pixels:
//                     a stamp never lowers a pixel below its Chebyshev distance).  A value that fails
//                     rejects at once; an accept waits until every earlier live candidate in the radius has
//                     decided.  The corner pixel's candidates (k_ct_as_round_corner, one workgroup over the
//                     last bin, once per batch of rounds, its own chains resolved behind barriers) decide
//                     only then: their value is not monotone in what is known.
//                     The earliest undecided candidate always decides, so n rounds end every input; no
//                     workgroup waits for another.
//   k_ct_as_count / k_ct_sel_scan / k_ct_as_write
//                     stable compaction: the OPTIMIZE records in walk order (host, then resident order)
//                     and the KEEP records in resident order; the counters go to mapped host memory
// No float atomics; no contraction.
#pragma once
#include <limits.h>
#include <math.h>

#include "k_ct_pyramid.h"
#include "k_ct_immature.h"
#include "k_ct_coarse_depth.h"

#pragma clang fp contract(off)

namespace {

constexpr int kAsSteps = 39;                        // growDistBFS: k = 1 .. 39
constexpr int kAsFar = 1000;                        // the map's initial value
constexpr int kAsTile = 50;                         // k_ct_as_grow's tile side
constexpr int kAsSide = kAsTile + 2 * kAsSteps;     // ... and its LDS region's: 128
constexpr int kAsGrowThreads = 1024;                // ... and its workgroup: four words of four pixels a thread
static_assert(kAsSide * kAsSide % (4 * kAsGrowThreads) == 0, "whole words per thread");
constexpr int kAsBinShift = 3;                      // 8 x 8 level-1 pixels per bin
constexpr int kAsMaxHosts = 16;                     // LDSO_BA_MAX_FRAMES
constexpr int kAsMaxSide = 32768;                   // a pixel packs into x | y << 16
constexpr int kAsAttempts = 4;                      // tries of an undecided candidate per launch
// a record's state: the ABI's dispositions, then the walk's own
enum : int { kAsKeep = 0, kAsDelete = 1, kAsOptimize = 2, kAsLive = 3, kAsKeepByDist = 4 };
// the counters of a call on the device; the first four are counts_out
enum : int { kAsCntKept, kAsCntDeleted, kAsCntSelected, kAsCntByDist, kAsCntMaxHost /* + 1 */, kAsCntUndecided, kAsCntLive, kAsCnts = 8 };

struct AsGrid {
    int w1, h1;  // level 1
    int bw, bh;  // bins per row / column
};
struct AsCand {  // a candidate of the walk
    int pix;     // x | y << 16
    int host;
    float thr, frac;  // currentMinActDist * my_type; ptp[0] - floorf(ptp[0])
};
struct AsEntry {  // a live candidate in its bin
    int pix, host, idx, pad;
};

// float -> int as x86's truncating conversion does it (k_ct_corners.h)
__device__ __forceinline__ int as_to_int(float f) {
    return (f >= -2147483648.f && f < 2147483648.f) ? (int)f : INT_MIN;
}

// ptp = KRKi (u, v, 1) + Kt d as Eigen evaluates it: each row three products summed left to right.
// H: [KRKi 9][Kt 3] of the point's host
__device__ __forceinline__ bool as_project(const float *__restrict__ H, float u, float v, float d, int w1, int h1,
                                           int &x, int &y, float &ptp0) {
    float ptp[3];
#pragma unroll
    for (int i = 0; i < 3; i++) ptp[i] = (H[3 * i] * u + H[3 * i + 1] * v + H[3 * i + 2] * 1.0f) + H[9 + i] * d;
    x = as_to_int(ptp[0] / ptp[2] + 0.5f);
    y = as_to_int(ptp[1] / ptp[2] + 0.5f);
    ptp0 = ptp[0];
    return x > 0 && y > 0 && x < w1 && y < h1;
}

// uvd [n] with `stride` floats between points ({u, v, idepth}), host [n]
__global__ __launch_bounds__(kCtThreads) void k_ct_as_seed(const float *__restrict__ uvd, int stride,
                                                           const int *__restrict__ host, int n, int n_hosts, int newest,
                                                           const float *__restrict__ hosts, AsGrid G,
                                                           int *__restrict__ map) {
    const int k = blockIdx.x * kCtThreads + threadIdx.x;
    if (k >= n) return;
    const int h = host[k];
    if (h < 0 || h >= n_hosts || h == newest) return;
    const float *p = uvd + (size_t)k * stride;
    int x, y;
    float ptp0;
    if (as_project(hosts + 12 * h, p[0], p[1], p[2], G.w1, G.h1, x, y, ptp0)) map[x + G.w1 * y] = 0;
}

// map: 0 at the seeds on entry (in place: a tile's halo may already hold a neighbour's result, whose zeros
// are the seeds and nothing else).  A thread owns four words of four pixels: a step loads them, and only
// a word with a byte equal to k - 1 (the frontier) does any more; a byte another thread turns into k
// meanwhile is no frontier either way.
__global__ __launch_bounds__(kAsGrowThreads) void k_ct_as_grow(int *map, AsGrid G) {
    __shared__ unsigned v_w[kAsSide * kAsSide / 4];
    uint8_t *v_s = reinterpret_cast<uint8_t *>(v_w);
    const int x0 = blockIdx.x * kAsTile - kAsSteps, y0 = blockIdx.y * kAsTile - kAsSteps;
    for (int i = threadIdx.x; i < kAsSide * kAsSide; i += kAsGrowThreads) {
        const int x = x0 + i % kAsSide, y = y0 + i / kAsSide;
        const bool in = x >= 0 && y >= 0 && x < G.w1 && y < G.h1;
        v_s[i] = in && map[x + G.w1 * y] == 0 ? 0 : 255;
    }
    __syncthreads();
    constexpr int kWords = kAsSide * kAsSide / 4 / kAsGrowThreads;
    for (int k = 1; k <= kAsSteps; k++) {
        unsigned word[kWords];
#pragma unroll
        for (int j = 0; j < kWords; j++) word[j] = v_w[threadIdx.x + j * kAsGrowThreads];
#pragma unroll
        for (int j = 0; j < kWords; j++) {
            const unsigned z = word[j] ^ (0x01010101u * (unsigned)(k - 1));  // a zero byte: a frontier pixel
            if (!((z - 0x01010101u) & ~z & 0x80808080u)) continue;
            for (int b = 0; b < 4; b++) {
                if (((word[j] >> (8 * b)) & 0xFFu) != (unsigned)(k - 1)) continue;
                const int i = 4 * (threadIdx.x + j * kAsGrowThreads) + b;
                const int lx = i % kAsSide, ly = i / kAsSide, x = x0 + lx, y = y0 + ly;
                // (a pixel outside the image is never written, so it is never here)
                if (x == 0 || y == 0 || x == G.w1 - 1 || y == G.h1 - 1) continue;
                const bool l = lx > 0, r = lx < kAsSide - 1, u = ly > 0, d = ly < kAsSide - 1;
                if (r && v_s[i + 1] > k) v_s[i + 1] = k;
                if (l && v_s[i - 1] > k) v_s[i - 1] = k;
                if (d && v_s[i + kAsSide] > k) v_s[i + kAsSide] = k;
                if (u && v_s[i - kAsSide] > k) v_s[i - kAsSide] = k;
                if (k & 1) {
                    if (r && d && v_s[i + 1 + kAsSide] > k) v_s[i + 1 + kAsSide] = k;
                    if (l && d && v_s[i - 1 + kAsSide] > k) v_s[i - 1 + kAsSide] = k;
                    if (l && u && v_s[i - 1 - kAsSide] > k) v_s[i - 1 - kAsSide] = k;
                    if (r && u && v_s[i + 1 - kAsSide] > k) v_s[i + 1 - kAsSide] = k;
                }
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < kAsTile * kAsTile; i += kAsGrowThreads) {
        const int tx = i % kAsTile, ty = i / kAsTile, x = x0 + kAsSteps + tx, y = y0 + kAsSteps + ty;
        if (x >= G.w1 || y >= G.h1) continue;
        const int v = v_s[(ty + kAsSteps) * kAsSide + tx + kAsSteps];
        map[x + G.w1 * y] = v == 255 ? kAsFar : v;
    }
}

struct AsClassify {
    const IpRec *__restrict__ recs;
    const float *__restrict__ hosts;       // [n_hosts][12]
    const uint8_t *__restrict__ flagged;   // [n_hosts] flaggedForMarginalization
    const int *__restrict__ map;
    int n, n_hosts, newest;
    float min_act_dist, min_quality;
    AsGrid G;
};

__global__ __launch_bounds__(kCtThreads) void k_ct_as_classify(AsClassify P, AsCand *__restrict__ cand,
                                                               int *__restrict__ disp, int *__restrict__ bin_cnt) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= P.n) return;
    const IpRec *q = P.recs + i;
    const int host = q->host, st = q->last_status;
    const float imin = q->idepth_min, imax = q->idepth_max;
    AsCand c{0, host, 0.f, 0.f};
    int d;
    if (host == P.newest) {
        d = kAsKeep;
    } else if (!isfinite(imax) || st == LDSO_CT_IPS_OUTLIER) {
        d = kAsDelete;
    } else {
        const bool canActivate = (st == LDSO_CT_IPS_GOOD || st == LDSO_CT_IPS_SKIPPED ||
                                  st == LDSO_CT_IPS_BADCONDITION || st == LDSO_CT_IPS_OOB) &&
                                 q->last_interval < 8 && q->quality > P.min_quality && (imax + imin) > 0;
        if (!canActivate) {
            d = (P.flagged[host] || st == LDSO_CT_IPS_OOB) ? kAsDelete : kAsKeep;
        } else {
            int x, y;
            float ptp0;
            if (!as_project(P.hosts + 12 * host, q->u, q->v, 0.5f * (imax + imin), P.G.w1, P.G.h1, x, y, ptp0)) {
                d = kAsDelete;
            } else {
                c.pix = x | (y << 16);
                c.frac = ptp0 - floorf(ptp0);
                c.thr = P.min_act_dist * q->type;
                const float dist = (float)P.map[x + P.G.w1 * y] + c.frac;
                d = dist >= c.thr ? kAsLive : kAsKeepByDist;
                if (d == kAsLive) atomicAdd(&bin_cnt[(y >> kAsBinShift) * P.G.bw + (x >> kAsBinShift)], 1);
            }
        }
    }
    cand[i] = c;
    disp[i] = d;
}

// bin_off: the bins' starts (exclusive prefix of the counts); cursor zeroed
__global__ __launch_bounds__(kCtThreads) void k_ct_as_scatter(const AsCand *__restrict__ cand,
                                                              const int *__restrict__ disp, int n, AsGrid G,
                                                              const int *__restrict__ bin_off, int *__restrict__ cursor,
                                                              AsEntry *__restrict__ entries) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= n || disp[i] != kAsLive) return;
    const AsCand c = cand[i];
    const int x = c.pix & 0xFFFF, y = c.pix >> 16, b = (y >> kAsBinShift) * G.bw + (x >> kAsBinShift);
    entries[bin_off[b] + atomicAdd(&cursor[b], 1)] = AsEntry{c.pix, c.host, i, 0};
}

// steps of the alternating 8 / 4 growth between two pixels in free space: the smallest k with
// max(|dx|, |dy|) <= k and |dx| + |dy| <= k + ceil(k / 2); kAsFar beyond the 39 steps
__device__ __forceinline__ int as_steps(int dx, int dy) {
    dx = abs(dx);
    dy = abs(dy);
    const int s = dx + dy;
    int k = max(dx, dy);
    while (s > k + (k + 1) / 2) k++;
    return k <= kAsSteps ? k : kAsFar;
}

__device__ __forceinline__ int as_state(const int *disp, int i) {
    return __hip_atomic_load(disp + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// f(x, y, host, idx) for every accepted candidate before (host, idx) in the walk within r pixels (Chebyshev) of
// (px, py); true if one of those candidates is undecided
template <typename F>
__device__ __forceinline__ bool as_for_earlier(AsGrid G, const AsEntry *__restrict__ entries,
                                               const int *__restrict__ bin_off, const int *disp, int px, int py, int r,
                                               int host, int idx, F &&f) {
    bool wait = false;
    const int bx0 = max(px - r, 0) >> kAsBinShift, bx1 = min(px + r, G.w1 - 1) >> kAsBinShift;
    const int by0 = max(py - r, 0) >> kAsBinShift, by1 = min(py + r, G.h1 - 1) >> kAsBinShift;
    for (int by = by0; by <= by1; by++)
        for (int bx = bx0; bx <= bx1; bx++) {
            const int b = by * G.bw + bx;
            for (int k = bin_off[b]; k < bin_off[b + 1]; k++) {
                const AsEntry e = entries[k];
                if (e.host > host || (e.host == host && e.idx >= idx)) continue;
                const int ex = e.pix & 0xFFFF, ey = e.pix >> 16;
                if (abs(ex - px) > r || abs(ey - py) > r) continue;
                const int s = as_state(disp, e.idx);
                if (s == kAsLive) wait = true;
                else if (s == kAsOptimize) f(ex, ey, e.host, e.idx);
            }
        }
    return wait;
}

struct AsRound {
    const AsCand *__restrict__ cand;
    const AsEntry *__restrict__ entries;
    const int *__restrict__ bin_off;  // [bins + 1]
    const int *__restrict__ map;      // after makeDistanceMap
    int *disp;
    int *cnt;
    AsGrid G;
    int n_bins, count_undecided;
};

__device__ __forceinline__ int as_radius(float thr) {
    const float rt = ceilf(thr);  // <= 16 for the reference's types
    return rt > (float)kAsSteps ? kAsSteps : rt < 0.f ? -1 : (int)rt - 1;
}

// every candidate but those on the corner pixel (k_ct_as_round_corner)
__global__ __launch_bounds__(kCtThreads) void k_ct_as_round(AsRound P) {
    const int k = blockIdx.x * kCtThreads + threadIdx.x;
    if (k >= P.bin_off[P.n_bins]) return;
    const AsEntry me = P.entries[k];
    const AsGrid G = P.G;
    const int w1 = G.w1, h1 = G.h1, px = me.pix & 0xFFFF, py = me.pix >> 16;
    const bool right = px == w1 - 1, bottom = py == h1 - 1;
    if ((right && bottom) || as_state(P.disp, me.idx) != kAsLive) return;
    const AsCand c = P.cand[me.idx];
    const int r = as_radius(c.thr);
    auto on_border = [&](int x, int y) { return x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1; };
    // An interior pixel takes the nearest accepted source that propagates.  One on the last column or row
    // takes its own stamps, V(m) + 1 of its interior 4-neighbour m and V(q) + 1 of an interior diagonal
    // neighbour q with V(q) even, V = min(initial map, nearest source).
    const bool edge = right || bottom;
    const int ax = right ? px - 1 : px, ay = bottom ? py - 1 : py;  // m; the pixel itself in the interior
    const int bx = px - 1, by = py - 1;                             // q
    const int cx = right ? px - 1 : px + 1, cy = right ? py + 1 : py - 1;  // q'
    const int m0 = P.map[px + w1 * py];
    const int ma = edge && !on_border(ax, ay) ? P.map[ax + w1 * ay] : -1;  // -1: no such neighbour
    const int mb = edge && !on_border(bx, by) ? P.map[bx + w1 * by] : -1;
    const int mc = edge && !on_border(cx, cy) ? P.map[cx + w1 * cy] : -1;
    for (int attempt = 0; attempt < kAsAttempts; attempt++) {
        int v = m0, da = kAsFar, db = kAsFar, dc = kAsFar;
        const bool wait = as_for_earlier(G, P.entries, P.bin_off, P.disp, px, py, r, me.host, me.idx, [&](int x, int y, int, int) {
            if (x == px && y == py) v = 0;
            if (on_border(x, y)) return;
            da = min(da, as_steps(x - ax, y - ay));
            if (edge) {
                db = min(db, as_steps(x - bx, y - by));
                dc = min(dc, as_steps(x - cx, y - cy));
            }
        });
        if (!edge) {
            v = min(v, da);
        } else {
            const int Va = min(ma, da), Vb = min(mb, db), Vc = min(mc, dc);
            if (ma >= 0 && Va + 1 <= kAsSteps) v = min(v, Va + 1);
            if (mb >= 0 && !(Vb & 1) && Vb + 1 <= kAsSteps) v = min(v, Vb + 1);
            if (mc >= 0 && !(Vc & 1) && Vc + 1 <= kAsSteps) v = min(v, Vc + 1);
        }
        // the map only decreases: a value that fails now fails for good
        const bool accept = (float)v + c.frac >= c.thr;
        if (!accept || !wait) {
            __hip_atomic_store(P.disp + me.idx, accept ? kAsOptimize : kAsKeepByDist, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    if (P.count_undecided) atomicAdd(&P.cnt[kAsCntUndecided], 1);
}

// The candidates on the corner (w1-1, h1-1), which are in the last bin: one workgroup strides over it.
// The corner is lowered only when (w1-2, h1-2) is lowered to an even value t, and then to t + 1, or by a
// stamp of its own: an accepted source counts if no accepted source before it in the walk had already
// brought that pixel as low (the running minimum of the walk, restated without the walk).  That is not monotone in what is known, so a candidate decides only when no
// earlier candidate in its radius is undecided -- or when an earlier accept on the corner itself has
// made the value 0 for good.  Chains among the corner's own candidates are resolved here, a barrier per
// round, until a round decides nobody.
__global__ __launch_bounds__(kCtThreads) void k_ct_as_round_corner(AsRound P) {
    __shared__ int progress;
    const AsGrid G = P.G;
    const int w1 = G.w1, h1 = G.h1, px = w1 - 1, py = h1 - 1, qx = w1 - 2, qy = h1 - 2;
    const bool q_ok = qx > 0 && qy > 0;
    const int m0 = P.map[px + w1 * py], q0 = q_ok ? P.map[qx + w1 * qy] : 0;
    const int k0 = P.bin_off[P.n_bins - 1], k1 = P.bin_off[P.n_bins];
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) progress = 0;
        __syncthreads();
        for (int k = k0 + threadIdx.x; k < k1; k += kCtThreads) {
            const AsEntry me = P.entries[k];
            if (me.pix != (px | (py << 16)) || as_state(P.disp, me.idx) != kAsLive) continue;
            const AsCand c = P.cand[me.idx];
            const int r = as_radius(c.thr);
            int v = m0;
            const bool wait = as_for_earlier(G, P.entries, P.bin_off, P.disp, px, py, r, me.host, me.idx,
                                             [&](int x, int y, int, int) {
                                                 if (x == px && y == py) v = 0;
                                             });
            if (wait && v != 0) continue;
            // Every earlier candidate in the radius has decided.  The source that lowers (w1-2, h1-2) to T
            // is the earliest in the walk of those within T steps of it, if it is at T exactly; the
            // smallest even T with such a source gives the corner T + 1.  T + 1 below the threshold means
            // T < r, and a source within T steps of that pixel is within the radius.
            for (int T = 0; q_ok && T <= r && T < q0 && T + 1 < v; T += 2) {
                unsigned long long first = ~0ull;
                int first_t = -1;
                (void)as_for_earlier(G, P.entries, P.bin_off, P.disp, px, py, r, me.host, me.idx,
                                     [&](int x, int y, int host, int idx) {
                                         if (x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1) return;
                                         const int t = as_steps(x - qx, y - qy);
                                         const unsigned long long key = ((unsigned long long)host << 32) | (unsigned)idx;
                                         if (t <= T && key < first) {
                                             first = key;
                                             first_t = t;
                                         }
                                     });
                if (first_t == T) v = T + 1;
            }
            __hip_atomic_store(P.disp + me.idx, (float)v + c.frac >= c.thr ? kAsOptimize : kAsKeepByDist, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            progress = 1;
        }
        __syncthreads();
        if (!progress) break;
    }
    if (!P.count_undecided) return;
    for (int k = k0 + threadIdx.x; k < k1; k += kCtThreads)
        if (P.entries[k].pix == (px | (py << 16)) && as_state(P.disp, P.entries[k].idx) == kAsLive)
            atomicAdd(&P.cnt[kAsCntUndecided], 1);
}

struct AsOut {
    const IpRec *__restrict__ recs;
    const int *__restrict__ disp;
    int *__restrict__ blk;  // [n_hosts + 1][nb]: the OPTIMIZE records per host, then the KEEP records
    int *__restrict__ cnt;
    int n, nb, n_hosts;
};

__global__ __launch_bounds__(kCtThreads) void k_ct_as_count(AsOut P) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    const int d = i < P.n ? P.disp[i] : -1, host = i < P.n ? P.recs[i].host : -1;
    int total;
    for (int h = 0; h < P.n_hosts; h++) {
        (void)cd_block_prefix(d == kAsOptimize && host == h, &total);
        if (threadIdx.x == 0) P.blk[(size_t)h * P.nb + blockIdx.x] = total;
        __syncthreads();
    }
    const bool keep = d == kAsKeep || d == kAsKeepByDist;
    (void)cd_block_prefix(keep, &total);
    if (threadIdx.x == 0) {
        P.blk[(size_t)P.n_hosts * P.nb + blockIdx.x] = total;
        if (total) atomicAdd(&P.cnt[kAsCntKept], total);
    }
    __syncthreads();
    (void)cd_block_prefix(d == kAsDelete, &total);
    if (threadIdx.x == 0 && total) atomicAdd(&P.cnt[kAsCntDeleted], total);
    __syncthreads();
    (void)cd_block_prefix(d == kAsOptimize, &total);
    if (threadIdx.x == 0 && total) atomicAdd(&P.cnt[kAsCntSelected], total);
    __syncthreads();
    (void)cd_block_prefix(d == kAsKeepByDist, &total);
    if (threadIdx.x == 0 && total) atomicAdd(&P.cnt[kAsCntByDist], total);
    if (keep) atomicMax(&P.cnt[kAsCntMaxHost], host + 1);
}

// blk scanned per array, tot [n_hosts + 1] its totals.  kept (may be null): the compacted resident set
__global__ __launch_bounds__(kCtThreads) void k_ct_as_write(AsOut P, const int *__restrict__ tot,
                                                            IpRec *__restrict__ selected, int *__restrict__ selected_idx,
                                                            IpRec *__restrict__ kept, int *__restrict__ disp_out,
                                                            int *__restrict__ counts_host) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    const int d = i < P.n ? P.disp[i] : -1, host = i < P.n ? P.recs[i].host : -1;
    if (blockIdx.x == 0 && threadIdx.x < kAsCnts) counts_host[threadIdx.x] = P.cnt[threadIdx.x];
    int total, base = 0, rank = -1;
    for (int h = 0; h < P.n_hosts; h++) {
        const bool mine = d == kAsOptimize && host == h;
        const int pre = cd_block_prefix(mine, &total);
        if (mine) rank = base + P.blk[(size_t)h * P.nb + blockIdx.x] + pre;
        base += tot[h];
        __syncthreads();
    }
    const bool keep = d == kAsKeep || d == kAsKeepByDist;
    const int kpre = cd_block_prefix(keep, &total);
    if (i >= P.n) return;
    disp_out[i] = keep ? kAsKeep : d;
    if (rank >= 0) {
        selected[rank] = P.recs[i];
        selected_idx[rank] = i;
    }
    if (keep && kept) kept[P.blk[(size_t)P.n_hosts * P.nb + blockIdx.x] + kpre] = P.recs[i];
}

}  // namespace
