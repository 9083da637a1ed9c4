// k_ct_select.h -- pixel selection on the resident pyramid (PixelSelector::makeHists / select / makeMaps,
// PixelSelector2.cc:27-316, setting_pointSelection == 0) and FullSystem::makeNewTraces' raster walk
// (FullSystem.cc:1439-1461).  What select() does sequentially is, per block of the three nested grids:
//   a pot cell picks (type 1) iff one of its pixels passes the level-0 threshold with dirNorm > 0 under the
//     cell's direction; the pick is the first maximum of dirNorm in scan order;
//   a 2 pot block picks (type 2) iff none of its cells picks and a pixel passes the level-1 threshold with
//     dirNorm > 0 under the block's direction (the -2 sentinel: a level-0 hit closes level 1 for the rest of
//     the block; `bestVal3 = 1e10` only ever follows such a hit, so it decides nothing further);
//   a 4 pot block picks (type 4) iff no level-0 hit and no level-1 hit happened anywhere in it -- a level-1
//     hit counts when it comes before the block's first level-0 hit in scan order, also where that 2 pot
//     block ends without a pick.
// A block's direction is randomPattern[n2] & 0xF with n2 = the level-0 picks made before the block starts,
// the one serial dependency.  Per select pass:
//   k_ct_sel_block<false>  workgroup per 4 pot block: per cell the 16-bit mask "picks under direction d"
//                          (LDS atomicOr: order-free), stored at the cell's rank in traversal order
//   k_ct_sel_cell_count / k_ct_sel_scan / k_ct_sel_cell_apply
//                          exclusive prefix over the cells of "mask == 0xFFFF" (picks whatever the
//                          direction) -> n2 at each cell's start if no other cell picked; the cells whose
//                          mask is neither 0 nor 0xFFFF are listed in order
//   k_ct_sel_fixup         one wave walks that list in order, 64 cells at a time: n2 = prefix + picks of the
//                          listed cells so far decides the cell, whose mask becomes 0 or 0xFFFF
//   (count / scan / apply again: n2 at every cell's start, exact)
//   k_ct_sel_block<true>   workgroup per 4 pot block with the three directions known: first maxima as LDS
//                          atomicMax over (dirNorm bits, reversed scan index) keys (dirNorm > 0, so its bits
//                          order as unsigned; max is order-free), first hits as LDS atomicMin over scan
//                          indices; the decisions above; picks to the map; n3, n4 counted with integer atomics
// and per makeMaps: k_ct_sel_hist (block per 32 x 32 block: LDS integer histogram, computeHistQuantil),
// k_ct_sel_smooth, the sub-selection (k_ct_sel_px_count / _scan / k_ct_sel_sub: ordered prefix count over
// the map's non-zero pixels) and the emit walk (k_ct_sel_emit count, scan, write: records by
// ip_make_record, in row-major order).  f32 denormals are kept (the gfx950 default); no contraction.
#pragma once
#include "k_ct_pyramid.h"
#include "k_ct_immature.h"
#include "k_ct_coarse_depth.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSelMaxPotential = 32767;  // (pot + 1)^2 and 4 pot stay ints
constexpr int kSelMaxSide = 16384;       // 16 pot^2 scan indices of a block stay below 2^32
// the counters of a makeMaps call on the device
enum : int { kSelCntN2, kSelCntNonUniform, kSelCntN3, kSelCntN4, kSelCntKept, kSelCntEmit, kSelCntScratch, kSelCnts = 8 };

// PixelSelector2.cc:186-202
__constant__ float kSelDirX[16] = {0.f,     0.3827f, 0.1951f, 0.9239f, 0.7071f, 0.3827f, 0.8315f, 0.8315f,
                                   0.5556f, 0.9808f, 0.9239f, 0.7071f, 0.5556f, 0.9808f, 1.0000f, 0.1951f};
__constant__ float kSelDirY[16] = {1.0000f,  0.9239f, 0.9808f,  0.3827f,  0.7071f, -0.9239f, 0.5556f, -0.5556f,
                                   -0.8315f, 0.1951f, -0.3827f, -0.7071f, 0.8315f, -0.1951f, 0.0000f, -0.9808f};

struct SelParams {
    const float4 *__restrict__ dI0, *__restrict__ dI1, *__restrict__ dI2;  // texels of levels 0-2 (.w = absSquaredGrad)
    const float *__restrict__ ths;                                         // thsSmoothed, unwritten entries 0
    const uint8_t *__restrict__ pattern;                                   // randomPattern [w*h]
    int w, h, w1, w2, w32;
    int pot, ncx, ncy;  // cell side (clamped to the image's longer side), cells per row / column
    float dw1, dw2, th_factor;
    int dir_dist;
};

// ---------------------------------------------------------------------------------------------
// makeHists (PixelSelector2.cc:36-109)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCtThreads) void k_ct_sel_hist(const float4 *__restrict__ dI0, int w, int h, int w32,
                                                            float cut, float add, float *__restrict__ ths) {
    __shared__ int hist[92];  // [0] the count, [1..49] the bins; the quantile walk reads up to [90]
    for (int i = threadIdx.x; i < 92; i += kCtThreads) hist[i] = 0;
    __syncthreads();
    const int x0 = 32 * blockIdx.x, y0 = 32 * blockIdx.y;
    for (int k = threadIdx.x; k < 1024; k += kCtThreads) {
        const int it = x0 + (k & 31), jt = y0 + (k >> 5);
        if (it > w - 2 || jt > h - 2 || it < 1 || jt < 1) continue;
        int g = (int)sqrtf(dI0[it + (size_t)jt * w].w);
        if (g > 48) g = 48;
        if (g < 0) g = 0;  // (not reachable from makeImages' gradients: keeps the bin inside the array)
        atomicAdd(&hist[g + 1], 1);
        atomicAdd(&hist[0], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // computeHistQuantil (PixelSelector2.cc:27-34)
        int th = (int)(hist[0] * cut + 0.5f), q = 90;
        for (int i = 0; i < 90; i++) {
            th -= hist[i + 1];
            if (th < 0) {
                q = i;
                break;
            }
        }
        ths[blockIdx.x + blockIdx.y * w32] = q + add;
    }
}

__global__ __launch_bounds__(kCtThreads) void k_ct_sel_smooth(const float *__restrict__ ths, int w32, int h32,
                                                              float *__restrict__ smoothed) {
    const int k = blockIdx.x * kCtThreads + threadIdx.x;
    if (k >= w32 * h32) return;
    const int x = k % w32, y = k / w32;
    float sum = 0, num = 0;
    auto take = [&](int xx, int yy) {
        num++;
        sum += ths[xx + yy * w32];
    };
    if (x > 0) {
        if (y > 0) take(x - 1, y - 1);
        if (y < h32 - 1) take(x - 1, y + 1);
        take(x - 1, y);
    }
    if (x < w32 - 1) {
        if (y > 0) take(x + 1, y - 1);
        if (y < h32 - 1) take(x + 1, y + 1);
        take(x + 1, y);
    }
    if (y > 0) take(x, y - 1);
    if (y < h32 - 1) take(x, y + 1);
    take(x, y);
    smoothed[k] = (sum / num) * (sum / num);
}

// ---------------------------------------------------------------------------------------------
// select (PixelSelector2.cc:171-316)
// ---------------------------------------------------------------------------------------------
// a cell's position in select's traversal: 4 pot blocks row-major, 2 pot blocks row-major inside them,
// cells row-major inside those, every grid clipped at the right and bottom edges
__device__ __forceinline__ int sel_cell_rank(int cx, int cy, int ncx, int ncy) {
    const int b4x = cx >> 2, b4y = cy >> 2;
    const int ch4 = min(4, ncy - 4 * b4y), cw4 = min(4, ncx - 4 * b4x);
    const int qx = cx & 3, qy = cy & 3, s2x = qx >> 1, s2y = qy >> 1;
    const int ch2 = min(2, ch4 - 2 * s2y), cw2 = min(2, cw4 - 2 * s2x);
    return b4y * 4 * ncx + b4x * 4 * ch4 + s2y * 2 * cw4 + s2x * 2 * ch2 + (qy & 1) * cw2 + (qx & 1);
}

// slot s = 0..15 of a 4 pot block in traversal order -> the cell's offsets in cells
__device__ __forceinline__ void sel_slot_cell(int s, int &ox, int &oy) {
    ox = ((s >> 2) & 1) * 2 + (s & 1);
    oy = (s >> 3) * 2 + ((s >> 1) & 1);
}

struct SelPixel {
    float dx, dy, a0, a1, a2;
    bool p0, p1, p2;
};
// the thresholds and the three tests of one pixel; false: a border pixel (skipped)
__device__ __forceinline__ bool sel_pixel(const SelParams &S, int xf, int yf, SelPixel &q) {
    if (xf < 4 || xf >= S.w - 5 || yf < 4 || yf > S.h - 4) return false;
    const float pixelTH0 = S.ths[(xf >> 5) + (yf >> 5) * S.w32];
    const float pixelTH1 = pixelTH0 * S.dw1;
    const float pixelTH2 = pixelTH1 * S.dw2;
    const float4 t = S.dI0[xf + (size_t)yf * S.w];
    q.dx = t.y;
    q.dy = t.z;
    q.a0 = t.w;
    q.a1 = S.dI1[(xf >> 1) + (size_t)(yf >> 1) * S.w1].w;
    q.a2 = S.dI2[(xf >> 2) + (size_t)(yf >> 2) * S.w2].w;
    q.p0 = q.a0 > pixelTH0 * S.th_factor;
    q.p1 = q.a1 > pixelTH1 * S.th_factor;
    q.p2 = q.a2 > pixelTH2 * S.th_factor;
    return true;
}
__device__ __forceinline__ float sel_dir_norm(const SelPixel &q, int d) {
    return fabsf(q.dx * kSelDirX[d] + q.dy * kSelDirY[d]);
}
// larger dirNorm first, then the earlier scan index (dn > 0: its bits order as unsigned integers)
__device__ __forceinline__ unsigned long long sel_key(float dn, unsigned i) {
    return ((unsigned long long)__float_as_uint(dn) << 32) | (unsigned)~i;
}

// kPick false: the cells' direction masks; true: the picks, with n2 at every cell's start known
template <bool kPick>
__global__ __launch_bounds__(kCtThreads) void k_ct_sel_block(SelParams S, unsigned *__restrict__ mask,
                                                             const int *__restrict__ n2_start,
                                                             uint8_t *__restrict__ map, int *__restrict__ cnt) {
    __shared__ unsigned long long key0[16], key1[4], key2;
    __shared__ unsigned first0[4], first1[4], bits[16];
    __shared__ int dir2[16], dir3[4], dir4;
    const int tid = threadIdx.x, cx0 = 4 * blockIdx.x, cy0 = 4 * blockIdx.y, pot = S.pot;
    if (tid < 16) {
        key0[tid] = 0;
        bits[tid] = 0;
        int ox, oy;
        sel_slot_cell(tid, ox, oy);
        int d = 0;
        if (kPick && cx0 + ox < S.ncx && cy0 + oy < S.ncy)
            d = S.pattern[n2_start[sel_cell_rank(cx0 + ox, cy0 + oy, S.ncx, S.ncy)]] & 0xF;
        dir2[tid] = d;
        if ((tid & 3) == 0) {  // the first cell of a 2 pot block starts it
            dir3[tid >> 2] = d;
            key1[tid >> 2] = 0;
            first0[tid >> 2] = first1[tid >> 2] = 0xFFFFFFFFu;
        }
        if (tid == 0) {
            dir4 = d;
            key2 = 0;
        }
    }
    __syncthreads();
    const unsigned pp = (unsigned)pot * pot, n_idx = 16u * pp;
    for (unsigned i = tid; i < n_idx; i += blockDim.x) {
        const int s = i / pp, j = i - s * pp;
        int ox, oy;
        sel_slot_cell(s, ox, oy);
        const int xf = (cx0 + ox) * pot + j % pot, yf = (cy0 + oy) * pot + j / pot;
        if (xf >= S.w || yf >= S.h) continue;
        SelPixel q;
        if (!sel_pixel(S, xf, yf, q)) continue;
        if (!kPick) {
            if (!q.p0) continue;
            unsigned b = 0;
            if (S.dir_dist) {
#pragma unroll
                for (int d = 0; d < 16; d++) b |= (sel_dir_norm(q, d) > 0 ? 1u : 0u) << d;
            } else {
                b = q.a0 > 0 ? 0xFFFFu : 0u;
            }
            if (b) atomicOr(&bits[s], b);
        } else {
            const int s2 = s >> 2;
            if (q.p0) {
                const float dn = S.dir_dist ? sel_dir_norm(q, dir2[s]) : q.a0;
                if (dn > 0) {
                    atomicMax(&key0[s], sel_key(dn, i));
                    atomicMin(&first0[s2], i);
                }
            }
            if (q.p1) {
                const float dn = S.dir_dist ? sel_dir_norm(q, dir3[s2]) : q.a1;
                if (dn > 0) {
                    atomicMax(&key1[s2], sel_key(dn, i));
                    atomicMin(&first1[s2], i);
                }
            }
            if (q.p2) {
                const float dn = S.dir_dist ? sel_dir_norm(q, dir4) : q.a2;
                if (dn > 0) atomicMax(&key2, sel_key(dn, i));
            }
        }
    }
    __syncthreads();
    if (!kPick) {
        if (tid < 16) {
            int ox, oy;
            sel_slot_cell(tid, ox, oy);
            if (cx0 + ox < S.ncx && cy0 + oy < S.ncy) mask[sel_cell_rank(cx0 + ox, cy0 + oy, S.ncx, S.ncy)] = bits[tid];
        }
        return;
    }
    unsigned long long k = 0;
    uint8_t type = 0;
    if (tid < 16) {
        k = key0[tid];
        type = 1;
    } else if (tid < 20) {
        if (first0[tid - 16] == 0xFFFFFFFFu) k = key1[tid - 16];
        type = 2;
    } else if (tid == 20) {
        bool open = true;  // no level-0 hit, and no level-1 hit before one, anywhere in the block
        for (int b = 0; b < 4; b++) open = open && first0[b] == 0xFFFFFFFFu && first1[b] == 0xFFFFFFFFu;
        if (open) k = key2;
        type = 4;
    }
    if (k) {
        const unsigned i = ~(unsigned)k;
        const int s = i / pp, j = i - s * pp;
        int ox, oy;
        sel_slot_cell(s, ox, oy);
        const int xf = (cx0 + ox) * pot + j % pot, yf = (cy0 + oy) * pot + j / pot;
        map[xf + (size_t)yf * S.w] = type;
    }
    // n3 and n4 (n2 is the cells' scan total): lanes 16-20 are in wave 0
    if (tid < kWave) {
        const unsigned long long picked = __ballot(k != 0);
        const int n3 = __popcll(picked & 0xF0000ull), n4 = (int)((picked >> 20) & 1);
        if (tid == 0 && n3) atomicAdd(&cnt[kSelCntN3], n3);
        if (tid == 0 && n4) atomicAdd(&cnt[kSelCntN4], n4);
    }
}

// per block of cells (in rank order): how many pick under every direction, how many under some only
__global__ __launch_bounds__(kCtThreads) void k_ct_sel_cell_count(const unsigned *__restrict__ mask, int nc, int nb,
                                                                  int *__restrict__ blk) {
    const int c = blockIdx.x * kCtThreads + threadIdx.x;
    const unsigned m = c < nc ? mask[c] : 0u;
    int all, some;
    (void)cd_block_prefix(m == 0xFFFFu, &all);
    __syncthreads();
    (void)cd_block_prefix(m != 0 && m != 0xFFFFu, &some);
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = all;
        blk[nb + blockIdx.x] = some;
    }
}

// exclusive prefix (in place) of na arrays of nb block counts, back to back; their totals to tot[0..na)
__global__ __launch_bounds__(kCtThreads) void k_ct_sel_scan(int *__restrict__ blk, int nb, int na, int *__restrict__ tot) {
    __shared__ int wave_sum[kCtThreads / kWave];
    __shared__ int carry_s;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    for (int a = 0; a < na; a++) {
        int *v_ = blk + (size_t)a * nb;
        if (threadIdx.x == 0) carry_s = 0;
        __syncthreads();
        for (int b0 = 0; b0 < nb; b0 += kCtThreads) {
            const int b = b0 + threadIdx.x;
            const int v = b < nb ? v_[b] : 0;
            int s = v;  // inclusive scan over the wave
#pragma unroll
            for (int m = 1; m < kWave; m <<= 1) {
                const int t = __shfl_up(s, m, kWave);
                if (lane >= m) s += t;
            }
            if (lane == kWave - 1) wave_sum[wv] = s;
            __syncthreads();
            int base = carry_s, all = 0;
#pragma unroll
            for (int k = 0; k < kCtThreads / kWave; k++) {
                if (k < wv) base += wave_sum[k];
                all += wave_sum[k];
            }
            if (b < nb) v_[b] = base + s - v;
            __syncthreads();
            if (threadIdx.x == 0) carry_s += all;
            __syncthreads();
        }
        if (threadIdx.x == 0) tot[a] = carry_s;
        __syncthreads();
    }
}

// n2 at every cell's start counting the cells that pick under every direction; the others in order
__global__ __launch_bounds__(kCtThreads) void k_ct_sel_cell_apply(const unsigned *__restrict__ mask, int nc, int nb,
                                                                  const int *__restrict__ blk,
                                                                  int *__restrict__ n2_start,
                                                                  int *__restrict__ non_uniform) {
    const int c = blockIdx.x * kCtThreads + threadIdx.x;
    const unsigned m = c < nc ? mask[c] : 0u;
    const bool some = m != 0 && m != 0xFFFFu;
    int total;
    const int pre_all = cd_block_prefix(m == 0xFFFFu, &total);
    __syncthreads();
    const int pre_some = cd_block_prefix(some, &total);
    if (c < nc) n2_start[c] = blk[blockIdx.x] + pre_all;
    if (some) non_uniform[blk[nb + blockIdx.x] + pre_some] = c;
}

// the serial part: the cells whose pick depends on their direction, in traversal order
// One wave, 64 listed cells at a time.  Cell k picks iff bit (pattern[base_k + carry_k] & 0xF) of its mask is
// set, carry_k = the picks of the listed cells before it.  The wave iterates to the fixed point: every lane
// evaluates its cell under the carries that the lanes' current picks give, until no pick changes.  After
// iteration j the first j lanes hold the sequential answer (lane 0 depends on nothing in the chunk, lane j
// only on the lanes before it), so the loop ends within 65 iterations, and a fixed point is that answer.
// The pattern bytes a chunk can index start at base_0 + carry and mostly span little: they are staged in
// LDS once per chunk when they fit (a run of such cells with no other picks between them spans 64), so that
// only the first evaluation waits for memory; a chunk that spans more reads the pattern directly.
constexpr int kSelFixWindow = 128;
__global__ __launch_bounds__(kWave) void k_ct_sel_fixup(const int *__restrict__ non_uniform,
                                                        const int *__restrict__ cnt,
                                                        const int *__restrict__ n2_start,
                                                        unsigned *__restrict__ mask,
                                                        const uint8_t *__restrict__ pattern, int n_pattern) {
    __shared__ uint8_t win[kSelFixWindow];
    const int n = cnt[kSelCntNonUniform], lane = threadIdx.x;
    int carry = 0;
    for (int k0 = 0; k0 < n; k0 += kWave) {
        const int k = k0 + lane, last = min(k0 + kWave, n) - 1 - k0;
        const bool valid = k < n;
        const int c = valid ? non_uniform[k] : 0;
        const int base = valid ? n2_start[c] : 0;  // non-decreasing along the list
        const unsigned m = valid ? mask[c] : 0u;
        // indices of this chunk: [lo, base_last + carry + last]
        const int lo = __shfl(base, 0, kWave) + carry;
        const bool staged = __shfl(base, last, kWave) + carry + last - lo < kSelFixWindow;
        if (staged) {
            __syncthreads();  // the previous chunk's reads of the window
            for (int j = lane; j < kSelFixWindow; j += kWave) win[j] = pattern[min(lo + j, n_pattern - 1)];
            __syncthreads();
        }
        int pick = valid ? 1 : 0;
        for (;;) {
            const unsigned long long picks = __ballot(pick != 0);
            const int at = base + carry + __popcll(picks & ((1ull << lane) - 1ull));
            const int dir = (staged ? win[valid ? at - lo : 0] : pattern[valid ? at : 0]) & 0xF;
            const int now = valid ? (int)((m >> dir) & 1u) : 0;
            const bool changed = __ballot(now != pick) != 0;
            pick = now;
            if (!changed) break;
        }
        if (valid) mask[c] = pick ? 0xFFFFu : 0u;
        carry += __popcll(__ballot(pick != 0));
    }
}

// ---------------------------------------------------------------------------------------------
// makeMaps' sub-selection (PixelSelector2.cc:150-164) and makeNewTraces' walk (FullSystem.cc:1445-1459)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCtThreads) void k_ct_sel_px_count(const uint8_t *__restrict__ map, int n,
                                                                int *__restrict__ blk) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    int total;
    (void)cd_block_prefix(i < n && map[i] != 0, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCtThreads) void k_ct_sel_sub(uint8_t *__restrict__ map, int n, const int *__restrict__ blk,
                                                           const uint8_t *__restrict__ pattern, int char_th,
                                                           int *__restrict__ cnt) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    const bool set = i < n && map[i] != 0;
    int total;
    const int rn = blk[blockIdx.x] + cd_block_prefix(set, &total);
    bool keep = set;
    if (set && pattern[rn] > char_th) {
        map[i] = 0;
        keep = false;
    }
    __syncthreads();
    (void)cd_block_prefix(keep, &total);
    if (threadIdx.x == 0 && total) atomicAdd(&cnt[kSelCntKept], total);
}

// kWrite false: the survivors of each block counted; true: written at their rank, below `capacity`
template <bool kWrite>
__global__ __launch_bounds__(kCtThreads) void k_ct_sel_emit(const float4 *__restrict__ dI0, int w, int h,
                                                            const uint8_t *__restrict__ map, int host,
                                                            int *__restrict__ blk, IpRec *__restrict__ out,
                                                            int capacity) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    bool emit = false;
    IpRec p;
    if (i < w * h) {
        const int x = i % w, y = i / w;
        const uint8_t t = map[i];
        if (t != 0 && x >= 3 && x < w - 4 && y >= 3 && y < h - 4) {
            p = ip_make_record(dI0, w, h, (float)x, (float)y, (float)t, host);
            emit = isfinite(p.energy_th);
        }
    }
    int total;
    const int pre = cd_block_prefix(emit, &total);
    if (!kWrite) {
        if (threadIdx.x == 0) blk[blockIdx.x] = total;
    } else if (emit) {
        const int k = blk[blockIdx.x] + pre;
        if (k < capacity) out[k] = p;
    }
}

}  // namespace
