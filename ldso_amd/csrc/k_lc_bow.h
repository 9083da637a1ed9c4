// k_lc_bow.h -- FeatureMatcher::SearchByBoW (FeatureMatcher.cc:66-124).
//
// The reference walks the two featVec maps together and, where the node ids differ, moves the smaller side
// forward with lower_bound: it visits exactly the nodes present in both maps, in ascending id -- the
// intersection of the two sorted node lists.  So a thread per entry of kf1's vector looks its node up in
// kf2's list by binary search, and an entry whose node is missing there has no match.
//
// Per entry the inner loop is the reference's, sequential in the node's order: best and second-best start at
// 256, a distance below the best moves the best down to second, else one below the second replaces it (two
// features at the minimum make the second-best equal the best); the partner is the first one at the minimum.
// Accepted: best <= th_low and (float)best < nn_ratio * (float)second.  The accepted entries are compacted in
// entry order (node ascending, then kf1's order within the node) by ballot prefix: one block, no atomics.
#pragma once
#include "k_lc_common.h"

#pragma clang fp contract(off)

namespace {

struct LcBowParams {
    LcStore S;
    int slot1, slot2, nodes1, nodes2, entries1, th_low;
    float nn_ratio;
    ldso_lc_match *__restrict__ matches;  // [entries1]
    int *__restrict__ count;              // mapped host memory
};

__global__ __launch_bounds__(kLcThreads) void k_lc_bow(LcBowParams P) {
    const LcStore &S = P.S;
    const ldso_lc_feature *f1 = S.feat + (size_t)P.slot1 * S.F, *f2 = S.feat + (size_t)P.slot2 * S.F;
    const int *node1 = S.bow_node + (size_t)P.slot1 * S.F, *node2 = S.bow_node + (size_t)P.slot2 * S.F;
    const int *begin1 = S.bow_begin + (size_t)P.slot1 * (S.F + 1), *begin2 = S.bow_begin + (size_t)P.slot2 * (S.F + 1);
    const int *idx1 = S.bow_feat + (size_t)P.slot1 * S.F, *idx2 = S.bow_feat + (size_t)P.slot2 * S.F;
    int n = 0;
    for (int e0 = 0; e0 < P.entries1; e0 += kLcThreads) {
        const int e = e0 + threadIdx.x;
        bool ok = false;
        ldso_lc_match m{-1, -1, 256};
        if (e < P.entries1) {
            int lo = 0, hi = P.nodes1;  // the node of entry e: the last one that begins at or before e and is not empty
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (begin1[mid] <= e) lo = mid;
                else hi = mid;
            }
            const int id = node1[lo];
            int a = 0, b = P.nodes2;  // lower_bound of id in kf2's node list
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (node2[mid] < id) a = mid + 1;
                else b = mid;
            }
            if (a < P.nodes2 && node2[a] == id) {
                const int i1 = idx1[e];
                const ldso_lc_feature &fa = f1[i1];
                int best1 = 256, best_idx2 = -1, best2 = 256;
                for (int k = begin2[a]; k < begin2[a + 1]; k++) {
                    const int i2 = idx2[k];
                    const int d = lc_distance(fa, f2[i2]);
                    if (d < best1) {
                        best2 = best1;
                        best1 = d;
                        best_idx2 = i2;
                    } else if (d < best2) {
                        best2 = d;
                    }
                }
                if (best1 <= P.th_low && (float)best1 < P.nn_ratio * (float)best2) {
                    ok = true;
                    m.index1 = i1;
                    m.index2 = best_idx2;
                    m.dist = best1;
                }
            }
        }
        int total;
        const int pre = lc_block_prefix(ok, &total);
        if (ok) P.matches[n + pre] = m;
        n += total;
    }
    if (threadIdx.x == 0) *P.count = n;
}

}  // namespace
