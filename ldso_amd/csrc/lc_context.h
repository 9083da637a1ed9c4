// lc_context.h -- the loop closer's host-side state: struct ldso_lc_ctx, whose members (hip_owning.h) own
// every buffer and event: deleting the context frees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../include/ldso_lc.h"
#include "hip_owning.h"
#include "k_lc_common.h"
#include "k_lc_index.h"
#include "k_lc_brute.h"
#include "k_lc_bow.h"
#include "k_lc_map.h"
#include "k_lc_project.h"

// one slot of the store as the host knows it
struct LcSlot {
    int64_t kf = -1;              // the caller's id; -1: free
    int n = 0, corners = 0;       // features, corners among them
    int bow_nodes = -1, bow_entries = 0;  // featVec; -1 nodes: none set
    std::vector<uint8_t> corner;  // [n] the corner flags (set_bow's check)
};

struct ldso_lc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int w = 0, h = 0, max_kf = 0, F = 0;
    // the store: max_kf + 1 slots, so that a put always has a free one to build in and a failed put leaves
    // the keyframe it would have replaced as it was
    std::vector<LcSlot> slots;
    std::unordered_map<int64_t, int> by_id;
    int n_stored = 0;
    DevBuf<ldso_lc_feature> d_feat;
    DevBuf<uint4> d_cdesc;
    DevBuf<int> d_cidx, d_cell_begin, d_cell_feat, d_bow_node, d_bow_begin, d_bow_feat;
    LcStore S{};
    // put: staging, the index kernel's scratch and what it reports (mapped host memory)
    PinBuf<ldso_lc_feature> h_feat;
    PinBuf<int> h_ints;  // set_bow's three lists, update's flags
    PinBuf<float> h_floats;
    DevBuf<int> d_ints;
    DevBuf<float> d_floats;
    DevBuf<int> d_ckey, d_skey;
    PinMappedOf<int> idx_status;
    PinMappedOf<uint8_t> idx_corner;
    // searches: the other keyframes of a brute-force call, its per-corner results and matches; the matches
    // of the BoW search and the records of the projection search; the counts in mapped host memory
    PinBuf<int2> h_pairs;
    DevBuf<int2> d_pairs;
    DevBuf<int> d_bf_idx, d_bf_dist, d_bf_counts;
    DevBuf<ldso_lc_match> d_matches;
    DevBuf<ldso_lc_projection> d_proj;
    PinMappedOf<int> count;
    // the inverse-depth map and its contributions
    DevBuf<float> d_map;
    DevBuf<float4> d_contrib;
    PinBuf<float4> h_contrib;
    bool have_map = false;
    StreamBorrow borrow;  // the tracker's detection, the BA pass's arrays
};
