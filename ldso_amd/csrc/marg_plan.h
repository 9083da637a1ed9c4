// marg_plan.h -- the host planner of ldso_ba_load_marginalization_device: checks a selection of a
// loaded window's points and residuals, lays the marginalisation window out with build_layout and
// says, per device-order residual and point of that layout, where its state lies in the parent's
// device arrays.  Host-only code like edit_plan.cpp (no offload architecture), so it runs on a CPU,
// under a sanitizer, and in tests that need no GPU.
#pragma once
#include <vector>

#include "edit_plan.h"
#include "layout.h"

namespace ldso_ba {

struct MargPlan {
    // build_layout(marg = true) of the selected structure: every index array is the one
    // ldso_ba_load_marginalization uploads for the explicit window.  Its value arrays (rs_state,
    // rs_energy, rs_flags, pt_data) are placeholders nobody uploads.
    Layout L;
    // per device-order residual / point of L: its device position in the parent's window
    std::vector<int> rs_gather, pt_gather;
    // the selected structure in the marginalisation window's caller order: per point its residual
    // range, per residual its caller index in the parent and its target frame
    std::vector<int> res_begin, res_parent, res_target, point_host;
};

// parent_h / parent_d: the parent's window as build_layout left it (unsharded).  frame_terms: only
// the frame-level fields are read (the point and residual fields are replaced by the selection).
// points [n_points]: distinct caller indices of the parent; res_live [parent R] or nullptr (all).
// item_order, top_chunk: the marginalisation context's tuning keys.  Returns 0, or -1 with the
// thread's error message set and `out` unspecified.
int plan_marg(const WinHost &parent_h, const WinDesc &parent_d, const ldso_ba_window &frame_terms, int n_points,
              const int32_t *points, const uint8_t *res_live, int item_order, int top_chunk, MargPlan &out);

}  // namespace ldso_ba
