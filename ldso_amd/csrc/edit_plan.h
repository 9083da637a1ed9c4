// edit_plan.h -- the host planner of ldso_ba_edit_window: checks an edit against the loaded window,
// lays the edited window out with build_layout and says, per device-order residual and point of the
// new layout, where its carried state lies in the old device arrays.  Host-only code like layout.cpp
// (no offload architecture), so it runs on a CPU, under a sanitizer, and in tests that need no GPU.
#pragma once
#include <vector>

#include "layout.h"

namespace ldso_ba {

// A loaded (unsharded) window's structure in caller order, read back from what build_layout left:
// what the planners and ldso_ba_flag_points translate the caller's indices with.
struct OldWindow {
    int N = 0, P = 0, R = 0;
    std::vector<int> pt_pos, rs_pos;       // caller index -> device position
    std::vector<int> pt_host;              // caller point -> host frame
    std::vector<int> rs_point, rs_target;  // caller residual -> caller point, target frame
};
void read_old(const WinHost &H, const WinDesc &D, OldWindow &o);
// The planners' self-check (ldso_ba_edit_plan_check, ldso_ba_marg_plan_check): the number of index
// arrays (work items, record slots, target lists, counts, the descriptor's bases, device orders,
// totals) in which two single-window layouts differ.
int layout_index_mismatches(const Layout &L, const Layout &A);

struct EditPlan {
    // build_layout(after) with item order 0 or 1: every index array is the one a fresh load of the
    // edited window uploads.  Its value arrays (rs_state, rs_energy, rs_flags, pt_data) hold the
    // caller's values at new entries only; at carried entries they are placeholders nobody uploads.
    Layout L;
    // per device-order residual / point of L: the old device position (>= 0), or ~rank (< 0) with
    // rank the entry's index in new_res / new_pts
    std::vector<int> rs_gather, pt_gather;
    // the new entries (src == -1) as caller indices of `after`, ascending: what the compact upload holds
    std::vector<int> new_res, new_pts;
};

// old_h / old_d: the loaded window as build_layout left it (one unsharded window).  item_order and
// top_chunk: the context's tuning keys.  Returns 0, or -1 with the thread's error message set and
// `out` unspecified; nothing else is touched.
int plan_edit(const WinHost &old_h, const WinDesc &old_d, const ldso_ba_edit &e, int item_order, int top_chunk,
              EditPlan &out);

}  // namespace ldso_ba
