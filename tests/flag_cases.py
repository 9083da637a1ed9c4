"""The windows and the per-point bookkeeping the ldso_ba_flag_points tests share (test_flag_cases on
the CPU, test_flag_parity on the GPU).

The windows are selections of edit_cases' ragged pool (160 x 120, states, energies and flags mixed
by ragged.frontend_window), a few of their records given idepth_scaled < 0 before the load.  The
bookkeeping -- frame_flagged, num_good, last_res, last_state -- is what the frontend would hold
without any read-back; here it is constructed, from the residual states and flags the decision
will see, so that every branch of the tree decides some point: each point takes, of the recipes it
can carry, the one used least so far.  test_flag_cases asserts from flag_ref alone that every
branch is indeed reached."""
import functools

import numpy as np

import edit_cases as ec
import flag_ref
from ldso_amd import _lib as L

IN, OOB, OUTLIER = L.RES_IN, L.RES_OOB, L.RES_OUTLIER

# name -> (selection of the pool, (min_good_active_res_for_marg, min_good_res_for_marg))
CASES = {
    "pool5": (lambda pool: ec.full_sel(pool, range(5)), (3, 4)),  # N = 5, 400 points, Setting.cc's 3 and 4
    "base4": (ec.base_sel, (2, 3)),                               # N = 4, 70 points: the layout's edges
}
# with no pass run idepth_hessian is 0 everywhere: -1 makes every inlier candidate MARGINALIZED, 50 (the
# default) every one OUT
THRESHOLDS = (-1.0, 50.0)


@functools.lru_cache(maxsize=None)
def window(name, ranked=False):
    """The case's window; every 23rd record has idepth_scaled < 0.  ranked: with a point_rank, so
    that the device's point order is not the caller's within a host either."""
    pool = ec.make_pool()
    w = ec.window_of(pool, CASES[name][0](pool), rank=ranked)
    w.point_data = w.point_data.copy()
    w.point_data[5::23, 2] = -np.abs(w.point_data[5::23, 2]) - np.float32(0.01)
    return w


def bookkeeping(w, state, flags, A, G, flagged_frames=(0,)):
    """(frame_flagged [N], num_good [P], last_res [P][2], last_state [P][2]) for the window w whose
    residuals have `state` and `flags` [R] when the decision is made."""
    P, N = w.n_points, w.n_frames
    ff = np.zeros(N, np.uint8)
    ff[list(flagged_frames)] = 1
    ng = np.zeros(P, np.int32)
    lr = np.full((P, 2), -1, np.int32)
    ls = np.full((P, 2), IN, np.int8)
    used = [0] * 8
    for p in range(P):
        ks = list(range(int(w.point_res_begin[p]), int(w.point_res_begin[p + 1])))
        live = [k for k in ks if flags[k] & L.FLAG_ACTIVE]
        n_live = len(live)
        vis = sum(1 for k in live if state[k] == IN and ff[w.res_target[k]])
        by_state = {s: [k for k in ks if state[k] == s] for s in (IN, OOB, OUTLIER)}

        def plain():  # not out of bounds by any exit: the host decides
            ng[p] = G
            if by_state[IN]:
                lr[p, 0] = by_state[IN][0]
            return True

        def exit1():  # many good residuals, too few left outside the flagged frames
            if not (n_live >= A and n_live - vis < A):
                return False
            ng[p] = G + 11
            lr[p, 0] = live[0]
            ls[p, 1] = OUTLIER
            return True

        def exit2_device():  # lastResiduals[0] is a residual of the window that went OOB
            if not by_state[OOB]:
                return False
            ng[p] = G
            lr[p, 0] = by_state[OOB][0]
            return True

        def exit2_retained(num_good=G):  # lastResiduals[0] was dropped earlier; its OOB state is retained
            ng[p] = num_good
            ls[p, 0] = OOB
            if by_state[IN]:
                lr[p, 1] = by_state[IN][-1]
            return True

        def exit3():  # both last residuals OUTLIER, from the device where the point has such residuals
            if n_live < 2:
                return False
            ng[p] = G
            ls[p] = OUTLIER
            for i, k in enumerate(by_state[OUTLIER][:2]):
                lr[p, i] = k
            return True

        def two_outliers_one_live():  # isOOB returns false at residuals.size() < 2
            if n_live >= 2:
                return False
            ng[p] = G
            ls[p] = OUTLIER
            return True

        def few_good():  # isInlierNew fails on numGoodResiduals alone
            if not (A <= n_live < G):
                return False
            return exit2_retained(num_good=0)

        def few_live():  # isInlierNew fails on residuals.size() alone
            if not (0 < n_live < A):
                return False
            return exit2_retained(num_good=G + 5)

        recipes = [plain, exit1, exit2_device, exit2_retained, exit3, two_outliers_one_live, few_good, few_live]
        for i in sorted(range(len(recipes)), key=lambda i: (used[i], i)):  # the least used recipe the point can carry
            if recipes[i]():
                used[i] += 1
                break
    return ff, ng, lr, ls


def reference(w, state, flags, idepth_scaled, idepth_hessian, book, A, G, th):
    return flag_ref.flag_points(w, state, flags, idepth_scaled, idepth_hessian, *book, min_good_active=A, min_good=G,
                                min_idepth_h=th)


def loaded_case(name, ranked=False):
    """(window, (A, G), bookkeeping) of a case decided on the states as they are loaded."""
    w = window(name, ranked)
    A, G = CASES[name][1]
    return w, (A, G), bookkeeping(w, w.res_state, w.res_flags, A, G)
