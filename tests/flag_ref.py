"""FullSystem::removeOutliers' and flagPointsForRemoval's decision restated in numpy, point by point,
from the reference's lines (paths relative to n-lalanne/LDSO):

  removeOutliers                 src/frontend/FullSystem.cc:1646-1665 (a point without residuals goes)
  linearizeAll_Reductor          :1795-1820 (a residual that is not isActive() after the fix pass is
                                 dropped; numGoodResiduals++ for every isNew one that stays, and LDSO
                                 never clears isNew)
  linearizeAll's lastResiduals   :1745-1751 (lastResiduals[i].second follows the residual's state)
  flagPointsForRemoval           :1356-1424
  PointHessian::isOOB            include/internal/PointHessian.h:53-73
  PointHessian::isInlierNew      :75-78

A residual counts for its point when it is live: flags & FLAG_ACTIVE.  The statuses are
ldso_ba.h's LDSO_BA_PT_*."""
import numpy as np

from ldso_amd import _lib as L

ACTIVE, OUTLIER, OUT, MARGINALIZED = L.PT_ACTIVE, L.PT_OUTLIER, L.PT_OUT, L.PT_MARGINALIZED


def flag_points(w, state, flags, idepth_scaled, idepth_hessian, frame_flagged, num_good, last_res, last_state,
                min_good_active=3, min_good=4, min_idepth_h=50.0):
    """w: the window's structure (point_host, point_res_begin, res_target); state, flags [R] and
    idepth_scaled, idepth_hessian [P] as the device holds them; the bookkeeping arrays as
    ldso_ba_flag_points takes them.  Returns its outputs (status, res_live, num_good, last_state, counts)
    and, for the coverage tests, what decided each point: n_res, n_live, vis, the three isOOB exits
    e1 / e2 / e3, host_flagged, and isInlierNew's halves inl_a / inl_g."""
    P, R = w.n_points, w.n_residuals
    A, G = int(min_good_active), int(min_good)
    th = np.float32(min_idepth_h)
    state = np.asarray(state, np.int8)
    flags = np.asarray(flags, np.uint8)
    idepth_scaled = np.asarray(idepth_scaled, np.float32)
    idepth_hessian = np.asarray(idepth_hessian, np.float32)
    last_res = np.asarray(last_res, np.int32).reshape(P, 2)
    last_state = np.asarray(last_state, np.int8).reshape(P, 2)
    o = dict(status=np.zeros(P, np.int8), res_live=(flags & L.FLAG_ACTIVE).astype(np.uint8), num_good=np.zeros(P, np.int32),
             last_state=np.zeros((P, 2), np.int8), counts=np.zeros(4, np.int32))
    d = {k: np.zeros(P, bool) for k in ("e1", "e2", "e3", "host_flagged", "inl_a", "inl_g")}
    d.update(n_res=np.diff(w.point_res_begin).astype(np.int32), n_live=np.zeros(P, np.int32), vis=np.zeros(P, np.int32))
    for p in range(P):
        ks = range(int(w.point_res_begin[p]), int(w.point_res_begin[p + 1]))
        live = [k for k in ks if flags[k] & L.FLAG_ACTIVE]
        n_live = len(live)  # residuals.size() after the reductor's drops
        vis = sum(1 for k in live if state[k] == L.RES_IN and frame_flagged[w.res_target[k]])  # isOOB: visInToMarg
        ls = [int(state[last_res[p, i]]) if last_res[p, i] >= 0 else int(last_state[p, i]) for i in range(2)]
        for i in range(2):
            assert last_res[p, i] == -1 or last_res[p, i] in ks, "last_res names a residual of another point"
        ng = int(num_good[p]) + n_live
        e1 = n_live >= A and ng > G + 10 and n_live - vis < A
        e2 = ls[0] == L.RES_OOB
        e3 = n_live >= 2 and ls[0] == L.RES_OUTLIER and ls[1] == L.RES_OUTLIER
        hf = bool(frame_flagged[w.point_host[p]])
        inl_a, inl_g = n_live >= A, ng >= G
        if idepth_scaled[p] < 0 or n_live == 0:
            st = OUTLIER
        elif e1 or e2 or e3 or hf:
            st = MARGINALIZED if inl_a and inl_g and idepth_hessian[p] > th else OUT
        else:
            st = ACTIVE
        o["status"][p] = st
        o["num_good"][p] = ng
        o["last_state"][p] = ls
        o["counts"][st] += 1
        for k, v in (("e1", e1), ("e2", e2), ("e3", e3), ("host_flagged", hf), ("inl_a", inl_a), ("inl_g", inl_g)):
            d[k][p] = v
        d["n_live"][p] = n_live
        d["vis"][p] = vis
    return o, d
