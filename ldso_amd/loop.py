"""ctypes face of include/ldso_lc.h: the loop closer's keyframe feature store and its three searches
(SearchBruteForce, SearchByBoW, ComputeOptimizedPose's projection search) on the device.  No compute of its
own: every method hands arrays to the C ABI and returns what it wrote."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class LoopMatcher:
    def __init__(self, width: int, height: int, max_keyframes: int = 64, max_features: int = 2048, device: int = 0):
        h = C.c_void_p()
        L.check(L.lib().ldso_lc_create(int(device), int(width), int(height), int(max_keyframes), int(max_features),
                                       C.byref(h)))
        self._h = h
        self.width, self.height = int(width), int(height)
        self.max_keyframes, self.max_features = int(max_keyframes), int(max_features)

    def close(self):
        if self._h and self._h.value:
            L.lib().ldso_lc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the store
    def put(self, kf: int, feats: np.ndarray):
        feats = _arr(feats, L.LC_FEATURE_DTYPE)
        L.check(L.lib().ldso_lc_keyframe_put(self._h, int(kf), int(feats.size), feats.ctypes.data))

    def put_tracker(self, kf: int, tracker):
        L.check(L.lib().ldso_lc_keyframe_put_tracker(self._h, int(kf), tracker._h))

    def update(self, kf: int, inv_d, usable):
        inv_d, usable = _arr(inv_d, np.float32), _arr(usable, np.int32)
        assert inv_d.size == usable.size
        L.check(L.lib().ldso_lc_keyframe_update(self._h, int(kf), int(inv_d.size), L.ptr(inv_d, L.f32p),
                                                L.ptr(usable, L.i32p)))

    def set_bow(self, kf: int, node_id, node_begin, feat_idx):
        node_id, node_begin, feat_idx = _arr(node_id, np.int32), _arr(node_begin, np.int32), _arr(feat_idx, np.int32)
        assert node_begin.size == node_id.size + 1
        L.check(L.lib().ldso_lc_keyframe_set_bow(self._h, int(kf), int(node_id.size), L.ptr(node_id, L.i32p),
                                                 L.ptr(node_begin, L.i32p), L.ptr(feat_idx, L.i32p)))

    def get(self, kf: int) -> np.ndarray:
        out = np.zeros(self.max_features, L.LC_FEATURE_DTYPE)
        n = C.c_int32()
        L.check(L.lib().ldso_lc_keyframe_get(self._h, int(kf), int(out.size), out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def drop(self, kf: int):
        L.check(L.lib().ldso_lc_keyframe_drop(self._h, int(kf)))

    # ---- the searches
    def search_brute_force(self, kf1: int, kf2: int, th_low: int = 50, capacity: int | None = None) -> np.ndarray:
        out = np.zeros(self.max_features if capacity is None else capacity, L.LC_MATCH_DTYPE)
        n = C.c_int32()
        L.check(L.lib().ldso_lc_search_brute_force(self._h, int(kf1), int(kf2), int(th_low), int(out.size),
                                                   out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def search_brute_force_many(self, kf1: int, kf_ids, n_corners: int, th_low: int = 50, details: bool = True):
        """(counts [n_kf], idx [n_kf][n_corners], dist [n_kf][n_corners]); n_corners: kf1's corner count."""
        ids = _arr(kf_ids, np.int64)
        counts = np.zeros(ids.size, np.int32)
        idx = np.zeros((ids.size, n_corners), np.int32) if details else None
        dist = np.zeros((ids.size, n_corners), np.int32) if details else None
        L.check(L.lib().ldso_lc_search_brute_force_many(self._h, int(kf1), int(ids.size), L.ptr(ids, L.i64p), int(th_low),
                                                        L.ptr(counts, L.i32p), L.ptr(idx, L.i32p), L.ptr(dist, L.i32p)))
        return counts, idx, dist

    def search_by_bow(self, kf1: int, kf2: int, th_low: int = 50, nn_ratio: float = 0.6,
                      capacity: int | None = None) -> np.ndarray:
        out = np.zeros(self.max_features if capacity is None else capacity, L.LC_MATCH_DTYPE)
        n = C.c_int32()
        L.check(L.lib().ldso_lc_search_by_bow(self._h, int(kf1), int(kf2), int(th_low), float(nn_ratio), int(out.size),
                                              out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def make_idepth_map(self, centers) -> np.ndarray:
        centers = _arr(centers, np.float32).reshape(-1, 3)
        L.check(L.lib().ldso_lc_make_idepth_map(self._h, int(centers.shape[0]), L.ptr(centers, L.f32p)))
        return self.idepth_map()

    def make_idepth_map_from(self, ba_ctx, win: int, target_frame: int = -1) -> np.ndarray:
        out = np.zeros((self.height, self.width), np.float32)
        L.check(L.lib().ldso_lc_make_idepth_map_ba(self._h, ba_ctx._h, int(win), int(target_frame), L.ptr(out, L.f32p)))
        return out

    def idepth_map(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), np.float32)
        L.check(L.lib().ldso_lc_get_idepth_map(self._h, L.ptr(out, L.f32p)))
        return out

    def search_by_projection(self, kf_cur: int, kf_cand: int, calib, scr, window_size: float = 5.0, th_high: int = 50,
                             capacity: int | None = None) -> np.ndarray:
        calib, scr = _arr(calib, np.float32), _arr(scr, np.float64)
        assert calib.size == 8 and scr.size == 7
        out = np.zeros(self.max_features if capacity is None else capacity, L.LC_PROJECTION_DTYPE)
        n = C.c_int32()
        L.check(L.lib().ldso_lc_search_by_projection(self._h, int(kf_cur), int(kf_cand), L.ptr(calib, L.f32p),
                                                     L.ptr(scr, L.f64p), float(window_size), int(th_high), int(out.size),
                                                     out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()
