"""CoarseTracker face over the C ABI in include/ldso_ct.h.

Mirrors the reference class (src/frontend/CoarseTracker.cc) for the parts that run on the GPU:

    CoarseTracker(w, h)                   -> CoarseTracker(width, height)
    makeK(HCalib)                         -> make_k(calib)                     CoarseTracker.cc:312-339
    newFrame->makeImages(color, HCalib)   -> set_new_frame(color, exposure)    FrameHessian.cc:59-115
    undistorter->undistort(raw, exposure) and makeImages of its image
                                          -> undistort_init(...) once, then
                                             set_new_frame_raw(raw, exposure)  Undistort.cc:190-230, 398-453
                                             undistorted() reads the image back
    Undistort's constructor (the tables)  -> make_remap(...), make_photometric(...)
                                                                               Undistort.cc:86-154, 558-1125
    setCoarseTrackingRef's pc_* outputs   -> set_reference(levels, ...)        CoarseTracker.cc:357-538
    makeCoarseDepthL0 on the device       -> make_reference(center, hdi, ...)  CoarseTracker.cc:357-538
                                             make_reference_from(ba_ctx, win)  FullSystem.cc:613-621
                                             reference(lvl) reads the cloud back
    calcRes(lvl, refToNew, aff, cutoff)   -> calc_res(lvl, T, aff, cutoff)     CoarseTracker.cc:540-673
    calcGSSSE(lvl, H, b, refToNew, aff)   -> calc_gs(lvl, T, aff)              CoarseTracker.cc:675-741
    calcRes + calcGSSSE at one pose       -> calc_res_gs(lvl, T, aff, cutoff)  CoarseTracker.cc:90-105, 218-245
    trackNewestCoarse(fh, T, aff, lvl, minRes)
                                          -> track(T, aff, min_res, ...)       CoarseTracker.cc:61-310
                                             lm_step(H, b, lambda, T, aff)     CoarseTracker.cc:130-213
    new ImmaturePoint(newFrame, feat, ..) -> make_immature(uv, type, host)     ImmaturePoint.cc:14-39
    traceNewCoarse -> ImmaturePoint::traceOn
                                          -> trace(krki, kt, aff)              FullSystem.cc:1157-1194,
                                             (records resident: immature_upload / immature_download /
                                              immature_append)                 ImmaturePoint.cc:47-317
    CoarseDistanceMap::makeDistanceMap    -> make_distance_map(krki1, kt1, uvd, host)
                                             make_distance_map_ba(ba_ctx, win) CoarseTracker.cc:795-932
    activatePointsMT's walk               -> select_activation(...)            FullSystem.cc:1220-1298
    PixelSelector(w, h)                   -> select_init(pattern, potential)   PixelSelector2.cc:9-18
    makeMaps(fh, map, density, ...)       -> select_pixels(density=..., ...)   PixelSelector2.cc:111-169
    makeNewTraces (pointSelection == 0)   -> make_new_traces(host, ...)        FullSystem.cc:1439-1461
    FeatureDetector()                     -> corners_init(bit_pattern)         FeatureDetector.cc:10-28
    DetectCorners + makeNewTraces (pointSelection == 1)
                                          -> detect_corners(n_features, host)  FeatureDetector.cc:34-189,
                                                                               FullSystem.cc:1428-1438

CoarseInitializer (src/frontend/CoarseInitializer.cc) on a tracker's frames:

    setFirst's state from ready-made lists -> CoarseInitializer(tracker).set_first(levels)   :656-737
    trackFrame(newFrame)                  -> track_frame(...)                  :45-183
    calcResAndGS                          -> eval(lvl, T, aff)                 :186-342
    the LM step                           -> init_lm_step(H, b, Hsc, bsc, ...) :95-116

No numerical work happens here; every call goes to libldso_ba.so (no fallback).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def track_params(**params) -> "L.LdsoCtTrackParams":
    """ldso_ct_track_params: the defaults with the given fields replaced (max_iterations: 5 ints)."""
    p = L.LdsoCtTrackParams()
    L.lib().ldso_ct_track_default_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError(f"unknown tracking parameter {k!r}")
        setattr(p, k, (C.c_int32 * 5)(*v) if k == "max_iterations" else v)
    return p


def lm_step(H, b, lam: float, ref_to_new, aff_ab, **params):
    """One LM step of trackNewestCoarse on the host (ldso_ct_lm_step) -> (inc [8], pose [3][4], aff [2])."""
    H = np.ascontiguousarray(H, np.float64).reshape(64)
    b = np.ascontiguousarray(b, np.float64).reshape(8)
    T = np.ascontiguousarray(np.asarray(ref_to_new, np.float64)[:3, :4])
    ab = np.ascontiguousarray(aff_ab, np.float64).reshape(2)
    inc, To, abo = np.zeros(8), np.zeros((3, 4)), np.zeros(2)
    p = track_params(**params)
    L.check(L.lib().ldso_ct_lm_step(L.ptr(H, L.f64p), L.ptr(b, L.f64p), float(lam), L.ptr(T, L.f64p), L.ptr(ab, L.f64p),
                                    C.byref(p), L.ptr(inc, L.f64p), L.ptr(To, L.f64p), L.ptr(abo, L.f64p)))
    return inc, To, abo


def make_remap(model: str, pars, w_org: int, h_org: int, w: int, h: int, out="crop"):
    """The remap tables of the reference's Undistort constructor on the host (ldso_ct_undistort_make_remap).
    model: one of _lib.UNDISTORT_MODELS; pars: the calibration's first line (5 or 8 numbers); out: "crop",
    "none" or the third line's (fx, fy, cx, cy) relative to the output size.
    Returns (K {fx, fy, cx, cy} float64, remap_x [h*w], remap_y [h*w], passthrough)."""
    p = np.zeros(8, np.float64)
    pars = np.asarray(pars, np.float64).reshape(-1)
    p[:pars.size] = pars
    if isinstance(out, str):
        mode, oc = L.UNDISTORT_OUT.index(out), None
    else:
        mode, oc = L.UNDISTORT_OUT.index("calib"), _f32(out).reshape(-1)[:4].copy()
    K = np.zeros(4, np.float64)
    rx, ry = np.zeros(int(w) * int(h), np.float32), np.zeros(int(w) * int(h), np.float32)
    passthrough = C.c_int32()
    L.check(L.lib().ldso_ct_undistort_make_remap(L.UNDISTORT_MODELS.index(model), L.ptr(p, L.f64p), int(w_org), int(h_org),
                                                 int(w), int(h), mode, L.ptr(oc, L.f32p), L.ptr(K, L.f64p),
                                                 L.ptr(rx, L.f32p), L.ptr(ry, L.f32p), C.byref(passthrough)))
    return K, rx, ry, bool(passthrough.value)


def make_photometric(g_raw, vignette, photometric_mode: int = 2):
    """G and vignetteMapInv of the reference's PhotometricUndistorter on the host
    (ldso_ct_undistort_make_photometric) from the photometric text's first line g_raw and the vignette
    image's pixels (uint8 or uint16) -> (g [g_depth], vignette_inv, shaped as vignette)."""
    g_raw = _f32(g_raw).reshape(-1)
    v = np.ascontiguousarray(vignette)
    assert v.dtype in (np.uint8, np.uint16), "vignette images are uint8 or uint16"
    g = np.zeros(g_raw.size, np.float32)
    vi = np.zeros(v.shape, np.float32)
    L.check(L.lib().ldso_ct_undistort_make_photometric(L.ptr(g_raw, L.f32p), int(g_raw.size), v.ctypes.data,
                                                       8 * v.itemsize, int(v.size), int(photometric_mode),
                                                       L.ptr(g, L.f32p), L.ptr(vi, L.f32p)))
    return g, vi


class CoarseTracker:
    def __init__(self, width: int, height: int, device: int = 0):
        lib = L.lib()
        h = C.c_void_p()
        nl = C.c_int32()
        L.check(lib.ldso_ct_create(int(device), int(width), int(height), C.byref(h), C.byref(nl)))
        self._h = h
        self.width, self.height, self.levels = int(width), int(height), int(nl.value)

    def close(self):
        if self._h and self._h.value:
            L.lib().ldso_ct_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def make_k(self, calib) -> np.ndarray:
        """Per level {fx, fy, cx, cy, Ki[9]} (13 floats)."""
        out = np.zeros((self.levels, 13), np.float32)
        L.check(L.lib().ldso_ct_make_k(self._h, L.ptr(_f32(calib), L.f32p), L.ptr(out, L.f32p)))
        return out

    def set_new_frame(self, color, ab_exposure: float = 1.0, b_response=None):
        color = _f32(color).reshape(-1)
        assert color.size == self.width * self.height
        B = None if b_response is None else _f32(b_response)
        assert B is None or B.size == 256
        L.check(L.lib().ldso_ct_set_new_frame(self._h, L.ptr(color, L.f32p), float(ab_exposure), L.ptr(B, L.f32p)))

    # ---- frame ingestion from the raw image (Undistort::undistort, PhotometricUndistorter::processFrame) ----
    def undistort_init(self, w_org: int, h_org: int, remap=None, g=None, vignette_inv=None,
                       photometric_mode: int = 2, use_exposure: bool = True) -> int:
        """The undistorter's tables, once (ldso_ct_undistort_init).  remap: (remap_x, remap_y), each
        [height*width] at the tracker's size (make_remap's), or None for passthrough; g, vignette_inv:
        make_photometric's tables, or None for no photometric calibration.  Returns how many entries the
        footprint rule (include/ldso_ct.h) stored as -1."""
        n = self.width * self.height
        rx = ry = None
        if remap is not None:
            rx, ry = (None if a is None else _f32(a).reshape(-1) for a in remap)
            assert all(a is None or a.size == n for a in (rx, ry)), "remap tables are [height*width]"
        G = None if g is None else _f32(g).reshape(-1)
        vi = None if vignette_inv is None else _f32(vignette_inv).reshape(-1)
        assert vi is None or vi.size == int(w_org) * int(h_org), "vignette_inv is [h_org*w_org]"
        d = L.LdsoCtUndistortDesc(int(w_org), int(h_org), L.ptr(rx, L.f32p), L.ptr(ry, L.f32p), L.ptr(G, L.f32p),
                                  0 if G is None else int(G.size), L.ptr(vi, L.f32p), int(photometric_mode),
                                  int(bool(use_exposure)))
        outside = C.c_int32()
        L.check(L.lib().ldso_ct_undistort_init(self._h, C.byref(d), C.byref(outside)))
        self._raw_n = int(w_org) * int(h_org)
        return int(outside.value)

    def set_new_frame_raw(self, raw, exposure: float = 1.0, factor: float = 1.0, b_response=None, stream=None) -> float:
        """Undistort::undistort of a raw frame [h_org*w_org] and makeImages of its image.  raw: a NumPy uint8 /
        uint16 array, or a torch tensor of those types on the GPU, read there with no host synchronisation
        (ldso_ct_set_new_frame_raw_device; stream: the torch stream or raw hipStream_t that produced it,
        None = torch's current stream; the tensor must stay alive until the stream work has run).  Returns
        ImageAndExposure::exposure_time."""
        B = None if b_response is None else _f32(b_response)
        assert B is None or B.size == 256
        out = C.c_float()
        lib = L.lib()
        if isinstance(raw, np.ndarray):
            assert raw.dtype in (np.uint8, np.uint16), "raw frames are uint8 or uint16"
            a = np.ascontiguousarray(raw).reshape(-1)
            assert a.size == getattr(self, "_raw_n", a.size), "raw is [h_org*w_org]"
            L.check(lib.ldso_ct_set_new_frame_raw(self._h, a.ctypes.data, 8 * a.itemsize, float(exposure), float(factor),
                                                  L.ptr(B, L.f32p), C.byref(out)))
            return float(out.value)
        import torch

        assert isinstance(raw, torch.Tensor) and raw.is_cuda and raw.is_contiguous(), \
            "raw frames are NumPy arrays or contiguous CUDA tensors"
        assert raw.dtype in (torch.uint8, torch.uint16), "raw frames are uint8 or uint16"
        assert raw.numel() == getattr(self, "_raw_n", raw.numel()), "raw is [h_org*w_org]"
        if stream is None:
            stream = torch.cuda.current_stream()
        sp = getattr(stream, "cuda_stream", stream)
        L.check(lib.ldso_ct_set_new_frame_raw_device(self._h, C.c_void_p(raw.data_ptr()), 8 * raw.element_size(),
                                                     float(exposure), float(factor), L.ptr(B, L.f32p),
                                                     C.c_void_p(int(sp or 0)), C.byref(out)))
        return float(out.value)

    def undistorted(self) -> np.ndarray:
        """The new frame's level-0 image [height, width] (ImageAndExposure::image), read back."""
        img = np.zeros((self.height, self.width), np.float32)
        L.check(L.lib().ldso_ct_get_undistorted(self._h, L.ptr(img, L.f32p)))
        return img

    def frame_level(self, lvl: int):
        wl, hl = self.width >> lvl, self.height >> lvl
        dI = np.zeros((hl * wl, 3), np.float32)
        ag = np.zeros(hl * wl, np.float32)
        L.check(L.lib().ldso_ct_get_frame_level(self._h, int(lvl), L.ptr(dI, L.f32p), L.ptr(ag, L.f32p)))
        return dI, ag

    def set_reference(self, pc, ab_exposure: float = 1.0, aff_ab=(0.0, 0.0)):
        """pc: per level a dict/tuple (u, v, idepth, color) of equal-length float arrays."""
        assert len(pc) == self.levels
        keep = []
        n = np.zeros(self.levels, np.int32)
        arrs = [(L.f32p * self.levels)() for _ in range(4)]
        for l, lv in enumerate(pc):
            cols = [lv[k] for k in ("u", "v", "idepth", "color")] if isinstance(lv, dict) else list(lv)
            cols = [_f32(c).reshape(-1) for c in cols]
            n[l] = cols[0].size
            assert all(c.size == n[l] for c in cols)
            for j in range(4):
                keep.append(cols[j])
                arrs[j][l] = L.ptr(cols[j], L.f32p)
        L.check(L.lib().ldso_ct_set_reference(self._h, L.ptr(n, L.i32p), *arrs, float(ab_exposure),
                                              float(aff_ab[0]), float(aff_ab[1])))

    def make_reference(self, center, hdi, ab_exposure: float = 1.0, aff_ab=(0.0, 0.0), frame_src=None) -> np.ndarray:
        """makeCoarseDepthL0 on the device from contributions in traversal order: center [n][3]
        (centerProjectedTo), hdi [n] (HdiF).  frame_src: the tracker whose new frame is the reference
        keyframe (None: this one).  Returns pc_n per level."""
        center = _f32(center).reshape(-1, 3)
        hdi = _f32(hdi).reshape(-1)
        assert center.shape[0] == hdi.size
        n = np.zeros(self.levels, np.int32)
        L.check(L.lib().ldso_ct_make_reference(self._h, None if frame_src is None else frame_src._h, int(hdi.size),
                                               L.ptr(center, L.f32p), L.ptr(hdi, L.f32p), float(ab_exposure),
                                               float(aff_ab[0]), float(aff_ab[1]), L.ptr(n, L.i32p)))
        return n

    def make_reference_from(self, ba_ctx, win: int, ref_frame: int = -1, frame_src=None, ab_exposure: float = 1.0,
                            aff_ab=(0.0, 0.0)) -> np.ndarray:
        """The same from the last pass of a BAContext's window, device to device (ref_frame -1: the
        window's last frame).  Returns pc_n per level."""
        n = np.zeros(self.levels, np.int32)
        L.check(L.lib().ldso_ct_make_reference_ba(self._h, None if frame_src is None else frame_src._h, ba_ctx._h,
                                                  int(win), int(ref_frame), float(ab_exposure), float(aff_ab[0]),
                                                  float(aff_ab[1]), L.ptr(n, L.i32p)))
        return n

    def reference(self, lvl: int) -> np.ndarray:
        """The resident cloud of level lvl as [n][4] {u, v, idepth, color}."""
        n = C.c_int32()
        lib = L.lib()
        L.check(lib.ldso_ct_get_reference(self._h, int(lvl), C.byref(n), L.ptr(None, L.f32p), 0))
        out = np.zeros((n.value, 4), np.float32)
        L.check(lib.ldso_ct_get_reference(self._h, int(lvl), C.byref(n), L.ptr(out, L.f32p), int(n.value)))
        return out

    def calc_res(self, lvl: int, ref_to_new, aff_ab=(0.0, 0.0), cutoff_th: float = 20.0) -> np.ndarray:
        T = np.ascontiguousarray(np.asarray(ref_to_new, np.float64)[:3, :4])
        rs = np.zeros(6, np.float64)
        L.check(L.lib().ldso_ct_calc_res(self._h, int(lvl), L.ptr(T, L.f64p), float(aff_ab[0]), float(aff_ab[1]),
                                         float(cutoff_th), L.ptr(rs, L.f64p)))
        return rs

    def calc_res_batch(self, lvl: int, ref_to_new, aff_ab, cutoff_th: float = 20.0) -> np.ndarray:
        T = np.ascontiguousarray(np.asarray(ref_to_new, np.float64)[:, :3, :4])
        ab = np.ascontiguousarray(aff_ab, np.float64).reshape(-1, 2)
        assert ab.shape[0] == T.shape[0]
        rs = np.zeros((T.shape[0], 6), np.float64)
        L.check(L.lib().ldso_ct_calc_res_batch(self._h, int(lvl), int(T.shape[0]), L.ptr(T, L.f64p),
                                               L.ptr(ab, L.f64p), float(cutoff_th), L.ptr(rs, L.f64p)))
        return rs

    def calc_gs(self, lvl: int, ref_to_new, aff_ab=(0.0, 0.0)):
        T = np.ascontiguousarray(np.asarray(ref_to_new, np.float64)[:3, :4])
        H = np.zeros((8, 8), np.float64)
        b = np.zeros(8, np.float64)
        L.check(L.lib().ldso_ct_calc_gs(self._h, int(lvl), L.ptr(T, L.f64p), float(aff_ab[0]), float(aff_ab[1]),
                                        L.ptr(H, L.f64p), L.ptr(b, L.f64p)))
        return H, b

    def calc_res_gs(self, lvl: int, ref_to_new, aff_ab=(0.0, 0.0), cutoff_th: float = 20.0):
        """calcRes + calcGSSSE at the same pose in one round trip -> (rs[6], H 8x8, b 8).
        The LM loop calls this once per iteration: the pose and result buffers and their ctypes
        pointers are made once per tracker, the results returned as copies."""
        if not hasattr(self, "_lm"):
            bufs = (np.zeros((3, 4), np.float64), np.zeros(6, np.float64), np.zeros((8, 8), np.float64),
                    np.zeros(8, np.float64))
            self._lm = (bufs, tuple(L.ptr(x, L.f64p) for x in bufs), L.lib().ldso_ct_calc_res_gs)
        (T, rs, H, b), (pT, prs, pH, pb), fn = self._lm
        T[...] = np.asarray(ref_to_new, np.float64)[:3, :4]
        L.check(fn(self._h, int(lvl), pT, float(aff_ab[0]), float(aff_ab[1]), float(cutoff_th), prs, pH, pb))
        return rs.copy(), H.copy(), b.copy()

    def track(self, ref_to_new, aff_ab=(0.0, 0.0), min_res_for_abort=None, coarsest_lvl: int | None = None,
              trace: int = 0, **params):
        """trackNewestCoarse on the device, the whole LM loop in one call (ldso_ct_track).  One start
        (ref_to_new [3][4], aff_ab [2]) or a batch ([n][3][4], [n][2]) run concurrently; min_res_for_abort
        [5] or [n][5] (None: NaN, which never aborts, as FullSystem's first try).  coarsest_lvl None: the
        coarsest level the reference tracks from, min(levels, 5) - 1.  params: the fields of
        ldso_ct_track_params.  Returns the result records (_lib.TRACK_RESULT_DTYPE; one record for a single
        start), and with trace > 0 also the first `trace` evaluations of start 0 (_lib.TRACK_STEP_DTYPE) and
        how many there were."""
        T = np.asarray(ref_to_new, np.float64)
        single = T.ndim == 2
        T = np.ascontiguousarray(T.reshape(-1, *T.shape[-2:])[:, :3, :4])
        n = T.shape[0]
        ab = np.ascontiguousarray(np.broadcast_to(np.asarray(aff_ab, np.float64).reshape(-1, 2), (n, 2)))
        mr = np.full(5, np.nan) if min_res_for_abort is None else np.asarray(min_res_for_abort, np.float64)
        mr = np.ascontiguousarray(np.broadcast_to(mr.reshape(-1, 5), (n, 5)))
        lvl = min(self.levels, 5) - 1 if coarsest_lvl is None else int(coarsest_lvl)
        p = track_params(**params)
        out = np.zeros(n, L.TRACK_RESULT_DTYPE)
        steps = np.zeros(max(int(trace), 0), L.TRACK_STEP_DTYPE)
        n_steps = C.c_int32()
        L.check(L.lib().ldso_ct_track(self._h, n, L.ptr(T, L.f64p), L.ptr(ab, L.f64p), lvl, L.ptr(mr, L.f64p),
                                      C.byref(p), out.ctypes.data, steps.ctypes.data if steps.size else None,
                                      int(steps.size), C.byref(n_steps)))
        res = out[0] if single else out
        if trace > 0:
            return res, steps[:min(n_steps.value, steps.size)].copy(), int(n_steps.value)
        return res

    def warped(self) -> np.ndarray:
        """buf_warped_* of the last calc_res as [n][8] {idepth, u, v, dx, dy, residual, weight, refColor}."""
        n = C.c_int32()
        lib = L.lib()
        L.check(lib.ldso_ct_get_warped(self._h, C.byref(n), L.ptr(None, L.f32p), 0))
        out = np.zeros((n.value, 8), np.float32)
        L.check(lib.ldso_ct_get_warped(self._h, C.byref(n), L.ptr(out, L.f32p), int(n.value)))
        return out

    def set_kernel_timing(self, on: bool):
        L.check(L.lib().ldso_ct_set_kernel_timing(self._h, int(bool(on))))

    def kernel_times(self) -> dict:
        lib = L.lib()
        k = lib.ldso_ct_num_kernels()
        ms = np.zeros(k, np.float64)
        cnt = np.zeros(k, np.int64)
        L.check(lib.ldso_ct_get_kernel_times(self._h, L.ptr(ms, L.f64p), L.ptr(cnt, L.i64p), int(k)))
        return {lib.ldso_ct_kernel_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(k)}

    # ---- immature points ----
    def make_immature(self, uv, type_: float = 1.0, host: int = 0) -> np.ndarray:
        """ImmaturePoint(newFrame, feat, type) for features uv [n][2] on the new frame -> records."""
        uv = _f32(uv).reshape(-1, 2)
        out = np.zeros(uv.shape[0], L.IMMATURE_DTYPE)
        L.check(L.lib().ldso_ct_make_immature(self._h, int(uv.shape[0]), L.ptr(uv, L.f32p), float(type_), int(host),
                                              out.ctypes.data))
        return out

    def immature_upload(self, pts: np.ndarray):
        assert pts.dtype == L.IMMATURE_DTYPE and pts.flags.c_contiguous
        L.check(L.lib().ldso_ct_immature_upload(self._h, int(pts.size), pts.ctypes.data))
        self._ip_n = int(pts.size)

    def immature_download(self) -> np.ndarray:
        out = np.zeros(getattr(self, "_ip_n", 0), L.IMMATURE_DTYPE)
        L.check(L.lib().ldso_ct_immature_download(self._h, int(out.size), out.ctypes.data))
        return out

    def trace(self, krki, kt, aff, counts: bool = True):
        """traceNewCoarse over the resident records: per host KRKi [9], Kt [3], aff [2] -> counts [6]
        (GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED) or None."""
        krki = _f32(krki).reshape(-1, 9)
        kt = _f32(kt).reshape(-1, 3)
        aff = _f32(aff).reshape(-1, 2)
        assert krki.shape[0] == kt.shape[0] == aff.shape[0]
        c = np.zeros(6, np.int32) if counts else None
        L.check(L.lib().ldso_ct_trace(self._h, int(krki.shape[0]), L.ptr(krki, L.f32p), L.ptr(kt, L.f32p),
                                      L.ptr(aff, L.f32p), L.ptr(c, L.i32p)))
        return c

    def immature_append(self, pts: np.ndarray):
        """More records behind the resident set (the new keyframe's)."""
        assert pts.dtype == L.IMMATURE_DTYPE and pts.flags.c_contiguous
        L.check(L.lib().ldso_ct_immature_append(self._h, int(pts.size), pts.ctypes.data))
        self._ip_n = getattr(self, "_ip_n", 0) + int(pts.size)

    # ---- activation candidates (CoarseDistanceMap, FullSystem::activatePointsMT's walk) ----
    @property
    def level1_shape(self):
        return self.height >> 1, self.width >> 1

    def make_distance_map(self, krki1, kt1, uvd, host, want_map: bool = True):
        """makeDistanceMap from active points uvd [n][3] {u, v, idepth} with host [n] indexing the level-1
        tables krki1 [n_hosts][9], kt1 [n_hosts][3] -> the map [h1, w1] (None without want_map)."""
        krki1 = _f32(krki1).reshape(-1, 9)
        kt1 = _f32(kt1).reshape(-1, 3)
        uvd = _f32(uvd).reshape(-1, 3)
        host = np.ascontiguousarray(host, np.int32).reshape(-1)
        assert krki1.shape[0] == kt1.shape[0] and uvd.shape[0] == host.size
        m = np.zeros(self.level1_shape, np.float32) if want_map else None
        L.check(L.lib().ldso_ct_make_distance_map(self._h, int(krki1.shape[0]), L.ptr(krki1, L.f32p), L.ptr(kt1, L.f32p),
                                                  int(host.size), L.ptr(uvd, L.f32p), L.ptr(host, L.i32p),
                                                  L.ptr(m, L.f32p)))
        return m

    def make_distance_map_ba(self, ba_ctx, win: int, krki1, kt1, newest: int = -1, want_map: bool = True):
        """The same with the points of a BAContext's window as seeds, device to device (newest -1: the
        window's last frame)."""
        krki1 = _f32(krki1).reshape(-1, 9)
        kt1 = _f32(kt1).reshape(-1, 3)
        assert krki1.shape[0] == kt1.shape[0]
        m = np.zeros(self.level1_shape, np.float32) if want_map else None
        L.check(L.lib().ldso_ct_make_distance_map_ba(self._h, ba_ctx._h, int(win), int(newest), L.ptr(krki1, L.f32p),
                                                     L.ptr(kt1, L.f32p), L.ptr(m, L.f32p)))
        return m

    def select_activation(self, current_min_act_dist: float = 2.0, min_trace_quality: float = 3.0,
                          newest_host: int = -2, flagged=None, compact: bool = False):
        """activatePointsMT's walk over the resident records -> (dispositions [n] of _lib.ACT_*, the
        OPTIMIZE records' indices in walk order, counts dict over _lib.ACTSEL_COUNTS).  newest_host -2:
        the last host of the distance-map call.  compact: the resident set becomes the KEEP records."""
        p = L.LdsoCtActselParams(float(current_min_act_dist), float(min_trace_quality), int(newest_host))
        fl = None if flagged is None else np.ascontiguousarray(flagged, np.uint8).reshape(-1)
        n = getattr(self, "_ip_n", 0)
        disp = np.zeros(n, np.int32)
        idx = np.zeros(n, np.int32)
        ns = C.c_int32()
        cnt = np.zeros(len(L.ACTSEL_COUNTS), np.int32)
        L.check(L.lib().ldso_ct_select_activation(self._h, C.byref(p), L.ptr(fl, L.u8p), int(bool(compact)),
                                                  L.ptr(disp, L.i32p), L.ptr(idx, L.i32p), C.byref(ns),
                                                  L.ptr(cnt, L.i32p)))
        self._as_sel_n = int(ns.value)
        if compact:
            self._ip_n = int(cnt[0])
        return disp, idx[:ns.value].copy(), dict(zip(L.ACTSEL_COUNTS, cnt.tolist()))

    def selection_download(self) -> np.ndarray:
        """The records the last select_activation selected, in walk order."""
        out = np.zeros(getattr(self, "_as_sel_n", 0), L.IMMATURE_DTYPE)
        L.check(L.lib().ldso_ct_selection_download(self._h, int(out.size), out.ctypes.data))
        return out

    # ---- pixel selection (PixelSelector::makeMaps, FullSystem::makeNewTraces with pointSelection 0) ----
    @staticmethod
    def _select_params(params: dict) -> "L.LdsoCtSelectParams":
        p = L.LdsoCtSelectParams()
        L.lib().ldso_ct_select_default_params(C.byref(p))
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise TypeError(f"unknown selection parameter {k!r}")
            setattr(p, k, v)
        return p

    def select_init(self, pattern, potential: int = 3):
        """The selector's randomPattern [width*height] (uint8) and its currentPotential."""
        pattern = np.ascontiguousarray(pattern, np.uint8).reshape(-1)
        assert pattern.size == self.width * self.height
        L.check(L.lib().ldso_ct_select_init(self._h, L.ptr(pattern, L.u8p), int(potential)))

    @property
    def select_potential(self) -> int:
        out = C.c_int32()
        L.check(L.lib().ldso_ct_select_potential(self._h, C.byref(out)))
        return int(out.value)

    def select_pixels(self, **params):
        """makeMaps on the new frame -> (map [height, width] of 0 / 1 / 2 / 4, stats dict over
        _lib.SELECT_STATS).  params: the fields of ldso_ct_select_params (density, recursions, ...)."""
        p = self._select_params(params)
        m = np.zeros((self.height, self.width), np.float32)
        st = np.zeros(len(L.SELECT_STATS), np.int32)
        L.check(L.lib().ldso_ct_select_pixels(self._h, C.byref(p), L.ptr(m, L.f32p), L.ptr(st, L.i32p)))
        return m, dict(zip(L.SELECT_STATS, st.tolist()))

    def make_new_traces(self, host: int = 0, capacity: int | None = None, **params):
        """makeMaps and makeNewTraces' walk on the device -> (records in row-major order, stats).
        capacity None: room for twice the density, and the call repeated once with the count it
        reports if that was too little."""
        p = self._select_params(params)
        st = np.zeros(len(L.SELECT_STATS), np.int32)
        n = C.c_int32()
        if capacity is not None:
            cap = int(capacity)
        else:  # (a density the library refuses still reaches it)
            cap = min(int(2 * p.density) + 64, self.width * self.height) if 0 < p.density < np.inf else 64
        for _ in range(2):
            out = np.zeros(cap, L.IMMATURE_DTYPE)
            rc = L.lib().ldso_ct_make_new_traces(self._h, C.byref(p), int(host), cap, out.ctypes.data, C.byref(n),
                                                 L.ptr(st, L.i32p))
            if rc == 0 or capacity is not None or n.value <= cap:
                break
            cap = int(n.value)  # the potential was put back: the retry repeats the selection
        L.check(rc)
        return out[:n.value].copy(), dict(zip(L.SELECT_STATS, st.tolist()))

    # ---- corner detection (FeatureDetector::DetectCorners, makeNewTraces with pointSelection 1) ----
    def corners_init(self, bit_pattern):
        """The ORB sampling table bit_pattern_31_ [256 * 4] (int32, entries in [-13, 13])."""
        bit_pattern = np.ascontiguousarray(bit_pattern, np.int32).reshape(-1)
        assert bit_pattern.size == 1024
        L.check(L.lib().ldso_ct_corners_init(self._h, L.ptr(bit_pattern, L.i32p)))

    def detect_corners(self, n_features: int, host: int = 0, capacity: int | None = None):
        """DetectCorners(n_features) and makeNewTraces' loop on the new frame -> (immature records,
        features (_lib.FEATURE_DTYPE), stats dict over _lib.CORNER_STATS), in feature order.
        capacity None: room for twice n_features, and the call repeated once with the count it reports
        if that was too little."""
        st = np.zeros(len(L.CORNER_STATS), np.int32)
        n = C.c_int32()
        cap = int(capacity) if capacity is not None else max(2 * int(n_features), 0) + 64
        for _ in range(2):
            rec = np.zeros(cap, L.IMMATURE_DTYPE)
            feat = np.zeros(cap, L.FEATURE_DTYPE)
            rc = L.lib().ldso_ct_detect_corners(self._h, int(n_features), int(host), cap, rec.ctypes.data,
                                                feat.ctypes.data, C.byref(n), L.ptr(st, L.i32p))
            if rc == 0 or capacity is not None or n.value <= cap:
                break
            cap = int(n.value)
        L.check(rc)
        return rec[:n.value].copy(), feat[:n.value].copy(), dict(zip(L.CORNER_STATS, st.tolist()))


def init_params(**params) -> "L.LdsoCtInitParams":
    """ldso_ct_init_params: the defaults with the given fields replaced (max_iterations: 5 ints)."""
    p = L.LdsoCtInitParams()
    L.lib().ldso_ct_init_default_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError(f"unknown initializer parameter {k!r}")
        setattr(p, k, (C.c_int32 * 5)(*v) if k == "max_iterations" else v)
    return p


def _point_lists(levels):
    levels = [np.ascontiguousarray(lv, L.INIT_POINT_DTYPE) for lv in levels]
    n = np.array([lv.size for lv in levels], np.int32)
    pp = (C.c_void_p * len(levels))(*[lv.ctypes.data for lv in levels])
    return levels, n, pp


def init_check_points(levels, width: int, height: int):
    """The list checks of set_first alone (ldso_ct_init_check_points); raises LdsoError on a bad list."""
    keep, n, pp = _point_lists(levels)
    L.check(L.lib().ldso_ct_init_check_points(len(keep), int(width), int(height), L.ptr(n, L.i32p), pp))


def init_lm_step(H, b, Hsc, bsc, lam: float, w: int, h: int, ref_to_new, aff_ab, **params):
    """Lines :95-116 of trackFrame on the host (ldso_ct_init_lm_step) -> (inc [8] float32, pose [3][4], aff [2])."""
    f = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in (H, b, Hsc, bsc)]
    T = np.ascontiguousarray(np.asarray(ref_to_new, np.float64)[:3, :4])
    ab = np.ascontiguousarray(aff_ab, np.float64).reshape(2)
    inc, To, abo = np.zeros(8, np.float32), np.zeros((3, 4)), np.zeros(2)
    p = init_params(**params)
    L.check(L.lib().ldso_ct_init_lm_step(*[L.ptr(x, L.f32p) for x in f], float(lam), int(w), int(h), L.ptr(T, L.f64p),
                                         L.ptr(ab, L.f64p), C.byref(p), L.ptr(inc, L.f32p), L.ptr(To, L.f64p),
                                         L.ptr(abo, L.f64p)))
    return inc, To, abo


class CoarseInitializer:
    """CoarseInitializer on the frames of a CoarseTracker: the tracker's new frame at set_first is
    firstFrame, every later new frame is trackFrame's newFrame."""

    def __init__(self, tracker: CoarseTracker):
        self.tracker = tracker
        self._h = tracker._h
        self.levels = tracker.levels

    def set_first(self, levels):
        """levels: per pyramid level an array of _lib.INIT_POINT_DTYPE (points with their neighbour and
        parent tables, as setFirst and makeNN leave them)."""
        keep, n, pp = _point_lists(levels)
        assert len(keep) == self.levels
        L.check(L.lib().ldso_ct_init_set_first(self._h, L.ptr(n, L.i32p), pp))
        self._n = n.copy()

    def points(self, lvl: int) -> np.ndarray:
        n = C.c_int32()
        lib = L.lib()
        L.check(lib.ldso_ct_init_get_points(self._h, int(lvl), None, 0, C.byref(n)))
        out = np.zeros(n.value, L.INIT_POINT_DTYPE)
        L.check(lib.ldso_ct_init_get_points(self._h, int(lvl), out.ctypes.data, int(n.value), C.byref(n)))
        return out

    def set_points(self, lvl: int, pts: np.ndarray):
        pts = np.ascontiguousarray(pts, L.INIT_POINT_DTYPE)
        L.check(L.lib().ldso_ct_init_set_points(self._h, int(lvl), int(pts.size), pts.ctypes.data))

    def rank_counts(self) -> np.ndarray:
        out = np.zeros(self.levels, np.int32)
        L.check(L.lib().ldso_ct_init_rank_counts(self._h, L.ptr(out, L.i32p)))
        return out

    def eval(self, lvl: int, ref_to_new, aff_ab=(0.0, 0.0), **params):
        """One calcResAndGS on the resident points -> (H [8][8], b [8], Hsc [8][8], bsc [8], res [3],
        alpha capped), float32."""
        T = np.ascontiguousarray(np.asarray(ref_to_new, np.float64)[:3, :4])
        ab = np.ascontiguousarray(aff_ab, np.float64).reshape(2)
        H, b, Hsc, bsc, res = (np.zeros(s, np.float32) for s in ((8, 8), 8, (8, 8), 8, 3))
        capped = C.c_int32()
        p = init_params(**params)
        L.check(L.lib().ldso_ct_init_eval(self._h, int(lvl), L.ptr(T, L.f64p), L.ptr(ab, L.f64p), C.byref(p),
                                          L.ptr(H, L.f32p), L.ptr(b, L.f32p), L.ptr(Hsc, L.f32p), L.ptr(bsc, L.f32p),
                                          L.ptr(res, L.f32p), C.byref(capped)))
        return H, b, Hsc, bsc, res, bool(capped.value)

    def opt_reg(self, lvl: int, reg_weight: float = 0.8, snapped: bool = True):
        L.check(L.lib().ldso_ct_init_opt_reg(self._h, int(lvl), float(reg_weight), int(bool(snapped))))

    def track_frame(self, trace: int = 0, **params):
        """trackFrame on the tracker's new frame, one launch -> the result record (_lib.INIT_RESULT_DTYPE), and
        with trace > 0 also the first `trace` evaluations (_lib.INIT_STEP_DTYPE) and how many there were."""
        p = init_params(**params)
        out = np.zeros(1, L.INIT_RESULT_DTYPE)
        steps = np.zeros(max(int(trace), 0), L.INIT_STEP_DTYPE)
        n_steps = C.c_int32()
        L.check(L.lib().ldso_ct_init_track_frame(self._h, C.byref(p), out.ctypes.data,
                                                 steps.ctypes.data if steps.size else None, int(steps.size),
                                                 C.byref(n_steps)))
        if trace > 0:
            return out[0], steps[:min(n_steps.value, steps.size)].copy(), int(n_steps.value)
        return out[0]
