"""Python face of the device context (one per FullSystem / group of windows).

Mirrors the reference's per-iteration call sequence (FullSystem::optimize, FullSystem.cc:844-1007):

    ctx.reset_oob()                         # PointFrameResidual::resetOOB for activeResiduals
    ctx.linearize(fix=False)                # linearizeAll(false) + applyRes + accumulate{AF,LF,SCF}
    x = ctx.solve(0, iteration, lam, ns)    # EnergyFunctional::solveSystemF (stitched system)
    ctx.resubstitute(0, x, lam)             # resubstituteF_MT
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .window import Window


class BAContext:
    def __init__(self, device: int = 0):
        self._lib = L.lib()
        h = C.c_void_p()
        L.check(self._lib.ldso_ba_create(int(device), C.byref(h)))
        self._h = h
        self.windows: list[Window] = []
        self._structs = None
        self._frame_shape = None  # (height, width) of the frame store once reserved

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ldso_ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- settings ----------------------------------------------------------------------
    def set_settings(self, settings=None):
        """ldso_ba_set_settings: the reference settings this context runs with (an L.OptSettings;
        None = the defaults).  Unsupported ones raise (the context keeps its previous settings)."""
        L.check(self._lib.ldso_ba_set_settings(self._h, C.byref(settings) if settings is not None else None))
        return self

    def settings(self) -> L.OptSettings:
        out = L.OptSettings()
        L.check(self._lib.ldso_ba_get_settings(self._h, C.byref(out)))
        return out

    # ---- structure ---------------------------------------------------------------------
    def load(self, windows, shard_rank: int = 0, shard_count: int = 1, *, frame_ids=None):
        """ldso_ba_load, or with frame_ids (the windows' frames back to back, as frame-store ids)
        ldso_ba_load_frames: the images come from the store and the windows' dI is not read (may be
        None).  A failed load leaves the context's windows as they were."""
        if isinstance(windows, Window):
            windows = [windows]
        windows = list(windows)
        if frame_ids is None:
            structs = (L.LdsoBaWindow * len(windows))(*[w.c_struct() for w in windows])
            L.check(self._lib.ldso_ba_load(self._h, len(windows), structs, int(shard_rank), int(shard_count)))
        else:
            ids = np.ascontiguousarray(np.asarray(frame_ids).reshape(-1), np.int64)
            assert ids.size == sum(w.n_frames for w in windows), "one frame id per frame of every window"
            structs = (L.LdsoBaWindow * len(windows))(*[w.c_struct(with_images=False) for w in windows])
            L.check(self._lib.ldso_ba_load_frames(self._h, len(windows), structs, L.ptr(ids, L.i64p), int(shard_rank),
                                                  int(shard_count)))
        self.windows = windows
        self._structs = structs
        for w in self.windows:
            w._keep = []  # host copies are no longer referenced by the device
        return self

    def edit(self, after: Window, frame_ids, frame_src, point_src, res_src, win: int = 0):
        """ldso_ba_edit_window: window `win` becomes `after`, the carried entries (src >= 0) taken from
        where the device holds them; after's point_data / res_state / res_energy / res_flags are read at
        entries whose src is -1 only.  A refused edit raises and leaves the context as it was."""
        s = after.c_struct(with_images=False)
        ids = np.ascontiguousarray(np.asarray(frame_ids).reshape(-1), np.int64)
        src = [np.ascontiguousarray(a, np.int32) for a in (frame_src, point_src, res_src)]
        assert ids.size == src[0].size == after.n_frames and src[1].size == after.n_points and src[2].size == after.n_residuals
        e = L.LdsoBaEdit(C.pointer(s), L.ptr(ids, L.i64p), *[L.ptr(a, L.i32p) for a in src])
        L.check(self._lib.ldso_ba_edit_window(self._h, int(win), C.byref(e)))
        self.windows[win] = after
        after._keep = []
        return self

    def point_data(self, win: int = 0) -> np.ndarray:
        """ldso_ba_get_point_data: the point records [P][24] as the device holds them, caller order."""
        out = np.zeros((self.windows[win].n_points, L.POINT_STRIDE), np.float32)
        L.check(self._lib.ldso_ba_get_point_data(self._h, int(win), L.ptr(out, L.f32p)))
        return out

    # ---- device-resident frame store -----------------------------------------------------
    def frames_reserve(self, capacity: int, width: int, height: int):
        """ldso_ba_frames_reserve: `capacity` image slots in the context's image layout
        (set_tuning(TILED_IMAGES) before this call).  Re-reserving drops every resident frame."""
        L.check(self._lib.ldso_ba_frames_reserve(self._h, int(capacity), int(width), int(height)))
        self._frame_shape = (int(height), int(width))
        return self

    def frame_put(self, frame_id: int, dI):
        """Host FrameHessian::dI [h*w][3] -> the slot of frame_id.  In layout 3 gradients that are
        not makeImages' raise with code L.ERR_GRADIENT_MISMATCH (reserve the store in layout 1)."""
        a = np.ascontiguousarray(dI, np.float32).reshape(-1)
        assert self._frame_shape is None or a.size == self._npix() * 3, "dI must be [h*w][3]"
        L.check(self._lib.ldso_ba_frame_put(self._h, int(frame_id), L.ptr(a, L.f32p)))

    def _npix(self) -> int:
        if self._frame_shape is None:  # the library refuses the call itself, with its message
            return 0
        return self._frame_shape[0] * self._frame_shape[1]

    @staticmethod
    def _dev_ptr(x, n_floats):
        """Raw device pointer of a torch CUDA tensor (float32, contiguous, n_floats elements) or an int."""
        if x is None:
            return None
        if isinstance(x, int):
            return C.c_void_p(x)
        import torch

        assert isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(), \
            "device sources are contiguous float32 CUDA tensors or raw pointers"
        assert not n_floats or x.numel() == n_floats, f"tensor of {x.numel()} floats where {n_floats} are read"
        return C.c_void_p(x.data_ptr())

    def frame_put_device(self, frame_id: int, intensity=None, texels=None, stream=None):
        """ldso_ba_frame_put_device: intensity [h*w] and / or texels [h*w][4] {I, dx, dy, *} on the
        device (torch CUDA tensors or raw pointers), produced on `stream` (a torch stream, a raw
        hipStream_t or None = torch's current stream when a tensor is given, else the null stream).
        No host synchronisation; the tensors must stay alive until the stream work has run."""
        n = self._npix()
        if stream is None and not all(isinstance(x, (int, type(None))) for x in (intensity, texels)):
            import torch

            stream = torch.cuda.current_stream()
        sp = getattr(stream, "cuda_stream", stream)
        L.check(self._lib.ldso_ba_frame_put_device(self._h, int(frame_id), self._dev_ptr(intensity, n),
                                                   self._dev_ptr(texels, n * 4), C.c_void_p(int(sp or 0))))

    def frame_put_tracker(self, frame_id: int, tracker):
        """The tracker's current new frame (CoarseTracker.set_new_frame), device to device."""
        L.check(self._lib.ldso_ba_frame_put_tracker(self._h, int(frame_id), tracker._h))

    def frame_put_initializer(self, frame_id: int, tracker):
        """The coarse initializer's first frame (the snapshot CoarseInitializer.set_first took), device to
        device.  tracker: a CoarseTracker or the CoarseInitializer on it."""
        L.check(self._lib.ldso_ba_frame_put_initializer(self._h, int(frame_id), tracker._h))

    def frame_drop(self, frame_id: int):
        L.check(self._lib.ldso_ba_frame_drop(self._h, int(frame_id)))

    def frame_get(self, frame_id: int, with_grad: bool = False):
        """A resident frame back on the host: intensity [h*w], and grad [h*w][2] (layout 1 only)."""
        n = max(self._npix(), 1)
        inten = np.zeros(n, np.float32)
        grad = np.zeros((n, 2), np.float32) if with_grad else None
        L.check(self._lib.ldso_ba_frame_get(self._h, int(frame_id), L.ptr(inten, L.f32p), L.ptr(grad, L.f32p)))
        return (inten, grad) if with_grad else inten

    def transfer_stats(self) -> dict:
        """Cumulative image traffic of this context (ldso_ba_transfer_stats)."""
        o = np.zeros(4, np.int64)
        L.check(self._lib.ldso_ba_transfer_stats(self._h, L.ptr(o, L.i64p)))
        return dict(h2d_bytes=int(o[0]), d2d_bytes=int(o[1]), allocs=int(o[2]), frames=int(o[3]))

    def optimize(self, n_its: int, calib_value=None, calib_value_zero=None, nullspaces=None, settings=None):
        """FullSystem::optimize on the device (ldso_ba_optimize): up to n_its GN iterations of every
        loaded window with no host round trip; each window leaves the loop on the reference's
        exits (canbreak after setting_minOptIterations, or lost on a NaN solution).
        calib_value / calib_value_zero: [n_windows][4] CalibHessian::value / value_zero (default:
        each window's calib / 50, i.e. no calibration delta); settings: an L.OptSettings (None =
        the reference's defaults).  Returns (energies [n_its + 1][n_windows][3], frames,
        calib_value, idepths, iterations [n_windows], status [n_windows] (L.OPT_*)).  Non-None settings
        are installed into the context first (ldso_ba_set_settings)."""
        nw = len(self.windows)
        frames = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(w.frames) for w in self.windows]))
        if calib_value is None:
            calib_value = np.stack([w.calib.astype(np.float64) * (1.0 / 50.0) for w in self.windows])
        calib_value = np.ascontiguousarray(calib_value, np.float64).reshape(nw, 4)
        cz = calib_value.copy() if calib_value_zero is None else np.ascontiguousarray(calib_value_zero, np.float64)
        ns = self._ns_all(nullspaces)
        e = np.zeros((n_its + 1, nw, 3), np.float64)
        fo = np.zeros_like(frames)
        co = np.zeros((nw, 4), np.float64)
        idep = np.zeros(sum(w.n_points for w in self.windows), np.float32)
        its = np.zeros(nw, np.int32)
        status = np.zeros(nw, np.int32)
        sp = C.byref(settings) if settings is not None else None
        L.check(self._lib.ldso_ba_optimize(self._h, int(n_its), sp, frames.ctypes.data, L.ptr(calib_value, L.f64p),
                                           L.ptr(cz, L.f64p), L.ptr(ns, L.f64p), L.ptr(e, L.f64p), fo.ctypes.data,
                                           L.ptr(co, L.f64p), L.ptr(idep, L.f32p), L.ptr(its, L.i32p),
                                           L.ptr(status, L.i32p)))
        return e, fo, co, self._split(idep, [w.n_points for w in self.windows]), its, status

    def loop_state(self, win: int = 0) -> dict:
        """ldso_ba_get_loop_state: the device loop's buffers of window `win` as they stand -- x [8N+4]
        (the last device solve), precalc [N*N][PRECALC_STRIDE], prior [8N+4][2] (HL diagonal, bL)."""
        if not 0 <= win < len(self.windows):  # refused by the library, with its message
            L.check(self._lib.ldso_ba_get_loop_state(self._h, int(win), L.ptr(None, L.f64p), L.ptr(None, L.f32p),
                                                     L.ptr(None, L.f64p)))
        N = self.windows[win].n_frames
        o = dict(x=np.zeros(8 * N + 4, np.float64), precalc=np.zeros((N * N, L.PRECALC_STRIDE), np.float32),
                 prior=np.zeros((8 * N + 4, 2), np.float64))
        L.check(self._lib.ldso_ba_get_loop_state(self._h, int(win), L.ptr(o["x"], L.f64p), L.ptr(o["precalc"], L.f32p),
                                                 L.ptr(o["prior"], L.f64p)))
        return o

    def comm_init(self, unique_id, rank: int, world: int):
        """Attach to an RCCL communicator (ldso_ba_comm_init); unique_id: 128 bytes from
        ldso_ba_comm_unique_id on rank 0.  See ldso_amd.dist.attach_rccl."""
        uid = np.frombuffer(bytes(unique_id), np.uint8).copy()
        L.check(self._lib.ldso_ba_comm_init(self._h, uid.ctypes.data, int(rank), int(world)))
        return self

    def load_marginalization(self, parent: "BAContext", parent_win: int, window: Window):
        """Make this context the marginalisation context of `parent`'s window `parent_win` for the
        points (and residuals) of `window` (ldso_ba_load_marginalization: images are borrowed)."""
        self.windows = [window]
        s = window.c_struct(with_images=False)
        L.check(self._lib.ldso_ba_load_marginalization(self._h, parent._h, int(parent_win), C.byref(s)))
        self._structs = s
        self._parent = parent  # the borrowed images must outlive this context
        window._keep = []
        return self

    def load_marginalization_device(self, parent: "BAContext", parent_win: int, frame_terms: Window, points, res_live=None):
        """ldso_ba_load_marginalization_device: this context becomes the marginalisation context of
        `parent`'s window `parent_win` for its points `points` (distinct caller indices, whose order is
        the marginalisation window's) and those of their residuals that res_live [parent R] selects
        (None: all), the point records and the residuals' state, energy and flags gathered from the
        parent's device arrays.  frame_terms: a Window of which only the frame-level fields are read
        (the parent's own window will do).  self.windows[0] is the selection's structure: its
        point_data / res_state / res_energy / res_flags are placeholders, the device holds the values."""
        pw = parent.windows[parent_win]
        pts = np.ascontiguousarray(np.asarray(points).reshape(-1), np.int32)
        live = None if res_live is None else np.ascontiguousarray(res_live, np.uint8)
        assert live is None or live.size == pw.n_residuals, "res_live has one entry per residual of the parent"
        s = frame_terms.c_struct(with_images=False)
        L.check(self._lib.ldso_ba_load_marginalization_device(self._h, parent._h, int(parent_win), C.byref(s), int(pts.size),
                                                              L.ptr(pts, L.i32p), L.ptr(live, L.u8p)))
        # the selection as a Window, so that residuals() / points() size their outputs
        b0 = np.asarray(pw.point_res_begin, np.int64)[pts]
        n = np.asarray(pw.point_res_begin, np.int64)[pts + 1] - b0
        ks = np.repeat(b0 - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))  # the points' residuals, in the list's order
        owner = np.repeat(np.arange(pts.size), n)
        if live is not None:
            owner, ks = owner[live[ks] != 0], ks[live[ks] != 0]
        begin = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=pts.size))]).astype(np.int32)
        w = Window(n_frames=frame_terms.n_frames, width=frame_terms.width, height=frame_terms.height,
                   calib=frame_terms.calib.copy(), frames=frame_terms.frames, dI=None,
                   frame_energy_th=frame_terms.frame_energy_th, point_host=pw.point_host[pts].astype(np.int32),
                   point_data=np.zeros((pts.size, L.POINT_STRIDE), np.float32), point_res_begin=begin,
                   res_target=np.asarray(pw.res_target)[ks].astype(np.int32), res_state=np.zeros(ks.size, np.int8),
                   res_energy=np.zeros(ks.size, np.float32), res_flags=np.zeros(ks.size, np.uint8),
                   settings=frame_terms.settings)
        self.windows = [w]
        self._structs = s
        self._parent = parent  # the borrowed images must outlive this context
        return self

    def flag_points(self, frame_flagged, num_good, last_res, last_state=None, params=None, win: int = 0) -> dict:
        """ldso_ba_flag_points: removeOutliers' and flagPointsForRemoval's decision for every point of
        window `win` from the device's residual states, flags, point records and idepth_hessian.
        frame_flagged [N], num_good [P], last_res [P][2] (residual index in the window or -1),
        last_state [P][2] (read where last_res is -1); params: an L.FlagParams (None = the defaults).
        -> status [P] (L.PT_*), res_live [R], num_good [P], last_state [P][2], counts [4]."""
        w = self.windows[win] if 0 <= win < len(self.windows) else None
        P, R = (w.n_points, w.n_residuals) if w is not None else (0, 0)
        ff = np.ascontiguousarray(frame_flagged, np.uint8)
        ng = np.ascontiguousarray(num_good, np.int32)
        lr = np.ascontiguousarray(last_res, np.int32).reshape(-1, 2)
        ls = None if last_state is None else np.ascontiguousarray(last_state, np.int8).reshape(-1, 2)
        assert w is None or (ff.size == w.n_frames and ng.size == P and lr.shape[0] == P and (ls is None or ls.shape[0] == P))
        o = dict(status=np.zeros(P, np.int8), res_live=np.zeros(R, np.uint8), num_good=np.zeros(P, np.int32),
                 last_state=np.zeros((P, 2), np.int8), counts=np.zeros(4, np.int32))
        L.check(self._lib.ldso_ba_flag_points(self._h, int(win), C.byref(params) if params is not None else None,
                                              L.ptr(ff, L.u8p), L.ptr(ng, L.i32p), L.ptr(lr, L.i32p), L.ptr(ls, L.i8p),
                                              L.ptr(o["status"], L.i8p), L.ptr(o["res_live"], L.u8p),
                                              L.ptr(o["num_good"], L.i32p), L.ptr(o["last_state"], L.i8p),
                                              L.ptr(o["counts"], L.i32p)))
        return o

    def marginalize_points(self, ad_ht_delta):
        """ldso_ba_marginalize_points -> (H, b) = (M - Msc, Mb - Mbsc) (EnergyFunctional.cc:226-243)."""
        n = self.windows[0].dim
        H = np.zeros((n, n), np.float64)
        b = np.zeros(n, np.float64)
        adh = np.ascontiguousarray(ad_ht_delta, np.float32)
        L.check(self._lib.ldso_ba_marginalize_points(self._h, L.ptr(adh, L.f32p), L.ptr(H, L.f64p), L.ptr(b, L.f64p)))
        return H, b

    def update(self, win: int, window: Window):
        s = window.c_struct()
        L.check(self._lib.ldso_ba_update(self._h, int(win), C.byref(s)))

    def activate_points(self, win: int, pts: np.ndarray, min_obs: int = 1) -> np.ndarray:
        """FullSystem::optimizeImmaturePoint for ldso_ct_immature records hosted in window `win`
        (FullSystem.cc:1035-1156) -> ldso_ba_activation records {idepth, status, in_mask, energy}."""
        assert pts.dtype == L.IMMATURE_DTYPE and pts.flags.c_contiguous
        out = np.zeros(pts.size, L.ACTIVATION_DTYPE)
        L.check(self._lib.ldso_ba_activate_points(self._h, int(win), int(pts.size), pts.ctypes.data, int(min_obs),
                                                  out.ctypes.data))
        return out

    def activate_points_tracker(self, win: int, tracker, min_obs: int = 1) -> np.ndarray:
        """The same for the records a CoarseTracker's last select_activation selected, read on the
        device (ldso_ba_activate_points_tracker) -> ldso_ba_activation records in the selection's order."""
        out = np.zeros(getattr(tracker, "_as_sel_n", 0), L.ACTIVATION_DTYPE)
        L.check(self._lib.ldso_ba_activate_points_tracker(self._h, int(win), tracker._h, int(min_obs), out.ctypes.data))
        return out

    def update_points(self, win: int, vals: np.ndarray):
        """ldso_ba_update_points: [P][4] (idepth_scaled, idepth_zero_scaled, priorF, deltaF), caller order."""
        v = np.ascontiguousarray(vals, np.float32).reshape(-1, 4)
        L.check(self._lib.ldso_ba_update_points(self._h, int(win), L.ptr(v, L.f32p)))

    def update_residuals(self, win: int, state, state_energy, new_energy, flags):
        """ldso_ba_update_residuals: residual states edited on the host (resetOOB / applyRes / setState)
        into the device mirror of window `win`, [R] each in the caller's residual order: state_state,
        state_energy, state_NewEnergy, flags (L.FLAG_*)."""
        L.check(self._lib.ldso_ba_update_residuals(
            self._h, int(win), L.ptr(np.ascontiguousarray(state, np.int8), L.i8p),
            L.ptr(np.ascontiguousarray(state_energy, np.float32), L.f32p),
            L.ptr(np.ascontiguousarray(new_energy, np.float32), L.f32p),
            L.ptr(np.ascontiguousarray(flags, np.uint8), L.u8p)))

    def linearize_residuals(self, win: int, only=None) -> dict:
        """ldso_ba_linearize_residuals: PointFrameResidual::linearize of every residual of window
        `win` as right after its resetOOB, on scratch copies (the context's states, records and
        system stay as they were) -> new_state, new_energy, new_energy_wo, center [R][3], center_ok,
        jpjdf [R][8] in the caller's residual order.  only: the outputs to request (the others are
        passed as NULL and left out of the result); None = all."""
        if not 0 <= win < len(self.windows):  # refused by the library, with its message
            L.check(self._lib.ldso_ba_linearize_residuals(self._h, int(win), None, None, None, None, None, None))
        R = self.windows[win].n_residuals
        o = dict(new_state=np.zeros(R, np.int8), new_energy=np.zeros(R, np.float32),
                 new_energy_wo=np.zeros(R, np.float32), center=np.zeros((R, 3), np.float32),
                 center_ok=np.zeros(R, np.uint8), jpjdf=np.zeros((R, 8), np.float32))
        if only is not None:
            o = {k: v for k, v in o.items() if k in only}
        types = dict(new_state=L.i8p, new_energy=L.f32p, new_energy_wo=L.f32p, center=L.f32p, center_ok=L.u8p,
                     jpjdf=L.f32p)
        L.check(self._lib.ldso_ba_linearize_residuals(self._h, int(win), *[L.ptr(o.get(k), t) for k, t in types.items()]))
        return o

    def reset_oob(self, win: int = -1):
        L.check(self._lib.ldso_ba_reset_oob(self._h, int(win)))

    # ---- hot path ----------------------------------------------------------------------
    def linearize(self, fix: bool = False, accumulate: bool = True):
        L.check(self._lib.ldso_ba_linearize(self._h, int(bool(fix)), int(bool(accumulate))))

    def sync(self):
        L.check(self._lib.ldso_ba_sync(self._h))

    @property
    def stream(self) -> int:
        return int(self._lib.ldso_ba_stream(self._h) or 0)

    # ---- results -----------------------------------------------------------------------
    def energy(self, win: int = 0):
        out = np.zeros(3, np.float64)
        L.check(self._lib.ldso_ba_get_energy(self._h, int(win), L.ptr(out, L.f64p)))
        return out

    def system(self, win: int = 0) -> dict:
        n = self.windows[win].dim
        out = {k: np.zeros((n, n) if k.startswith("H") else n, np.float64) for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc")}
        L.check(self._lib.ldso_ba_get_system(self._h, int(win), *[L.ptr(out[k], L.f64p) for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc")]))
        return out

    def residuals(self, win: int = 0) -> dict:
        R = self.windows[win].n_residuals
        o = dict(new_state=np.zeros(R, np.int8), state=np.zeros(R, np.int8), state_energy=np.zeros(R, np.float32),
                 new_energy_wo=np.zeros(R, np.float32), center=np.zeros((R, 3), np.float32),
                 flags=np.zeros(R, np.uint8), jpjdf=np.zeros((R, 8), np.float32), rel_bs=np.zeros(R, np.float32))
        L.check(self._lib.ldso_ba_get_residuals(
            self._h, int(win), L.ptr(o["new_state"], L.i8p), L.ptr(o["state"], L.i8p), L.ptr(o["state_energy"], L.f32p),
            L.ptr(o["new_energy_wo"], L.f32p), L.ptr(o["center"], L.f32p), L.ptr(o["flags"], L.u8p),
            L.ptr(o["jpjdf"], L.f32p), L.ptr(o["rel_bs"], L.f32p)))
        return o

    def points(self, win: int = 0) -> dict:
        P = self.windows[win].n_points
        o = dict(HdiF=np.zeros(P, np.float32), bdSumF=np.zeros(P, np.float32), idepth_hessian=np.zeros(P, np.float32),
                 Hdd=np.zeros(P, np.float32), bd=np.zeros(P, np.float32), Hcd=np.zeros((P, 4), np.float32))
        L.check(self._lib.ldso_ba_get_points(self._h, int(win), *[L.ptr(o[k], L.f32p) for k in
                                                                  ("HdiF", "bdSumF", "idepth_hessian", "Hdd", "bd", "Hcd")]))
        return o

    def frame_energy_th(self, win: int = 0):
        out = np.zeros(self.windows[win].n_frames, np.float32)
        L.check(self._lib.ldso_ba_get_frame_energy_th(self._h, int(win), L.ptr(out, L.f32p)))
        return out

    def solve(self, win: int = 0, iteration: int = 0, lam: float = 1e-5, nullspaces=None):
        x = np.zeros(self.windows[win].dim, np.float64)
        ns = None if nullspaces is None else np.ascontiguousarray(nullspaces, np.float64)
        L.check(self._lib.ldso_ba_solve(self._h, int(win), int(iteration), float(lam), L.ptr(ns, L.f64p),
                                        0 if ns is None else ns.shape[0], L.ptr(x, L.f64p)))
        return x

    def resubstitute(self, win: int, x, lam: float = 1e-5, fetch: bool = True):
        x = np.ascontiguousarray(x, np.float64)
        step = np.zeros(self.windows[win].n_points, np.float32) if fetch else None
        L.check(self._lib.ldso_ba_resubstitute(self._h, int(win), L.ptr(x, L.f64p), float(lam), L.ptr(step, L.f32p)))
        return step

    # ---- device-side solve ---------------------------------------------
    def _ns_all(self, nullspaces):
        if nullspaces is None:
            return None
        return np.ascontiguousarray(np.concatenate([np.asarray(n, np.float64).ravel() for n in nullspaces]))

    def _split(self, flat, sizes):
        out, o = [], 0
        for n in sizes:
            out.append(flat[o:o + n])
            o += n
        return out

    def solve_device(self, iteration: int = 0, lam: float = 1e-5, nullspaces=None, n_null: int = 7):
        """x of every window (solveSystemF on the GPU); nullspaces: list of [7][8N+4] arrays, of
        which the first n_null rows project."""
        ns = self._ns_all(nullspaces)
        x = np.zeros(sum(w.dim for w in self.windows), np.float64)
        L.check(self._lib.ldso_ba_solve_device(self._h, int(iteration), float(lam), L.ptr(ns, L.f64p),
                                               0 if ns is None else int(n_null), L.ptr(x, L.f64p)))
        return self._split(x, [w.dim for w in self.windows])

    def resubstitute_device(self, lam: float = 1e-5):
        """Point steps of every window from the device x (caller point order per window)."""
        st = np.zeros(sum(w.n_points for w in self.windows), np.float32)
        L.check(self._lib.ldso_ba_resubstitute_device(self._h, float(lam), L.ptr(st, L.f32p)))
        return self._split(st, [w.n_points for w in self.windows])

    def iterate(self, iteration: int = 0, lam: float = 1e-5, nullspaces=None, fetch_steps: bool = True):
        """One fused GN iteration on the device: pass + solve + resubstitute, one synchronisation."""
        ns = self._ns_all(nullspaces)
        x = np.zeros(sum(w.dim for w in self.windows), np.float64)
        st = np.zeros(sum(w.n_points for w in self.windows), np.float32) if fetch_steps else None
        e = np.zeros((len(self.windows), 3), np.float64)
        L.check(self._lib.ldso_ba_iterate(self._h, int(iteration), float(lam), L.ptr(ns, L.f64p),
                                          0 if ns is None else 7, L.ptr(x, L.f64p), L.ptr(st, L.f32p),
                                          L.ptr(e, L.f64p)))
        xs = self._split(x, [w.dim for w in self.windows])
        sts = self._split(st, [w.n_points for w in self.windows]) if fetch_steps else None
        return e, xs, sts

    # ---- multi-GPU / profiling -----------------------------------------------------------
    def packed_system(self):
        p = C.c_void_p()
        n = C.c_int64()
        s = C.c_int64()
        L.check(self._lib.ldso_ba_packed_system(self._h, C.byref(p), C.byref(n), C.byref(s)))
        return int(p.value or 0), int(n.value), int(s.value)

    def unpack_system(self):
        L.check(self._lib.ldso_ba_unpack_system(self._h))

    def set_tuning(self, key: int, value: int):
        L.check(self._lib.ldso_ba_set_tuning(self._h, int(key), int(value)))

    def set_kernel_timing(self, on: bool):
        L.check(self._lib.ldso_ba_set_kernel_timing(self._h, int(bool(on))))

    def kernel_times(self) -> dict:
        n = int(self._lib.ldso_ba_num_kernels())
        ms = np.zeros(n, np.float64)
        cnt = np.zeros(n, np.int64)
        L.check(self._lib.ldso_ba_get_kernel_times(self._h, L.ptr(ms, L.f64p), L.ptr(cnt, L.i64p), n))
        return {self._lib.ldso_ba_kernel_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}

    def stats(self):
        b, p, r = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self._lib.ldso_ba_stats(self._h, C.byref(b), C.byref(p), C.byref(r)))
        return dict(device_bytes=b.value, points=p.value, residuals=r.value)
