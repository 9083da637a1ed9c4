"""Device-resident frame store (ldso_ba_frames_reserve / frame_put* / load_frames).

Keyframe images enter a context once -- from the host, from the coarse tracker's new frame, or from
any device buffer -- and windows are loaded by frame id.  Every path must give the pass the oracle
gives on the same window (compare_pass of test_gpu_parity with its bars: per-residual state
bit-exact, stitched blocks within BLOCK_TOL), and the transfer counters must show that a keyframe
cycle moves one image in, not the window.

Shapes: 160x120 (aligned) and 162x118 (width % 8 != 0, height % 4 != 0: the band / tile index
arithmetic and the padding; the tracker gets 2 pyramid levels); edge_frac=0.3 draws points 4..9 px
from the border so that taps reach the outermost rows and columns.
"""
import copy
import functools

import numpy as np
import pytest

import oracle
from ldso_amd import BAContext, synth
from ldso_amd import _lib as L
from ldso_amd import dist as ldist
from ldso_amd.tracker import CoarseTracker
from ldso_amd.window import Window
from test_gpu_parity import compare_pass
from test_marginalization import ad_ht_delta, marg_points

pytestmark = pytest.mark.gpu

CFGS = {
    "N3P64_160x120": dict(n_frames=3, n_points=64, width=160, height=120, seed=11, edge_frac=0.3),
    "N5P400_162x118": dict(n_frames=5, n_points=400, width=162, height=118, seed=3, edge_frac=0.3),
}
CYCLE = dict(n_frames=6, n_points=400, width=162, height=118, seed=5, edge_frac=0.3)
TILED_IMAGES = 2  # LDSO_BA_TUNE_TILED_IMAGES


def sub_window(w, keep):
    """The window of the frame subset `keep` of w: points whose host is kept, residuals whose
    target is kept, frame indices remapped, frame-pair terms recomputed."""
    keep = [int(f) for f in keep]
    remap = {f: i for i, f in enumerate(keep)}
    host, data, begin, tgt, st, en, fl = [], [], [0], [], [], [], []
    for p in range(w.n_points):
        if int(w.point_host[p]) not in remap:
            continue
        host.append(remap[int(w.point_host[p])])
        data.append(w.point_data[p])
        for k in range(int(w.point_res_begin[p]), int(w.point_res_begin[p + 1])):
            if int(w.res_target[k]) in remap:
                tgt.append(remap[int(w.res_target[k])])
                st.append(w.res_state[k])
                en.append(w.res_energy[k])
                fl.append(w.res_flags[k])
        begin.append(len(tgt))
    s = Window(n_frames=len(keep), width=w.width, height=w.height, calib=w.calib.copy(), frames=w.frames[keep].copy(),
               dI=np.ascontiguousarray(w.dI[keep]), frame_energy_th=w.frame_energy_th[keep].copy(),
               point_host=np.array(host, np.int32), point_data=np.array(data, np.float32).reshape(-1, L.POINT_STRIDE),
               point_res_begin=np.array(begin, np.int32), res_target=np.array(tgt, np.int32),
               res_state=np.array(st, np.int8), res_energy=np.array(en, np.float32), res_flags=np.array(fl, np.uint8),
               settings=w.settings)
    return s.refresh_frame_terms()


@functools.lru_cache(maxsize=None)
def base_window(name):
    return synth.make_window(**(CYCLE if name == "cycle" else CFGS[name]))


def window(name, keep=None):
    """A fresh Window (its own mutable state) of a named configuration, or of a frame subset of it."""
    w = base_window(name)
    return sub_window(w, keep) if keep is not None else sub_window(w, range(w.n_frames))


@functools.lru_cache(maxsize=None)
def reference(name, keep=None):
    """The oracle's pass over window(name, keep), computed once and only read afterwards."""
    ow = oracle.OracleWindow(window(name, keep), threads=0)
    e_cpu, s_cpu = ow.iteration()
    return ow, e_cpu, s_cpu


def without_images(w):
    w = copy.copy(w)
    w.dI = None
    w._keep = []
    return w


def make_ctx(layout, capacity, w):
    c = BAContext(0)
    c.set_tuning(TILED_IMAGES, layout)  # before reserve: the store keeps this layout for its life
    c.frames_reserve(capacity, w.width, w.height)
    return c


def check_pass(c, name, keep=None):
    c.linearize(fix=False, accumulate=True)
    ow, e_cpu, s_cpu = reference(name, keep)
    compare_pass(c, ow, 0, e_cpu, s_cpu)


def slot_bytes(w, layout):
    hp = (w.height + 3) // 4 * 4
    if layout == 3:
        return (w.width + 7) // 8 * 8 * hp * 4
    return (w.width + 1) // 2 * 2 * hp * 16


def delta(a, b):
    return {k: b[k] - a[k] for k in a}


# ---- 1. host put ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [3, 1])
@pytest.mark.parametrize("name", list(CFGS))
def test_host_put_then_load_by_id_matches_oracle(built, name, layout):
    w = window(name)
    c = make_ctx(layout, w.n_frames + 1, w)
    ids = [100 + 7 * f for f in range(w.n_frames)]
    s0 = c.transfer_stats()
    for f, i in enumerate(ids):
        c.frame_put(i, w.dI[f])
    d = delta(s0, c.transfer_stats())
    assert d["h2d_bytes"] == w.n_frames * w.width * w.height * 12 and d["frames"] == w.n_frames and d["allocs"] == 0
    c.load([without_images(w)], frame_ids=ids)
    check_pass(c, name)
    assert c.stats()["device_bytes"] >= (w.n_frames + 1) * slot_bytes(w, layout)
    c.close()


# ---- 2. tracker hand-off -------------------------------------------------------------------
@pytest.mark.parametrize("layout", [3, 1])
@pytest.mark.parametrize("name", list(CFGS))
def test_tracker_handoff_matches_oracle_without_host_image_bytes(built, name, layout):
    """One tracker serves every frame: set_new_frame then frame_put_tracker back to back, so each
    set_new_frame overwrites the buffers the previous ingest reads (ordered by events only)."""
    w = window(name)
    c = make_ctx(layout, w.n_frames, w)
    tr = CoarseTracker(w.width, w.height)
    if name == "N5P400_162x118":
        assert tr.levels == 2
    s0 = c.transfer_stats()
    for f in range(w.n_frames):
        tr.set_new_frame(w.dI[f, :, 0])
        c.frame_put_tracker(f, tr)
    c.load([without_images(w)], frame_ids=list(range(w.n_frames)))
    d = delta(s0, c.transfer_stats())
    assert d["h2d_bytes"] == 0 and d["frames"] == w.n_frames
    check_pass(c, name)
    c.close()
    tr.close()


# ---- 3. torch tensors ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", [3, 1])
def test_put_from_torch_tensors_on_torch_streams(built, layout):
    """Layout 3 from the intensity plane alone on torch's current stream; layout 1 from texels
    produced on a side stream.  No synchronisation between the producing kernel and the put."""
    import torch

    name = "N5P400_162x118"
    w = window(name)
    c = make_ctx(layout, w.n_frames, w)
    side = torch.cuda.Stream() if layout == 1 else None
    alive = []
    for f in range(w.n_frames):
        host = torch.from_numpy(np.ascontiguousarray(w.dI[f]))
        if layout == 3:
            plane = host[:, 0].contiguous().cuda() * 1.0  # a kernel on the current stream writes it
            alive.append(plane)
            c.frame_put_device(f, intensity=plane)
        else:
            with torch.cuda.stream(side):
                dev = host.cuda()
                tex = torch.cat([dev, torch.full((dev.shape[0], 1), 7.0, device="cuda")], dim=1).contiguous()
            alive.append(tex)
            c.frame_put_device(f, texels=tex, stream=side)
    assert c.transfer_stats()["h2d_bytes"] == 0
    c.load([without_images(w)], frame_ids=list(range(w.n_frames)))
    check_pass(c, name)
    c.close()
    del alive


# ---- 4. keyframe cycle ---------------------------------------------------------------------
@pytest.mark.parametrize("layout", [3, 1])
def test_keyframe_cycle_moves_one_image(built, layout):
    base = base_window("cycle")
    W, H = base.width, base.height
    first, second = (0, 1, 2, 3, 4), (0, 2, 3, 4, 5)
    N = len(first)
    c = make_ctx(layout, 6, base)
    tr = CoarseTracker(W, H)
    for f in first:
        c.frame_put(f, base.dI[f])
    c.load([without_images(window("cycle", first))], frame_ids=first)
    check_pass(c, "cycle", first)

    # frame 1 leaves, frame 5 arrives from the tracker
    s0 = c.transfer_stats()
    c.frame_drop(1)
    tr.set_new_frame(base.dI[5, :, 0])
    c.frame_put_tracker(5, tr)
    c.load([without_images(window("cycle", second))], frame_ids=second)
    check_pass(c, "cycle", second)
    d = delta(s0, c.transfer_stats())
    print("tracker cycle:", d)
    assert d["allocs"] == 0
    assert d["h2d_bytes"] == 0
    assert 0 < d["d2d_bytes"] <= N * slot_bytes(base, layout)
    assert d["frames"] == 1

    # the same arrival as a host put: exactly one frame of host -> device bytes, one position copied
    s0 = c.transfer_stats()
    c.frame_put(5, base.dI[5])
    c.load([without_images(window("cycle", second))], frame_ids=second)
    check_pass(c, "cycle", second)
    d = delta(s0, c.transfer_stats())
    print("host-put cycle:", d)
    assert d["h2d_bytes"] == W * H * 12 and d["allocs"] == 0 and d["d2d_bytes"] == slot_bytes(base, layout)

    # ldso_ba_load still works on the same context and uploads the whole window ...
    s0 = c.transfer_stats()
    c.load([window("cycle", second)])
    check_pass(c, "cycle", second)
    d = delta(s0, c.transfer_stats())
    assert d["h2d_bytes"] == N * W * H * 12
    # ... and invalidates the position tags: the next load by id copies every position again
    s0 = c.transfer_stats()
    c.load([without_images(window("cycle", second))], frame_ids=second)
    check_pass(c, "cycle", second)
    d = delta(s0, c.transfer_stats())
    assert d["h2d_bytes"] == 0 and d["d2d_bytes"] == N * slot_bytes(base, layout)
    c.close()
    tr.close()


# ---- 5. frame_get round trip ----------------------------------------------------------------
@pytest.mark.parametrize("layout", [3, 1])
def test_frame_get_round_trip_and_slot_reuse(built, layout):
    import torch

    w = base_window("N5P400_162x118")
    c = make_ctx(layout, 2, w)  # two slots: the third frame must reuse a dropped one
    tr = CoarseTracker(w.width, w.height)

    def check(fid, f):
        if layout == 1:
            inten, grad = c.frame_get(fid, with_grad=True)
            np.testing.assert_array_equal(grad.view(np.uint32), np.ascontiguousarray(w.dI[f, :, 1:3]).view(np.uint32))
        else:
            inten = c.frame_get(fid)
            with pytest.raises(L.LdsoError):
                c.frame_get(fid, with_grad=True)
        np.testing.assert_array_equal(inten.view(np.uint32), np.ascontiguousarray(w.dI[f, :, 0]).view(np.uint32))

    c.frame_put(10, w.dI[0])
    c.frame_put(11, w.dI[1])
    check(10, 0)
    check(11, 1)
    c.frame_drop(10)
    tr.set_new_frame(w.dI[2, :, 0])
    c.frame_put_tracker(12, tr)  # into frame 10's slot
    check(12, 2)
    check(11, 1)
    c.frame_put(11, w.dI[3])  # overwrite a resident id
    check(11, 3)
    c.frame_drop(12)
    dev = torch.from_numpy(np.ascontiguousarray(w.dI[4])).cuda()
    tex = torch.cat([dev, torch.zeros((dev.shape[0], 1), device="cuda")], dim=1).contiguous()
    c.frame_put_device(13, intensity=dev[:, 0].contiguous(), texels=tex)
    check(13, 4)
    c.close()
    tr.close()


# ---- 6. errors -------------------------------------------------------------------------------
def raises(code, match=None):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(L.LdsoError, match=match)
            self.info = self.cm.__enter__()
            return self

        def __exit__(self, *a):
            r = self.cm.__exit__(*a)
            assert self.info.value.code == code, (self.info.value.code, str(self.info.value))
            return r

    return Ctx()


def test_errors_are_codes_and_messages(built):
    name = "N3P64_160x120"
    w = window(name)
    c = BAContext(0)
    with raises(L.ERR_FRAME_STORE, "frames_reserve"):  # put before reserve
        c.frame_put(0, w.dI[0])
    with raises(L.ERR_FRAME_STORE, "frames_reserve"):
        c.load([without_images(w)], frame_ids=[0, 1, 2])
    c.frames_reserve(3, w.width, w.height)
    for f in range(3):
        c.frame_put(f, w.dI[f])
    with raises(L.ERR_FRAME_STORE, "full"):  # put beyond capacity
        c.frame_put(3, w.dI[0])
    with raises(L.ERR_FRAME_STORE, "77"):  # drop of an unknown id
        c.frame_drop(77)
    c.load([without_images(w)], frame_ids=[0, 1, 2])
    before = c.transfer_stats()
    with raises(L.ERR_FRAME_STORE, "999"):  # load with a non-resident id names it ...
        c.load([without_images(w)], frame_ids=[0, 999, 2])
    assert c.transfer_stats() == before
    check_pass(c, name)  # ... and leaves the previous load usable

    other = CoarseTracker(w.width * 2, w.height * 2)
    other.set_new_frame(np.zeros(w.width * w.height * 4, np.float32))
    with raises(L.ERR_FRAME_STORE, "320x240"):  # a tracker of another size
        c.frame_put_tracker(0, other)
    other.close()
    unset = CoarseTracker(w.width, w.height)
    with raises(-1, "set_new_frame"):  # a tracker with no frame set
        c.frame_put_tracker(0, unset)
    unset.close()

    bad = w.dI[1].copy()
    bad[:, 1] += np.float32(0.125)
    with raises(L.ERR_GRADIENT_MISMATCH, "layout 1"):  # layout 3 cannot hold foreign gradients
        c.frame_put(1, bad)
    with raises(L.ERR_FRAME_STORE):  # and says so instead of keeping the frame
        c.frame_drop(1)
    with raises(-1):
        c.frame_put_device(1)
    import torch

    with raises(-1, "intensity"):  # layout 3 needs the intensity plane
        c.frame_put_device(1, texels=torch.zeros(w.width * w.height * 4, device="cuda"))
    c.close()

    c1 = make_ctx(1, 2, w)
    plane = torch.zeros(w.width * w.height, device="cuda")
    with raises(-1, "texels"):  # layout 1 needs texels
        c1.frame_put_device(0, intensity=plane)
    c1.frame_put(1, bad)  # layout 1 keeps the caller's gradients
    _, g = c1.frame_get(1, with_grad=True)
    np.testing.assert_array_equal(g, bad[:, 1:3])
    c1.close()


# ---- 6b. a store whose layout differs from the loads' -------------------------------------------
def test_store_layout_differs_from_load_layout(built):
    """The store keeps the layout it was reserved in (1), ldso_ba_load the preferred one (3): loads
    by id run in the store's layout without changing the preference, a plain load returns to it, a
    new store takes it, and ldso_ba_load's gradient fallback becomes it."""
    name = "N3P64_160x120"
    w = window(name)
    ids = [40 + f for f in range(w.n_frames)]
    c = make_ctx(1, w.n_frames, w)
    c.set_tuning(TILED_IMAGES, 3)  # nothing is loaded yet
    # (a) a plain load, in layout 3
    c.load([w])
    check_pass(c, name)
    bytes_a = c.stats()["device_bytes"]
    # (b) by id, in the store's layout 1: the window's image array is four times layout 3's
    for f, i in enumerate(ids):
        c.frame_put(i, w.dI[f])
    c.load([without_images(window(name))], frame_ids=ids)
    check_pass(c, name)
    assert c.stats()["device_bytes"] == bytes_a + w.n_frames * (slot_bytes(w, 1) - slot_bytes(w, 3))
    # (c) a plain load again: one image allocation (no fallback's second), back in layout 3
    s0 = c.transfer_stats()
    c.load([window(name)])
    check_pass(c, name)
    assert delta(s0, c.transfer_stats())["allocs"] == 1
    assert c.stats()["device_bytes"] == bytes_a
    # (d) a store reserved while a load by id is active takes the preference, 3
    c.load([without_images(window(name))], frame_ids=ids)
    c.frames_reserve(w.n_frames, w.width, w.height)
    c.frame_put(ids[0], w.dI[0])
    with raises(-1, "layout 3"):
        c.frame_get(ids[0], with_grad=True)
    c.close()

    # (e) ldso_ba_load's fallback to layout 1 is the preference of a store reserved afterwards
    bad = window(name)
    bad.dI = bad.dI.copy()
    bad.dI[:, :, 1] += np.float32(0.125)
    c = BAContext(0)
    c.set_tuning(TILED_IMAGES, 3)
    c.load([bad])
    c.frames_reserve(1, w.width, w.height)
    c.frame_put(7, bad.dI[0])
    _, g = c.frame_get(7, with_grad=True)
    np.testing.assert_array_equal(g, bad.dI[0][:, 1:3])
    c.close()


# ---- 7. marginalisation context over a parent loaded by id ------------------------------------
def test_marginalization_context_borrows_images_loaded_by_id(built):
    name = "N5P400_162x118"
    w = window(name)
    S = marg_points(w)
    adh = ad_ht_delta(w)
    out = []
    for by_id in (True, False):
        parent = BAContext(0)
        if by_id:
            parent.frames_reserve(w.n_frames, w.width, w.height)
            for f in range(w.n_frames):
                parent.frame_put(f, w.dI[f])
            parent.load([without_images(window(name))], frame_ids=list(range(w.n_frames)))
        else:
            parent.load([window(name)])
        parent.linearize()
        parent.sync()
        m = BAContext(0).load_marginalization(parent, 0, ldist.subset_window(window(name), S))
        out.append(m.marginalize_points(adh))
        m.close()
        parent.close()
    assert np.abs(out[1][0]).max() > 0
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
