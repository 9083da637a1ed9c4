"""ldso_ba_edit_window's host planner on the CPU (ldso_ba_edit_plan_check): for every edit of
edit_cases the planned layout is build_layout(after)'s, array for array; the gather indices are an
injection into the loaded window's device arrays that sends every carried entry to its old self and
ranks the new ones in caller order; every refusal the planner owns returns < 0 with its message and
leaves the next plan as it was.  (The refusals that need a context -- a window not loaded by id, a
sharded or marginalisation context, a frame that is not resident -- are in test_edit_parity.)"""
import ctypes as C

import numpy as np
import pytest

import edit_cases as ec
from ldso_amd import _lib as L


def plan(before, after, srcs, item_order=0, top_chunk=0):
    """-> (rc, dict of the plan's outputs)"""
    lib = L.lib()
    sb, sa = before.c_struct(with_images=False), after.c_struct(with_images=False)
    ids = np.zeros(after.n_frames, np.int64)
    src = [np.ascontiguousarray(a, np.int32) for a in srcs]
    e = L.LdsoBaEdit(C.pointer(sa), L.ptr(ids, L.i64p), *[L.ptr(a, L.i32p) for a in src])
    o = dict(res_gather=np.full(after.n_residuals, -999, np.int32), point_gather=np.full(after.n_points, -999, np.int32),
             before_res=np.zeros(before.n_residuals, np.int32), before_pt=np.zeros(before.n_points, np.int32),
             after_res=np.zeros(after.n_residuals, np.int32), after_pt=np.zeros(after.n_points, np.int32),
             n_mismatch=np.full(1, -1, np.int32))
    rc = lib.ldso_ba_edit_plan_check(C.byref(sb), C.byref(e), item_order, top_chunk, *[L.ptr(v, L.i32p) for v in o.values()])
    return rc, o


def check_plan(before, after, srcs, o):
    _, point_src, res_src = srcs
    assert o["n_mismatch"][0] == 0
    for gather, order, old_order, src, n_old in ((o["res_gather"], o["after_res"], o["before_res"], res_src, before.n_residuals),
                                                 (o["point_gather"], o["after_pt"], o["before_pt"], point_src, before.n_points)):
        assert sorted(order.tolist()) == list(range(len(src)))  # a device order of the edited window
        carried = gather >= 0
        # every carried destination reads the old device position of its own source entry ...
        assert np.all(gather[carried] < n_old)
        np.testing.assert_array_equal(old_order[gather[carried]], src[order[carried]])
        assert np.all(src[order[carried]] >= 0) and np.all(src[order[~carried]] == -1)
        # ... no old position twice, and the new entries by their rank among the new ones in caller order
        assert len(set(gather[carried].tolist())) == int(carried.sum())
        fresh = np.flatnonzero(src == -1)
        np.testing.assert_array_equal(fresh[~gather[~carried]], order[~carried])


@pytest.mark.parametrize("rank", [False, True], ids=["caller_order", "point_rank"])
@pytest.mark.parametrize("item_order", [0, 1])
@pytest.mark.parametrize("name", list(ec.EDITS))
def test_plan_is_the_layout_of_after(built, name, item_order, rank):
    pool = ec.make_pool()
    sel = ec.base_sel(pool)
    before = ec.window_of(pool, sel, rank=rank)
    after, srcs = ec.window_of(pool, ec.EDITS[name](pool, sel), sel, rank=rank)
    rc, o = plan(before, after, srcs, item_order)
    assert rc == 0, L.lib().ldso_ba_last_error()
    check_plan(before, after, srcs, o)
    if name == "g_identity":
        np.testing.assert_array_equal(o["res_gather"], np.arange(before.n_residuals))
        np.testing.assert_array_equal(o["point_gather"], np.arange(before.n_points))


def test_plan_two_edits_in_a_row(built):
    pool = ec.make_pool()
    s0 = ec.base_sel(pool)
    s1 = ec.edit_drop(pool, s0)
    s2 = ec.edit_insert_points(pool, s1)
    w0 = ec.window_of(pool, s0)
    w1, src1 = ec.window_of(pool, s1, s0)
    rc, o = plan(w0, w1, src1)
    assert rc == 0
    check_plan(w0, w1, src1, o)
    w2, src2 = ec.window_of(pool, s2, s1)
    rc, o = plan(ec.window_of(pool, s1), w2, src2)
    assert rc == 0
    check_plan(w1, w2, src2, o)


def test_plan_of_the_large_cycle(built):
    """N = 7 -> 6 -> 7 at an S7 window's point count: chunks of 16 over buckets of hundreds."""
    pool = ec.make_pool(n_frames=8, n_points=2300, seed=43)
    s7 = ec.full_sel(pool, range(7))
    s6 = ec.edit_remove_frame(pool, s7, 0)
    s7b = ec.edit_append(pool, s6, 7)
    assert len(s7.pts) >= 1900
    for a, b in ((s7, s6), (s6, s7b)):
        wa = ec.window_of(pool, a)
        wb, src = ec.window_of(pool, b, a)
        rc, o = plan(wa, wb, src)
        assert rc == 0, L.lib().ldso_ba_last_error()
        check_plan(wa, wb, src, o)


def test_plan_reads_no_carried_value(built):
    """after's per-entry arrays may be NULL when nothing is new, and must be given when something is."""
    pool = ec.make_pool()
    sel = ec.base_sel(pool)
    before = ec.window_of(pool, sel)
    lib = L.lib()

    def run(edit):
        after, srcs = ec.window_of(pool, edit(pool, sel), sel)
        sb, sa = before.c_struct(with_images=False), after.c_struct(with_images=False)
        for k, t in (("point_data", L.f32p), ("res_state", L.i8p), ("res_energy", L.f32p), ("res_flags", L.u8p)):
            setattr(sa, k, C.cast(None, t))
        src = [np.ascontiguousarray(a, np.int32) for a in srcs]
        e = L.LdsoBaEdit(C.pointer(sa), None, *[L.ptr(a, L.i32p) for a in src])
        g = np.full(after.n_residuals, -999, np.int32)
        none = L.ptr(None, L.i32p)
        return lib.ldso_ba_edit_plan_check(C.byref(sb), C.byref(e), 0, 0, L.ptr(g, L.i32p), none, none, none, none, none, none), g

    rc, g = run(ec.edit_drop)
    assert rc == 0 and np.all(g >= 0)
    rc, _ = run(ec.edit_append)
    assert rc < 0 and b"new residuals need" in lib.ldso_ba_last_error()
    rc, _ = run(ec.edit_insert_points)
    assert rc < 0 and b"new points need" in lib.ldso_ba_last_error()


def _bad_twice(after, srcs, before):
    srcs[2][1] = srcs[2][0]
    return b"twice"


def _bad_range(after, srcs, before):
    srcs[1][0] = before.n_points
    return b"not an index of the loaded window"


def _bad_point(after, srcs, before):
    # two carried residuals of different points trade places
    b = after.point_res_begin
    p, q = [i for i in range(after.n_points) if b[i + 1] > b[i]][:2]
    srcs[2][b[p]], srcs[2][b[q]] = srcs[2][b[q]], srcs[2][b[p]]
    return b"image of its old point"


def _bad_host(after, srcs, before):
    p = next(i for i in range(after.n_points) if after.point_res_begin[i + 1] == after.point_res_begin[i])
    after.point_host[p] = (after.point_host[p] + 1) % after.n_frames
    return b"image of its old host"


def _bad_target(after, srcs, before):
    b = after.point_res_begin
    p = next(i for i in range(after.n_points) if b[i + 1] - b[i] == 1)
    free = [t for t in range(after.n_frames) if t not in (after.point_host[p], after.res_target[b[p]])]
    after.res_target[b[p]] = free[0]
    return b"image of its old target"


def _bad_removed_frame(after, srcs, before):
    srcs[0][0] = -1  # frame 0 is said to be a new frame: its points and the residuals into it are still carried
    return b"removed frame"


def _bad_window(after, srcs, before):
    b = after.point_res_begin
    p = next(i for i in range(after.n_points) if b[i + 1] - b[i] >= 2)
    after.res_target[b[p] + 1] = after.res_target[b[p]]
    return b"duplicate"


def _bad_frames(after, srcs, before):
    srcs[0][1] = srcs[0][0]
    return b"twice"


REFUSALS = {"index_twice": _bad_twice, "index_out_of_range": _bad_range, "residual_on_another_point": _bad_point,
            "host_not_the_image": _bad_host, "target_not_the_image": _bad_target, "carried_from_removed_frame": _bad_removed_frame,
            "invalid_window": _bad_window, "frame_twice": _bad_frames}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_plan_refusals(built, name):
    pool = ec.make_pool()
    sel = ec.base_sel(pool)
    before = ec.window_of(pool, sel)
    good, good_src = ec.window_of(pool, ec.edit_drop(pool, sel), sel)
    rc, ref = plan(before, good, good_src)
    assert rc == 0
    after, srcs = ec.window_of(pool, ec.edit_drop(pool, sel), sel)
    srcs = [s.copy() for s in srcs]
    msg = REFUSALS[name](after, srcs, before)
    rc, _ = plan(before, after, srcs)
    assert rc < 0
    assert msg in L.lib().ldso_ba_last_error(), L.lib().ldso_ba_last_error()
    rc, again = plan(before, good, good_src)  # the refusal left nothing behind
    assert rc == 0
    for k in ref:
        np.testing.assert_array_equal(ref[k], again[k])


def test_plan_refuses_item_order_2(built):
    pool = ec.make_pool()
    sel = ec.base_sel(pool)
    before = ec.window_of(pool, sel)
    after, srcs = ec.window_of(pool, ec.edit_identity(pool, sel), sel)
    after = ec.filled(after, srcs, before.res_state, before.res_energy, before.res_flags, before.point_data)
    rc, _ = plan(before, after, srcs, item_order=2)
    assert rc < 0 and b"ITEM_ORDER 2" in L.lib().ldso_ba_last_error()


def test_abi_has_the_edit_entry_points(built):
    lib = L.lib()
    assert lib.ldso_ba_edit_window(None, 0, None) < 0 and b"bad arguments" in lib.ldso_ba_last_error()
    assert lib.ldso_ba_get_point_data(None, 0, None) < 0
    assert C.sizeof(L.LdsoBaEdit) == 40
