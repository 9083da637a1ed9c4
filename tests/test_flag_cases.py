"""The ldso_ba_flag_points cases are well posed: from flag_ref alone (no GPU), every branch of the
decision tree decides at least one point of every case, and each of the four statuses is taken by
at least three.  test_flag_parity runs the same cases on the device."""
import numpy as np
import pytest

import flag_cases as fc
import flag_ref
from ldso_amd import _lib as L


@pytest.mark.parametrize("name", list(fc.CASES))
def test_every_branch_decides_a_point(built, name):
    w, (A, G), book = fc.loaded_case(name)
    ff, ng, lr, ls = book
    ih = np.zeros(w.n_points, np.float32)  # no pass has run
    o, d = fc.reference(w, w.res_state, w.res_flags, w.point_data[:, 2], ih, book, A, G, -1.0)
    neg = w.point_data[:, 2] < 0
    alive = ~neg & (d["n_live"] > 0)  # the points the tree's second step sees
    oob = d["e1"] | d["e2"] | d["e3"]
    cand = alive & (oob | d["host_flagged"])
    # each isOOB exit alone
    assert np.any(alive & d["e1"] & ~d["e2"] & ~d["e3"])
    assert np.any(alive & ~d["e1"] & d["e2"] & ~d["e3"])
    assert np.any(alive & ~d["e1"] & ~d["e2"] & d["e3"])
    # ... the second from a residual of the window and from a retained state
    assert np.any(alive & d["e2"] & (lr[:, 0] >= 0)) and np.any(alive & d["e2"] & (lr[:, 0] == -1) & (ls[:, 0] == L.RES_OOB))
    # ... and the third; only the larger window has a point with two live residuals beside an OUTLIER one
    assert np.any(alive & d["e3"] & (lr[:, 0] == -1))
    if name == "pool5":
        assert np.any(alive & d["e3"] & (lr[:, 0] >= 0))
    # fewer than two residuals with two OUTLIER last states: not out of bounds
    two_out = np.all(o["last_state"] == L.RES_OUTLIER, axis=1)
    assert np.any(alive & two_out & (d["n_live"] < 2) & ~oob)
    # the host alone
    assert np.any(alive & ~oob & d["host_flagged"])
    assert np.any(alive & ~oob & ~d["host_flagged"])
    # idepth_scaled < 0 on a point with live residuals; no residual at all; residuals but none live
    assert np.any(neg & (d["n_live"] > 0))
    assert np.any(~neg & (d["n_res"] == 0)) and np.any(~neg & (d["n_res"] > 0) & (d["n_live"] == 0))
    # isInlierNew false on either half alone, and true
    assert np.any(cand & ~d["inl_a"] & d["inl_g"]) and np.any(cand & d["inl_a"] & ~d["inl_g"])
    assert np.any(cand & d["inl_a"] & d["inl_g"])
    # the statuses
    assert np.all(o["counts"] >= 3), o["counts"]
    assert o["counts"].sum() == w.n_points and np.array_equal(np.bincount(o["status"], minlength=4), o["counts"])
    assert np.array_equal(o["status"] == flag_ref.OUTLIER, ~alive)
    assert np.array_equal(o["status"] == flag_ref.MARGINALIZED, cand & d["inl_a"] & d["inl_g"])
    assert np.array_equal(o["status"] == flag_ref.ACTIVE, alive & ~cand)
    # at the default threshold nothing is marginalised: idepth_hessian is 0
    o50, _ = fc.reference(w, w.res_state, w.res_flags, w.point_data[:, 2], ih, book, A, G, 50.0)
    assert o50["counts"][flag_ref.MARGINALIZED] == 0 and o50["counts"][flag_ref.OUT] == np.sum(cand)
    for k in ("res_live", "num_good", "last_state"):
        assert np.array_equal(o[k], o50[k])


def test_last_res_of_another_point_is_an_error(built):
    w, (A, G), (ff, ng, lr, ls) = fc.loaded_case("base4")
    p = int(np.flatnonzero(np.diff(w.point_res_begin) > 0)[0])
    bad = lr.copy()
    bad[p, 0] = int(w.point_res_begin[p + 1]) % w.n_residuals  # the next point's first residual
    with pytest.raises(AssertionError):
        flag_ref.flag_points(w, w.res_state, w.res_flags, w.point_data[:, 2], np.zeros(w.n_points, np.float32), ff, ng, bad, ls)
