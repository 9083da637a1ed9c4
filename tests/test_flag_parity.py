"""ldso_ba_flag_points against flag_ref, exactly: the decision is integer logic plus two float
compares on bit-identical inputs.

(a) the CPU cases (flag_cases: every branch of the tree, test_flag_cases) on the states as loaded;
(b) after the fix pass, and after ldso_ba_optimize plus the fix pass, with flag_ref fed from
    ldso_ba_get_residuals / _get_points / _get_point_data and the idepth_hessian threshold at the
    median of the inlier candidates, so that MARGINALIZED and OUT both occur among them;
(c) the call only reads: a twin context that never flagged holds the same bytes and runs the same
    next pass.
Then the refusals that need a context."""
import numpy as np
import pytest

import flag_cases as fc
import flag_ref
import ragged
import test_edit_parity as tep
from ldso_amd import BAContext
from ldso_amd import _lib as L

pytestmark = pytest.mark.gpu


def params(A, G, th):
    return L.FlagParams.default(min_good_active_res_for_marg=A, min_good_res_for_marg=G, min_idepth_h_marg=th)


def assert_equal(got, ref, what):
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), f"{what}: {k}"


@pytest.mark.parametrize("th", fc.THRESHOLDS)
@pytest.mark.parametrize("ranked", [False, True])
@pytest.mark.parametrize("name", list(fc.CASES))
def test_loaded_cases_equal_the_reference(built, name, ranked, th):
    """(a)"""
    w, (A, G), book = fc.loaded_case(name, ranked)
    c = BAContext(0).load(ragged.clone(w))
    got = c.flag_points(*book, params=params(A, G, th))
    ref, _ = fc.reference(w, w.res_state, w.res_flags, w.point_data[:, 2], np.zeros(w.n_points, np.float32), book, A, G, th)
    assert_equal(got, ref, name)
    assert ref["counts"][flag_ref.OUTLIER] >= 3 and ref["counts"][flag_ref.ACTIVE] >= 3
    # NULL outputs are skipped, NULL params are the defaults
    lib = L.lib()
    st = np.zeros(w.n_points, np.int8)
    ff, ng, lr, ls = [np.ascontiguousarray(a) for a in book]
    L.check(lib.ldso_ba_flag_points(c._h, 0, None, L.ptr(ff, L.u8p), L.ptr(ng, L.i32p), L.ptr(lr, L.i32p), L.ptr(ls, L.i8p),
                                    L.ptr(st, L.i8p), None, None, None, None))
    dflt, _ = fc.reference(w, w.res_state, w.res_flags, w.point_data[:, 2], np.zeros(w.n_points, np.float32), book, 3, 4, 50.0)
    assert np.array_equal(st, dflt["status"])
    c.close()


@pytest.mark.parametrize("stage", ["fix_pass", "optimize_then_fix_pass"])
def test_after_a_pass_equals_the_reference(built, stage):
    """(b)"""
    name = "pool5"
    w = ragged.clone(fc.window(name))
    A, G = fc.CASES[name][1]
    c = BAContext(0).load(w)
    if stage == "optimize_then_fix_pass":
        before = c.point_data(0)[:, 2].copy()
        c.optimize(2, nullspaces=[w.nullspaces()])
        assert not np.array_equal(before, c.point_data(0)[:, 2])
    c.linearize(fix=True, accumulate=True)
    r, pts, idepth = c.residuals(0), c.points(0), c.point_data(0)[:, 2]
    ih = pts["idepth_hessian"]
    book = fc.bookkeeping(w, r["state"], r["flags"], A, G)
    _, d = fc.reference(w, r["state"], r["flags"], idepth, ih, book, A, G, 0.0)
    cand = ~(idepth < 0) & (d["n_live"] > 0) & (d["e1"] | d["e2"] | d["e3"] | d["host_flagged"]) & d["inl_a"] & d["inl_g"]
    assert cand.sum() >= 6, "too few inlier candidates"
    th = float(np.float32(np.median(ih[cand])))
    ref, _ = fc.reference(w, r["state"], r["flags"], idepth, ih, book, A, G, th)
    print(stage, "candidates", int(cand.sum()), "threshold", th, "counts", ref["counts"])
    assert np.any(ref["status"][cand] == flag_ref.MARGINALIZED) and np.any(ref["status"][cand] == flag_ref.OUT)
    got = c.flag_points(*book, params=params(A, G, th))
    assert_equal(got, ref, stage)
    # toRemove's complement is the residuals the pass left active
    assert np.array_equal(got["res_live"], r["flags"] & L.FLAG_ACTIVE)
    c.close()


def test_the_call_only_reads(built):
    """(c)"""
    name = "base4"
    w0 = fc.window(name)
    A, G = fc.CASES[name][1]
    ctxs = []
    for _ in range(2):
        c = BAContext(0).load(ragged.clone(w0))
        c.linearize(fix=True, accumulate=True)
        ctxs.append(c)
    a, b = ctxs
    r = a.residuals(0)
    book = fc.bookkeeping(w0, r["state"], r["flags"], A, G)
    for _ in range(2):  # the second call reuses the staging
        a.flag_points(*book, params=params(A, G, 1.0))
    tep.compare(a, b, "after flag_points")
    for c in ctxs:
        c.linearize(fix=False, accumulate=True)
    tep.compare(a, b, "the next pass")
    for c in ctxs:
        c.close()


def test_refusals(built):
    w, (A, G), book = fc.loaded_case("base4")
    ff, ng, lr, ls = book
    c = BAContext(0).load(ragged.clone(w))
    p = int(np.flatnonzero(np.diff(w.point_res_begin) > 0)[0])
    for wrong in (int(w.point_res_begin[p + 1]) % w.n_residuals, w.n_residuals, -2):
        bad = lr.copy()
        bad[p, 1] = wrong
        with pytest.raises(L.LdsoError, match="neither -1 nor a residual of its point"):
            c.flag_points(ff, ng, bad, ls)
    with pytest.raises(L.LdsoError, match="last_state is null"):
        c.flag_points(ff, ng, lr, None)
    ok = c.flag_points(ff, ng, lr, ls, params=params(A, G, -1.0))  # the refusals left nothing behind
    ref, _ = fc.reference(w, w.res_state, w.res_flags, w.point_data[:, 2], np.zeros(w.n_points, np.float32), book, A, G, -1.0)
    assert_equal(ok, ref, "after refusals")
    m = BAContext(0).load_marginalization(c, 0, ragged.clone(w))
    with pytest.raises(L.LdsoError, match="marginalisation"):
        m.flag_points(ff, ng, lr, ls)
    m.close()
    c.load(ragged.clone(w), 0, 2)
    with pytest.raises(L.LdsoError, match="sharded"):
        c.flag_points(ff, ng, lr, ls)
    c.close()
