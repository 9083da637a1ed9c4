"""The coarse initializer's scenes are well posed (CPU): tests/init_ref.py, the numpy restatement of
CoarseInitializer::trackFrame, runs free over every scene of tests/init_scenes.py.

 - the shifted scenes snap and recover t = (0.03, 0, 0) up to scale and sign; the unshifted one never snaps;
 - every decision the restatement takes from a float sum -- the alpha cap, accept, the inc.norm() > eps
   exit -- keeps a margin above what the any-order bound (n - 1) 2^-24 sum|term| of the sums behind it can
   move it (init_ref.Initializer.margins; for the exit the bound goes through the first-order sensitivity
   of the solve, init_ref.inc_bound).  Zero undecidable decisions: a device run whose sums differ from the
   restatement's within the bound must take the same decisions, which is what tests/test_init.py demands.
   A scene that fails this gets another seed, not an allowance.
Ranks of the library's optReg sweep on these scenes (init_ref.sweep_ranks): 88 / 45 / 24 for the 600 / 150 /
40 point lists of "shift"; at most 120 on any committed list.
"""
import numpy as np
import pytest

import init_ref as IR
import init_scenes as S

f32 = np.float32
RUNS = [(name, 1, None) for name in S.CASES] + [("shift", 8, None), ("same", 3, None), ("shift", 1, (1, 1, 1, 1, 1)),
                                                 ("shift", 1, (0, 0, 0, 0, 0))]


@pytest.mark.parametrize("name,frames,iters", RUNS)
def test_scene_is_well_posed(name, frames, iters):
    sc = S.scene(name)
    ref = sc.reference(**({} if iters is None else dict(max_iterations=iters)))
    res = None
    for k in range(1, frames + 1):
        dI, e = sc.frame_dI(k)
        res, log = ref.track_frame(dI, e)
        assert res["frame_id"] == k and len(log) >= 2 * sc.levels
        if sc.kind == "same":
            assert not res["snapped"] and not any(l["alpha_capped"] for l in log)
    undecidable = [(kind, m, b) for kind, m, b in ref.margins if not m > b]
    assert not undecidable, undecidable
    assert {"alpha_cap", "accept", "inc_norm"} <= {kind for kind, _, _ in ref.margins}
    if sc.kind != "same" and iters is None:
        t = res["this_to_next"][:, 3]
        assert res["snapped"] and np.linalg.norm(t) > 1 / 60
        assert abs(t[0]) / np.linalg.norm(t) > 0.99, t  # t = (0.03, 0, 0) up to scale and sign
        if sc.kind == "expo":
            assert abs(res["this_to_next_aff"][0] - np.log(1.3)) < 0.02
    if frames == 8:  # snapped && frameID > snappedAt + 5
        assert res["snapped_at"] == 1 and res["ret"] == 1


def test_rank_counts_of_the_scenes():
    ranks = {name: [IR.sweep_ranks(p["neighbours"]) for p in S.scene(name).points] for name in S.CASES}
    assert ranks["shift"] == [88, 45, 24]
    assert max(max(r) for r in ranks.values()) <= 120
    assert ranks["one_point_level"][2] == 1


def test_accumulator_shift_up_rule():
    rng = np.random.default_rng(3)
    t = rng.standard_normal(2500).astype(f32) * f32(1000)
    a, a1k, a1m, n1, n1k = f32(0), f32(0), f32(0), 0, 0  # Accumulator11::updateSingle, lane 0
    for v in t:
        a = a + v
        n1 += 1
        if n1 > 1000:
            a1k, a, n1k, n1 = a + a1k, f32(0), n1k + n1, 0
        if n1k > 1000:
            a1m, a1k, n1k = a1k + a1m, f32(0), 0
    a1k = a + a1k
    a1m = a1k + a1m
    assert IR.acc_sum(t) == a1m
    exact, bound = IR.sum_bound(t)
    assert abs(float(a1m) - exact) <= bound


def test_fmaf_is_one_rounding():
    a, b, c = f32(1 + 2 ** -12), f32(1 + 2 ** -12), f32(-1)
    assert float(IR.fmaf(a, b, c)) == 2 ** -11 + 2 ** -24          # the product's low bits survive
    assert float(a * b + c) == 2 ** -11                              # two roundings lose them
    assert float(IR.fmaf(f32(3), f32(5), f32(7))) == 22.0
