"""The device's stitched system HA, bA, Hsc, bsc against the float64 normal equations rebuilt from
the oracle's per-residual Jacobians, ELEMENT BY ELEMENT within a rounding bound (both tiers of
tests/system_bound.py), where test_gpu_parity's bar is a relative Frobenius error of 1e-4 per 8x8
block.  The windows are the smallest at which the accumulation layout can go wrong:

  * edit_cases.base_sel: buckets of exactly 16, 17 and 1 residuals (k_linearize's chunk is 16), hosts
    of exactly 16 and 17 points (k_point_sc's block is 16);
  * ragged.EDGE_CASES up to 11 keyframes: one-residual points, empty hosts and targets, a point_rank
    permutation, hosts of 1, 17 and 65 points;
  * ragged.batch_windows(): a window with points and no residuals between two others;
  * synth.KITTI00 at 5 keyframes and 300 points: the wide-footprint path.

The twelve 160 x 120 windows share one context (so each also sits behind other windows' item and
residual ranges), the KITTI window has its own; both run under every chunk size and item order that
test_chunk_sizes_agree / test_item_orders_agree sweep and every stitch path of
test_stitch_paths_agree.  The oracle's pass and the rebuild are made once per module."""
import numpy as np
import pytest

import edit_cases
import oracle
import ragged
import system_bound as sb
from ldso_amd import BAContext, synth

pytestmark = pytest.mark.gpu

EDGE_NAMES = ["N2P40", "N3_one_each", "N7_holes_rank", "N8P200", "N11P200", "host1_1", "host1_17", "host1_65"]
KITTI_CFG = dict(synth.KITTI00, n_frames=5, n_points=300, seed=13)

TUNE_TOP_CHUNK, TUNE_ITEM_ORDER = 6, 10
# (name, tuning, environment)
VARIANTS = ([(f"chunk{c}", ((TUNE_TOP_CHUNK, c),), {}) for c in (16, 32, 64)]
            + [(f"order{o}-chunk{c}", ((TUNE_TOP_CHUNK, c), (TUNE_ITEM_ORDER, o)), {}) for o in (1, 2) for c in (16, 64)]
            + [("stitch-split", (), dict(LDSO_BA_HS_SPLIT="1")), ("stitch-whole", (), dict(LDSO_BA_HS_SPLIT="0")),
               ("stitch-records", (), dict(LDSO_BA_STITCH_RECORDS="1"))])


def group_windows(group):
    """[(name, window)] of a group, made afresh on every call."""
    if group == "kitti":
        return [("kitti00_N5P300", synth.make_window(**KITTI_CFG))]
    pool = edit_cases.make_pool()
    out = [("base_sel", edit_cases.window_of(pool, edit_cases.base_sel(pool)))]
    out += [(n, ragged.edge_window(n)) for n in EDGE_NAMES]
    out += [(f"batch{i}", w) for i, w in enumerate(ragged.batch_windows())]
    return out


@pytest.fixture(scope="module")
def references(built):
    """group -> [(name, O, D, B, cnt, active residuals)]: one oracle pass and one rebuild per window."""
    out = {}
    for group in ("small", "kitti"):
        refs = []
        for name, w in group_windows(group):
            ow = oracle.OracleWindow(w, threads=0)
            _, O = ow.iteration()
            res = ow.residuals()
            D, B, cnt = sb.dense_bound(ow.window, ow.jacobians(), res, ow.points()["HdiF"])
            refs.append((name, O, D, B, cnt, int((res["flags"] & 1).sum())))
            ow.close()
        out[group] = refs
    return out


def test_the_windows_are_what_they_are_named_for(references):
    pool = edit_cases.make_pool()
    sel = edit_cases.base_sel(pool)  # asserts its 16 / 17 / 1 buckets and 16 / 17 hosts
    assert len(sel.pts) == 70
    for n in EDGE_NAMES:
        case = ragged.EDGE_CASES[n]
        ragged.check_properties(ragged.edge_window(n), case["opts"], case["want"])
    ws = ragged.batch_windows()
    assert ws[1].n_points > 0 and ws[1].n_residuals == 0
    active = {name: a for refs in references.values() for name, *_, a in refs}
    assert active["batch1"] == 0 and all(a > 0 for n, a in active.items() if n != "batch1"), active
    assert all(w.n_points <= 320 for g in ("small", "kitti") for _, w in group_windows(g))  # host1_*: 320 less the cut


@pytest.mark.parametrize("group", ["small", "kitti"])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_system_is_elementwise_within_rounding(references, monkeypatch, variant, group):
    vname, tuning, env = variant
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = BAContext(0)
    try:
        for key, value in tuning:
            c.set_tuning(key, value)
        c.load([w for _, w in group_windows(group)])
        c.linearize(fix=False, accumulate=True)
        for i, (name, O, D, B, cnt, active) in enumerate(references[group]):
            G = c.system(i)
            if active == 0:
                assert not any(np.any(G[k]) for k in sb.KEYS), name
            sb.assert_elementwise(G, O, D, B, cnt, f"{vname} {name}")
    finally:
        c.close()
