"""Randomised sweep of the activation selection: seeded draws over test_fuzz_immature.py's frame sizes
with random host counts, seed densities, thresholds and flagged hosts, on records as ldso_ct_trace leaves
them after three traces -- the map, the dispositions, the selected indices, the counts, the selected
records and the compacted set against tests/activation_select_ref.py, byte for byte."""
import numpy as np
import pytest

import activation_select_ref as R
import actsel_scenes as S
from ldso_amd import _lib as L
from test_fuzz_immature import SIZES, pose_tables
from test_immature import blob_image

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", range(10))
def test_random_selection_matches_walk(built, case):
    from ldso_amd.tracker import CoarseTracker

    rng = np.random.default_rng(31000 + case)
    w, h = SIZES[case % len(SIZES)]
    w1, h1 = w >> 1, h >> 1
    n_hosts = int(rng.integers(2, 9))  # the last one is the newest
    cmad = float(rng.choice([0.0, 0.7, 1.3, 2.0, 4.0]))
    per_host = int(rng.integers(50, 260))
    n_seeds = int(w1 * h1 / rng.uniform(20, 200))
    print(f"case {case}: {w}x{h}, {n_hosts} hosts, {per_host} records per host, {n_seeds} seeds, cmad {cmad}")
    host_img = blob_image(w, h, seed=case)
    new_img = blob_image(w, h, shift=float(rng.uniform(-6, 6)), seed=case, a=1.05, b=-2.0)
    krki, kt, aff = pose_tables(rng, w, h, n_hosts)
    ct = CoarseTracker(w, h)
    ct.set_new_frame(host_img)
    recs = []
    for i in range(n_hosts):
        uv = np.stack([rng.uniform(5, w - 6, per_host), rng.uniform(5, h - 6, per_host)], 1).astype(np.float32)
        recs.append(ct.make_immature(uv, float(rng.choice([1.0, 2.0, 4.0])), i))
    ct.immature_upload(np.concatenate(recs))
    ct.set_new_frame(new_img)
    for _ in range(3):
        ct.trace(krki, kt, aff)
    pts = ct.immature_download()
    # the level-1 tables of activatePointsMT: K[1] R Ki[0] = D KRKi with D = K[1] Ki[0] (S.PLAIN), and D Kt
    D = S.PLAIN.reshape(3, 3).astype(np.float64)
    krki1 = np.stack([(D @ k.reshape(3, 3).astype(np.float64)).astype(np.float32).reshape(9) for k in krki])
    kt1 = np.stack([(D @ t.astype(np.float64)).astype(np.float32) for t in kt])
    uvd = np.stack([rng.uniform(0, w, n_seeds), rng.uniform(0, h, n_seeds), rng.uniform(0.05, 1.5, n_seeds)], 1)
    uvd = uvd.astype(np.float32)
    seed_host = rng.integers(0, n_hosts - 1, n_seeds).astype(np.int32)
    flagged = (rng.random(n_hosts) < 0.3).astype(np.uint8)
    dm = R.make_distance_map(w1, h1, krki1, kt1, uvd, seed_host)
    m0 = dm.array().copy()
    disp_ref, sel_ref, counts_ref = R.walk(dm, pts, krki1, kt1, cmad, n_hosts - 1, flagged)
    m = ct.make_distance_map(krki1, kt1, uvd, seed_host)
    assert m.tobytes() == m0.tobytes()
    disp, sel, counts = ct.select_activation(cmad, 3.0, n_hosts - 1, flagged, compact=True)
    print("  ", counts)
    assert np.array_equal(disp, disp_ref), np.flatnonzero(disp != disp_ref)[:10]
    assert np.array_equal(sel, sel_ref) and list(counts.values()) == counts_ref
    assert ct.selection_download().tobytes() == pts[sel_ref].tobytes()
    assert ct.immature_download().tobytes() == pts[disp_ref == R.KEEP].tobytes()
    ct.close()
