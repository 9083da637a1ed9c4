"""bench.py's plain run and --dump-outputs: a plain run prints the headline alone (every leg that
takes runs of its own is null without --full), --steps sets the number of timed steps, and
--dump-outputs writes the last timed step's results as float32 / float64 .npy files, the rows
above the caps being a sample fixed by the counts alone."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("ms_per_step_without_kernel_events", "gn_iteration_batched", "single_window", "s11", "sharded_window",
             "tracker", "cpp_face", "cpu_baseline", "cpu_baseline_single_window", "cpu_baseline_six_threads")


def test_dump_sample_is_whole_below_the_cap_and_fixed_above_it():
    np.testing.assert_array_equal(bench.dump_sample(5, 5, 1), np.arange(5))
    a, b = bench.dump_sample(1000, 10, 2), bench.dump_sample(1000, 10, 2)
    np.testing.assert_array_equal(a, b)
    assert a.size == 10 and np.all(np.diff(a) > 0) and a.min() >= 0 and a.max() < 1000


class StubContext:
    """The getters dump_outputs reads, over three windows of different shapes."""

    def __init__(self):
        self.windows = [types.SimpleNamespace(dim=4 + 8 * n, n_frames=n, n_residuals=r, n_points=p)
                        for n, r, p in ((2, 7, 3), (3, 11, 5), (2, 5, 2))]

    def energy(self, i):
        return np.array([i + 0.5, 0.0, 10.0 * i])

    def system(self, i):
        n = self.windows[i].dim
        return {k: np.full((n, n) if k.startswith("H") else n, float(i + 1)) for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc")}

    def frame_energy_th(self, i):
        return np.full(self.windows[i].n_frames, i + 1, np.float32)

    def residuals(self, i):
        R = self.windows[i].n_residuals
        return dict(state=np.full(R, i, np.int8), state_energy=100.0 * i + np.arange(R, dtype=np.float32),
                    jpjdf=np.full((R, 8), i, np.float32))

    def points(self, i):
        P = self.windows[i].n_points
        return dict(Hdd=100.0 * i + np.arange(P, dtype=np.float32), Hcd=np.full((P, 4), i, np.float32))


def test_dump_outputs_writes_float_arrays_of_every_window(tmp_path):
    total = bench.dump_outputs(StubContext(), str(tmp_path))
    d = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(d) == {"energy", "HA", "bA", "HL", "bL", "Hsc", "bsc", "frame_energy_th",
                      "res_state", "res_state_energy", "res_jpjdf", "pt_Hdd", "pt_Hcd"}
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert total == sum(v.nbytes for v in d.values())
    assert d["energy"].shape == (3, 3) and d["energy"].dtype == np.float64
    assert d["HA"].shape == (3, 28, 28) and d["bsc"].shape == (3, 28) and d["frame_energy_th"].shape == (3, 3)
    # a smaller window fills its own rows and columns, the padding stays zero
    assert np.all(d["HA"][0, :20, :20] == 1.0) and not d["HA"][0, 20:, :].any() and not d["HA"][0, :, 20:].any()
    assert np.all(d["HA"][1] == 2.0)
    np.testing.assert_array_equal(d["frame_energy_th"][2], [3, 3, 0])
    # residual and point rows: the windows concatenated in order
    np.testing.assert_array_equal(d["res_state"], np.repeat([0, 1, 2], [7, 11, 5]).astype(np.float32))
    np.testing.assert_array_equal(d["res_state_energy"][7:18], 100.0 + np.arange(11))
    assert d["res_jpjdf"].shape == (23, 8) and d["pt_Hcd"].shape == (10, 4)
    np.testing.assert_array_equal(d["pt_Hdd"], np.concatenate([np.arange(3), 100.0 + np.arange(5), 200.0 + np.arange(2)]))


def test_dump_outputs_samples_the_same_rows_above_the_caps(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_WINDOWS", 2)
    monkeypatch.setattr(bench, "DUMP_MAX_RESIDUALS", 6)
    monkeypatch.setattr(bench, "DUMP_MAX_POINTS", 4)
    bench.dump_outputs(StubContext(), str(tmp_path / "a"))
    bench.dump_outputs(StubContext(), str(tmp_path / "b"))
    for f in os.listdir(tmp_path / "a"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert a["HA"].shape[0] == a["energy"].shape[0] == 2
    assert a["res_state"].shape == (6,) and a["res_jpjdf"].shape == (6, 8) and a["pt_Hdd"].shape == (4,)
    # a sample in ascending row order: window by window, rows ascending inside a window
    assert np.all(np.diff(a["res_state"]) >= 0)
    rows = bench.dump_sample(23, 6, 2)
    full = np.concatenate([100.0 * i + np.arange(r) for i, r in enumerate((7, 11, 5))])
    np.testing.assert_array_equal(a["res_state_energy"], full[rows].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_dumps_the_last_step(built, tmp_path):
    from ldso_amd import BAContext, synth

    steps, warmup = 7, 1
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--windows", "2", "--frames", "5", "--points", "300", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert d["unit"] == "point-residuals/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value = gathering residuals per second of the timed steps
    assert d["value"] == pytest.approx(d["config"]["residuals_active_per_step"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # the event pair brackets k_linearize on timed steps 0 and 5 of the 7: the loop ran --steps steps
    assert d["roofline"]["event_launches"] == 2 and d["roofline"]["frac"] > 0
    for k in FULL_ONLY:
        assert d[k] is None, k
    assert d["kernel_ms_per_step"] == {} and d["roofline"]["frac_step"] is None

    out = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 * 2 ** 20
    # the same windows through the same number of passes in this process
    ws = [synth.make_window(n_frames=5, n_points=300, seed=1000 + i) for i in range(2)]
    ctx = BAContext(0).load(ws)
    for _ in range(warmup + steps):
        ctx.linearize(fix=False, accumulate=True)
    res = [ctx.residuals(i) for i in range(2)]
    pts = [ctx.points(i) for i in range(2)]
    sys_ = [ctx.system(i) for i in range(2)]
    e = np.stack([ctx.energy(i) for i in range(2)])
    ctx.close()
    assert out["res_state"].shape == (sum(w.n_residuals for w in ws),)
    for k in res[0]:
        np.testing.assert_array_equal(out["res_" + k], np.concatenate([r[k] for r in res]).astype(np.float32))
    for k in pts[0]:
        np.testing.assert_array_equal(out["pt_" + k], np.concatenate([q[k] for q in pts]).astype(np.float32))
    # the f64 sums are accumulated with atomics: equal up to their order (the suite's parity bound)
    np.testing.assert_allclose(out["energy"], e, rtol=1e-9)
    for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc"):
        ref = np.stack([s[k] for s in sys_])
        assert out[k].shape == ref.shape
        assert np.abs(out[k] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-30), k
