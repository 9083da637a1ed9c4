"""Sharded contexts on the ragged windows of tests/ragged.py, in one process on one GPU.

The multi-rank path of SURVEY.md §8e without the RCCL exchange: `world` contexts on device 0, each
loaded with its run of the host-frame partition (ldso_ba_load(rank, world)), and the test doing the
reduction and the gather itself through the library's documented calls -- ldso_ba_copy_packed out,
the float64 sum in rank order, ldso_ba_copy_packed in; ldso_ba_newest_stride (max over the ranks),
ldso_ba_export_newest into one [world][n_windows][stride] buffer, ldso_ba_frame_threshold_gathered on
every rank.  Shards does that; union_* put the ranks' caller-order reads back together into the
window's arrays and assert that a shard writes only its own run.  SHARD_CASES are the windows and
world sizes tests/test_sharded_cases.py (CPU, the oracle alone) and tests/test_sharded_parity.py (GPU)
share; shard_properties counts what each case is named for, from ldso_ba_shard_points alone.
"""
import ctypes as C

import numpy as np

import ragged
from ldso_amd import _lib as L
from ldso_amd import dist as ldist
from ldso_amd import synth

WORLDS = (1, 2, 3, 4, 7, 16)  # the shard rule is checked on every case window at each of these
TUNE_TOP_CHUNK, TUNE_SOLVE_EXACT = 6, 12  # LDSO_BA_TUNE_*
RESIDUAL_KEYS = ("new_state", "state", "flags", "state_energy", "new_energy_wo", "center")
POINT_KEYS = ("Hdd", "bd", "Hcd", "HdiF", "bdSumF", "idepth_hessian")
DEFAULT_TH = np.float32(12 * 12 * 8)  # setNewFrameEnergyTH without a candidate: 12 * 12 * patternNum


def device_order(w):
    """The caller's point indices in the device (host-frame) order: host frames in window order, each
    host's points by point_rank, in the caller's order without it."""
    rank = np.arange(w.n_points) if w.point_rank is None else np.asarray(w.point_rank)
    return np.lexsort((rank, w.point_host))


def residual_mask(w, points):
    """[R] bool: the residuals of `points` (caller indices)."""
    m = np.zeros(w.n_residuals, bool)
    for p in points:
        m[w.point_res_begin[p]:w.point_res_begin[p + 1]] = True
    return m


def shard_properties(w, world):
    """What a sharded case is named for, counted from ldist.shard_points: per rank the points P, the
    residuals R, the residuals into the newest frame and the hosts touched, and from those
      empty_ranks             ranks with P = 0
      ranks_without_residuals ranks with P > 0 and R = 0
      ranks_without_newest    ranks with P > 0 and no residual into frame N - 1
      split_hosts             hosts whose points lie on more than one rank (a cut inside the host)
      largest_piece           the most points of one split host on one rank (0: no host is split);
                              k_point_sc's items are blocks of one host's points within the shard,
                              so a piece of 17 is one point past a block of 16
    and frames = N."""
    N = w.n_frames
    nres = np.diff(w.point_res_begin)
    P, R, newest, hosts = [], [], [], []
    for r in range(world):
        mine = ldist.shard_points(w, r, world)
        P.append(int(len(mine)))
        R.append(int(nres[mine].sum()))
        newest.append(int(np.sum(w.res_target[residual_mask(w, mine)] == N - 1)))
        hosts.append(sorted(set(w.point_host[mine].tolist())))
    split, largest = 0, 0
    for h in range(N):
        on = [r for r in range(world) if h in hosts[r]]
        if len(on) > 1:
            split += 1
            for r in on:
                largest = max(largest, int(np.sum(w.point_host[ldist.shard_points(w, r, world)] == h)))
    return dict(P=P, R=R, newest=newest, hosts=hosts, frames=N,
                empty_ranks=sum(1 for p in P if p == 0),
                ranks_without_residuals=sum(1 for p, r in zip(P, R) if p > 0 and r == 0),
                ranks_without_newest=sum(1 for p, n in zip(P, newest) if p > 0 and n == 0),
                split_hosts=split, largest_piece=largest)


# ---- the cases -------------------------------------------------------------------------------------
# windows: an edge window of ragged.EDGE_CASES by name, or a callable -> list of windows; world: the
# number of shards; want: lower bounds on shard_properties' counts (for a batch: met by at least one
# of its windows), the reason the case is there.  A draw that stops meeting one is replaced, never
# the bound.
_S = dict(width=160, height=120)


def _n2p6():
    return [ragged.frontend_window(synth.make_window(n_frames=2, n_points=6, seed=321, **_S), np.random.default_rng(15001))]


def _no_newest():
    return [ragged.frontend_window(synth.make_window(n_frames=5, n_points=120, seed=311, **_S),
                                   np.random.default_rng(15004), untargeted=4)]


SHARD_CASES = {
    "N2P40": dict(windows="N2P40", world=4, want=dict(ranks_without_newest=2)),
    "N3_one_each": dict(windows="N3_one_each", world=3, want=dict(ranks_without_newest=1)),
    "N7_holes_rank": dict(windows="N7_holes_rank", world=3, want=dict(split_hosts=1)),
    "N8P200": dict(windows="N8P200", world=4, want=dict(split_hosts=1)),
    "N11P200": dict(windows="N11P200", world=7, want=dict(split_hosts=3)),
    "N16P120": dict(windows="N16P120", world=2, want=dict(frames=12)),  # k_stitch's records path
    # pieces of split hosts: 65 / 11, 35 / 47 and 17 / 64 points -- one past four blocks of 16, and one past one
    "host1_17": dict(windows="host1_17", world=4, want=dict(ranks_without_newest=1, split_hosts=3, largest_piece=65)),
    # 30 / 35 and 64 / 18: the 65-point host is cut, and a piece of exactly four blocks (loads this small
    # run k_point_sc in blocks of 16 whatever the shard count, so no piece here meets a block of 64)
    "host1_65": dict(windows="host1_65", world=3, want=dict(split_hosts=2, largest_piece=64)),
    "N2P6": dict(windows=_n2p6, world=8, want=dict(empty_ranks=2, ranks_without_newest=3)),
    "no_newest": dict(windows=_no_newest, world=3, want=dict(ranks_without_newest=3)),
    "batch": dict(windows=ragged.batch_windows, world=3, want=dict(ranks_without_residuals=3, split_hosts=1)),
}
SOLVE_CASES = ["N3_one_each", "N7_holes_rank", "N8P200", "N11P200"]  # GN lock-step (<= 11 keyframes)


def case_windows(name, settings=None):
    src = SHARD_CASES[name]["windows"]
    if isinstance(src, str):
        return [ragged.edge_window(src, settings)]
    ws = src()
    for w in ws:
        if settings is not None:
            w.settings = settings
            w.refresh_frame_terms()
    return ws


def check_case_properties(name, ws=None):
    """Assert that the case has what it is named for; returns shard_properties per window."""
    case = SHARD_CASES[name]
    ws = case_windows(name) if ws is None else ws
    props = [shard_properties(w, case["world"]) for w in ws]
    for k, v in case["want"].items():
        assert max(pr[k] for pr in props) >= v, (name, k, [pr[k] for pr in props], v)
    if name == "no_newest":  # no rank has a slot to export: stride 0 before the clamp
        assert all(not any(pr["newest"]) for pr in props)
    return props


# ---- the ranks ---------------------------------------------------------------------------------------
class Shards:
    """`world` contexts on device 0, rank r holding shard r of every window (loaded from
    ragged.clone); mine[r][i]: the caller point indices of window i on rank r."""

    def __init__(self, windows, world, settings=None, tuning=()):
        from ldso_amd import BAContext

        self.windows = list(windows)
        self.world = world
        self.mine = [[ldist.shard_points(w, r, world) for w in self.windows] for r in range(world)]
        self.ctxs = []
        for r in range(world):
            c = BAContext(0)
            for key, value in tuning:
                c.set_tuning(key, value)
            if settings is not None:
                c.set_settings(settings)
            c.load([ragged.clone(w) for w in self.windows], shard_rank=r, shard_count=world)
            self.ctxs.append(c)
        self.partials = self.energy = self.stride = self.gathered = None

    def close(self):
        for c in self.ctxs:
            c.close()
        self.ctxs = []

    def pass_and_exchange(self, fix=False, accumulate=True):
        """One pass on every rank and the exchange a communicator would run after it.  Leaves
        partials [world][sys_n] (the ranks' packed systems before the reduction; accumulate only),
        energy [n_windows][3] (summed on the host), stride and gathered [world][n_windows][stride]."""
        import torch

        lib = L.lib()
        for c in self.ctxs:
            c.linearize(fix=fix, accumulate=accumulate)
        if accumulate:
            n = self.ctxs[0].packed_system()[1]
            dev = torch.zeros(n, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()  # torch's stream wrote dev; the library copies on its own stream
            self.partials, total = [], np.zeros(n, np.float64)
            for c in self.ctxs:
                L.check(lib.ldso_ba_copy_packed(c._h, dev.data_ptr(), n, 0))
                self.partials.append(dev.cpu().numpy().copy())
                total += self.partials[-1]  # float64, in rank order
            dev.copy_(torch.from_numpy(total))
            torch.cuda.synchronize()
            for c in self.ctxs:
                L.check(lib.ldso_ba_copy_packed(c._h, dev.data_ptr(), n, 1))
        self.energy = [sum(c.energy(i) for c in self.ctxs) for i in range(len(self.windows))]
        return self.exchange_threshold()

    def exchange_threshold(self):
        """The documented three-call route alone: the stride agreed as the maximum over the ranks,
        every rank's export into its slot of one buffer, the gathered re-selection on every rank."""
        import torch

        lib = L.lib()
        strides = []
        for c in self.ctxs:
            st = C.c_int64(-1)
            L.check(lib.ldso_ba_newest_stride(c._h, C.byref(st)))
            strides.append(st.value)
        self.stride = max(strides)
        # a slot the export missed would put 3e38 among the candidates
        g = torch.full((self.world, len(self.windows), self.stride), 3e38, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for r, c in enumerate(self.ctxs):
            L.check(lib.ldso_ba_export_newest(c._h, g[r].data_ptr(), self.stride))
        for c in self.ctxs:
            L.check(lib.ldso_ba_frame_threshold_gathered(c._h, g.data_ptr(), self.world, self.stride))
        self.gathered = g.cpu().numpy()
        return self

    def _union(self, i, reads, masks):
        """The ranks' caller-order reads of window i put together: from rank r the slots of masks[r];
        every other slot of rank r's read must still hold the zero bytes it was given."""
        out = None
        for r, (got, m) in enumerate(zip(reads, masks)):
            if out is None:
                out = {k: np.zeros_like(v) for k, v in got.items()}
            for k, v in got.items():
                assert not np.ascontiguousarray(v[~m]).view(np.uint8).any(), \
                    f"rank {r} wrote {k} of window {i} outside its own run"
                out[k][m] = v[m]
        return out

    def union_residuals(self, i):
        w = self.windows[i]
        return self._union(i, [c.residuals(i) for c in self.ctxs],
                           [residual_mask(w, self.mine[r][i]) for r in range(self.world)])

    def _point_masks(self, i):
        masks = []
        for r in range(self.world):
            m = np.zeros(self.windows[i].n_points, bool)
            m[self.mine[r][i]] = True
            masks.append(m)
        return masks

    def union_points(self, i):
        return self._union(i, [c.points(i) for c in self.ctxs], self._point_masks(i))

    def union_steps(self, lam=1e-5):
        """resubstitute_device on every rank -> the point steps of every window in caller order."""
        steps = [c.resubstitute_device(lam) for c in self.ctxs]
        return [self._union(i, [dict(step=steps[r][i]) for r in range(self.world)], self._point_masks(i))["step"]
                for i in range(len(self.windows))]
