"""Every entry point that takes a caller-owned workspace, on a workspace of EXACTLY the queried size: a 256-byte-aligned view
inside a larger uint8 allocation whose surroundings hold a canary (tests/guarded.py's idea, for bytes), and again on one four
times that size filled with 0xFF.  Outputs and status words are bit-equal between the two calls and the canary is intact: the
layout stays inside what the size query promises and no result depends on what the workspace held or on what lies behind it.
A layout check on the smallest inputs of the entries' own tests; what the entries compute is those tests' business."""
import types

import numpy as np
import pytest
import torch

import imuref as ir
import propref as pr
from trackerkit import cu

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5


class Arena:
    """stands in for the package's scratch allocator.  factor 1: the exact view between canaries; 4: four times, 0xFF"""

    def __init__(self, factor):
        self.factor, self.made = factor, []

    def workspace(self, nbytes, device, tag="ws"):
        n = int(nbytes) * self.factor
        if self.factor != 1:
            return torch.full((max(n, 1),), 0xFF, dtype=torch.uint8, device=device)
        buf = torch.full((n + 2 * GUARD + 256,), CANARY, dtype=torch.uint8, device=device)
        at = GUARD + (-(buf.data_ptr() + GUARD)) % 256
        view = buf[at:at + n]
        view.fill_(0x5A)
        assert view.data_ptr() % 256 == 0 and view.numel() == n
        self.made.append((buf, at, n))
        return view

    def sized_workspace(self, query, dims, device, tag="ws"):
        from rampvo_amd import _lib
        ws = self.workspace(getattr(_lib.lib(), query)(*dims), device, tag)
        return ws, ws.numel()

    def intact(self):
        torch.cuda.synchronize()
        assert self.made or self.factor != 1, "the call took no workspace"
        return all(bool((buf[:at] == CANARY).all()) and bool((buf[at + n:] == CANARY).all()) for buf, at, n in self.made)


def tensors(r):
    if r is None:
        return []
    if torch.is_tensor(r):
        return [r]
    if isinstance(r, dict):
        return [t for k in sorted(r) for t in tensors(r[k])]
    if isinstance(r, (tuple, list)):
        return [t for v in r for t in tensors(v)]
    names = getattr(r, "__slots__", None) or sorted(getattr(r, "__dict__", {}))       # (ops.Groups, a plan)
    return [t for k in names for t in tensors(getattr(r, k))]


def same_bits(a, b):
    a, b = tensors(a), tensors(b)
    assert len(a) == len(b) and len(a) > 0
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert torch.equal(u.contiguous().reshape(-1).view(torch.uint8), v.contiguous().reshape(-1).view(torch.uint8))


def exact_then_wide(monkeypatch, call):
    """call() under the exact arena, then under the wide one; its results compared, the canary checked.  Output tensors start
    from zero in both calls, so that a tail an entry documents as unwritten compares equal"""
    from rampvo_amd import _lib, ops
    out = []
    for factor in (1, 4):
        arena = Arena(factor)
        monkeypatch.setattr(torch, "empty", torch.zeros)
        monkeypatch.setattr(_lib, "workspace", arena.workspace)
        monkeypatch.setattr(ops, "_lib_workspace", arena.workspace)
        monkeypatch.setattr(ops, "sized_workspace", arena.sized_workspace, raising=False)
        out.append(call())
        assert arena.intact()
    same_bits(out[0], out[1])
    return out[0]


def _edges(E, n_kk=40, n_jj=7, seed=5):
    rng = np.random.default_rng(seed)
    return cu(rng.integers(0, n_kk, E)), cu(rng.integers(0, n_jj, E))


def test_group_by_and_neighbors(monkeypatch):
    from rampvo_amd import ops
    kk, jj = _edges(257)
    g = exact_then_wide(monkeypatch, lambda: ops.group_by(kk, 40))
    assert int(g.ngroups) == len(np.unique(kk.cpu().numpy()))
    exact_then_wide(monkeypatch, lambda: ops.group_by(kk, 0))                        # (every key bit sorted)
    exact_then_wide(monkeypatch, lambda: ops.neighbors(kk, jj, 40, 7))              # one composite pass
    exact_then_wide(monkeypatch, lambda: ops.neighbors(kk, jj, 0, 0))               # two passes: order1 and order2


def test_group_by_small(monkeypatch):
    from rampvo_amd import ops
    kk, _ = _edges(257, n_kk=5)
    g = exact_then_wide(monkeypatch, lambda: ops.group_by_small(kk, None, 1, 0, 5))
    assert int(g.ngroups) == 5


def _events(n, h, w, seed=11):
    rng = np.random.default_rng(seed)
    return (cu(rng.uniform(0, w - 1, n).astype(np.float32)), cu(rng.uniform(0, h - 1, n).astype(np.float32)),
            cu(np.sort(rng.uniform(0.0, 1.0, n))), cu(rng.choice([-1, 1], n).astype(np.int8)))


def test_event_filter(monkeypatch):
    from rampvo_amd import ops
    x, y, t, _ = _events(4099, 13, 17)
    r = exact_then_wide(monkeypatch, lambda: ops.event_filter(x, y, t, 13, 17, support_dt=0.5, refractory=1e-4, hot_count=25,
                                                              want_index=True))
    assert int(r["status"][0]) == 0 and 0 < int(r["count"]) < 4099


def _trajectory(T=5):
    times = np.linspace(0.0, 1.0, T)
    knots = np.zeros((T, 7), np.float32)
    knots[:, 0], knots[:, 1] = 0.02 * times, -0.01 * times
    phi = np.stack([0.02 * times, 0.01 * times, -0.03 * times], 1)
    knots[:, 3:6], knots[:, 6] = 0.5 * phi, 1.0
    knots[:, 3:] /= np.linalg.norm(knots[:, 3:], axis=1, keepdims=True)
    return cu(knots), cu(times)


WARP = dict(h=24, w=32, K=np.array([30.0, 30.0, 16.0, 12.0], np.float32))


def test_event_warp(monkeypatch):
    from rampvo_amd import ops
    x, y, t, p = _events(1000, WARP["h"], WARP["w"])
    knots, times = _trajectory()
    args = (x, y, t, p, knots, times, 0.5, cu(WARP["K"]), 0.5, WARP["h"], WARP["w"])
    r = exact_then_wide(monkeypatch, lambda: ops.event_warp(*args, num_bins=5, want_xy=True, want_iwe=True, stack="f32"))
    assert int(r["status"][0]) == 0 and torch.isfinite(r["stack"]).all()
    exact_then_wide(monkeypatch, lambda: ops.event_warp(*args, num_bins=5, want_iwe=False, stack="f32"))    # the stack alone
    exact_then_wide(monkeypatch, lambda: ops.event_warp(*args, want_iwe=True))                                  # the image alone
    exact_then_wide(monkeypatch, lambda: ops.event_stack(x, y, p, WARP["h"], WARP["w"], num_bins=5))            # the identity warp


def test_event_contrast_and_align(monkeypatch):
    from rampvo_amd import ops
    x, y, t, p = _events(1000, WARP["h"], WARP["w"])
    knots, times = _trajectory()
    args = (x, y, t, p, knots, times, 0.5, cu(WARP["K"]), 0.5, WARP["h"], WARP["w"])
    r = exact_then_wide(monkeypatch, lambda: ops.event_contrast(*args, want_grad=True, want_iwe=True))
    assert torch.isfinite(r["stats"]).all() and torch.isfinite(r["grad"]).all()
    r = exact_then_wide(monkeypatch, lambda: ops.event_align(*args, iters=2, resident=True))
    assert ops.event_align_info(r["info"])["n_evals"] >= 1


def test_event_voxel_in_chunks(monkeypatch):
    from rampvo_amd import ops
    monkeypatch.setattr(ops, "VOXEL_WORKSPACE_CAP", 0)                   # the workspace of one slice: three chunks
    x, y, t, p = _events(1500, 13, 17)
    off = cu(np.array([0, 400, 900, 1500], np.int64))
    r = exact_then_wide(monkeypatch, lambda: ops.event_voxel_grid(x, y, t, p, 13, 17, num_bins=5, offsets=off))
    assert int(r["status"][0]) == 0 and r["grid"].shape == (3, 5, 13, 17)
    monkeypatch.undo()
    whole = ops.event_voxel_grid(x, y, t, p, 13, 17, num_bins=5, offsets=off)
    same_bits(whole, r)                                                   # (any chunking, the same bits)


def test_event_stack_and_topk(monkeypatch):
    from rampvo_amd import ops
    x, y, _, p = _events(1000, 32, 48)
    stack = exact_then_wide(monkeypatch, lambda: ops.event_stack(x.to(torch.int32), y.to(torch.int32), p, 32, 48, num_bins=5))
    exact_then_wide(monkeypatch, lambda: ops.event_topk(stack, 8, nms_kernel_size=3, want_indices=True))


def test_invdepth_map(monkeypatch):
    from rampvo_amd import ops
    rng = np.random.default_rng(2)
    K, h, w, R = 24, 24, 32, 2.0                                          # K points, each seen from its own identity camera
    ident = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
    patches = np.zeros((K, 3, 3, 3), np.float32)
    patches[:, 0] = rng.uniform(-R, w - 1 + R, (K, 1, 1))
    patches[:, 1] = rng.uniform(-R, h - 1 + R, (K, 1, 1))
    patches[:, 2] = rng.uniform(0.2, 1.0, (K, 1, 1))
    K4 = np.array([30.0, 20.0, 19.5, 11.25], np.float32)
    r = exact_then_wide(monkeypatch, lambda: ops.invdepth_map(cu(np.repeat(ident[None], K, 0)), cu(patches), cu(K4), cu(ident), h, w,
                                                              R, prior=0.4, prior_weight=0.7, want_records=True))
    assert int(r["status"][1]) == K


def test_imu_align(monkeypatch):
    from rampvo_amd import ops
    s = ir.scene()
    times = np.array([0.5, 1.5, 2.5, 3.5, 4.5])
    tau, gyro, accel = (cu(s[k][:1000]) for k in ("tau", "gyro", "accel"))
    r = exact_then_wide(monkeypatch, lambda: ops.imu_align(tau, gyro, accel, cu(ir.knots_at(times)), cu(times), R_bc=ir.R_BC,
                                                           p_bc=ir.P_BC, gyro_steps=2))
    assert int(r["status"][2]) == 4                                       # (the intervals of five knots)
    exact_then_wide(monkeypatch, lambda: ops.imu_align(tau, gyro, accel, cu(ir.knots_at(times)), cu(times), R_bc=ir.R_BC,
                                                       p_bc=ir.P_BC, want_preint=True))


def test_imu_propagate(monkeypatch):
    from rampvo_amd import ops
    N = 4097                                                              # one sample into the second tile
    tau = 5.0 + (np.arange(N) - 3.5) / 400.0
    gyro = np.stack([0.3 * np.sin(tau), 0.2 * np.cos(1.3 * tau), 0.1 * np.sin(0.7 * tau)], 1)
    accel = np.stack([0.5 * np.cos(tau), 0.4 * np.sin(0.9 * tau), 9.8 + 0.2 * np.sin(2.0 * tau)], 1)
    anchor = cu(pr.scene_anchor(5.0))
    r = exact_then_wide(monkeypatch, lambda: ops.imu_propagate(cu(tau), cu(gyro), cu(accel), anchor, R_bc=ir.R_BC, p_bc=ir.P_BC,
                                                               want_state=True))
    st = ops.imu_propagate_status(r["status"])
    assert int(r["status"][0]) == 0 and st["n_held"] == 4 and st["n_propagated"] == N - 4


def test_se3_interp(monkeypatch):
    """(ops.se3_interp allocates its segment table itself: the entry is called directly)"""
    from rampvo_amd import _lib
    lib = _lib.lib()
    knots, times = _trajectory(9)
    query = cu(np.linspace(-0.1, 1.1, 301))
    nbytes = lib.ramp_se3_interp_workspace_bytes(9)
    out = []
    for factor in (1, 4):
        arena = Arena(factor)
        ws = arena.workspace(nbytes, knots.device)
        r = dict(out=torch.empty((301, 7), device="cuda"), tw=torch.empty((301, 6), device="cuda"),
                 status=torch.zeros(4, dtype=torch.int32, device="cuda"))
        _lib.check(lib.ramp_se3_interp(_lib.ptr(knots), _lib.ptr(times), 9, _lib.ptr(query), 301, 0, _lib.ptr(r["out"]),
                                       _lib.ptr(r["tw"]), _lib.ptr(ws), ws.numel(), _lib.ptr(r["status"]), _lib.stream()),
                   "ramp_se3_interp")
        assert arena.intact()
        out.append(r)
    same_bits(out[0], out[1])
    assert torch.isfinite(out[0]["out"]).all()


@pytest.fixture(scope="module")
def ba_problem():
    """the (E, n_poses, n_patches, t0, t1) = (100, 11, 88, 1, 11) problem"""
    from scenes import ba_scene
    s = ba_scene(seed=3, n_frames=11, M=8, lifetime=4)
    pick = np.random.default_rng(0).permutation(len(s["ii"]))[:100]
    for k in ("ii", "jj", "kk", "target", "weight"):
        s[k] = s[k][pick]
    assert s["poses"].shape[0] == 11 and s["patches"].shape[0] == 88
    return {k: cu(v) for k, v in s.items() if isinstance(v, np.ndarray)}


def _ba_plan(s):
    from rampvo_amd import ops
    g_kk = ops.group_by(s["kk"], 88)
    g_ij = ops.group_by(s["jj"] * 11 + s["ii"], 121)
    return types.SimpleNamespace(g_kk=g_kk, g_ij=g_ij, max_kk=int(g_kk.ngroups), max_ij=int(g_ij.ngroups))


@pytest.mark.parametrize("planned", [False, True])
def test_bundle_adjustment(monkeypatch, ba_problem, planned):
    from rampvo_amd import ops
    s = ba_problem
    plan = _ba_plan(s) if planned else None
    graph = (s["intr"], s["target"], s["weight"], s["lmbda"], s["ii"], s["jj"], s["kk"], 1, 11)

    def solve():
        poses, patches = s["poses"].clone(), s["patches"].clone()
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.ba(poses, patches, *graph, iterations=2, info=info, plan=plan)
        return poses, patches, info

    poses, _, _ = exact_then_wide(monkeypatch, solve)
    assert not torch.equal(poses, s["poses"])
    exact_then_wide(monkeypatch, lambda: ops.ba_covariance(s["poses"], s["patches"], *graph, plan=plan))
    exact_then_wide(monkeypatch, lambda: ops.ba_map_covariance(s["poses"], s["patches"], *graph, plan=plan))
