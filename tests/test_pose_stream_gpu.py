"""Live poses on the GPU: the pose records a tracker publishes while it stays device resident (csrc/publish.hip::
trk_publish_kernel, Ramp_vo.pose_stream / latest_pose / poses_since) and the trajectory so far as one launch
(traj_resolve_kernel, Ramp_vo.trajectory) -- bit for bit against the host-driven tracker and terminate().

Trackers run at 240 x 320 with 48 patches per frame (the size test_pipeline_gpu.py's device-resident test uses) on
SyntheticStream(240, 320, 44, seed=77) with the synthetic `wide` weights, fp16 features (tests/trackerkit.py's tracker with
the default d_gain; the trajectory test runs the kit's own stream and d_gain = 14.5)."""
import numpy as np
import pytest
import torch

import trackerkit as kit
from trackerkit import drop as _drop, tstamp as _tstamp

pytestmark = pytest.mark.gpu

T_FRAMES = 44
_cache = {}


def _frames():
    return kit.frames(240, 320, T_FRAMES, 77, T_FRAMES)


def _tracker(device_steps=True, ready=True):
    return kit.tracker(device_steps, ready, d_gain=None)


def _final_state(slam):
    traj, ts = slam.terminate()          # (hands the state back first)
    n = slam.n
    return dict(n=n, ii=slam._ii.copy(), jj=slam._jj.copy(), kk=slam._kk.copy(), poses=slam.poses_[:n].cpu().numpy(),
                patches=slam.patches_[:n].cpu().numpy(), points=slam.points_[:slam.m].cpu().numpy(), traj=traj, ts=ts)


@torch.no_grad()
def _host_driven_reference():
    """tracker B: device_steps = False; after every call poses_[n - 1] and its inverse, read back"""
    if "B" not in _cache:
        from rampvo_amd.lietorch import SE3
        slam = _tracker(device_steps=False, ready=False)
        rows = []
        for t, (im, ev, K, mask) in enumerate(_frames()):
            slam(_tstamp(t), input_tensor=(ev, im, mask), intrinsics=K)
            p = slam.poses_[slam.n - 1]
            rows.append((t, _tstamp(t), p.cpu().numpy().copy(), SE3(p).inv().data.cpu().numpy().copy()))
        assert slam.stats["device_frames"] == 0
        _cache["B"] = (rows, _final_state(slam))
        _drop(slam)
    return _cache["B"]


@torch.no_grad()
def _resident_run(publish):
    """device resident, frames pipelined (inputs_ready = True); publish: with a pose stream and a poll per call"""
    key = "A" if publish else "C"
    if key not in _cache:
        slam = _tracker()
        if publish:
            slam.pose_stream()
        resident, polled = 0, []
        for t, (im, ev, K, mask) in enumerate(_frames()):
            slam(_tstamp(t), input_tensor=(ev, im, mask), intrinsics=K)
            resident += slam._dev is not None and slam._dev.active
            if publish:
                r = slam.latest_pose()
                polled.append(-1 if r is None else r.frame)
        info = dict(resident=resident, settles=slam.stats["settles"], polled=polled, peek=slam.peek())
        if publish:
            torch.cuda.synchronize()
            info["records"], info["lost"] = slam.poses_since(-1)
            info["latest"] = slam.latest_pose()
            info["settles_after_reads"] = slam.stats["settles"]
            info["still_resident"] = slam._dev is not None and slam._dev.active
        _cache[key] = (info, _final_state(slam))
        _drop(slam)
    return _cache[key]


def test_published_poses_equal_the_host_driven_trackers_bit_for_bit():
    """tracker A (device resident, pipelined, pose_stream(), latest_pose() after every call) against tracker B (host driven,
    poses_[n - 1] and SE3.inv() read back after every call): frame tags, time stamps, poses and inverse poses of every
    frame, np.array_equal; A was never handed back while it published and polled, and its terminate() equals B's"""
    rows, final_b = _host_driven_reference()
    info, final_a = _resident_run(True)
    assert info["resident"] > 20, info["resident"]
    assert info["settles"] == 0 and info["settles_after_reads"] == 0 and info["still_resident"]
    assert info["peek"]["resident"]
    recs = info["records"]
    assert info["lost"] == 0 and len(recs) == len(rows) == T_FRAMES
    assert [r.frame for r in recs] == [b[0] for b in rows]
    assert np.array_equal(np.array([r.tstamp for r in recs]), np.array([b[1] for b in rows]))
    assert np.array_equal(np.stack([r.pose for r in recs]), np.stack([b[2] for b in rows]))
    assert np.array_equal(np.stack([r.pose_inv for r in recs]), np.stack([b[3] for b in rows]))
    assert info["latest"].frame == T_FRAMES - 1
    # the polls never waited: whatever had arrived, in order, never ahead of the call
    assert all(a <= b for a, b in zip(info["polled"], info["polled"][1:]))
    assert all(p <= t for t, p in enumerate(info["polled"]))
    # the records' bookkeeping against the final state: every drop names a delta entry, n counts the keyframes
    assert all((r.delta is not None) == r.dropped for r in recs)
    assert recs[-1].n - int(recs[-1].dropped) == final_a["n"]
    assert final_a["n"] == final_b["n"]
    assert np.array_equal(final_a["traj"], final_b["traj"]) and np.array_equal(final_a["ts"], final_b["ts"])


def test_publishing_perturbs_nothing():
    """the same stream device resident with and without pose_stream(): n, the graph, poses_, patches_, points_ and
    terminate() agree bit for bit"""
    _, with_stream = _resident_run(True)
    info, without = _resident_run(False)
    assert info["resident"] > 20 and info["settles"] == 0
    assert with_stream["n"] == without["n"]
    for k in ("ii", "jj", "kk", "poses", "patches", "points", "traj", "ts"):
        assert np.array_equal(with_stream[k], without[k]), k


def _chain_depths(log):
    """log: {t1: t0}; depth of every entry's chain down to a frame that has no entry (a keyframe)"""
    def depth(t):
        return 0 if t not in log else 1 + depth(log[t])
    return {t: depth(t) for t in log}


@torch.no_grad()
def test_trajectory_equals_terminate_without_a_hand_back():
    """Ramp_vo.trajectory() mid-run, device resident (frame 37: no settle, the next frame still resident) and at the end,
    against terminate() -- of a second tracker stopped at the same frame, and of the tracker itself -- bit for bit; one
    forced settle() at frame 40 in between, so that the end's entries come from the host's _delta (the first residency's
    log among them) AND the second residency's device log.  The conditions the case needs are asserted from the logs: at
    the mid-run call a keyframe was dropped while resident (an entry in the DEVICE log), and a frame's t0 is itself a dropped
    frame (a chain of depth >= 2).

    Stream: SyntheticStream(240, 320, 46, seed=77), default speed, the `wide` weights with d_gain = 14.5 instead of 20.
    keyframe() chains a dropped keyframe to the keyframe before it, which no later test looks at again, so in steady state
    every chain has depth 1 (the CPU twin, oracle/host_cpu.py, over 24 seeds of the default weights: none deeper).  Deeper
    chains come from the initialisation, which chains a frame its motion probe rejects to the frame before it, kept or
    not: with d_gain = 14.5 the probe's median sits at its threshold and the twin rejects frames 1 .. 6 in a row (chain depth
    6) and 8, 9, 10 (depth 3), initialises at frame 16, has its window full at frame 19 and drops 15 keyframes behind that
    (21 -> 20, 23 -> 22, 24 -> 22, ... 41 -> 38), 25 entries in all over the 46 frames."""
    from rampvo_amd import track_dev
    MID, SETTLE = 37, 40
    frames = kit.frames(240, 320, 46, 77, 46)
    slam = kit.tracker()
    mid = None
    for t, (im, ev, K, mask) in enumerate(frames):
        slam(_tstamp(t), input_tensor=(ev, im, mask), intrinsics=K)
        if t == MID:
            assert slam._dev is not None and slam._dev.active and slam.stats["settles"] == 0
            poses_t, ts_t = slam.trajectory(as_tensor=True)               # (no synchronisation)
            assert poses_t.is_cuda and poses_t.shape == (MID + 1, 7)
            poses_m, ts_m = slam.trajectory()
            assert np.array_equal(poses_t.cpu().numpy(), poses_m)
            dv = slam._dev
            d = dv.dyn.cpu().numpy()
            nlog = int(d[track_dev.DYN_NLOG])
            ints = dv.dlog[:nlog, :2].contiguous().view(torch.int32).cpu().numpy()
            log = {int(k): int(v[0]) for k, v in slam._delta.items()}
            dev_log = {int(a): int(b) for a, b in ints}
            log.update(dev_log)
            mid = dict(poses=poses_m, ts=ts_m, dev_entries=len(dev_log), depths=_chain_depths(log))
            assert slam.stats["settles"] == 0 and dv.active and not hasattr(slam, "traj")
        if t == MID + 1:
            assert slam.stats["device_frames"] > 0 and slam._dev.active and slam.stats["settles"] == 0   # still resident
        if t == SETTLE:
            slam.settle()
            assert slam.stats["settles"] == 1
    assert slam._dev.active, "the tracker did not become device resident again behind the forced settle()"
    assert int(slam._dev.dyn.cpu()[track_dev.DYN_NLOG]) >= 0
    end_poses, end_ts = slam.trajectory()
    assert slam.stats["settles"] == 1 and slam._dev.active
    host_entries, dev_entries_end = len(slam._delta), int(slam._dev.dyn.cpu()[track_dev.DYN_NLOG])
    traj, ts = slam.terminate()
    assert np.array_equal(end_poses, traj) and np.array_equal(end_ts, ts)
    host_poses, _ = slam.trajectory()                                     # (host driven now: the same launch)
    assert np.array_equal(host_poses, traj)
    _drop(slam)
    # what terminate() returns at frame MID: a second tracker on the same frames, stopped there
    ref = kit.tracker()
    for t, (im, ev, K, mask) in enumerate(frames[:MID + 1]):
        ref(_tstamp(t), input_tensor=(ev, im, mask), intrinsics=K)
    traj_m, ts_m = ref.terminate()
    _drop(ref)
    assert np.array_equal(mid["poses"], traj_m) and np.array_equal(mid["ts"], ts_m)
    print("mid-run: device-log entries %d, chain depths %s; end: host entries %d, device-log entries %d"
          % (mid["dev_entries"], sorted(set(mid["depths"].values())), host_entries, dev_entries_end))
    assert host_entries > 0
    assert mid["dev_entries"] >= 1, "no keyframe was dropped while resident"
    assert max(mid["depths"].values()) >= 2, "no delta chain of depth >= 2 (a frame whose t0 is itself a dropped frame)"


# ------------------------------------------------------------------------------------------ the resolve kernel alone
def _resolve(kf_poses, kf_ts, extra, dlog, T):
    import ctypes
    from rampvo_amd import _lib, track_dev
    cu = kit.cu

    def pack(entries):
        a = np.zeros((max(len(entries), 1), track_dev.LOG_WORDS), np.float32)
        for r, (t1, t0, dP) in enumerate(entries):
            a[r, :2] = np.array([t1, t0], np.int32).view(np.float32)
            a[r, 2:9] = dP
        return cu(a)
    kp, kt, ex, dl = cu(kf_poses.astype(np.float32)), cu(np.asarray(kf_ts, np.int64)), pack(extra), pack(dlog)
    out = torch.full((T, 7), float("nan"), device="cuda")
    ws = torch.empty(3 * T, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().ramp_trajectory_resolve(_lib.ptr(kp), _lib.ptr(kt), len(kf_ts), None, _lib.ptr(dl), len(dlog),
                                                  _lib.ptr(ex), len(extra), T, _lib.ptr(out), _lib.ptr(ws), _lib.ptr(status),
                                                  _lib.stream()), "ramp_trajectory_resolve")
    return out.cpu().numpy(), int(status.cpu())


def _recursion(kf_poses, kf_ts, entries, T):
    """Ramp_vo.get_pose / terminate() over rampvo_amd.lietorch.SE3 (ramp_se3_mul / ramp_se3_inv launches)"""
    from rampvo_amd import lietorch
    from rampvo_amd.lietorch import SE3
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    traj = {int(t): cu(p) for t, p in zip(kf_ts, kf_poses)}
    delta = {int(t1): (int(t0), SE3(cu(dP))) for t1, t0, dP in entries}

    def get_pose(t):
        if t in traj:
            return SE3(traj[t])
        t0, dP = delta[t]
        return dP * get_pose(t0)
    return lietorch.stack([get_pose(t) for t in range(T)], dim=0).inv().data.cpu().numpy()


def _rand_se3(rng, k):
    q = rng.standard_normal((k, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([rng.standard_normal((k, 3)) * 2.0, q], axis=1).astype(np.float32)


@torch.no_grad()
def test_resolve_kernel_alone():
    """ramp_trajectory_resolve without a tracker: 6 keyframes, 40 frames, a hand-built log with chains of depth 1, 2 and 17
    split across the two log arguments in shuffled order, one frame both a keyframe and a log entry (the keyframe wins, as in
    get_pose) -- against the Python recursion over lietorch.SE3, np.array_equal; T = 1; nlog = 0; a frame with neither a
    keyframe nor an entry sets the status bit, gets the identity and leaves every row that does not chain to it correct"""
    from rampvo_amd import track_dev
    rng = np.random.default_rng(11)
    T = 40
    kf_ts = [0, 5, 11, 29, 34, 39]
    kf_poses = _rand_se3(rng, 6)
    links = {1: 0, 2: 0, 3: 2, 4: 0, 30: 29, 31: 30, 32: 29, 33: 32, 35: 34, 36: 35, 37: 34, 38: 34}
    links.update({t: 5 for t in range(6, 11)})
    links.update({t: t - 1 for t in range(12, 29)})            # 12 -> 11 (a keyframe), 13 -> 12, ... 28 -> 27: depth 17
    depths = _chain_depths({t: t0 for t, t0 in links.items()})
    assert {1, 2, 17} <= set(depths.values()) and depths[28] == 17
    links[11] = 5                                               # a keyframe that also has an entry
    dPs = _rand_se3(rng, len(links))
    entries = [(t1, t0, dPs[i]) for i, (t1, t0) in enumerate(links.items())]
    order = rng.permutation(len(entries))
    entries = [entries[i] for i in order]
    extra, dlog = entries[0::2], entries[1::2]
    want = _recursion(kf_poses, kf_ts, [e for e in entries if e[0] != 11], T)
    got, status = _resolve(kf_poses, kf_ts, extra, dlog, T)
    assert status == 0 and np.array_equal(got, want)
    # nlog = 0: everything in the other argument
    got, status = _resolve(kf_poses, kf_ts, entries, [], T)
    assert status == 0 and np.array_equal(got, want)
    got, status = _resolve(kf_poses, kf_ts, [], entries, T)
    assert status == 0 and np.array_equal(got, want)
    # T = 1
    got, status = _resolve(kf_poses[:1], kf_ts[:1], [], [], 1)
    assert status == 0 and np.array_equal(got, _recursion(kf_poses[:1], kf_ts[:1], [], 1))
    # an inconsistent log: frame 20 has neither (frames 21 .. 28 chain to it), frame 7 points outside the trajectory
    broken = [e for e in entries if e[0] not in (20, 7)] + [(7, 4000, dPs[0])]
    got, status = _resolve(kf_poses, kf_ts, broken[0::2], broken[1::2], T)
    assert status == track_dev.TRAJ_UNRESOLVED
    lost = [7] + list(range(20, 29))
    ok = [t for t in range(T) if t not in lost]
    assert np.array_equal(got[ok], want[ok])
    assert np.array_equal(got[lost], np.tile(np.array([0, 0, 0, 0, 0, 0, 1], np.float32), (len(lost), 1)))


# ------------------------------------------------------------------------------------------ ring wrap, several trackers
@torch.no_grad()
def test_ring_wrap_and_two_trackers_with_a_ring_each():
    """capacity = 4 over 12 device-resident frames: poses_since(-1) returns the last 4 and reports 8 lost, latest_pose()
    carries the last frame's tag.  A second tracker in the same process, fed the same frames under other time stamps,
    publishes to its own ring: neither ring holds a record of the other tracker"""
    frames = _frames()
    a, b = _tracker(ready=False), _tracker(ready=False)
    b.pose_stream(capacity=64)
    first = None
    for t, (im, ev, K, mask) in enumerate(frames):
        a(_tstamp(t), input_tensor=(ev, im, mask), intrinsics=K)
        b(5000.0 + t, input_tensor=(ev, im, mask), intrinsics=K)
        if first is None and a._dev is not None and a._dev.active:
            first = t + 1
            a.pose_stream(capacity=4)                   # frames first .. first + 11 run resident and publish
        if first is not None and t == first + 11:
            break
    assert first is not None and t == first + 11 and a._dev.active and a.stats["settles"] == 0
    torch.cuda.synchronize()
    recs, lost = a.poses_since(-1)
    assert [r.frame for r in recs] == list(range(first + 8, first + 12)) and lost == 8
    assert a.latest_pose().frame == first + 11
    newer, lost_newer = a.poses_since(first + 9)
    assert [r.frame for r in newer] == [first + 10, first + 11] and lost_newer == 0
    assert all(r.tstamp == _tstamp(r.frame) for r in recs)
    recs_b, lost_b = b.poses_since(-1)
    assert lost_b == 0 and [r.frame for r in recs_b] == list(range(first + 12))
    assert all(r.tstamp == 5000.0 + r.frame for r in recs_b)
    assert a._pose_ring.buf.data_ptr() != b._pose_ring.buf.data_ptr()
    # each ring's newest record is its OWN tracker's newest pose (the two trackers draw their initial depths from one
    # generator in turn, so their trajectories differ), read without a hand-back
    for slam, rec in ((a, recs[-1]), (b, recs_b[-1])):
        n = slam.peek()["n"]
        assert np.array_equal(rec.pose, slam.poses_[n - 1].cpu().numpy()) and rec.n - int(rec.dropped) == n
    assert not np.array_equal(recs[-1].pose, recs_b[-1].pose)
    assert a.stats["settles"] == 0 and b.stats["settles"] == 0
    _drop(a)
    _drop(b)
