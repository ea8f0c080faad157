"""What the tracker tests share: uploads and bit-for-bit comparison, the small synthetic tracker and its frames, and the
device-resident run around one block of queries.

The small tracker: 240 x 320, 48 patches per frame, SyntheticStream(240, 320, 46, seed=77) of which 44 frames are fed, the
`wide` weights with d_gain = 14.5 (keyframes are dropped while it is device resident from frame 21 on), fp16 features, time
stamps 100.0 + 0.5 f.  The covariance tests use 192 x 256 with 16 patches per frame and the default weights."""
import contextlib
import gc

import numpy as np
import torch

import georef

SMALL_STREAM = (240, 320, 46, 77, 44)               # h, w, the stream's length, its seed, the frames that are fed
SMALL_TRACKER = dict(patches=48, size=(240, 320), d_gain=14.5)
COV_STREAM = (192, 256, 30, 11, 30)
COV_TRACKER = dict(patches=16, size=(192, 256), d_gain=None)
T_FRAMES, T_QUERY = 44, 41                          # frames 0 .. 41 are tracked before the queries, 42 and 43 behind them
RADIUS = 24.0
_frames, _controls = {}, {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(v):
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy()
    if isinstance(v, dict):
        return {k: host(x) for k, x in v.items()}
    return v


def same(a, b, path):
    """bit for bit: float arrays and numbers as words, integer arrays and everything else by value"""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            same(a[k], b[k], path + "." + k)
    elif isinstance(a, np.ndarray) and a.dtype.kind == "f":
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and georef.same_bits(a, b), path
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), path
    elif isinstance(a, float):
        assert georef.same_bits(np.float64(a), np.float64(b)), path
    else:
        assert type(a) is type(b) and a == b, path


def frames(h=240, w=320, length=46, seed=77, count=44):
    """the first ``count`` frames of a stream, made once per session (the canvas depends on the stream's length)"""
    key = (h, w, length, seed, count)
    if key not in _frames:
        from rampvo_amd.synthetic import SyntheticStream
        stream = SyntheticStream(h, w, length, seed=seed, device="cuda")
        _frames[key] = [stream.frame(t) for t in range(count)]
        torch.cuda.synchronize()
    return _frames[key]


def tracker(device_steps=True, ready=True, patches=48, size=(240, 320), d_gain=14.5):
    from rampvo_amd.config import make_cfg
    from rampvo_amd.Ramp_vo import Ramp_vo
    from rampvo_amd.synthetic import make_network
    torch.manual_seed(5)
    slam = Ramp_vo(make_cfg("default", PATCHES_PER_FRAME=patches, MIXED_PRECISION=True),
                   make_network("SingleScale", **({} if d_gain is None else {"d_gain": d_gain})),
                   {"event_bias": True}, ht=size[0], wd=size[1])
    slam.device_steps, slam.inputs_ready = device_steps, ready
    return slam


def tstamp(f):
    return 100.0 + 0.5 * f              # (the caller's time stamps: not the frame counter)


def quiesce():
    """(several trackers in one test: each is dropped -- with its hipGraphs -- at a quiescent point, test_pipeline_gpu.py)"""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def drop(slam):
    del slam
    quiesce()


def feed(slam, f, frame):
    """one frame; inputs_ready = "stream": its tensors are produced on the current stream right before the call and
    overwritten right behind it (test_pipeline_gpu.py), two intrinsics of three as device tensors"""
    im, ev, K, mask = frame
    if slam.inputs_ready != "stream":
        slam(tstamp(f), input_tensor=(ev, im, mask), intrinsics=K)
        return
    ev2, im2 = ev * 1.0, im * 1.0
    K2 = K.cuda() * 1.0 if f % 3 else K
    slam(tstamp(f), input_tensor=(ev2, im2, mask), intrinsics=K2)
    ev2.fill_(float("nan"))
    im2.fill_(float("nan"))
    if K2.is_cuda:
        K2.fill_(float("nan"))


def resident(slam):
    return bool(slam._dev is not None and slam._dev.active and slam.stats["settles"] == 0)


def query_events(f, n=5000):
    """(x, y, t, p) on the device: sub-pixel coordinates over the 240 x 320 image, time stamps behind the two newest frames"""
    rng = np.random.default_rng(21)
    return (cu(rng.uniform(0, 319, n).astype(np.float32)), cu(rng.uniform(0, 239, n).astype(np.float32)),
            cu(rng.uniform(tstamp(f - 2), tstamp(f), n)), cu(rng.choice([-1, 1], n).astype(np.int8)))


def imu_samples(f):
    """(tau, gyro, accel) at 200 Hz from one second ahead of the first frame to one second behind frame ``f``"""
    rng = np.random.default_rng(41)
    tau = 99.0 + np.arange(int((0.5 * f + 2.0) * 200)) / 200.0 + 0.00123
    return tau, (0.2 * rng.normal(size=(len(tau), 3))).astype(np.float32), (rng.normal(size=(len(tau), 3)) + [0, 0, 9.8]).astype(np.float32)


@torch.no_grad()
def run_resident(ready, ask):
    """the small tracker, device resident, over its 44 frames; ``ask(slam, f, frame)`` behind frame T_QUERY returns what goes
    into the result, ``None`` never asks (the control: one run per ``ready`` and session, shared and not to be changed).
    ``ready == "stream"``: the whole run on a side stream"""
    if ask is None and ready in _controls:
        return _controls[ready]
    slam = tracker(True, ready)
    side = torch.cuda.Stream() if ready == "stream" else None
    res = {}
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        for f, frame in enumerate(frames()):
            feed(slam, f, frame)
            if f == T_QUERY and ask is not None:
                res["resident_before"] = resident(slam)
                res.update(ask(slam, f, frame))
                res["resident_after"] = resident(slam)
            if f > T_QUERY:                                        # the state after frames 42 and 43
                n = slam.peek()["n"]
                res["state", f] = dict(n=n, poses=slam.poses_[:n].cpu().numpy(), patches=slam.patches_[:n].cpu().numpy())
        res["resident_at_end"] = resident(slam)
    del slam
    quiesce()
    if ask is None:
        _controls[ready] = res
    return res
