"""Sequence-level harness around Ramp_vo (reference: evaluate.py:73-95, 185-260, 263-306; ramp/utils.py:633-656).

``run`` / ``run_pose_pred`` make the same calls in the same order as the reference's functions of the same
name, on any iterable of ``(image, events, intrinsics, mask)``.  The reference scores a run with evo
(``main_ape.ape(pose_relation=translation_part, align=True, correct_scale=True)['rmse']``, evaluate.py:295-304)
-- a third-party package that is not in this image; ``ate_rmse`` is that definition written out: Umeyama
Sim(3) alignment of the estimated positions onto the reference positions, then the RMS position error.
``Trajectory`` carries the three attributes of evo's PoseTrajectory3D the writers use.
"""
import os
import os.path as osp
from pathlib import Path

import numpy as np
import torch

from .Ramp_vo import Ramp_vo


class Trajectory:
    """positions_xyz [T,3], orientations_quat_wxyz [T,4], timestamps [T] (evo.core.trajectory.PoseTrajectory3D's
    fields as used by evaluate.py:86-95 and ramp/utils.py:641-645)"""

    def __init__(self, positions_xyz, orientations_quat_wxyz, timestamps):
        self.positions_xyz = np.asarray(positions_xyz, dtype=float)
        self.orientations_quat_wxyz = np.asarray(orientations_quat_wxyz, dtype=float)
        self.timestamps = np.asarray(timestamps, dtype=float)
        assert len(self.positions_xyz) == len(self.orientations_quat_wxyz) == len(self.timestamps)

    @classmethod
    def from_terminate(cls, poses, tstamps):
        """poses [T,7] = (tx ty tz qx qy qz qw) as returned by Ramp_vo.terminate() (evaluate.py:276-281 reorders
        the quaternion the same way)"""
        poses = np.asarray(poses, dtype=float)
        return cls(poses[:, :3], poses[:, [6, 3, 4, 5]], tstamps)

    @property
    def num_poses(self):
        return len(self.timestamps)


KALIBR_MODELS = {"none": "pinhole", "pinhole": "pinhole", "radtan": "radtan", "plumb_bob": "radtan", "equidistant": "equidistant"}


def camera_from_kalibr(data, cam="cam0", resize_to=None):
    """The camera of a Kalibr cam-chain, from the PARSED file (``yaml.safe_load``'s dict; this function imports no yaml): the
    reference reads ``intrinsics`` and ``resolution`` from it (evaluate.py:44-70) and ignores ``distortion_model`` and
    ``distortion_coeffs``, which ``Ramp_vo.set_camera`` / ``ops.camera`` take.  ``resize_to`` (width, height): the
    principal-point shift of the reference's ``set_global_params`` for an image padded or cropped about its centre,
    ``c += (resize_to - resolution) / 2``.  Returns a dict ``model``, ``raw_intrinsics`` (fx, fy, cx, cy), ``coeffs``,
    ``resolution`` (width, height) -- ``slam.set_camera(**{k: c[k] for k in ("model", "raw_intrinsics", "coeffs")})``.
    Raises ``ValueError`` on a distortion model this package has no kernel for."""
    entry = data[cam]
    name = str(entry.get("distortion_model", "none")).lower()
    if name not in KALIBR_MODELS:
        raise ValueError("camera_from_kalibr: unknown distortion model %r (known: %s)" % (name, ", ".join(sorted(KALIBR_MODELS))))
    if str(entry.get("camera_model", "pinhole")).lower() != "pinhole":
        raise ValueError("camera_from_kalibr: unknown camera model %r (known: pinhole)" % entry["camera_model"])
    fx, fy, cx, cy = (float(v) for v in entry["intrinsics"])
    resolution = tuple(int(v) for v in entry["resolution"])
    model = KALIBR_MODELS[name]
    coeffs = tuple(float(v) for v in entry.get("distortion_coeffs", ())) if model != "pinhole" else ()
    if model == "radtan" and len(coeffs) not in (4, 5) or model == "equidistant" and len(coeffs) != 4:
        raise ValueError("camera_from_kalibr: %s with %d coefficients" % (model, len(coeffs)))
    if resize_to is not None:
        cx += (float(resize_to[0]) - resolution[0]) / 2
        cy += (float(resize_to[1]) - resolution[1]) / 2
    return dict(model=model, raw_intrinsics=(fx, fy, cx, cy), coeffs=coeffs, resolution=resolution)


@torch.no_grad()
def run(cfg_VO, network, eval_cfg, data_list, ht=480, wd=640, device="cuda", inputs_ready="stream", on_pose=None,
        query_times=None):
    """reference evaluate.py:232-260 (without the dataset-specific resize): returns poses, tstamps, points, colors.
    The loop hands the tracker tensors that were produced on the current stream right before the call, as the
    reference's loop does; ``inputs_ready = "stream"`` lets the frames pipeline anyway (Ramp_vo.__init__: the tracker
    orders its front end behind the caller's stream with an event and runs on its own stream; results are identical).
    ``inputs_ready=False``: everything on the caller's stream, frame after frame.
    ``on_pose``: optional callback, called with every frame's pose record (track_dev.PoseRecord) as the loop goes --
    whatever the GPU has finished by then, never waited for (Ramp_vo.pose_stream); the records still in flight when the
    loop ends are delivered behind the closing updates.  None (default): the call sequence is the reference's.
    ``query_times``: optional time stamps, in the unit of the frame time stamps (the loop feeds the frame index); the
    poses there (Ramp_vo.poses_at, behind the closing updates) are returned as a fifth value [Q,7]."""
    train_cfg = eval_cfg["data_loader"]["train"]["args"]
    slam = Ramp_vo(cfg=cfg_VO, network=network, train_cfg=train_cfg, ht=ht, wd=wd, device=device)
    slam.inputs_ready = inputs_ready
    seen = -1
    if on_pose is not None:
        slam.pose_stream()
    for t, (image, events, intrinsics, mask) in enumerate(data_list):
        slam(t, input_tensor=(events, image, mask), intrinsics=intrinsics)
        if on_pose is not None:
            for rec in slam.poses_since(seen)[0]:
                on_pose(rec)
                seen = rec.frame
    for _ in range(12):
        slam.update()
    if on_pose is not None:
        torch.cuda.current_stream().synchronize()
        for rec in slam.poses_since(seen)[0]:
            on_pose(rec)
    points = slam.points_.cpu().numpy()[:slam.m]
    colors = slam.colors_.view(-1, 3).cpu().numpy()[:slam.m]
    at = slam.poses_at(query_times)[0] if query_times is not None else None
    poses, tstamps = slam.terminate()
    if query_times is not None:
        return poses, tstamps, points, colors, at
    return poses, tstamps, points, colors


@torch.no_grad()
def run_pose_pred(cfg_VO, network, eval_cfg, data_list, t_horizon_to_pred, t_to_pred, deg_approx=4, ht=480, wd=640,
                  device="cuda", corrected=False):
    """reference evaluate.py:185-229: track up to frame t_to_pred, then extrapolate virtual keyframes for
    t_horizon_to_pred frames; returns terminate()'s (poses, tstamps).  corrected=False reproduces upstream's pose
    prediction bugs included (Ramp_vo.predict_future_pose's docstring); corrected=True opts out of them"""
    train_cfg = eval_cfg["data_loader"]["train"]["args"]
    slam = Ramp_vo(cfg=cfg_VO, network=network, train_cfg=train_cfg, ht=ht, wd=wd, device=device)
    last_keyframe_number = 0
    for t, (image, events, intrinsics, mask) in enumerate(data_list):
        if t < t_to_pred or t_to_pred < 0:
            slam(t, input_tensor=(events, image, mask), intrinsics=intrinsics)
            last_keyframe_number = slam.n
        if t == t_to_pred and t_to_pred > 0:
            for _ in range(12):
                slam.update()
        if t >= t_to_pred and t_to_pred > 0:
            slam.predict_future_pose(last_keyframe_number=last_keyframe_number, sec_to_pred_future=t - t_to_pred,
                                     abs_time=t, deg=deg_approx, corrected=corrected)
        if t == t_to_pred + t_horizon_to_pred:
            break
    for _ in range(12):
        slam.update()
    return slam.terminate()


# ------------------------------------------------------------------------ metric
def umeyama_sim3(src, dst):
    """least-squares s, R, t with dst ~ s R src + t (Umeyama 1991; evo's align(correct_scale=True))"""
    src, dst = np.asarray(src, float), np.asarray(dst, float)
    mu_s, mu_d = src.mean(0), dst.mean(0)
    xs, xd = src - mu_s, dst - mu_d
    cov = xd.T @ xs / len(src)
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    var_s = (xs ** 2).sum() / len(src)
    s = float(np.trace(np.diag(D) @ S) / var_s) if var_s > 0 else 1.0
    return s, R, mu_d - s * R @ mu_s


def ate_rmse(est_xyz, ref_xyz):
    """ATE as the reference reports it (evaluate.py:295-304): RMS translation error after Sim(3) alignment"""
    est_xyz, ref_xyz = np.asarray(est_xyz, float), np.asarray(ref_xyz, float)
    assert est_xyz.shape == ref_xyz.shape and est_xyz.shape[0] >= 3
    s, R, t = umeyama_sim3(est_xyz, ref_xyz)
    err = (s * (R @ est_xyz.T).T + t) - ref_xyz
    return float(np.sqrt((err ** 2).sum(1).mean()))


# ----------------------------------------------------------------------- writers
def save_results(traj_ref, traj_est, scene, j=0, eval_type="None", root=None):
    """stamped_groundtruth.txt / stamped_traj_estimate.txt: time[s] x y z qw qx qy qz (reference evaluate.py:73-95)"""
    save_dir = osp.join(root or os.getcwd(), "trajectory_evaluation", f"{eval_type}", "trial_" + str(j), scene)
    os.makedirs(save_dir, exist_ok=True)
    for name, tr in (("stamped_groundtruth.txt", traj_ref), ("stamped_traj_estimate.txt", traj_est)):
        time_s = (tr.timestamps * 10 ** -9)[..., np.newaxis]
        np.savetxt(osp.join(save_dir, name), np.concatenate((time_s, tr.positions_xyz, tr.orientations_quat_wxyz), axis=1))
    return save_dir


def resample_trajectory(poses, tstamps, rate_hz, device="cuda"):
    """poses [T,7] at tstamps [T] (seconds; what terminate() / trajectory() return) -> (poses [K,7], times [K]) at the fixed
    rate ``rate_hz``: times tstamps[0] + k / rate_hz up to tstamps[-1], poses on the SE(3) geodesic between the two frames
    around each time (ops.se3_interp).  Raises when tstamps decrease or are not finite."""
    from . import ops
    tstamps = np.asarray(tstamps, dtype=np.float64).reshape(-1)
    poses = np.asarray(poses, dtype=np.float32).reshape(-1, 7)
    assert len(poses) == len(tstamps) >= 1 and rate_hz > 0
    k = int(np.floor((tstamps[-1] - tstamps[0]) * rate_hz * (1.0 + 1e-12))) + 1 if np.isfinite(tstamps[[0, -1]]).all() else 1
    times = tstamps[0] + np.arange(max(k, 1), dtype=np.float64) / float(rate_hz)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out, _, status = ops.se3_interp(cu(poses), cu(tstamps), cu(times))
    if ops.se3_interp_status(status)["bad_times"]:
        raise RuntimeError("resample_trajectory: the time stamps decrease or are not finite")
    return out.cpu().numpy(), times


def metric_trajectory(poses, align, down=(0.0, 0.0, -1.0)):
    """A trajectory in metres with gravity along ``down``: poses [T,7] camera-to-world (tx ty tz qx qy qz qw; what
    trajectory() returns) and ``align``, the dict of ``align_imu`` (or anything with ``scale`` and ``gravity``) ->
    poses [T,7] float64 whose translations are scaled by s and whose world frame is turned by the smallest rotation R that
    takes g / |g| to ``down``: t' = R (s t), q' = q_R q.  Host numpy, a convenience.  Raises when the scale or gravity is not
    finite (a failed alignment is NaN)."""
    to_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
    s, g, d = float(to_np(align["scale"])[0]), to_np(align["gravity"]), to_np(down)
    if not (np.isfinite(s) and s > 0 and np.isfinite(g).all() and np.linalg.norm(g) > 0 and np.linalg.norm(d) > 0):
        raise RuntimeError("metric_trajectory: the alignment holds no finite positive scale and gravity")
    g, d = g / np.linalg.norm(g), d / np.linalg.norm(d)
    axis, c = np.cross(g, d), float(g @ d)
    n = np.linalg.norm(axis)
    half = 0.5 * np.arctan2(n, c)
    if n < 1e-12:                                              # parallel: nothing to turn; opposite: half a turn about any normal
        axis = np.cross(g, np.eye(3)[int(np.argmin(np.abs(g)))])
        n, half = np.linalg.norm(axis), (0.0 if c > 0 else 0.5 * np.pi)
    qr = np.concatenate([np.sin(half) * axis / n, [np.cos(half)]])
    x, y, z, w = qr
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    out = np.empty_like(poses)
    out[:, :3] = (s * poses[:, :3]) @ R.T
    qx, qy, qz, qw = poses[:, 3], poses[:, 4], poses[:, 5], poses[:, 6]
    out[:, 3] = w * qx + x * qw + y * qz - z * qy
    out[:, 4] = w * qy + y * qw + z * qx - x * qz
    out[:, 5] = w * qz + z * qw + x * qy - y * qx
    out[:, 6] = w * qw - x * qx - y * qy - z * qz
    return out


def save_fixed_rate_trajectory(path, poses, tstamps, rate_hz, device="cuda"):
    """the trajectory resampled at ``rate_hz`` (resample_trajectory) as a text file in the row format of save_results:
    time[s] x y z qw qx qy qz"""
    out, times = resample_trajectory(poses, tstamps, rate_hz, device=device)
    Path(path).parent.mkdir(exist_ok=True, parents=True)
    np.savetxt(path, np.concatenate((times[:, None], out[:, :3], out[:, [6, 3, 4, 5]]), axis=1))
    return path


def save_output_for_COLMAP(name, traj, points, colors, fx, fy, cx, cy, H=480, W=640):
    """images.txt / points3D.txt / cameras.txt of a COLMAP text model (reference ramp/utils.py:633-656; x10 scale
    for visualisation, colours given in [0, 1])"""
    colmap_dir = Path(name)
    colmap_dir.mkdir(exist_ok=True, parents=True)
    scale = 10
    images = ""
    for idx, (x, y, z), (qw, qx, qy, qz) in zip(range(1, traj.num_poses + 1), traj.positions_xyz * scale,
                                                 traj.orientations_quat_wxyz):
        images += f"{idx} {qw} {qx} {qy} {qz} {x} {y} {z} 1\n\n"
    (colmap_dir / "images.txt").write_text(images)
    points3D = ""
    colors_uint = (np.asarray(colors) * 255).astype(np.uint8).tolist()
    for i, (p, c) in enumerate(zip((np.asarray(points) * scale).tolist(), colors_uint), start=1):
        points3D += f"{i} " + ' '.join(map(str, p + c)) + " 0.0 0 0 0 0 0 0\n"
    (colmap_dir / "points3D.txt").write_text(points3D)
    (colmap_dir / "cameras.txt").write_text(f"1 PINHOLE {W} {H} {fx} {fy} {cx} {cy}")
    return colmap_dir


def save_map_ply(path, map_dict, scale=1.0):
    """the dict of ``Ramp_vo.map()`` as a binary little-endian PLY point cloud: x y z (float, times ``scale``), red green
    blue (uchar) and ``sigma`` (float): the square root of the trace of the point's covariance, in the units of x y z"""
    cpu = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    xyz = cpu(map_dict["points"]).reshape(-1, 3).astype(np.float64) * scale
    cov = cpu(map_dict["point_cov"]).reshape(-1, 3, 3).astype(np.float64)
    rec = np.zeros(len(xyz), np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3), ("sigma", "<f4")]))
    rec["xyz"], rec["rgb"] = xyz, cpu(map_dict["colors"]).reshape(-1, 3)
    rec["sigma"] = scale * np.sqrt(np.trace(cov, axis1=1, axis2=2))
    Path(path).parent.mkdir(exist_ok=True, parents=True)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float sigma\nend_header\n" % len(rec))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(rec.tobytes())
    return path


def save_points_ply(path, points, scalar=None, name="scalar"):
    """points [K, 3] (``Ramp_vo.event_map_points()["points"]``, ``ops.PointMap.export``) as a binary little-endian PLY point
    cloud: x y z (float) and, with ``scalar`` [K] (a confidence, a count), one more float property called ``name``"""
    cpu = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    xyz = cpu(points).reshape(-1, 3)
    fields = [("xyz", "<f4", 3)] + ([] if scalar is None else [("s", "<f4")])
    rec = np.zeros(len(xyz), np.dtype(fields))
    rec["xyz"] = xyz
    if scalar is not None:
        s = cpu(scalar).reshape(-1)
        if len(s) != len(xyz):
            raise RuntimeError("save_points_ply: scalar holds one number per point")
        rec["s"] = s
    Path(path).parent.mkdir(exist_ok=True, parents=True)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(rec)
            + ("" if scalar is None else "property float %s\n" % name) + "end_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(rec.tobytes())
    return path
