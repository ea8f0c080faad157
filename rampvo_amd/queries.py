"""What a caller may ask a tracker between two frames (``Ramp_vo`` inherits ``TrackerQueries``): live poses, the trajectory
at the frames' and at any time stamps, denoised, compensated and rectified events, rectified frames, the inverse-depth map, the window's uncertainty and the map.  The
tracker keeps the state (``_traj_extra``, ``_traj_times``, ``_traj_status``, ``_pose_ring``).  ``StateStream`` is the one place
that knows on which stream the state is read and how results cross, ``_check_status`` the one that reads status words."""
import contextlib

import numpy as np
import torch

from . import _lib, ops, track_dev


class StateStream:
    """``with tracker._state_stream(inputs) as sc:`` -- the body runs under ``torch.no_grad()`` on the stream the tracker's
    state lives on: the tracker's own while work of an ``inputs_ready = "stream"`` frame is queued there, else the caller's.
    ``sc.resident`` / ``sc.dv``: whether the steady state is device resident, and its DeviceTrack.  ``inputs``: tensors made on
    the caller's stream that the body reads -- the state stream is ordered behind the caller's first.  The body names what it
    hands out with ``sc.leaves(...)``; on exit the caller's stream waits for the state stream once and every tensor named is
    recorded on it.  Where the two streams are one, entry and exit order nothing."""

    def __init__(self, tracker, inputs=()):
        self.dv, self._own, self._cur = tracker._dev, tracker._main_used, torch.cuda.current_stream(tracker.device)
        self.resident = self.dv is not None and self.dv.active
        self._st = tracker._main_stream if self._own else self._cur
        self._inputs, self._leaving, self._ctx = inputs, [], contextlib.ExitStack()

    def __enter__(self):
        self._ctx.enter_context(torch.no_grad())
        if self._own and self._inputs:
            self._order(self._st, self._cur, self._inputs)
        self._ctx.enter_context(torch.cuda.stream(self._st))
        return self

    def __exit__(self, exc_type, exc, tb):
        self._ctx.close()
        if self._own and exc_type is None:
            self._order(self._cur, self._st, self._leaving)

    @staticmethod
    def _order(behind, ahead, tensors):
        """stream ``behind`` waits for what ``ahead`` holds now; ``tensors``, allocated on ``ahead``, are used on ``behind``"""
        ev = torch.cuda.Event()
        ev.record(ahead)
        behind.wait_event(ev)
        for x in tensors:
            x.record_stream(behind)

    def leaves(self, *things):
        """tensors, tuples of tensors or dicts of them that cross to the caller's stream; anything else is ignored"""
        for x in things if self._own else ():
            if isinstance(x, torch.Tensor):
                self._leaving.append(x)
            elif isinstance(x, (dict, tuple, list)):
                self.leaves(*(x.values() if isinstance(x, dict) else x))


def _check_status(name, **roles):
    """The closing check of a query's numpy form -- its one wait.  Each keyword is a role of ``ops.STATUS_ROLES`` (anything else
    is a TypeError) with the device status tensor of that role's entry, or None (not part of this query).  Word 0 of each
    goes to the host in one copy; raises on the first bit set in the order of ``ops.STATUS_ORDER``, with the text the
    table ``ops._STATUS`` holds for it."""
    for k in roles:
        if k not in ops.STATUS_ROLES:
            raise TypeError("_check_status() got an unexpected keyword argument %r" % k)
    given = [(k, s.reshape(-1)[:1]) for k, s in roles.items() if s is not None]
    if not given:
        return
    first = given[0][1] if len(given) == 1 else torch.cat([s for _, s in given])
    _raise_on_words(name, dict(zip((k for k, _ in given), first.cpu().tolist())))          # (the one wait)


def _raise_on_words(name, word):
    """``_check_status`` behind its copy: ``word`` maps roles to word 0 of each, on the host"""
    for role, bit in ops.STATUS_ORDER:
        message = role in word and ops.status_message(role, bit, word[role])
        if message:
            raise RuntimeError(name + ": " + message)


def _se3_log_between(a, b):
    """Log(a^-1 b) of two poses (t, q) on the host, float64 -> (translation 3, rotation 3); NaN where a pose is.  Through the
    relative quaternion: the angle is 2 atan2(|v|, w) (no loss near 0 or pi), with the series of the two coefficients below
    1e-4 rad"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return np.full(6, np.nan)

    def mul(p, q):                                            # Hamilton, xyzw
        return np.array([p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1], p[3] * q[1] - p[0] * q[2] + p[1] * q[3] + p[2] * q[0],
                         p[3] * q[2] + p[0] * q[1] - p[1] * q[0] + p[2] * q[3], p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2]])

    def rot(q, v):
        return mul(mul(q, np.r_[v, 0.0]), q * [-1, -1, -1, 1])[:3]

    qa, qb = a[3:] / np.linalg.norm(a[3:]), b[3:] / np.linalg.norm(b[3:])
    qi = qa * [-1, -1, -1, 1]
    q, t = mul(qi, qb), rot(qi, b[:3] - a[:3])
    if q[3] < 0:
        q = -q                                                # (the shorter way round)
    n = np.linalg.norm(q[:3])
    angle = 2.0 * np.arctan2(n, q[3])
    w = q[:3] * ((2.0 + angle * angle / 12.0) if angle < 1e-4 else angle / n)
    # V^-1 = I - W / 2 + c W^2,  c = (1 - (angle / 2) cot(angle / 2)) / angle^2
    c = (1.0 / 12.0 + angle * angle / 720.0) if angle < 1e-4 else (1.0 - 0.5 * angle * q[3] / n) / (angle * angle)
    wt = np.cross(w, t)
    return np.concatenate([t - 0.5 * wt + c * np.cross(w, wt), w])


def _dof_sigma0(s):
    """(dof, sigma0_sq) of ops.ba_covariance_stats' dict: ``dof = 2 n_valid - 6 N - Mu``, ``sigma0_sq = chi2 / max(dof, 1)``"""
    dof = 2 * s["n_valid"] - 6 * s["N"] - s["Mu"]
    return dof, s["chi2"] / max(dof, 1)


class TrackerQueries:
    """the query surface of ``Ramp_vo`` (a mixin: it reads the tracker's buffers, streams and host mirror as they are)"""

    _NUMPY = {torch.float32: np.float32, torch.float64: np.float64, torch.int8: np.int8, torch.int64: np.int64,
              torch.int32: np.int32}
    _camera = None              # set_camera(): the record's host part on the device, without the rectified intrinsics
    _filter_params = None       # set_event_filter(): the keywords of ops.event_filter
    _filter_state = None        # the filter's last-time-stamp map, carried by filter_events()
    _flow_state = None          # the surface of active events, carried by event_flow()
    _corner_state = None        # the surface of active events, carried by event_corners(): its own, not the flow's
    _track_state = None         # (surface, track state, next id), carried by event_corner_tracks(): its own surface too
    _imu = None                 # set_imu(): the keywords of ops.imu_align that describe the sensor

    def _state_stream(self, inputs=()):
        return StateStream(self, inputs)

    def _as_device(self, a, dtype):
        """tensor -> device tensor of ``dtype``; array-like -> converted on the host, flattened and uploaded"""
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype)
        return self._upload(np.asarray(a, dtype=self._NUMPY[dtype]).reshape(-1))

    # ---------------------------------------------------------------- live poses
    def pose_stream(self, capacity=256):
        """switch pose publishing on: from the next accepted frame on, every frame -- device resident or host driven --
        enqueues ONE extra one-wave launch behind its own work that writes a 128-byte record (frame, time stamp, the newest
        frame's pose and its inverse, sizes, the keyframe test's outcome: track_dev.PoseRecord) into a ring of `capacity`
        records in pinned host memory.  latest_pose() / poses_since() read the ring with plain loads: no hand-back, no
        synchronisation, no HIP call.  A frame rejected by its mask publishes nothing.  Returns the ring."""
        if self._pose_ring is not None:
            if self._pose_ring.capacity == int(capacity):
                return self._pose_ring
            self._pose_rings_retired.append(self._pose_ring)
        with torch.cuda.device(self.device):
            self._pose_ring = track_dev.PoseRing(capacity, first=self.counter)
        return self._pose_ring

    def latest_pose(self):
        """the newest complete record (track_dev.PoseRecord) or None -- never waits: what the GPU has finished, which may
        be a few frames behind the last call"""
        return self._pose_ring.latest() if self._pose_ring is not None else None

    def poses_since(self, frame):
        """(the complete records of frames above `frame`, in order; how many of those were overwritten before this read --
        the ring holds the last `capacity` frames)"""
        return self._pose_ring.since(frame) if self._pose_ring is not None else ([], 0)

    def _publish(self, tstamp, counter, dv=None, n=None, dropped=False, t1=-1, t0=-1):
        """(behind a frame's work) the record of frame `counter`; dv: the frame ran device resident -- everything is read on
        the device; else n = the keyframe count the frame's update() saw (default: the current one)"""
        ring = self._pose_ring
        if dv is not None:
            ring.publish(dv.t, counter, tstamp)
        else:
            ring.publish(None, counter, tstamp, poses=self.poses_, tstamps=self.tstamps_, n_rows=self.N,
                         n=self._n if n is None else n, row=max(self._n - 1, 0), E=len(self._hii),
                         status=self._ba_flags & track_dev.STATUS_BA, dropped=dropped, t1=t1, t0=t0)

    def trajectory(self, as_tensor=False):
        """what terminate() would return now -- (inverse poses [T,7], tstamps) -- as ONE launch (csrc/publish.hip::
        traj_resolve_kernel) over the keyframe rows and the delta log where they are: a device-resident state stays device
        resident (no settle(), the next frame is still one C call), a host-driven one works the same.  as_tensor=True:
        the poses as a device tensor, ordered on the current stream, nothing synchronised (its status word, bit 1 = a
        frame that neither is a keyframe nor has a delta entry, is left in ``_traj_status`` unread); otherwise numpy, which
        waits for that one launch.  Does not set ``traj``."""
        T, dev = int(self.counter), self.device
        tst = np.array(self.tlist, dtype=float)
        with self._state_stream() as sc:
            dv, resident = sc.dv, sc.resident
            key, extra = self._traj_extra
            ne = len(self._delta)
            if key != (id(self._delta), ne):
                head = np.zeros((max(ne, 1), track_dev.LOG_WORDS), np.int32)
                head[:ne, 0] = list(self._delta.keys())
                head[:ne, 1] = [v[0] for v in self._delta.values()]
                extra = self._upload(head).view(torch.float32)
                if ne:
                    extra[:ne, 2:9] = torch.stack([v[1].data.reshape(7) for v in self._delta.values()]).to(torch.float32)
                self._traj_extra = ((id(self._delta), ne), extra)
            out = torch.empty((T, 7), dtype=torch.float32, device=dev)
            ws = torch.empty(3 * max(T, 1), dtype=torch.int32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().ramp_trajectory_resolve(
                _lib.ptr(self.poses_), _lib.ptr(self.tstamps_), self.N if resident else self._n,
                _lib.ptr(dv.dyn) if resident else None, _lib.ptr(dv.dlog) if resident else None,
                dv.log_cap if resident else 0, _lib.ptr(extra), ne, T, _lib.ptr(out), _lib.ptr(ws), _lib.ptr(status),
                _lib.stream()), "ramp_trajectory_resolve")
            sc.leaves(out, ws, status, extra)
        self._traj_status = status
        if as_tensor:
            return out, tst
        poses = out.cpu().numpy()
        _check_status("trajectory()", traj=status)
        return poses, tst

    def _frame_times_dev(self):
        """the frames' time stamps on the device (float64), uploaded once per new frame count"""
        key, tdev = self._traj_times
        now = (id(self.tlist), len(self.tlist), self.tlist[-1] if self.tlist else None)
        if key != now:
            tdev = self._upload(np.asarray(self.tlist, dtype=np.float64).reshape(-1))
            self._traj_times = (now, tdev)
        return tdev

    def poses_at(self, times, extrapolate=False, twist=False, as_tensor=False):
        """The trajectory at ANY time stamps: ``trajectory(as_tensor=True)`` and, behind it on the same stream, the SE(3)
        geodesic between the frames' poses (ops.se3_interp: ``X(t) = Exp(alpha Log(X[s+1] X[s]^-1)) X[s]`` on the segment
        [tlist[s], tlist[s+1]] that holds t) -- one pose per event, per IMU sample, per row of a fixed-rate file.  Same
        convention as ``trajectory()``: inverse poses (interpolating the inverses gives the inverse of the interpolated
        pose).  ``times``: array or tensor, in the unit of the time stamps the frames were fed with; outside their range
        the end pose is held, or with ``extrapolate`` the end segment's motion is continued.  ``twist=True`` adds the
        segment's constant left twist [Q,6] per query.

        A device-resident state stays device resident (no settle(), the next frame is still one C call); the frames' time
        stamps are uploaded once per new frame count.  ``as_tensor=True``: device tensors ``(poses [Q,7], twist or None,
        status int32 [4])``, ordered on the current stream, nothing synchronised (status: ops.se3_interp; trajectory()'s own
        word stays in ``_traj_status``).  Otherwise numpy ``(poses, twist or None)``, which waits for that one result and
        raises when the frames' time stamps decrease or are not finite, or on trajectory()'s unresolved bit."""
        knots, _ = self.trajectory(as_tensor=True)
        with torch.no_grad():
            poses, tw, status = ops.se3_interp(knots, self._frame_times_dev(), self._as_device(times, torch.float64),
                                               extrapolate=extrapolate, twist=twist)
        if as_tensor:
            return poses, tw, status
        _check_status("poses_at()", traj=self._traj_status, interp=status)
        return poses.cpu().numpy(), (tw.cpu().numpy() if twist else None)

    # ---------------------------------------------------------------- IMU
    def set_imu(self, R_bc=None, p_bc=None, bias_g=None, bias_a=None):
        """The IMU the samples of ``align_imu`` come from: the camera in the IMU (body) frame -- ``R_bc`` [3,3], ``p_bc`` [3], as
        Kalibr's ``T_cam_imu`` inverted; None: identity, zero -- the gyro bias the alignment starts from and the accelerometer
        bias it uses as it is (None: zero).  All four are HOST values (lists, arrays, CPU tensors; a device tensor is refused, as in
        ``ops.imu_align``).  Nothing is uploaded, nothing synchronised."""
        as_list = lambda k, v: None if v is None else np.asarray(ops._host_value("set_imu(): " + k, v), np.float64).tolist()
        self._imu = dict(R_bc=as_list("R_bc", R_bc), p_bc=as_list("p_bc", p_bc), bias_g=as_list("bias_g", bias_g),
                         bias_a=as_list("bias_a", bias_a))

    def _imu_inputs(self, name, tau, gyro, accel):
        """The prologue of the IMU queries -> (td, gd, ad, knots, tdev): the samples on the device (``tau`` float64; ``gyro``,
        ``accel`` [N,3], float64 input stays float64), the trajectory as it is now and the cached time stamps.  Raises without a
        sensor and below two frames."""
        if self._imu is None:
            raise RuntimeError(name + ": no IMU has been set (set_imu())")
        if len(self.tlist) < 2:
            raise RuntimeError(name + ": fewer than two frames have been tracked")
        fl = lambda v: torch.float64 if (v.dtype == torch.float64 if isinstance(v, torch.Tensor) else np.asarray(v).dtype == np.float64) else torch.float32
        td = self._as_device(tau, torch.float64)
        gd, ad = self._as_device(gyro, fl(gyro)).reshape(-1, 3), self._as_device(accel, fl(accel)).reshape(-1, 3)
        knots, _ = self.trajectory(as_tensor=True)
        return td, gd, ad, knots, self._frame_times_dev()

    def align_imu(self, tau, gyro, accel, stride=1, gravity_norm=9.80665, max_gap=float("inf"), gyro_steps=1,
                  want_preint=False, as_tensor=False):
        """Metric scale, gravity direction and gyro bias of the trajectory as it is now, from raw IMU samples (``ops.imu_align``
        over ``trajectory(as_tensor=True)`` and the cached time stamps, with the sensor of ``set_imu``; raises without one):
        ``tau`` [N] in the unit of the frames' time stamps, ``gyro``, ``accel`` [N,3] in the IMU frame (arrays or tensors;
        float64 input stays float64).  ``stride``: every stride-th frame is a knot.  ``gravity_norm``: the known norm, or None
        to leave it free.  ``evaluate.metric_trajectory`` applies the result to a trajectory.

        A device-resident state stays device resident (no settle(), the next frame is still one C call).  ``as_tensor=True``:
        the dict of device tensors of ``ops.imu_align``, ordered on the current stream, nothing synchronised, nothing raised.
        Otherwise numpy arrays (``scale`` a float), which reads once at the end and raises on the status bits: the order of
        the time stamps, a failed gyro step, a failed scale solve, and trajectory()'s unresolved bit."""
        td, gd, ad, knots, tdev = self._imu_inputs("align_imu()", tau, gyro, accel)
        with torch.no_grad():                                  # (on the caller's stream, behind trajectory()'s launch: as poses_at)
            out = ops.imu_align(td, gd, ad, knots, tdev, stride=stride, max_gap=max_gap, gravity_norm=gravity_norm,
                                gyro_steps=gyro_steps, want_preint=want_preint, **self._imu)
        res = self._answer("align_imu()", out, {}, as_tensor, traj=self._traj_status, imu=out["status"])
        if not as_tensor:
            res["scale"] = float(res["scale"][0])
        return res

    def propagate_imu(self, tau, gyro, accel, align=None, stride=1, gravity_norm=9.80665, max_gap=float("inf"),
                      horizon=float("inf"), gyro_steps=1, want_state=False, as_tensor=False):
        """Poses at the IMU's rate ahead of the newest frame: the alignment (``align=None``: ``ops.imu_align`` exactly as
        ``align_imu`` runs it; else the device dict of ``align_imu(as_tensor=True)``, reused; raises when its knot count is not
        the current one), the anchor on the last knot used (``ops.imu_anchor``) and the propagation through every sample behind
        it (``ops.imu_propagate``), all on one stream with the sensor of ``set_imu`` (raises without one).  ``horizon``: rows
        further than this many seconds from the anchor are NaN.  The result holds ``poses`` [N,7] camera-to-world rows in the
        tracker's unit, ``times`` [N], ``status``, ``state`` on request, and ``align``.  ``poses, times`` are knots and time
        stamps for ``ops.se3_interp`` / ``ops.event_warp``: appended behind ``trajectory(as_tensor=True)`` and the frames' time
        stamps from the first row with a time above the newest frame's, they warp the events newer than that frame.

        A device-resident state stays device resident.  ``as_tensor=True``: device tensors, ordered on the current stream,
        nothing synchronised, nothing raised.  Otherwise numpy arrays, which reads once at the end and raises on the status
        bits of the alignment and of the propagation, and on trajectory()'s unresolved bit."""
        td, gd, ad, knots, tdev = self._imu_inputs("propagate_imu()", tau, gyro, accel)
        K = (len(self.tlist) - 1) // max(int(stride), 1) + 1
        if align is not None and (not isinstance(align.get("velocity"), torch.Tensor) or align["velocity"].shape[0] != K):
            raise RuntimeError("propagate_imu(): align= is the device dict of align_imu(as_tensor=True) at this stride and "
                               "frame count (%d knots)" % K)
        with torch.no_grad():                                  # (on the caller's stream, behind trajectory()'s launch: as align_imu)
            if align is None:
                align = ops.imu_align(td, gd, ad, knots, tdev, stride=stride, max_gap=max_gap, gravity_norm=gravity_norm,
                                      gyro_steps=gyro_steps, **self._imu)
            anchor = ops.imu_anchor(align, knots, tdev, stride=stride)
            out = ops.imu_propagate(td, gd, ad, anchor, R_bc=self._imu["R_bc"], p_bc=self._imu["p_bc"],
                                    bias_a=self._imu["bias_a"], max_gap=max_gap, horizon=horizon, want_state=want_state)
        res = self._answer("propagate_imu()", out, {}, as_tensor, traj=self._traj_status, imu=align["status"],
                           propagate=out["status"])
        res["align"] = align if as_tensor else {k: v.cpu().numpy() for k, v in align.items()}
        return res

    # ---------------------------------------------------------------- event denoising
    _FILTER_KEYS = ("support_dt", "refractory", "hot_count", "hot_sigma", "hot_mask")

    def set_event_filter(self, **params):
        """The parameters of the event filter (``ops.event_filter``: ``support_dt``, ``refractory``, ``hot_count``,
        ``hot_sigma``, ``hot_mask``) and a fresh state -- no event seen yet -- at the tracker's image size.  ``filter_events``
        and ``denoise=True`` of the event queries filter with them.  Nothing is synchronised."""
        unknown = sorted(set(params) - set(self._FILTER_KEYS))
        if unknown:
            raise RuntimeError("set_event_filter(): unknown parameter %s (known: %s)" % (unknown[0], ", ".join(self._FILTER_KEYS)))
        if params.get("hot_mask") is not None:
            m = params["hot_mask"]
            m = m.to(self.device) if isinstance(m, torch.Tensor) else self._upload(np.asarray(m))
            params["hot_mask"] = (m != 0).to(torch.uint8).reshape(self.ht, self.wd)
        self._filter_params = params
        self.reset_event_filter()

    def reset_event_filter(self):
        """forget the events ``filter_events`` has seen: the next call starts from the empty state (the parameters stay)"""
        self._filter_state = None

    def _filter(self, name, x, y, t, height=None, width=None):
        """ops.event_filter with the stored parameters and state, on the stream the tracker's state lives on"""
        if self._filter_params is None:
            raise RuntimeError(name + ": no event filter has been set (set_event_filter())")
        H, W = self.ht if height is None else int(height), self.wd if width is None else int(width)
        xd, yd, td = self._raw_pixels(x), self._raw_pixels(y), self._as_device(t, torch.float64)
        state = self._filter_state
        if state is not None and tuple(state.shape) != (H, W):
            raise RuntimeError(name + ": the filter's state is %d x %d, the call asks for %d x %d (reset_event_filter())"
                               % (state.shape[0], state.shape[1], H, W))
        with self._state_stream(inputs=tuple(v for v in (xd, yd, td, state, self._filter_params.get("hot_mask")) if v is not None)) as sc:
            out = ops.event_filter(xd, yd, td, H, W, last_t=state, want_xy=True, want_index=True, **self._filter_params)
            sc.leaves(out)
        return out

    def filter_events(self, x, y, t, as_tensor=False, height=None, width=None):
        """Denoise the next stretch of the sensor's event stream (``ops.event_filter`` with the parameters of
        ``set_event_filter``; raises without them): hot pixels, refractory period, 8-neighbour background activity.  The
        filter's state -- every pixel's last time stamp -- is CARRIED from call to call, so feeding a stream in pieces gives
        the events of feeding it whole (the hot-pixel statistics are those of each call's own events).  ``x, y``: integer
        input takes the int32 path; ``height, width`` default to the tracker's.  ``xy`` [N,2] is what the event queries take as
        ``x=xy[:, 0], y=xy[:, 1]``: a dropped event is a NaN row, which they skip and count.

        A device-resident state stays device resident.  ``as_tensor=True``: the dict of device tensors of
        ``ops.event_filter`` (``keep``, ``xy``, ``index``, ``count``, ``hot``, ``stats``, ``status``, ``last_t``), ordered on
        the current stream, nothing synchronised.  Otherwise numpy arrays, which waits and raises when a pixel's events
        decrease in time or lie before the state (the state is then left as it was)."""
        out = self._filter("filter_events()", x, y, t, height, width)
        res = self._answer("filter_events()", out, {}, as_tensor, filter=out["status"])
        self._filter_state = out["last_t"]                 # (behind a clean check; as_tensor: a bad order leaves NaN, every later call then has no state to hold against)
        return res

    def _denoised(self, name, x, y, t):
        """``denoise=True`` of an event query: (x, y, filter_status) with the filter's xy -- NaN rows for the dropped events --
        in the place of the coordinates given.  The filter reads the state ``filter_events`` carries and leaves it as it is:
        a query changes nothing, and several queries may be asked about the same events."""
        if self._filter_params is None:
            raise RuntimeError(name + ": denoise=True needs the filter's parameters (set_event_filter())")
        out = self._filter(name, x, y, t)
        return out["xy"][:, 0], out["xy"][:, 1], out["status"]

    # ---------------------------------------------------------------- event optical flow
    _FLOW_KEYS = ("radius", "window_dt", "min_points", "refine", "outlier_dt", "max_speed", "want_map", "want_fit")

    def reset_event_flow(self):
        """forget the events ``event_flow`` has seen: the next call starts from the empty surface"""
        self._flow_state = None

    def event_flow(self, x, y, t, p=None, as_tensor=False, denoise=False, carry=True, **params):
        """How the image moves at each event of the next stretch of the sensor's stream, without a trajectory and without a
        depth (``ops.event_flow``; ``params``: its ``radius``, ``window_dt``, ``min_points``, ``refine``, ``outlier_dt``,
        ``max_speed``, ``want_map``, ``want_fit``): the normal flow of a plane fitted to the surface of active events around
        the event, in pixels per unit of ``t``, at the tracker's image size.  ``x, y`` are RAW SENSOR PIXELS -- the fit lives on
        the integer lattice, so it sits where the filter sits, ahead of any rectification; integer input takes the int32
        path.  ``p``: with it each polarity has its own surface.  The surface -- every cell's last time stamp -- is CARRIED
        from call to call, so feeding a stream in pieces gives the flows of feeding it whole (``reset_event_flow`` forgets it;
        ``carry=False``: these events alone, the carried surface neither read nor advanced).  ``denoise=True``: filtered first
        (``set_event_filter``; raises without one; the filter's state is read, not advanced); a dropped event is a NaN row and
        falls in class 2, and the result gains ``filter_status``.

        A device-resident state stays device resident.  ``as_tensor=True``: the dict of device tensors of ``ops.event_flow``,
        ordered on the current stream, nothing synchronised.  Otherwise numpy arrays, which waits and raises when a pixel's
        events decrease in time or lie before the carried surface (which is then left as it was) -- with ``denoise`` the
        denoiser's word is looked at first, the flow's second."""
        return self._surface_query("event_flow", "_flow_state", self._FLOW_KEYS, x, y, t, p, as_tensor, denoise, carry, params)

    def _surface_query(self, entry, attr, keys, x, y, t, p, as_tensor, denoise, carry, params):
        """The body of a query on a carried surface of active events (``event_flow``, ``event_corners``): ``ops.<entry>`` on
        raw sensor pixels at the tracker's image size with the surface held in ``self.<attr>``.  Not ``_event_inputs`` /
        ``_answer``: integer pixels keep the int32 path, and with ``denoise`` two words of the ``filter`` role are looked at,
        the denoiser's first."""
        name = entry + "()"
        unknown = sorted(set(params) - set(keys))
        if unknown:
            raise RuntimeError(name + ": unknown parameter %s (known: %s)" % (unknown[0], ", ".join(keys)))
        td = self._as_device(t, torch.float64)
        pd = None if p is None else self._as_device(p, torch.int8)
        filt = None
        if denoise:
            xd, yd, filt = self._denoised(name, x, y, td)
        else:
            xd, yd = self._raw_pixels(x), self._raw_pixels(y)
        state = getattr(self, attr) if carry else None
        shape = (self.ht, self.wd) if pd is None else (2, self.ht, self.wd)
        if state is not None and tuple(state.shape) != shape:
            raise RuntimeError(name + ": the carried surface is %s, the call asks for %s -- with and without p do not mix "
                               "(reset_%s())" % (" x ".join(map(str, state.shape)), " x ".join(map(str, shape)), entry))
        with self._state_stream(inputs=tuple(v for v in (xd, yd, td, pd, state) if v is not None)) as sc:
            out = getattr(ops, entry)(xd, yd, td, self.ht, self.wd, p=pd, last_t=state, **params)
            sc.leaves(out)
        if filt is not None:
            out["filter_status"] = filt
        if not as_tensor:
            words = [s.reshape(-1)[:1] for s in (filt, out["status"]) if s is not None]
            for word in (words[0] if len(words) == 1 else torch.cat(words)).cpu().tolist():      # (the one wait)
                _raise_on_words(name, {"filter": word})
            res = {k: v.cpu().numpy() for k, v in out.items()}
        else:
            res = out
        if carry:
            setattr(self, attr, out["last_t"])             # (behind a clean check; as_tensor: a bad order leaves NaN)
        return res

    # ---------------------------------------------------------------- event corner detection
    _CORNER_KEYS = ("inner", "outer", "wide", "want_arc", "want_index", "want_map")

    def reset_event_corners(self):
        """forget the events ``event_corners`` has seen: the next call starts from the empty surface"""
        self._corner_state = None

    def event_corners(self, x, y, t, p=None, as_tensor=False, denoise=False, carry=True, **params):
        """Which events of the next stretch of the sensor's stream are corners (``ops.event_corners``; ``params``: its
        ``inner``, ``outer``, ``wide``, ``want_arc``, ``want_index``, ``want_map``): arcs of newest events on two circles of
        the surface of active events around each event, at the tracker's image size.  ``x, y`` are RAW SENSOR PIXELS -- the
        circles live on the integer lattice, so the detector sits where the filter and the flow sit, ahead of any
        rectification; integer input takes the int32 path.  ``p``: with it each polarity has its own surface.  The surface --
        every cell's last time stamp -- is CARRIED from call to call, so feeding a stream in pieces gives the corners of
        feeding it whole (``reset_event_corners`` forgets it; ``carry=False``: these events alone, the carried surface neither
        read nor advanced).  It is this query's own surface, not ``event_flow``'s: each query advances only its own.
        ``denoise=True``: filtered first (``set_event_filter``; raises without one; the filter's state is read, not
        advanced); a dropped event is a NaN row and falls in class 2, and the result gains ``filter_status``.

        A device-resident state stays device resident.  ``as_tensor=True``: the dict of device tensors of
        ``ops.event_corners``, ordered on the current stream, nothing synchronised.  Otherwise numpy arrays, which waits and
        raises when a pixel's events decrease in time or lie before the carried surface (which is then left as it was) -- with
        ``denoise`` the denoiser's word is looked at first, the detector's second."""
        return self._surface_query("event_corners", "_corner_state", self._CORNER_KEYS, x, y, t, p, as_tensor, denoise, carry, params)

    # ---------------------------------------------------------------- event corner tracks
    _TRACK_KEYS = ("radius", "max_dt", "want_parent", "want_birth", "want_velocity")

    def reset_event_corner_tracks(self):
        """forget the events ``event_corner_tracks`` has seen: the next call starts without a surface and without a track"""
        self._track_state = None

    def event_corner_tracks(self, x, y, t, p=None, as_tensor=False, denoise=False, carry=True, **params):
        """Feature tracks over the next stretch of the sensor's stream, without a trajectory and without a depth:
        ``ops.event_corners`` says which events are corners, ``ops.event_corner_tracks`` links them in space and time
        (``params``: the detector's ``inner``, ``outer``, ``wide``, ``want_arc``, ``want_index``, ``want_map`` and the linker's
        ``radius``, ``max_dt`` -- required --, ``want_parent``, ``want_birth``, ``want_velocity``).  ``x, y`` are RAW SENSOR
        PIXELS at the tracker's image size; integer input takes the int32 path.  ``p``: with it each polarity has its own
        surface and its own tracks.  The detector's surface, the track state and the next id are CARRIED from call to call,
        so feeding a stream in pieces gives the tracks and ids of feeding it whole (``reset_event_corner_tracks`` forgets
        them; ``carry=False``: these events alone, nothing read and nothing advanced).  The surface is this query's own, not
        the one ``event_corners`` carries.  ``denoise=True``: filtered first (``set_event_filter``; raises without one; the
        filter's state is read, not advanced); a dropped event is a NaN row and falls in class 2, and the result gains
        ``filter_status``.

        Returns the union of both operators' dicts: the linker's under its own names (``cls``, ``status``, ``track``,
        ``length``, ``state``, ``next_id``, ...), the detector's too (``corner``, ``last_t``, ``index``, ...) except its ``cls``
        and ``status``, which are ``corner_cls`` and ``corner_status``.  A device-resident state stays device resident.
        ``as_tensor=True``: device tensors, ordered on the current stream, nothing synchronised.  Otherwise numpy arrays,
        which waits and raises when a pixel's events decrease in time or lie before what is carried (all of which is then
        left as it was) -- the denoiser's word is looked at first, the detector's second, the linker's third."""
        name = "event_corner_tracks()"
        keys = self._CORNER_KEYS + self._TRACK_KEYS
        unknown = sorted(set(params) - set(keys))
        if unknown:
            raise RuntimeError(name + ": unknown parameter %s (known: %s)" % (unknown[0], ", ".join(keys)))
        td = self._as_device(t, torch.float64)
        pd = None if p is None else self._as_device(p, torch.int8)
        filt = None
        if denoise:
            xd, yd, filt = self._denoised(name, x, y, td)
        else:
            xd, yd = self._raw_pixels(x), self._raw_pixels(y)
        surface, state, next_id = (self._track_state if carry else None) or (None, None, None)
        shape = (self.ht, self.wd) if pd is None else (2, self.ht, self.wd)
        if surface is not None and tuple(surface.shape) != shape:
            raise RuntimeError(name + ": the carried surface is %s, the call asks for %s -- with and without p do not mix "
                               "(reset_event_corner_tracks())" % (" x ".join(map(str, surface.shape)), " x ".join(map(str, shape))))
        with self._state_stream(inputs=tuple(v for v in (xd, yd, td, pd, surface, state, next_id) if v is not None)) as sc:
            det = ops.event_corners(xd, yd, td, self.ht, self.wd, p=pd, last_t=surface,
                                    **{k: v for k, v in params.items() if k in self._CORNER_KEYS})
            trk = ops.event_corner_tracks(xd, yd, td, self.ht, self.wd, corner=det["corner"], p=pd, state=state, next_id=next_id,
                                          **{k: v for k, v in params.items() if k in self._TRACK_KEYS})
            out = {**det, **trk, "corner_cls": det["cls"], "corner_status": det["status"]}
            sc.leaves(out)
        if filt is not None:
            out["filter_status"] = filt
        if not as_tensor:
            words = [s.reshape(-1)[:1] for s in (filt, out["corner_status"], out["status"]) if s is not None]
            for word in torch.cat(words).cpu().tolist():           # (the one wait)
                _raise_on_words(name, {"filter": word})
            res = {k: v.cpu().numpy() for k, v in out.items()}
        else:
            res = out
        if carry:
            self._track_state = (out["last_t"], out["state"], out["next_id"])      # (behind a clean check; as_tensor: a bad order leaves them empty)
        return res

    # ---------------------------------------------------------------- lens distortion
    def set_camera(self, model, raw_intrinsics, coeffs=(), rotation=None):
        """The sensor the raw events and frames come from (``ops.camera``): ``model`` 'pinhole', 'radtan' or 'equidistant',
        its raw intrinsics (fx, fy, cx, cy), distortion coefficients and an optional rotation raw -> rectified camera --
        ``evaluate.camera_from_kalibr`` reads them from a Kalibr cam-chain.  The rectified camera is the pinhole the tracker is
        fed with: row 0 of its own intrinsics times the patch stride, read on the device at every query.  One upload, nothing
        synchronised."""
        self._camera = self._upload(np.asarray(ops.camera_words(model, raw_intrinsics, coeffs, rotation), np.float32))

    def _rectified_camera(self, name):
        """the camera record with the rectified intrinsics ``_event_query`` forms, read on the stream the state lives on"""
        if self._camera is None:
            raise RuntimeError(name + ": no camera has been set (set_camera())")
        if not self.tlist:
            raise RuntimeError(name + ": no frame has been tracked yet")
        with self._state_stream(inputs=(self._camera,)) as sc:
            cam = self._camera.clone()
            cam[_lib.RAMP_CAMERA_NEW:_lib.RAMP_CAMERA_NEW + 4] = self.intrinsics_[0] * float(self.RES)
            sc.leaves(cam)
        return cam

    def _raw_pixels(self, a):
        """event coordinates as the rectifier takes them: integer input stays integer (the int32 path), anything else fp32"""
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.float32 if a.is_floating_point() else torch.int32)
        a = np.asarray(a)
        return self._as_device(a, torch.int32 if a.dtype.kind in "iu" else torch.float32)

    def rectify_events(self, x, y, as_tensor=False):
        """Raw sensor events -> sub-pixel coordinates of the images the tracker is fed (``ops.event_rectify`` with the camera of
        ``set_camera``).  ``xy`` [N,2] is what the event queries take as ``x=xy[:, 0], y=xy[:, 1]``; an event without a
        solution is a NaN row, which they skip and count.  A device-resident state stays device resident.  ``as_tensor=True``:
        the dict of device tensors (``xy``, ``status``, ``valid``), ordered on the current stream, nothing synchronised;
        otherwise numpy arrays, which waits and raises when the camera record is not finite."""
        cam = self._rectified_camera("rectify_events()")
        with torch.no_grad():
            out = ops.event_rectify(self._raw_pixels(x), self._raw_pixels(y), cam, self.ht, self.wd, want_valid=True)
        return self._answer("rectify_events()", out, {}, as_tensor, rectify=out["status"])

    def rectify_image(self, image, normalize="half", as_tensor=False):
        """A raw frame [C,Hs,Ws] or [Hs,Ws] (uint8 or float32; a tensor or an array) resampled into the camera the tracker is
        fed, at its image size, with the reference's normalisation (``ops.image_rectify``; ``normalize`` None, "half" or
        "unit").  Returns a dict ``image``, ``mask`` (1 where the source was sampled), ``status``: device tensors with
        ``as_tensor=True``, ordered on the current stream, nothing synchronised; otherwise numpy arrays, which waits and raises
        when the camera record is not finite."""
        cam = self._rectified_camera("rectify_image()")
        if not isinstance(image, torch.Tensor):
            image = np.asarray(image)
            image = self._upload(image if image.dtype == np.uint8 else image.astype(np.float32))
        with torch.no_grad():
            out = ops.image_rectify(image.to(self.device), cam, self.ht, self.wd, normalize=normalize, want_mask=True)
        out.pop("map")
        return self._answer("rectify_image()", out, {}, as_tensor, rectify=out["status"])

    def _undistorted(self, name, x, y):
        """``distorted=True`` of an event query: (x, y, rectify_status) with the rectified coordinates in the place of the raw"""
        if self._camera is None:
            raise RuntimeError(name + ": distorted=True needs the sensor's camera (set_camera())")
        rect = self.rectify_events(x, y, as_tensor=True)
        return rect["xy"][:, 0], rect["xy"][:, 1], rect["status"]

    def _event_inputs(self, name, x, y, t, p, denoise, distorted):
        """The prologue of an event query -> (x, y, t, p, extra): the events as the kernels take them (fp32, fp32, float64, int8
        on the device; ``p=None``: a query without polarity) and ``extra``, the ``rectify_status`` / ``filter_status`` the result gains.  ``denoise`` filters first, in
        the coordinates given (integer raw pixels stay int32), then ``distorted`` rectifies."""
        td, pd = self._as_device(t, torch.float64), None if p is None else self._as_device(p, torch.int8)
        rect = filt = None
        if denoise:
            x, y, filt = self._denoised(name, x, y, td)
        if distorted:
            x, y, rect = self._undistorted(name, x, y)
        extra = {k: s for k, s in (("rectify_status", rect), ("filter_status", filt)) if s is not None}
        return self._as_device(x, torch.float32), self._as_device(y, torch.float32), td, pd, extra

    @staticmethod
    def _answer(name, out, extra, as_tensor, **roles):
        """The epilogue of a query with a numpy form: ``out`` gains ``extra`` (an event query's ``rectify_status`` /
        ``filter_status``; else empty); ``as_tensor``: the device dict as it is, else the one ``_check_status`` call
        (``roles``: its arguments, beside those two words) and numpy arrays."""
        out.update(extra)
        if as_tensor:
            return out
        _check_status(name, **{"rectify": extra.get("rectify_status"), "filter": extra.get("filter_status"), **roles})
        return {k: v.cpu().numpy() for k, v in out.items()}

    def compensate_events(self, x, y, t, p, t_ref=None, invdepth=None, num_bins=0, extrapolate=False, want_xy=False,
                          want_iwe=True, stack=None, height=None, width=None, as_tensor=False, radius=None,
                          weights="variance", distorted=False, denoise=False):
        """Motion compensation with the trajectory as it is now: every event (``x, y`` pixel coordinates of the images the
        tracker is fed, ``t`` in the unit of the frames' time stamps, ``p`` polarity) is warped from the camera pose at its
        own time stamp to the pose at ``t_ref`` and splat bilinearly into an image of warped events and / or a bin stack
        (``ops.event_warp``, one pass over the events; the poses are those of ``poses_at``: ``trajectory(as_tensor=True)``
        and the cached time stamps, never written per event).

        ``t_ref=None``: the newest frame's time stamp.  ``invdepth=None``: the lower median inverse depth of the last three
        frames' patches -- the value the next frame's patches start from -- computed into a device word the host never
        reads; otherwise a float, a one-element device tensor or a [height, width] map; ``"map"``: the map
        ``invdepth_map(t_ref, radius, weights)`` renders from the window's patches at the reference pose, so that every event is
        warped with the depth the tracker has estimated near its pixel (``radius``, ``weights`` are read in this mode only);
        ``"events"``: the map ``event_depth(x, y, t, t_ref, fill="median")`` sweeps from these very events (at the tracker's
        image size), so that the events are warped with the depth they vote for themselves and with the median elsewhere;
        ``"event_map"``: the map ``event_map_depth(t_ref, fill="median")`` renders from the persistent event map at the
        reference pose (raises before the first ``event_map()``): the depth of every view inserted so far, at the cost of a
        table read instead of a sweep, and the median where the map renders nothing.
        Intrinsics: row 0 of the tracker's own times the patch stride, i.e. those of the images it was fed.  ``height, width``
        default to the tracker's.  ``distorted=True``: ``x, y`` are RAW sensor pixels; they are rectified first
        (``rectify_events``, the camera of ``set_camera``; raises without one), the events without a solution are skipped and
        counted like any NaN row, and the result gains ``rectify_status``.  ``denoise=True``: the events are filtered first
        (``set_event_filter``; raises without one), in the coordinates given and ahead of the rectification; the dropped
        events are NaN rows, skipped and counted, and the result gains ``filter_status``.  The filter's state is read, not
        advanced (``filter_events`` does that).

        A device-resident state stays device resident (no settle(), the next frame is still one C call).  ``as_tensor=True``:
        the dict of device tensors of ``ops.event_warp`` (``status``, ``xy``, ``iwe``, ``stack`` as requested), ordered on
        the current stream, nothing synchronised.  Otherwise numpy arrays, which waits for that result and raises when the
        frames' time stamps decrease or are not finite, or on trajectory()'s unresolved bit."""
        name = "compensate_events()"
        xd, yd, td, pd, extra = self._event_inputs(name, x, y, t, p, denoise, distorted)
        knots, tdev, K, invdepth, t_ref, H, W = self._event_query(name, t_ref, invdepth, radius, weights, height, width,
                                                                  events=(xd, yd, td))
        with torch.no_grad():
            out = ops.event_warp(xd, yd, td, pd, knots, tdev, t_ref, K, invdepth, H, W, num_bins=num_bins,
                                 extrapolate=extrapolate, want_xy=want_xy, want_iwe=want_iwe, stack=stack)
        return self._answer(name, out, extra, as_tensor, traj=self._traj_status, interp=out["status"])

    def _event_query(self, name, t_ref, invdepth, radius, weights, height, width, events=None):
        """what the event queries share: the trajectory as it is now, the cached time stamps, the image intrinsics and the
        inverse depth (None: the median word; ``"map"``: ``invdepth_map`` at the reference pose; ``"events"``: ``event_depth``
        of the query's own ``events`` = (x, y, t) at the reference time, the median where nothing is detected;
        ``"event_map"``: ``event_map_depth`` at the reference pose, the median where the map renders nothing), read on the
        stream the state lives on -> (knots, times, K, invdepth, t_ref, height, width)"""
        if not self.tlist:
            raise RuntimeError(name + ": no frame has been tracked yet")
        if isinstance(invdepth, str):
            if invdepth == "map":
                invdepth = self.invdepth_map(t_ref=t_ref, radius=radius, weights=weights, height=height, width=width,
                                             as_tensor=True)["invdepth"]
            elif invdepth == "events" and events is not None:
                invdepth = self.event_depth(*events, t_ref=t_ref, fill="median", as_tensor=True)["invdepth"]
            elif invdepth == "event_map":
                invdepth = self.event_map_depth(t_ref=t_ref, fill="median", height=height, width=width, as_tensor=True)["invdepth"]
            else:
                raise RuntimeError(name + ": invdepth is None, a number, a tensor, 'map' or 'events', or 'event_map'")
        knots, _ = self.trajectory(as_tensor=True)
        tdev = self._frame_times_dev()
        with self._state_stream() as sc:                      # reads of the state, on the stream it lives on
            K = self.intrinsics_[0] * float(self.RES)
            if invdepth is None:
                invdepth = self._depth_median_word(sc.resident)
            sc.leaves(K, invdepth)
        return (knots, tdev, K, invdepth, self.tlist[-1] if t_ref is None else float(t_ref),
                self.ht if height is None else height, self.wd if width is None else width)

    def event_contrast(self, x, y, t, p, t_ref=None, invdepth=None, correction=None, signed=True, want_grad=True,
                       want_iwe=False, extrapolate=False, height=None, width=None, as_tensor=False, radius=None,
                       weights="variance", distorted=False, denoise=False):
        """How sharp the compensated events are with the trajectory as it is now: the variance of the image of warped events
        ``compensate_events`` would return (the same events, poses, intrinsics and inverse depth -- ``invdepth`` as there,
        ``"map"``, ``"events"`` and ``"event_map"`` included) and its gradient with respect to a small correction ``(v[3], w[3], lam)`` of velocity, rotation
        rate and log depth scale in the reference camera frame (``ops.event_contrast``).  The only figure of quality an
        event tracker can give about its own trajectory without ground truth.  ``distorted=True``: raw sensor pixels, as in
        ``compensate_events``; the result gains ``rectify_status``.  ``denoise=True``: filtered first, as there; the result
        gains ``filter_status``.

        A device-resident state stays device resident (no settle(), the next frame is still one C call).  ``as_tensor=True``:
        the dict of device tensors of ``ops.event_contrast`` (``variance``, ``stats``, ``sums``, ``status``, ``grad``, ``iwe``
        as requested), ordered on the current stream, nothing synchronised.  Otherwise numpy arrays (``variance`` a float),
        which waits for that result and raises when the frames' time stamps decrease or are not finite, or on trajectory()'s
        unresolved bit."""
        name = "event_contrast()"
        xd, yd, td, pd, extra = self._event_inputs(name, x, y, t, p, denoise, distorted)
        knots, tdev, K, invdepth, t_ref, H, W = self._event_query(name, t_ref, invdepth, radius, weights, height, width,
                                                                  events=(xd, yd, td))
        with torch.no_grad():
            out = ops.event_contrast(xd, yd, td, pd, knots, tdev, t_ref, K, invdepth, H, W, correction=correction,
                                     signed=signed, extrapolate=extrapolate, want_grad=want_grad, want_iwe=want_iwe)
        res = self._answer(name, out, extra, as_tensor, traj=self._traj_status, interp=out["status"])
        if not as_tensor:
            res["variance"] = float(res["stats"][0])
        return res

    def align_events(self, x, y, t, p, t_ref=None, invdepth=None, correction=None, free=(0, 0, 0, 1, 1, 1, 0), step=0.05,
                     iters=20, signed=True, extrapolate=False, height=None, width=None, radius=None, weights="variance",
                     distorted=False, denoise=False, resident=False, max_evals=None, as_tensor=False):
        """Refine the compensation by contrast maximisation (``ops.event_align``: normalised gradient ascent with
        backtracking over ``event_contrast``, the components ``free`` marks -- by default the rotation rate).  The
        trajectory, intrinsics and inverse depth (``invdepth`` as in ``compensate_events``, ``"event_map"`` included) are read
        ONCE, as ``event_contrast`` reads them.  A device-resident state
        stays device resident on every path.  ``distorted=True``: raw sensor pixels, rectified once in front of the loop; the
        result gains ``rectify_status``.  ``denoise=True``: filtered once in front of the loop, as in ``compensate_events``;
        the result gains ``filter_status``.

        ``resident=False``: the host loop; every evaluation reads 8 + 7 doubles back, so this form is a convenience between
        two frames, not a hot path.  Returns ``ops.event_align``'s dict: ``correction``, ``variance``, ``variance0``,
        ``history`` (the status words on the host); raises on the conditions ``event_contrast`` raises on.

        ``resident=True``: the loop runs on the device (one C call, ``max_evals`` as in ``ops.event_align``) and ONE read at
        the end gives the same keys plus ``reason`` (``ops.event_align_info``), ``n_evals`` and ``n_accepted``; ``correction``
        a list of 7 floats, ``history`` a list cut at ``n_accepted``.  Raises on the same conditions.  ``as_tensor=True``
        (implies ``resident``): the dict of device tensors of ``ops.event_align(resident=True)``, ordered on the current
        stream; nothing is synchronised and nothing raised, as ``event_contrast(as_tensor=True)``: ``correction_f32`` goes
        straight into ``event_contrast(correction=...)``."""
        resident = resident or as_tensor
        name = "align_events()"
        xd, yd, td, pd, extra = self._event_inputs(name, x, y, t, p, denoise, distorted)
        knots, tdev, K, invdepth, t_ref, H, W = self._event_query(name, t_ref, invdepth, radius, weights, height, width,
                                                                  events=(xd, yd, td))
        with torch.no_grad():
            out = ops.event_align(xd, yd, td, pd, knots, tdev, t_ref, K, invdepth, H, W, correction=correction, free=free,
                                  step=step, iters=iters, signed=signed, extrapolate=extrapolate, resident=resident,
                                  max_evals=max_evals)
        if as_tensor:
            return self._answer(name, out, extra, True)
        rect, filt = extra.get("rectify_status"), extra.get("filter_status")
        if resident:
            # the one read: every word is an int32 or a double, so one float64 row holds them all exactly
            words_of = [(k, s) for k, s in (("traj", self._traj_status), ("rectify", rect), ("filter", filt)) if s is not None]
            with torch.no_grad():
                row = torch.cat([out["correction"], out["result"], out["info"].double(), out["history"]]
                                + [s.reshape(-1).double() for _, s in words_of]).cpu().tolist()
            info, tail = [int(v) for v in row[11:19]], row[19 + int(iters):]
            word, res = {"interp": info[4]}, {}
            for k, s in words_of:
                words, tail = [int(v) for v in tail[:s.numel()]], tail[s.numel():]
                word[k] = words[0]
                if k != "traj":
                    res[k + "_status"] = np.asarray(words, np.int32)
            _raise_on_words("align_events()", word)
            res.update(correction=row[:7], variance=row[7], variance0=row[8], history=row[19:19 + info[1]],
                       reason=ops.ALIGN_REASONS.get(info[0], "unknown"), n_evals=info[2], n_accepted=info[1])
            return res
        _check_status(name, traj=self._traj_status, rectify=rect, filter=filt)
        out.update({k: s.cpu().numpy() for k, s in extra.items()})
        if out["variance0"] != out["variance0"]:              # (NaN: the kernel's answer to bad time stamps)
            raise RuntimeError("align_events(): the frames' time stamps decrease or are not finite")
        return out

    def event_voxel_grid(self, x, y, t, p, num_bins=5, offsets=None, normalize=True, compensate=False, t_ref=None,
                         invdepth=None, as_tensor=False, extrapolate=False, radius=None, weights="variance", distorted=False,
                         denoise=False):
        """The reference's voxel-grid event representation at the tracker's image size (``ops.event_voxel_grid``: every event
        votes into the two time bins next to its normalised time stamp, each slice standardised over its non-zero cells):
        ``grid`` [S, num_bins, ht, wd] for the slices ``offsets`` (a device int64 tensor [S + 1], ``ops.event_slices``) marks,
        or [num_bins, ht, wd] for all events as one slice -- the shape the net takes as ``events[None, None]``.

        ``compensate=True``: a MOTION-COMPENSATED voxel grid.  The events are first warped to the camera pose at ``t_ref``
        with the trajectory as it is now (``compensate_events(want_xy=True, want_iwe=False, as_tensor=True)``; ``t_ref``,
        ``invdepth`` -- ``"event_map"`` included --, ``extrapolate``, ``radius`` and ``weights`` are read in this mode only, as
        there) and their sub-pixel
        coordinates are splat bilinearly; the events the warp rejects are NaN rows, which the grid skips and counts.  The time
        bins are those of the events' own time stamps.

        ``distorted=True``: ``x, y`` are RAW sensor pixels; they are rectified first (``rectify_events``; raises without
        ``set_camera``) and splat bilinearly at their sub-pixel coordinates, compensated or not; the result gains
        ``rectify_status``.

        ``denoise=True``: the events are filtered first (``set_event_filter``; raises without one), in the coordinates given
        and ahead of the rectification; the dropped events are NaN rows, which the grid skips and counts in every mode; the
        result gains ``filter_status``.  The filter's state is read, not advanced.

        A device-resident state stays device resident (no settle(), the next frame is still one C call).  ``as_tensor=True``:
        the dict of device tensors of ``ops.event_voxel_grid`` (``grid``, ``stats``, ``status``; with ``compensate`` also
        ``warp_status``, the words of ``ops.event_warp``), ordered on the current stream, nothing synchronised.  Otherwise
        numpy arrays, which waits for that result and raises on offsets that decrease or leave the event list, on a slice
        whose first or last time stamp is not finite and, with ``compensate``, on the conditions ``compensate_events`` raises
        on."""
        name, warp = "event_voxel_grid()", {}
        xd, yd, td, pd, extra = self._event_inputs(name, x, y, t, p, denoise, distorted)
        if compensate:
            warp = self.compensate_events(xd, yd, td, pd, t_ref=t_ref, invdepth=invdepth, extrapolate=extrapolate, want_xy=True,
                                          want_iwe=False, as_tensor=True, radius=radius, weights=weights)
            xd, yd = warp["xy"][:, 0], warp["xy"][:, 1]
        with torch.no_grad():
            out = ops.event_voxel_grid(xd, yd, td, pd, self.ht, self.wd, num_bins=num_bins,
                                       offsets=None if offsets is None else self._as_device(offsets, torch.int64),
                                       normalize=normalize, subpixel=compensate or distorted)
        if compensate:
            extra = {"warp_status": warp["status"], **extra}
        return self._answer(name, out, extra, as_tensor, traj=self._traj_status if compensate else None,
                            interp=warp.get("status"), voxel=out["status"])

    def event_depth(self, x, y, t, t_ref=None, planes=64, range=None, rel_range=4.0, min_votes=4.0, adaptive_radius=0,
                    adaptive_offset=0.0, fill=None, distorted=False, denoise=False, as_tensor=False):
        """Semi-dense inverse depth from the events themselves (``ops.event_dsi``: a plane sweep of the events' rays through
        ``planes`` planes of inverse depth of the camera at ``t_ref``, with the trajectory as it is now -- event multi-view
        stereo), at the tracker's image size and intrinsics: depth at the pixels where events fire, depth edges included,
        which ``invdepth_map``'s regression of the patches cannot know.  Events, ``t_ref``, ``distorted`` and ``denoise`` as
        ``compensate_events`` (no polarity).

        ``range=None``: ``(median / rel_range, median * rel_range)`` around the median inverse depth ``compensate_events``
        uses by default, formed on the device; else ``(d_lo, d_hi)`` as numbers or a device tensor [2].  ``min_votes``,
        ``adaptive_radius``, ``adaptive_offset``: the detection of ``ops.event_dsi``.  ``fill``: what an undetected pixel
        gets -- None (NaN), a number, a one-element device tensor, or ``"median"`` (that median word).  ``planes``,
        ``rel_range`` and ``min_votes`` are defaults nobody has tuned.

        A device-resident state stays device resident (no settle(), the next frame is still one C call).  ``as_tensor=True``:
        the dict of device tensors of ``ops.event_dsi`` (``dsi``, ``invdepth``, ``confidence``, ``plane``, ``status``) and
        ``range``, ordered on the current stream, nothing synchronised.  Otherwise numpy arrays, which reads once and raises
        when the frames' time stamps decrease or are not finite, when the range is not finite, negative or empty (a median
        of 0: no frame's patches yet), or on trajectory()'s unresolved bit."""
        name = "event_depth()"
        if not rel_range > 1:
            raise RuntimeError(name + ": rel_range is above 1")
        xd, yd, td, _, extra = self._event_inputs(name, x, y, t, None, denoise, distorted)
        knots, tdev, K, median, t_ref, H, W = self._event_query(name, t_ref, None, None, None, None, None)
        with torch.no_grad():
            if range is None:
                range = torch.cat([median / float(rel_range), median * float(rel_range)])
            out = ops.event_dsi(xd, yd, td, knots, tdev, t_ref, K, H, W, planes=planes, range=range, min_votes=min_votes,
                                adaptive_radius=adaptive_radius, adaptive_offset=adaptive_offset,
                                fill=median if isinstance(fill, str) and fill == "median" else fill)
            out["range"] = range if isinstance(range, torch.Tensor) else torch.tensor([float(v) for v in range], device=self.device)
        return self._answer(name, out, extra, as_tensor, traj=self._traj_status, dsi=out["status"])

    # ---------------------------------------------------------------- event map
    _event_map = None           # event_map(): the ops.PointMap the event queries merge their clouds in

    def event_map(self, voxel=None, capacity=2 ** 20):
        """The persistent semi-dense map of the scene: an ``ops.PointMap`` (a voxel hash table on the device) that
        ``event_map_insert`` merges the cleaned clouds of successive reference views in.  Created at the first call, returned
        by every later one (``voxel`` and ``capacity`` are then not read); it lives as long as the tracker.

        ``voxel=None``: ``0.01 / median``, one hundredth of the median depth -- the median inverse depth ``compensate_events``
        uses by default, read ONCE, here (the one wait of this call; raises while it is 0: no frame's patches yet).  A default
        nobody has tuned.  A device-resident state stays device resident."""
        if self._event_map is None:
            if voxel is None:
                with self._state_stream() as sc:
                    word = self._depth_median_word(sc.resident)
                    sc.leaves(word)
                median = float(word.cpu())
                if not (median > 0.0 and median < float("inf")):
                    raise RuntimeError("event_map(): no depth median yet to size the voxels from (track a frame, or give voxel)")
                voxel = 0.01 / median
            with torch.cuda.device(self.device):
                self._event_map = ops.PointMap(voxel, capacity=capacity, device=self.device)
        return self._event_map

    def event_map_insert(self, x, y, t, t_ref=None, median_radius=2, min_support=3, min_invdepth=None, as_tensor=False,
                         **event_depth_arguments):
        """One reference view into the event map: ``event_depth(x, y, t, t_ref, **event_depth_arguments)`` (the plane sweep of
        these events), ``ops.depth_points`` of its ``invdepth`` / ``plane`` / ``confidence`` at the camera pose
        ``poses_at([t_ref])`` (median filter of radius ``median_radius`` over the detected pixels, detections with fewer than
        ``min_support`` detected pixels in their window dropped, lift to world points), and ``event_map().insert`` of the
        cloud with the frame counter as the view id (the map's mask of views wraps at 64).  ``min_invdepth=None``: 0, every
        positive inverse depth of the sweep's range is lifted.

        A device-resident state stays device resident (no settle(), the next frame is still one C call); nothing of the
        tracker's state is written.  ``as_tensor=True``: a dict of device tensors, ordered on the current stream, nothing
        synchronised: ``depth_status`` (ops.event_dsi), ``points_status`` (ops.depth_points), ``map_status``
        (PointMap.insert), ``pose_status`` (ops.se3_interp), ``count`` (the points inserted from).  Otherwise the three status
        words as dicts (``ops.event_dsi_status``, ``ops.depth_points_status``, ``ops.point_map_status``) and ``count`` as an
        int, which reads once and raises on the conditions ``event_depth`` raises on and when the pose at ``t_ref`` is not
        finite."""
        name = "event_map_insert()"
        if event_depth_arguments.get("fill") is not None:
            raise RuntimeError(name + ": fill stays None (an undetected pixel has no depth to lift)")
        pm = self.event_map()
        out = self.event_depth(x, y, t, t_ref=t_ref, as_tensor=True, **event_depth_arguments)
        cams, _, pose_status = self.poses_at([self.tlist[-1] if t_ref is None else float(t_ref)], as_tensor=True)
        with self._state_stream() as sc:
            K = self.intrinsics_[0] * float(self.RES)
            sc.leaves(K)
        with torch.no_grad():
            pts = ops.depth_points(out["invdepth"], cams[0], K, plane=out["plane"], confidence=out["confidence"],
                                   median_radius=median_radius, min_support=min_support,
                                   min_invdepth=0.0 if min_invdepth is None else float(min_invdepth))
            map_status = pm.insert(pts["points"], conf=pts["conf"], count=pts["count"], view=int(self.counter))
        res = dict(depth_status=out["status"], points_status=pts["status"], map_status=map_status, pose_status=pose_status,
                   count=pts["count"])
        if as_tensor:
            return res
        _check_status(name, traj=self._traj_status, interp=pose_status, dsi=out["status"], depth_points=pts["status"])
        st = ops.depth_points_status(pts["status"])
        return dict(depth_status=ops.event_dsi_status(out["status"]), points_status=st,
                    map_status=ops.point_map_status(map_status), count=st["n_lifted"])

    # ---------------------------------------------------------------- event landmarks
    _LANDMARK_KEYS = ("min_obs", "refine", "min_parallax", "max_rms", "sigma_px", "max_landmarks", "extrapolate", "want_index",
                      "want_residual", "want_rays")

    def event_landmarks(self, x, y, t, p=None, distorted=False, denoise=False, carry=True, insert=False, as_tensor=False, **params):
        """The sparse landmark map of the next stretch of the sensor's stream: ``event_corner_tracks`` links the corners of
        these events into tracks, ``ops.event_landmarks`` triangulates every track from the camera poses at its own events'
        time stamps, with the trajectory as it is now (``params``: the detector's and the linker's -- ``max_dt`` is required --
        and the triangulation's ``min_obs``, ``refine``, ``min_parallax``, ``max_rms``, ``sigma_px``, ``max_landmarks``,
        ``extrapolate``, ``want_index``, ``want_residual``, ``want_rays``; its defaults are numbers nobody has tuned).

        ``x, y`` are RAW SENSOR PIXELS at the tracker's image size: the tracks are linked on them, with ``p``, ``denoise`` and
        ``carry`` exactly as ``event_corner_tracks`` takes them.  The rays take the coordinates of the images the tracker is
        fed: the same pixels, or with ``distorted=True`` those of ``rectify_events`` (the camera of ``set_camera``; raises
        without one) -- an event without a solution is a NaN row and is counted in word [2].  Trajectory, time stamps and
        intrinsics are those of ``compensate_events``.  ONLY THE OBSERVATIONS OF THIS CALL are triangulated: the track ids
        carry on from call to call, partial sums of a track do not.  ``insert=True``: the points go into ``event_map()`` with
        the confidence 1 / trace(cov) and the frame counter as the view; a landmark that is not valid is a NaN row, which
        the map drops and counts; the result gains ``map_status``.

        Returns the union of ``event_corner_tracks``' dict and ``ops.event_landmarks``' -- per event ``track`` and the
        linker's other outputs, per landmark ``lm_track`` (the id), ``point``, ``cov``, ``n_obs``, ``lm_cls``, ``rms``,
        ``parallax``, ``span``, ``count``, ``status`` (the triangulation's; the linker's ``cls`` and ``status`` stay ``cls``
        and ``track_status``).  A device-resident state stays device resident.  ``as_tensor=True``: device tensors, ordered on
        the current stream, nothing synchronised.  Otherwise numpy arrays, the per-landmark ones cut to ``count`` (an int),
        which waits and raises on what ``event_corner_tracks`` raises on, when the frames' time stamps decrease or are not
        finite, and on trajectory()'s unresolved bit."""
        name = "event_landmarks()"
        keys = self._CORNER_KEYS + self._TRACK_KEYS + self._LANDMARK_KEYS
        unknown = sorted(set(params) - set(keys))
        if unknown:
            raise RuntimeError(name + ": unknown parameter %s (known: %s)" % (unknown[0], ", ".join(keys)))
        if not self.tlist:
            raise RuntimeError(name + ": no frame has been tracked yet")
        if insert:
            pm = self.event_map()
        td = self._as_device(t, torch.float64)
        rect = None
        if distorted:
            xr, yr, rect = self._undistorted(name, x, y)
        else:
            xr, yr = self._as_device(x, torch.float32), self._as_device(y, torch.float32)
        carried = self._track_state
        trk = self.event_corner_tracks(x, y, td, p=p, as_tensor=True, denoise=denoise, carry=carry,
                                       **{k: v for k, v in params.items() if k not in self._LANDMARK_KEYS})
        knots, _ = self.trajectory(as_tensor=True)
        tdev = self._frame_times_dev()
        with self._state_stream() as sc:                      # reads of the state, on the stream it lives on
            K = self.intrinsics_[0] * float(self.RES)
            sc.leaves(K)
        with torch.no_grad():
            lm = ops.event_landmarks(xr, yr, td, trk["track"], knots, tdev, K,
                                     **{k: v for k, v in params.items() if k in self._LANDMARK_KEYS})
            out = {**trk, **lm, "track": trk["track"], "lm_track": lm["track"], "cls": trk["cls"], "lm_cls": lm["cls"],
                   "track_status": trk["status"]}
            if insert:
                c = lm["cov"]
                out["map_status"] = pm.insert(lm["point"], conf=1.0 / (c[:, 0] + c[:, 3] + c[:, 5]), count=lm["count"],
                                              view=int(self.counter))
        if rect is not None:
            out["rectify_status"] = rect
        if as_tensor:
            return out
        # (the one wait: the linker's words were not looked at by its as_tensor form)
        words = [s.reshape(-1)[:1] for s in (out.get("filter_status"), out["corner_status"], out["track_status"]) if s is not None]
        try:
            for word in torch.cat(words).cpu().tolist():
                _raise_on_words(name, {"filter": word})
        except RuntimeError:
            if carry:
                self._track_state = carried                    # (a bad order leaves what is carried as it was)
            raise
        _check_status(name, rectify=rect, traj=self._traj_status, interp=lm["status"])
        k = int(out["count"].cpu())
        per_landmark = ("lm_track", "point", "cov", "n_obs", "lm_cls", "rms", "parallax", "span")
        res = {key: (v[:k] if key in per_landmark else v).cpu().numpy() for key, v in out.items()}
        res["count"] = k
        return res

    def event_map_points(self, min_points=2, min_views=1, as_tensor=False):
        """The event map as it is now (``event_map().export``): the mean point of every voxel that holds at least ``min_points``
        points from at least ``min_views`` views (of 64: view ids wrap), sorted by voxel key.  ``as_tensor=True``: the dict of
        device tensors of ``PointMap.export`` (``points``, ``n``, ``conf``, ``n_views``, ``key`` over the table's capacity, the
        first ``count`` rows written; ``status``), nothing synchronised.  Otherwise numpy arrays cut to the count (one wait),
        ready for ``evaluate.save_points_ply(path, points, conf)``.  Raises before the first ``event_map()``."""
        if self._event_map is None:
            raise RuntimeError("event_map_points(): there is no event map yet (event_map() or event_map_insert())")
        with torch.no_grad():
            out = self._event_map.export(min_points=min_points, min_views=min_views)
        if as_tensor:
            return out
        k = int(out["count"].cpu())
        return {**{key: out[key][:k].cpu().numpy() for key in ("points", "n", "conf", "n_views", "key")},
                "count": k, "status": out["status"].cpu().numpy()}

    def event_map_depth(self, t_ref=None, radius=2, footprint=True, min_points=2, min_views=1, fill=None, height=None,
                        width=None, as_tensor=False):
        """What the event map looks like from the camera pose at ``t_ref`` (default: the newest frame): a z-buffered inverse
        depth map [height, width] (``event_map().render`` at ``poses_at([t_ref])`` with the image intrinsics, row 0 of the
        tracker's own times the patch stride).  It carries the evidence of every view inserted so far and can be asked at a
        pose the map has never been swept at; it is what ``compensate_events(invdepth="event_map")`` and its siblings sample.
        ``radius``, ``footprint``, ``min_points``, ``min_views``: as ``ops.PointMap.render``; ``fill``: what a pixel no voxel
        covers gets -- None (NaN), a number, a one-element device tensor, or ``"median"`` (the median inverse depth
        ``compensate_events`` uses by default, a device word the host never reads).  ``radius=2``, ``min_points=2`` and the
        footprint rule are defaults nobody has tuned.  ``height, width`` default to the tracker's.

        A device-resident state stays device resident (no settle(), the next frame is still one C call); neither the map nor
        the tracker's state is written.  ``as_tensor=True``: the dict of device tensors of ``PointMap.render`` (``invdepth``,
        ``key``, ``n``, ``conf``, ``status``) and ``pose_status`` (ops.se3_interp), ordered on the current stream, nothing
        synchronised.  Otherwise numpy arrays, which reads once and raises when the pose at ``t_ref`` is not finite, when the
        frames' time stamps decrease or are not finite, or on trajectory()'s unresolved bit.  Raises before the first
        ``event_map()``."""
        name = "event_map_depth()"
        if self._event_map is None:
            raise RuntimeError(name + ": there is no event map yet (event_map() or event_map_insert())")
        if not self.tlist:
            raise RuntimeError(name + ": no frame has been tracked yet")
        if isinstance(fill, str) and fill != "median":
            raise RuntimeError(name + ": fill is None, a number, a one-element device tensor or 'median'")
        cams, _, pose_status = self.poses_at([self.tlist[-1] if t_ref is None else float(t_ref)], as_tensor=True)
        with self._state_stream() as sc:                      # reads of the state, on the stream it lives on
            K = self.intrinsics_[0] * float(self.RES)
            if isinstance(fill, str):
                fill = self._depth_median_word(sc.resident)
            sc.leaves(K, fill)
        with torch.no_grad():
            out = self._event_map.render(cams[0], K, self.ht if height is None else int(height),
                                         self.wd if width is None else int(width), radius=radius, footprint=footprint,
                                         min_points=min_points, min_views=min_views, fill=fill)
        out["pose_status"] = pose_status
        return self._answer(name, out, {}, as_tensor, traj=self._traj_status, interp=pose_status, depth_points=out["status"])

    def event_map_localize(self, x, y, t, t_ref=None, tau=None, cam=None, smooth=2, min_points=2, min_views=1, huber=0.0,
                           iters=10, max_evals=None, distorted=False, denoise=False, as_tensor=False):
        """Where is the camera in the event map at ``t_ref`` (default: the newest frame)?  The events become a smoothed negative
        time surface at the tracker's image size (``ops.time_surface``: decay ``tau``, ``smooth`` passes), and
        ``event_map().localize`` moves the start pose ``cam`` [7] (camera to world; None: ``poses_at([t_ref])``) until the map's
        voxels, projected with the image intrinsics (row 0 of the tracker's own times the patch stride), sample small values of
        that surface -- Levenberg-Marquardt on the device, the tracking half of EVO / ESVO.  Events, ``distorted`` and ``denoise``
        as ``compensate_events`` (no polarity).  ``tau=None``: the time between the last two frames; it, ``smooth``,
        ``min_points=2`` and ``iters`` are defaults nobody has tuned.  ``min_points``, ``min_views``, ``huber``, ``iters``,
        ``max_evals``: as ``ops.PointMap.localize``.

        A device-resident state stays device resident (no settle(), the next frame is still one C call); NOTHING of the tracker
        or of the map is written: the pose is an answer, not fed back into the window.  ``as_tensor=True``: the dict of device
        tensors of ``PointMap.localize`` with ``pose_prior`` (the start, float32 [7]), ``surface_status`` (ops.time_surface) and
        ``pose_status`` (ops.se3_interp; None with a ``cam`` given), ordered on the current stream, nothing synchronised.
        Otherwise numpy arrays and numbers (a few small copies): ``pose``, ``pose_prior``, ``delta`` (the 6-vector Log(pose^-1
        pose_prior), translation then rotation), ``cost``, ``cost0``, ``hessian``, ``reason`` (``ops.LOCALIZE_REASONS``: ``few``,
        ``singular``, ``stalled`` and ``budget`` are reported, not raised), ``n_accepted``, ``n_evals`` and ``counts``
        (``ops.point_map_localize_status`` of the evaluation at ``pose``); raises when the start pose is not finite, when the
        frames' time stamps decrease or are not finite, or on trajectory()'s unresolved bit.  Raises before the first
        ``event_map()``."""
        name = "event_map_localize()"
        if self._event_map is None:
            raise RuntimeError(name + ": there is no event map yet (event_map() or event_map_insert())")
        if not self.tlist:
            raise RuntimeError(name + ": no frame has been tracked yet")
        t_ref = float(self.tlist[-1] if t_ref is None else t_ref)
        if tau is None:
            if len(self.tlist) < 2:
                raise RuntimeError(name + ": tau=None needs two frames (the time between the last two)")
            tau = float(self.tlist[-1]) - float(self.tlist[-2])
        if not (0.0 < float(tau) < float("inf")) or t_ref != t_ref or abs(t_ref) == float("inf"):
            raise RuntimeError(name + ": tau is finite and positive, t_ref finite")
        xd, yd, td, _, extra = self._event_inputs(name, x, y, t, None, denoise, distorted)
        pose_status = None
        if cam is None:
            cams, _, pose_status = self.poses_at([t_ref], as_tensor=True)
            cam = cams[0]
        else:
            cam = self._as_device(cam, torch.float32).reshape(-1)
        with self._state_stream() as sc:                      # reads of the state, on the stream it lives on
            K = self.intrinsics_[0] * float(self.RES)
            sc.leaves(K)
        with torch.no_grad():
            ts = ops.time_surface(xd, yd, td, t_ref, float(tau), self.ht, self.wd, smooth=smooth)
            out = self._event_map.localize(ts["surface"], cam, K, min_points=min_points, min_views=min_views, huber=huber,
                                           iters=iters, max_evals=max_evals)
            out["pose_prior"] = cam.reshape(7).to(torch.float32)
        out["surface_status"], out["pose_status"] = ts["status"], pose_status
        out.update(extra)
        if as_tensor:
            return out
        info = torch.zeros(8, dtype=torch.int32, device=self.device)
        info[0] = out["info"][4]                              # (every evaluation's word 0: the bad-camera bit rides on the one copy)
        _check_status(name, rectify=extra.get("rectify_status"), filter=extra.get("filter_status"),
                      traj=self._traj_status if pose_status is not None else None, interp=pose_status, depth_points=info)
        pose, prior = out["pose"].cpu().numpy(), out["pose_prior"].cpu().numpy()
        words = ops.point_map_localize_info(out["info"])
        return dict(pose=pose, pose_prior=prior, delta=_se3_log_between(pose, prior), cost=float(out["cost"].cpu()),
                    cost0=float(out["cost0"].cpu()), hessian=out["hessian"].cpu().numpy(), reason=words["reason"],
                    n_accepted=words["n_accepted"], n_evals=words["n_evals"], counts=ops.point_map_localize_status(out["status"]),
                    surface_counts=ops.time_surface_status(out["surface_status"]))

    def _depth_median_word(self, resident):
        """(on the stream the state lives on) the lower median inverse depth of the last three frames' patches as a device
        word the host never reads; 0 without a frame"""
        word = torch.zeros(1, dtype=torch.float32, device=self.device)
        if resident:
            ops.depth_median_rows(self.patches_, self._dev.dyn[track_dev.DYN_NROW:], 3, word)
        elif self._n > 0:
            ops.depth_median(self.patches_, self._n, min(3, self._n), word)
        return word

    def invdepth_map(self, t_ref=None, radius=None, weights="variance", max_rel_depth_sigma=None, min_obs=2,
                     prior_rel_sigma=1.0, height=None, width=None, as_tensor=False):
        """A dense inverse-depth map [height, width] of the scene as the tracker has estimated it, at the camera pose of time
        ``t_ref`` (default: the newest frame): the window's patches are projected into that pose (one row of ``poses_at``)
        and regressed with a biweight kernel of support ``radius`` image pixels (``ops.invdepth_map``).  The map is what
        ``compensate_events(invdepth=...)`` and ``ops.event_warp`` sample at an event's pixel.

        ``weights="variance"``: the patches ``map(max_rel_depth_sigma=..., min_obs=...)`` selects (the same query: one C call
        for the covariance, one for the selection), each weighted by the inverse of its marginal depth variance, against a
        prior of RELATIVE sigma ``prior_rel_sigma`` -- weight ``prior_rel_sigma**-2 / prior**2``, formed on the device.
        ``weights="uniform"``: no covariance call; the patches of the newest ``REMOVAL_WINDOW`` frames with weight 1 against a
        prior of weight ``prior_rel_sigma**-2``.  The prior is the median inverse depth ``compensate_events`` uses by default,
        so a pixel no patch reaches gets the median and a pixel between patches is drawn to it as the kernel weight falls.
        ``radius=None``: ``max(height, width) / 10`` -- a default nobody has tuned.  ``height, width`` default to the
        tracker's.

        A device-resident state stays device resident (no settle(), nothing of the state written; the row count, the selection
        and the median are read on the device).  ``as_tensor=True``: a dict of device tensors ``invdepth``, ``weight`` (the
        summed kernel weight per pixel), ``status`` (ops.invdepth_map_status) and ``pose_status`` (ops.se3_interp), ordered on
        the current stream, nothing synchronised.  Otherwise numpy arrays, which waits for the result and raises when the
        pose at ``t_ref`` is not finite and on the conditions ``poses_at`` raises on."""
        if not self.tlist:
            raise RuntimeError("invdepth_map(): no frame has been tracked yet")
        if weights not in ("variance", "uniform"):
            raise RuntimeError("invdepth_map(): weights is 'variance' or 'uniform'")
        if not prior_rel_sigma > 0:
            raise RuntimeError("invdepth_map(): prior_rel_sigma is positive")
        H, W = self.ht if height is None else int(height), self.wd if width is None else int(width)
        R = max(H, W) / 10.0 if radius is None else float(radius)
        pw = float(prior_rel_sigma) ** -2
        cams, _, pose_status = self.poses_at([self.tlist[-1] if t_ref is None else float(t_ref)], as_tensor=True)

        def render(resident, index=None, count=None, dvar=None):
            dyn = self._dev.dyn[track_dev.DYN_NROW:] if resident else None
            prior = self._depth_median_word(resident)
            if dvar is not None:
                r = ops.invdepth_map(self.poses_, self.patches_, self.intrinsics_[0], cams[0], H, W, R, scale=self.RES,
                                     index=index, count=count, conf=dvar, conf_is_variance=True, prior=prior, prior_weight=pw,
                                     prior_relative=True, dyn_rows=dyn, per_row=self.M)
            else:
                n = self.N if resident else self._n
                r = ops.invdepth_map(self.poses_[:n], self.patches_[:n], self.intrinsics_[0], cams[0], H, W, R, scale=self.RES,
                                     prior=prior, prior_weight=pw, dyn_rows=dyn, per_row=self.M,
                                     last_rows=int(self.cfg.REMOVAL_WINDOW))
            return r["invdepth"], r["weight"], r["status"]

        # inputs=(cams,): the pose was made on the caller's stream and is read on the one the state lives on
        if weights == "variance":
            def then(resident, out):
                index, count = self._select(resident, out, None, max_rel_depth_sigma, min_obs)
                return render(resident, index, count, out[1])

            inv, wgt, status = self._window_query("invdepth_map()", with_map=True, then=then, inputs=(cams,))[-3:]
        else:
            with self._state_stream(inputs=(cams,)) as sc:
                if not sc.resident:
                    self._join_main()
                inv, wgt, status = render(sc.resident)
                sc.leaves(inv, wgt, status)
        out = dict(invdepth=inv, weight=wgt, status=status, pose_status=pose_status)
        return self._answer("invdepth_map()", out, {}, as_tensor, traj=self._traj_status, interp=pose_status, cam=status)

    # --------------------------------------------------------------- uncertainty
    def _window_query(self, name, with_map=False, then=None, inputs=()):
        """what uncertainty() and map() share: the one C call on the stream the state lives on, ordered in front of the
        current stream.  Returns the call's raw device tensors (cov, depth_var, stats words[, point, point_cov,
        pose_depth_cov, n_obs]) followed by what ``then(resident, tensors)`` enqueued behind it on the same stream."""
        dv = self._dev
        last_t, last_w = getattr(self, "last_target", None), getattr(self, "last_weight", None)
        if (last_t is None or last_w is None) and not (dv is not None and dv.active and dv._frames):
            raise RuntimeError(name + ": no update has run yet -- there are no targets and weights to form the "
                               "system from (track at least until the first update())")
        W = int(self.cfg.OPTIMIZATION_WINDOW)
        with self._state_stream(inputs) as sc:
            if sc.resident:
                if not dv._frames:                            # (handed over, no device step yet: the last update ran host-driven)
                    k = last_t.shape[1]
                    dv.target[:k].copy_(last_t[0])
                    dv.weight[:k].copy_(last_w[0])
                out = dv.map() if with_map else dv.uncertainty()
            else:
                self._join_main()
                n = self._n
                rows = self._net_map_dev if self._net_map_dev is not None else self._upload(self._net_rows())
                if rows.numel() != self._dii.numel() or rows.numel() == 0:
                    raise RuntimeError(name + ": the factor graph has changed since the last update()")
                t0 = max(n - W, 1) if self.is_initialized else 1
                op = ops.ba_map_covariance if with_map else ops.ba_covariance
                out = op(self.poses_, self.patches_, self.intrinsics_, last_t[0][rows], last_w[0][rows], self.lmbda,
                         self._dii, self._djj, self._dkk, t0, n)
            if then is not None:
                out = tuple(out) + tuple(then(sc.resident, out))
            sc.leaves(out)
        return out

    def _select(self, resident, out, max_sigma, max_rel_depth_sigma, min_obs):
        """(on the state's stream) ops.map_select over a with_map window query's tensors; resident: the count is read on the device"""
        _, dvar, _, _, pcov, _, nobs = out
        rows = dict(dyn_rows=self._dev.dyn[track_dev.DYN_NROW:], per_row=self.M) if resident else dict(n=self._n * self.M)
        return ops.map_select(pcov, dvar, self.patches_, nobs, max_sigma, max_rel_depth_sigma, min_obs, **rows)

    def uncertainty(self):
        """How good the window's poses and depths are right now: the marginal covariance of the free poses and the marginal
        variance of every patch depth (``fastba.covariance``: the damped system the step is solved with), from the LAST
        update's targets and confidence weights at the poses and patches as they are now, over the factors that survived
        the keyframe test -- the state between two frames.  Returns a dict:

        ``frames`` (t0 .. t1-1: the keyframe rows the blocks of ``cov`` belong to), ``cov`` [6N, 6N], ``pose_cov`` [N, 6, 6]
        (its diagonal blocks; translation 3, rotation 3, left perturbation of the world-to-camera pose), ``depth_var`` [n, M]
        (inf for a patch without a factor), ``chi2``, ``n_valid``, ``dof = 2 n_valid - 6N - Mu``, ``sigma0_sq = chi2 /
        max(dof, 1)``.  Tensors are on the device.

        A device-resident state stays device resident: ONE C call (csrc/track.hip::ramp_track_uncertainty) that reads the
        sizes on the device, no settle(), no hand-back; the host synchronises only to read the result.  Nothing of the
        tracker's state is written, so a queried tracker tracks the same bits as one that is never asked."""
        cov_c, dvar_c, raw = self._window_query("uncertainty()")
        s = ops.ba_covariance_stats(raw)                      # (the one synchronisation: 32 bytes)
        N, t0 = s["N"], s["t0"]
        n = t0 + N
        cov = cov_c[:6 * N, :6 * N]
        pose_cov = torch.stack([cov[6 * a:6 * a + 6, 6 * a:6 * a + 6] for a in range(N)]) if N else cov.new_zeros((0, 6, 6))
        dof, sigma0_sq = _dof_sigma0(s)
        return dict(frames=list(range(t0, n)), cov=cov, pose_cov=pose_cov, depth_var=dvar_c[:n * self.M].view(n, self.M),
                    chi2=s["chi2"], n_valid=s["n_valid"], dof=dof, sigma0_sq=sigma0_sq, failed=s["failed"])

    def map(self, max_sigma=None, max_rel_depth_sigma=None, min_obs=2):
        """The map with its uncertainty, filtered: the window's patch centres as world points, each with the 3 x 3 covariance
        ``fastba.map_covariance`` propagates from the system behind ``uncertainty()`` (same factors, same state between two
        frames), compacted on the device to the K points that pass

        ``sqrt(trace(point_cov)) <= max_sigma`` (world units), ``sqrt(depth_var) / d <= max_rel_depth_sigma`` and
        ``n_obs >= min_obs`` (valid factors of the patch); ``None`` (or ``min_obs=0``) switches a criterion off.  A point
        whose covariance is not finite never passes.

        Returns a dict of device tensors in patch order: ``index`` [K] (flat patch id ``frame * M + m``), ``frame`` [K],
        ``points`` [K, 3], ``point_cov`` [K, 3, 3], ``colors`` [K, 3] uint8, ``depth_sigma_rel`` [K], ``n_obs`` [K]; and
        ``n_total`` (patches with a factor, before the selection), ``chi2``, ``dof``, ``sigma0_sq``, ``failed`` as
        ``uncertainty()``.

        As ``uncertainty()``, a device-resident state stays resident and nothing of the tracker's state is written: one C
        call for the covariance and the map (csrc/track.hip::ramp_track_map), one for the selection (ramp_map_select); the
        host waits only for the stats words and the count."""
        M = self.M
        select = lambda resident, out: self._select(resident, out, max_sigma, max_rel_depth_sigma, min_obs)
        _, dvar, raw, point, pcov, _, nobs, index, count = self._window_query("map()", with_map=True, then=select)
        s = ops.ba_covariance_stats(raw)                      # (the two synchronisations: 32 bytes and 4 bytes)
        K = int(count.cpu())
        idx = index[:K].long()
        P = self.patches_.shape[-1]
        d = self.patches_.view(-1, 3, P, P)[:, 2, 1, 1]
        sym = torch.tensor([0, 1, 2, 1, 3, 4, 2, 4, 5], device=idx.device)
        dof, sigma0_sq = _dof_sigma0(s)
        return dict(index=idx, frame=idx // M, points=point[idx], point_cov=pcov[idx][:, sym].view(K, 3, 3),
                    colors=self.colors_.view(-1, 3)[idx], depth_sigma_rel=dvar[idx].sqrt() / d[idx], n_obs=nobs[idx],
                    n_total=s["Mu"], chi2=s["chi2"], dof=dof, sigma0_sq=sigma0_sq, failed=s["failed"])
