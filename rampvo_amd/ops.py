"""Tensor-level wrappers over the C ABI (include/ramp_hip.h).

Each function takes/returns torch CUDA tensors and enqueues one HIP kernel (or a
short fixed pipeline) on torch's current stream.  No CPU fallbacks.
"""
import ctypes

import torch

from . import _lib, switches, track_dev
from ._lib import RAMP_CORR_MFMA32 as _LIB_CORR_MFMA32
from ._lib import RAMP_CORR_X2 as _LIB_CORR_X2
from ._lib import sized_workspace, workspace as _lib_workspace
from ._lib import KPLANE, RAMP_NHWC32, RAMP_NCHW, RAMP_NHWC, CorrLevel, check, dtype_code, kplane, lib, ptr, require_cuda, stream


# ------------------------------------------------------------------- status words
# The one table of status words.  Per entry point ramp_<key>: the bits of status word 0 as name -> (mask, message), and the names
# of words 1 and up.  The message is what the numpy form of a query raises with when the bit is set (queries._check_status):
# a text, None for a bit that is decoded but never raises, or (head, ((refining mask, text), ...), default text) for a bit
# whose text the word's other bits refine.  Entries whose words share a bit share its row.
_BAD_TIMES = (_lib.RAMP_INTERP_BAD_TIMES, "the frames' time stamps decrease or are not finite")
_BAD_CAMERA = (_lib.RAMP_RECTIFY_BAD_CAMERA, "the camera record is not finite or a focal length is not positive")
# (RAMP_MAP_RENDER_BAD_CAMERA is the same bit, raised on the same condition: the two entries share the row and the role)
_BAD_POSE = (_lib.RAMP_DEPTH_POINTS_BAD_CAMERA, "the camera pose at t_ref is not finite")
assert _lib.RAMP_MAP_RENDER_BAD_CAMERA == _lib.RAMP_DEPTH_POINTS_BAD_CAMERA == _lib.RAMP_MAP_LOCALIZE_BAD_CAMERA
# (RAMP_FLOW_BAD_ORDER, RAMP_CORNER_BAD_ORDER and RAMP_CORNER_TRACK_BAD_ORDER are the same bit, raised on the same condition:
# event_flow, event_corners and event_corner_tracks share the row and the ``filter`` role)
_BAD_ORDER = (_lib.RAMP_FILTER_BAD_ORDER, "a pixel's events decrease in time, or lie before the filter's state")
assert _lib.RAMP_FLOW_BAD_ORDER == _lib.RAMP_CORNER_BAD_ORDER == _lib.RAMP_CORNER_TRACK_BAD_ORDER == _lib.RAMP_FILTER_BAD_ORDER
_STATUS = {
    "trajectory": ({"unresolved": (track_dev.TRAJ_UNRESOLVED,
                                   "a frame is neither a keyframe nor reachable through the delta chain")}, ()),
    "event_warp": ({"bad_times": _BAD_TIMES}, ("n_below", "n_above", "n_not_finite", "n_rejected", "n_outside", "n_contributed")),
    "event_dsi": ({"bad_times": _BAD_TIMES,
                   "bad_range": (_lib.RAMP_DSI_BAD_RANGE,
                                 "the range of inverse depths is not finite, negative or empty (no depth median yet?)")},
                  ("n_below", "n_above", "n_not_finite", "n_no_vote", "n_voted", "n_detected")),
    "depth_points": ({"bad_camera": _BAD_POSE}, ("n_detected", "n_isolated", "n_depth_rejected", "n_lifted")),
    "point_map": ({}, ("n_seen", "n_not_finite", "n_out_of_range", "n_dropped_full", "n_accumulated", "n_occupied")),
    "point_map_export": ({}, ("n_passing", "n_cut_off", "n_occupied")),
    "point_map_render": ({"bad_camera": _BAD_POSE},
                         ("n_occupied", "n_filtered", "n_rejected", "n_outside", "n_rendered", "n_pixels")),
    "point_map_localize": ({"bad_camera": _BAD_POSE}, ("n_occupied", "n_filtered", "n_rejected", "n_out_of_reach", "n_in_reach")),
    "time_surface": ({"bad_args": (_lib.RAMP_TIME_SURFACE_BAD_ARGS, None)},
                     ("n_events", "n_not_finite", "n_outside", "n_late", "n_used", "n_pixels")),
    "event_voxel": ({"bad_offsets": (_lib.RAMP_VOXEL_BAD_OFFSETS, "the slice offsets decrease or leave the event list"),
                     "bad_times": (_lib.RAMP_VOXEL_BAD_TIMES, "the first or last time stamp of a slice is not finite")},
                    ("n_events", "n_not_finite", "n_outside", "n_no_bin", "n_contributed")),
    "event_rectify": ({"bad_camera": _BAD_CAMERA},
                      ("n_events", "n_not_finite", "n_not_invertible", "n_behind", "n_outside", "n_inside")),
    "image_rectify": ({"bad_camera": _BAD_CAMERA}, ("n_pixels", "n_invalid", "n_outside", "n_sampled")),
    "event_filter": ({"bad_order": _BAD_ORDER},
                     ("n_events", "n_not_finite", "n_outside", "n_hot", "n_refractory", "n_no_support", "n_kept")),
    "event_flow": ({"bad_order": _BAD_ORDER},
                   ("n_events", "n_not_finite", "n_outside", "n_few_points", "n_collinear", "n_flat", "n_valid")),
    "event_corners": ({"bad_order": _BAD_ORDER},
                      ("n_events", "n_not_finite", "n_outside", "n_border", "n_no_inner_arc", "n_no_outer_arc", "n_corners")),
    "event_corner_tracks": ({"bad_order": _BAD_ORDER},
                            ("n_events", "n_not_finite", "n_outside", "n_not_corner", "n_born", "n_carried", "n_linked")),
    "event_landmarks": ({"bad_times": _BAD_TIMES},
                        ("n_no_track", "n_not_finite", "n_out_of_range", "n_observations", "n_tracks", "n_cut_off", "n_valid")),
    "invdepth_map": ({"bad_cam": (_lib.RAMP_DEPTHMAP_BAD_CAM, "the camera pose at t_ref is not finite")},
                     ("n_considered", "n_bad_depth", "n_rejected", "n_out_of_reach", "n_contributing", "n_empty_pixels")),
    "se3_interp": ({"bad_times": _BAD_TIMES}, ("n_below", "n_above", "n_nan")),
    "imu": ({"bad_order": (_lib.RAMP_IMU_BAD_ORDER, "the IMU samples' or the frames' time stamps decrease or are not finite"),
             "gyro_failed": (_lib.RAMP_IMU_GYRO_FAILED, "the gyro bias step failed (no interval between two frames is covered "
                                                        "by the samples, or its system is not finite)"),
             "scale_failed": (_lib.RAMP_IMU_SCALE_FAILED,
                              ("the scale and gravity solve failed: ",
                               ((_lib.RAMP_IMU_FEW_TRIPLES, "fewer than two triples of frames are covered by the samples"),
                                (_lib.RAMP_IMU_BAD_SCALE, "the scale is not positive")), "the system is singular")),
             "few_triples": (_lib.RAMP_IMU_FEW_TRIPLES, None), "singular": (_lib.RAMP_IMU_SINGULAR, None),
             "bad_scale": (_lib.RAMP_IMU_BAD_SCALE, None)},
            ("n_samples", "n_intervals", "n_uncovered", "n_dt_not_positive", "n_gyro_intervals", "n_triples")),
    "imu_propagate": ({"bad_order": (_lib.RAMP_IMU_BAD_ORDER, "the IMU samples' time stamps decrease or are not finite"),
                       "bad_anchor": (_lib.RAMP_IMU_BAD_ANCHOR, "the anchor is not finite or its scale is not positive "
                                                                "(a failed alignment leaves NaN)"),
                       "no_start": (_lib.RAMP_IMU_NO_START, "no IMU sample lies at or before the anchor's time stamp")},
                      ("n_samples", "n_held", "n_propagated", "n_cut_off", "n_beyond_horizon")),
}
# the roles of queries._check_status (its keywords): the entry whose word 0 each one carries -- ``interp`` also the words of
# ops.event_warp and word 4 of ops.event_align's info, ``rectify`` also those of ops.image_rectify, ``depth_points`` also
# those of PointMap.render
STATUS_ROLES = {"traj": "trajectory", "interp": "se3_interp", "cam": "invdepth_map", "voxel": "event_voxel",
                "rectify": "event_rectify", "filter": "event_filter", "imu": "imu", "propagate": "imu_propagate",
                "dsi": "event_dsi", "depth_points": "depth_points"}
# the order in which the bits that raise are looked at, as (role, bit): the first one set gives the message
STATUS_ORDER = (("filter", "bad_order"), ("rectify", "bad_camera"), ("traj", "unresolved"), ("interp", "bad_times"),
                ("cam", "bad_cam"), ("voxel", "bad_offsets"), ("voxel", "bad_times"), ("imu", "bad_order"),
                ("imu", "gyro_failed"), ("imu", "scale_failed"), ("propagate", "bad_order"), ("propagate", "bad_anchor"),
                ("propagate", "no_start"), ("dsi", "bad_times"), ("dsi", "bad_range"), ("depth_points", "bad_camera"))


def _status(entry, status):
    """the status words of ramp_<entry> as a dict (synchronises: one copy of the words); ``<entry>_status`` binds it below,
    beside each wrapper"""
    bits, names = _STATUS[entry]
    w = status.detach().cpu().tolist()
    return {**{k: bool(int(w[0]) & m) for k, (m, _) in bits.items()}, **{k: int(w[1 + i]) for i, k in enumerate(names)}}


def status_message(role, bit, word):
    """what a query raises with for ``bit`` of a role's word 0 = ``word``, or None while the bit is clear or never raises"""
    mask, message = _STATUS[STATUS_ROLES[role]][0][bit]
    if message is None or not word & mask:
        return None
    if isinstance(message, str):
        return message
    head, refined, default = message
    return head + next((text for m, text in refined if word & m), default)


# ------------------------------------------------------------------- altcorr
def patchify(net, coords, radius, bilinear=True, layout=RAMP_NCHW, out_layout=RAMP_NCHW):
    """net [n,C,H,W] (NCHW) or [n,H,W,C] (NHWC); coords [n,M,2] -> [n,M,C,d,d] (or [n,M,d,d,C])"""
    require_cuda(net, coords)
    net = net.contiguous()
    coords = coords.contiguous().float()
    if layout == RAMP_NCHW:
        n, C, H, W = net.shape
    else:
        n, H, W, C = net.shape
    M = coords.shape[1]
    d = 2 * radius + 1 if bilinear else 2 * radius + 2
    shape = (n, M, C, d, d) if out_layout == RAMP_NCHW else (n, M, d, d, C)
    out = torch.empty(shape, dtype=net.dtype, device=net.device)
    check(lib().ramp_patchify_fwd(ptr(net), ptr(coords), ptr(out), n, C, H, W, M, radius,
                                  int(bilinear), dtype_code(net), layout, out_layout, stream()),
          "ramp_patchify_fwd")
    return out


def frame_gather(f_nhwc, i_nhwc, image, coords):
    """all gathers of one frame at its patch centres, one launch (csrc/altcorr.hip::frame_gather_kernel):
    f_nhwc [h,w,CF], i_nhwc [h,w,CI] (same dtype), image [3,H,W] fp32, coords [M,2] ->
    gmap [M,3,3,CF], imap [M,CI], patches [M,3,3,3] fp32, clr [M,3] fp32, colors [M,3] uint8 BGR"""
    require_cuda(f_nhwc, i_nhwc, image, coords)
    assert f_nhwc.is_contiguous() and i_nhwc.is_contiguous() and f_nhwc.dtype == i_nhwc.dtype
    image, coords = image.contiguous(), coords.contiguous()
    assert image.dtype == torch.float32 and coords.dtype == torch.float32
    (h, w, CF), CI, M = f_nhwc.shape, i_nhwc.shape[-1], coords.shape[0]
    dev = f_nhwc.device
    gmap = torch.empty(M, 3, 3, CF, dtype=f_nhwc.dtype, device=dev)
    imap = torch.empty(M, CI, dtype=f_nhwc.dtype, device=dev)
    patches = torch.empty(M, 3, 3, 3, dtype=torch.float32, device=dev)
    clr = torch.empty(M, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(M, 3, dtype=torch.uint8, device=dev)
    check(lib().ramp_frame_gather(ptr(f_nhwc), ptr(i_nhwc), ptr(image), ptr(coords), ptr(gmap), ptr(imap),
                                  ptr(patches), ptr(clr), ptr(colors), M, h, w, image.shape[1], image.shape[2], CF,
                                  CI, dtype_code(f_nhwc), stream()), "ramp_frame_gather")
    return gmap, imap, patches, clr, colors


def corr(fmap1, fmaps2, coords, ii, jj, radius=3, coord_divs=(1.0,), layout=RAMP_NCHW, order=None, row_elems=0,
         fast_f32=None, mod_ii=0, mod_jj=0):
    """fused multi-level patch correlation.  order: optional int32 [E] schedule (a permutation of
    the edges, e.g. target-frame-major) -- affects which XCD computes an edge, never a value.

    fmap1  [N1,C,P,P] (NCHW) / [N1,P,P,C] (NHWC) patch features
    fmaps2 list of per-level target maps [N2,C,H,W] / [N2,H,W,C]
    coords [E,2,P,P] float32;  ii,jj [E] int64
    -> [E, 2r+1, 2r+1, P, P, nlevels]

    fp32 features: fast_f32 picks the kernel -- False / 0 corr_kernel<float> (the reference's fmaf chain), True / 1
    corr_mfma_kernel<float>, 2 with RAMP_NHWC32 corr_mfma_kernel<CorrX2> on planes of split fp16 pairs.  None: 1 when
    RAMP_CORR_F32_MFMA is 1 (switches.read()), else 0 -- the split mode, RAMP_CORR_F32_MFMA's default, is the tracker's
    packing and is asked for explicitly (the tracker passes fast_f32 itself)
    """
    require_cuda(fmap1, coords, ii, jj, *fmaps2)
    fmap1 = fmap1.contiguous()
    fmaps2 = [f.contiguous() for f in fmaps2]
    coords = coords.contiguous().float()
    ii = ii.contiguous()
    jj = jj.contiguous()
    assert ii.dtype == torch.int64 and jj.dtype == torch.int64
    if layout == RAMP_NCHW:
        N1, C, P, _ = fmap1.shape
    else:
        N1, P, _, C = fmap1.shape
    if layout == RAMP_NHWC32:     # target maps [N2][H][C/32][W][32] (fp16) / [N2][H][C/16][W][16] (fp32) (pyramid_pack); fmap1 stays NHWC
        kp = kplane(fmap1.dtype)
        assert fmap1.dtype in (torch.float16, torch.float32) and all(f.dim() == 5 and f.shape[2] * kp == C and f.shape[4] == kp
                                                                     for f in fmaps2)
    E = coords.shape[0]
    L = len(fmaps2)
    levels = (CorrLevel * L)()
    N2 = fmaps2[0].shape[0]
    for l, f in enumerate(fmaps2):
        assert f.dtype == fmap1.dtype and f.shape[0] == N2
        H2, W2 = ((f.shape[2], f.shape[3]) if layout == RAMP_NCHW else
                  (f.shape[1], f.shape[3]) if layout == RAMP_NHWC32 else (f.shape[1], f.shape[2]))
        levels[l] = CorrLevel(f.data_ptr(), H2, W2, float(coord_divs[l]))
    d = 2 * radius + 1
    dense = d * d * P * P * L
    if row_elems and row_elems != dense:      # padded rows [E, row_elems] (tail zero filled by the kernel)
        assert row_elems > dense
        out = torch.empty((E, row_elems), dtype=fmap1.dtype, device=fmap1.device)
    else:
        row_elems = 0
        out = torch.empty((E, d, d, P, P, L), dtype=fmap1.dtype, device=fmap1.device)
    if order is not None:
        assert order.dtype == torch.int32 and order.is_contiguous() and order.shape[0] == E
    code = dtype_code(fmap1)
    if fast_f32 is None:
        fast_f32 = switches.read().corr_f32_mfma == 1
    if fast_f32 and fmap1.dtype == torch.float32 and layout in (RAMP_NHWC, RAMP_NHWC32):
        # opt-in: MFMA accumulation order instead of the reference's fmaf chain.  fast_f32 = 2 with RAMP_NHWC32: the target
        # maps are planes of split fp16 pairs (pyramid_pack(split=True)) -> corr_mfma_kernel<CorrX2>
        code |= _LIB_CORR_X2 if (int(fast_f32) == 2 and layout == RAMP_NHWC32) else _LIB_CORR_MFMA32
    assert not (fmap1.dtype == torch.float32 and layout == RAMP_NHWC32 and not fast_f32), \
        "chunked fp32 target maps are read by the MFMA kernels only (fast_f32)"
    check(lib().ramp_corr_fwd_ordered(ptr(fmap1), levels, L, ptr(coords), ptr(ii), ptr(jj),
                                      ptr(order) if order is not None else None, ptr(out), int(row_elems), int(mod_ii),
                                      int(mod_jj), E,
                                      N1, N2, C, P, radius, code, layout, stream()),
          "ramp_corr_fwd_ordered")
    return out


def event_stack(x, y, p, height, width, num_bins=5, as_float=True):
    """EventToStack_Numpy on the device (reference utils/transformers.py:128-161): pixel coordinates x, y [N] and
    polarities p [N] (int8, +-1; 0 is read as -1 like data/events.py:29) -> the [num_bins, height, width] stack (float32
    values of the int8 stack, or int8 with as_float=False).

    Integer coordinate tensors: ramp_event_stack.  Floating-point coordinates take the sub-pixel bilinear path: an identity
    warp of ramp_event_warp (four fixed-point weights per event, integer atomics, the same bins); the int8 stack is the
    weighted sum truncated toward zero and wrapped, ``as_float`` its float32 values as above.  Integer-valued float
    coordinates give the integer path's bits."""
    require_cuda(x, y, p)
    N = x.shape[0]
    pi = p.to(torch.int8)
    pi = torch.where(pi == 0, torch.full_like(pi, -1), pi).contiguous()
    if x.is_floating_point() or y.is_floating_point():
        out = torch.zeros((num_bins, height, width), dtype=torch.int8, device=x.device)
        if N >= 2:      # fewer than 2 events: an empty grid (transformers.py:151-152)
            xf, yf = x.to(torch.float32).contiguous(), y.to(torch.float32).contiguous()
            ws, nbytes = sized_workspace("ramp_event_warp_workspace_bytes", (1, num_bins, height, width), x.device, "evwarp")
            status = torch.empty(8, dtype=torch.int32, device=x.device)
            check(lib().ramp_event_warp(ptr(xf), ptr(yf), None, ptr(pi), N, None, None, 1, 0.0, None, None,
                                        _lib.RAMP_WARP_IDENTITY, num_bins, height, width, None, None, None, ptr(out),
                                        ptr(ws), nbytes, ptr(status), stream()), "ramp_event_warp")
        return out.float() if as_float else out
    xi, yi = x.to(torch.int32).contiguous(), y.to(torch.int32).contiguous()
    out = torch.empty((num_bins, height, width), dtype=torch.float32 if as_float else torch.int8, device=x.device)
    ws, nbytes = sized_workspace("ramp_event_stack_workspace_bytes", (num_bins, height, width), x.device, "evstack")
    check(lib().ramp_event_stack(ptr(xi), ptr(yi), ptr(pi), N, num_bins, height, width,
                                 None if as_float else ptr(out), ptr(out) if as_float else None, ptr(ws), nbytes,
                                 stream()), "ramp_event_stack")
    return out


def _events(x, y, t, p):
    """an event list as the kernels take it -> (xf, yf, tf, pi): fp32, fp32, float64, int8 with 0 read as -1 (``p=None``: no
    polarity, ``pi`` None)"""
    xf, yf = x.reshape(-1).to(torch.float32).contiguous(), y.reshape(-1).to(torch.float32).contiguous()
    tf = t.reshape(-1).to(torch.float64).contiguous()
    if p is None:
        return xf, yf, tf, None
    pi = p.reshape(-1).to(torch.int8)
    return xf, yf, tf, torch.where(pi == 0, torch.full_like(pi, -1), pi).contiguous()


def _same_length(name, which, N, *lists):
    """raises in the entry's own words (``which``: the lists it names) unless every list given holds N events"""
    if any(v is not None and v.shape[0] != N for v in lists):
        raise RuntimeError("%s: %s differ in length" % (name, which))


def _event_arguments(name, x, y, t, p, knots, times, intrinsics, invdepth, height, width, extrapolate, which="x, y, t and p"):
    """the argument handling of ``event_warp``, for the entries that take its arguments -> (xf, yf, tf, pi, knots, times,
    K, d, flags); ``p=None``: no polarity, ``invdepth=None``: no inverse depth (``pi``, ``d`` None)"""
    require_cuda(x, y, t, p, knots, times)
    dev = x.device
    xf, yf, tf, pi = _events(x, y, t, p)
    knots = knots.reshape(-1, 7).contiguous().float()
    times = times.reshape(-1).contiguous().double()
    T = knots.shape[0]
    if times.shape[0] != T:
        raise RuntimeError("%s: %d knots but %d time stamps" % (name, T, times.shape[0]))
    _same_length(name, which, x.shape[0], yf, tf, pi)
    K = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev).reshape(4).contiguous()
    flags = _lib.RAMP_INTERP_EXTRAPOLATE if extrapolate else 0
    if invdepth is None:
        d = None
    elif isinstance(invdepth, torch.Tensor) and invdepth.numel() != 1:
        if tuple(invdepth.shape) != (height, width):
            raise RuntimeError("%s: an inverse depth map is [height, width]" % name)
        require_cuda(invdepth)
        d = invdepth.to(torch.float32).contiguous()
        flags |= _lib.RAMP_WARP_DEPTH_MAP
    elif isinstance(invdepth, torch.Tensor):
        require_cuda(invdepth)
        d = invdepth.reshape(1).to(torch.float32).contiguous()
    else:
        d = torch.full((1,), float(invdepth), dtype=torch.float32, device=dev)
    return xf, yf, tf, pi, knots, times, K, d, flags


def _correction(name, correction, dev):
    """``correction`` of ``event_contrast`` / ``event_align`` as the kernels read it: None, or float32 [7] on the device"""
    if correction is None:
        return None
    cor = torch.as_tensor(correction, dtype=torch.float32, device=dev).reshape(-1).contiguous()
    if cor.numel() != 7:
        raise RuntimeError("%s: a correction is (v[3], w[3], lam): 7 numbers" % name)
    return cor


def event_warp(x, y, t, p, knots, times, t_ref, intrinsics, invdepth, height, width, num_bins=0, extrapolate=False,
               want_xy=False, want_iwe=True, stack=None):
    """Motion compensation of an event list (include/ramp_hip.h ``ramp_event_warp``): every event is warped from the camera
    pose at its own time stamp to the pose at ``t_ref`` and splat bilinearly, in one pass over the events.

    ``x, y`` [N] pixel coordinates (fractions allowed), ``t`` [N] float64, ``p`` [N] polarity (+-1; 0 is read as -1);
    ``knots`` [T,7] CAMERA-TO-WORLD with ``times`` [T] float64, as ``Ramp_vo.trajectory()`` returns them; ``intrinsics`` [4]
    (fx, fy, cx, cy); ``invdepth`` a float, a 0-d / 1-element device tensor, or an [height, width] map (sampled at the
    event's rounded pixel); 0 compensates the rotation alone.  Device tensors, ordered on the current stream, nothing
    synchronised.

    Returns a dict: ``status`` int32 [8] (``event_warp_status``) and, as requested, ``xy`` [N,2] (NaN rows for invalid
    events), ``iwe`` [2,height,width] (polarity-signed sum, unsigned count), ``stack`` [num_bins,height,width] float32
    (``stack="f32"``) or int8 (``"i8"``).  The sums are fixed point over integer atomics: the same bits for any order of
    the events."""
    if stack not in (None, "f32", "i8"):
        raise RuntimeError("event_warp: stack is 'f32', 'i8' or None")
    if stack is not None and num_bins < 1:
        raise RuntimeError("event_warp: a stack needs num_bins >= 1")
    xf, yf, tf, pi, knots, times, K, d, flags = _event_arguments("event_warp", x, y, t, p, knots, times, intrinsics, invdepth,
                                                                 height, width, extrapolate)
    dev, N, T = xf.device, x.shape[0], knots.shape[0]
    bins = num_bins if stack is not None else 1
    res = {"status": torch.zeros(8, dtype=torch.int32, device=dev)}
    if want_xy:
        res["xy"] = torch.empty((N, 2), dtype=torch.float32, device=dev)
    if want_iwe:
        res["iwe"] = torch.zeros((2, height, width), dtype=torch.float32, device=dev)
    if stack is not None:
        res["stack"] = torch.zeros((num_bins, height, width), dtype=torch.float32 if stack == "f32" else torch.int8, device=dev)
    if N == 0:
        return res
    ws, nbytes = sized_workspace("ramp_event_warp_workspace_bytes", (T, bins, height, width), dev, "evwarp")
    check(lib().ramp_event_warp(ptr(xf), ptr(yf), ptr(tf), ptr(pi), N, ptr(knots), ptr(times), T, float(t_ref), ptr(K), ptr(d),
                                flags, bins, height, width, ptr(res.get("xy")), ptr(res.get("iwe")),
                                ptr(res["stack"]) if stack == "f32" else None, ptr(res["stack"]) if stack == "i8" else None,
                                ptr(ws), nbytes, ptr(res["status"]), stream()), "ramp_event_warp")
    return res


def event_warp_status(status):
    """The status words of ``event_warp`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_warp", status)


def event_dsi(x, y, t, knots, times, t_ref, intrinsics, height, width, planes=64, range=(0.05, 2.0), min_votes=4.0,
              adaptive_radius=0, adaptive_offset=0.0, fill=None, extrapolate=False, want_coords=False):
    """Depth from a plane sweep of an event list (include/ramp_hip.h ``ramp_event_dsi``; EMVS, Rebecq et al. 2018): every
    event is back-projected from the camera pose at its own time stamp and swept through ``planes`` planes of constant inverse
    depth of the camera at ``t_ref``, each plane taking ``event_warp``'s bilinear splat; per pixel the plane with the most
    votes (the lowest on a tie), refined by a parabola, is the inverse depth -- at the pixels where events fire.

    ``x, y, t, knots, times, t_ref, intrinsics`` as ``event_warp`` (no polarity).  ``range``: ``(d_lo, d_hi)`` inverse depths,
    a pair of numbers or a device tensor [2] the host never reads; the planes are uniform in inverse depth.  A pixel is
    detected when its best plane holds ``min_votes`` votes and, with ``adaptive_radius`` r in 1 .. 15, at least the mean of
    the best votes over its (2r + 1)^2 window (clipped to the image) plus ``adaptive_offset``.  ``fill``: what an undetected
    pixel's ``invdepth`` gets -- None (NaN), a number or a one-element device tensor.  The defaults of ``planes``, ``range`` and
    ``min_votes`` are defaults nobody has tuned.  Device tensors, ordered on the current stream, nothing synchronised.

    Returns a dict of device tensors: ``dsi`` int64 [planes, height, width] (votes in fixed point, 2^24 per event and plane),
    ``invdepth`` and ``confidence`` (= best votes) [height, width] float32, ``plane`` int32 (-1: not detected), ``status``
    int32 [8] (``event_dsi_status``) and, with ``want_coords``, ``coords`` [N, planes, 2] (NaN where a plane got no vote;
    N x planes x 8 bytes: for tests and small calls).  ``invdepth`` goes straight into ``event_warp(invdepth=...)``.  The
    votes are integers: the same bits for any order of the events.  Time stamps of the knots that decrease, or a range that is
    not finite, negative or empty: NaN / -1 / zero outputs, never a plausible number."""
    dev, N = x.device, x.numel()
    T, D, H, W = knots.numel() // 7, int(planes), int(height), int(width)
    if times.numel() != T:
        raise RuntimeError("event_dsi: %d knots but %d time stamps" % (T, times.numel()))
    if not (y.numel() == N and t.numel() == N):
        raise RuntimeError("event_dsi: x, y and t differ in length")
    if T < 1 or D < 1 or H < 1 or W < 1:
        raise RuntimeError("event_dsi: at least one knot, one plane and one pixel")
    if not 0 <= int(adaptive_radius) <= 15:
        raise RuntimeError("event_dsi: adaptive_radius is 0 .. 15")
    if D * H * W >= 1 << 31 or N * D >= 1 << 38:
        raise RuntimeError("event_dsi: planes x height x width is below 2^31 and events x planes below 2^38")
    xf, yf, tf, _, knots, times, K, _, flags = _event_arguments("event_dsi", x, y, t, None, knots, times, intrinsics, None, H, W,
                                                                extrapolate, which="x, y and t")

    def word(name, v, n):
        if isinstance(v, torch.Tensor):
            require_cuda(v)
            v = v.reshape(-1).to(torch.float32).contiguous()
        else:
            v = torch.tensor([float(u) for u in (v if n > 1 else [v])], dtype=torch.float32, device=dev)
        if v.numel() != n:
            raise RuntimeError("event_dsi: %s holds %d number%s" % (name, n, "s" if n > 1 else ""))
        return v

    rng = word("range", range, 2)
    fl = None if fill is None else word("fill", fill, 1)
    res = {"status": torch.empty(8, dtype=torch.int32, device=dev),
           "dsi": torch.empty((D, H, W), dtype=torch.int64, device=dev),
           "invdepth": torch.empty((H, W), dtype=torch.float32, device=dev),
           "confidence": torch.empty((H, W), dtype=torch.float32, device=dev),
           "plane": torch.empty((H, W), dtype=torch.int32, device=dev)}
    if want_coords:
        res["coords"] = torch.empty((N, D, 2), dtype=torch.float32, device=dev)
    ws, nbytes = sized_workspace("ramp_event_dsi_ws_bytes", (T, H, W), dev, "evdsi")
    check(lib().ramp_event_dsi(ptr(xf), ptr(yf), ptr(tf), N, ptr(knots), ptr(times), T, float(t_ref), ptr(K), ptr(rng),
                               flags, D, H, W, float(min_votes),
                               int(adaptive_radius), float(adaptive_offset), ptr(fl), ptr(res["dsi"]), ptr(res.get("coords")),
                               ptr(res["invdepth"]), ptr(res["confidence"]), ptr(res["plane"]), ptr(ws), nbytes,
                               ptr(res["status"]), stream()), "ramp_event_dsi")
    return res


def event_dsi_status(status):
    """The status words of ``event_dsi`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_dsi", status)


def depth_points(invdepth, cam, intrinsics, plane=None, confidence=None, median_radius=2, min_support=3, min_invdepth=0.0,
                 want_filtered=False):
    """A semi-dense inverse depth map, cleaned and lifted to world points (include/ramp_hip.h ``ramp_depth_points``; what EMVS
    does behind its detection).  ``invdepth`` [H, W]; ``plane`` [H, W] int32: a pixel is detected when ``plane >= 0`` (None:
    when ``invdepth`` is finite and positive); ``confidence`` [H, W] (None: 1) -- the ``invdepth``, ``plane`` and ``confidence``
    of ``event_dsi`` as they are.  ``cam`` [7]: the CAMERA-TO-WORLD pose of the view, a row of ``trajectory()`` / ``poses_at()``;
    ``intrinsics`` (fx, fy, cx, cy) at the map's resolution.

    Per detected pixel: the LOWER median of the detected inverse depths of the (2 ``median_radius`` + 1)^2 window clipped to
    the image (``median_radius`` 0 .. 3; 0: the pixel's own value); fewer than ``min_support`` detected pixels in the window
    (the pixel itself counts): dropped as isolated.  A filtered value that is not finite, not positive or below
    ``min_invdepth``, or a world point that is not finite, is dropped as well.  The defaults are defaults nobody has tuned.

    Returns a dict of device tensors, nothing synchronised: ``points`` [H*W, 3], ``conf`` [H*W] and ``pixel`` [H*W] int32 (v * W
    + u) of which the first ``count`` rows (int32 [1], ascending pixel index) are written, ``status`` int32 [8]
    (``depth_points_status``) and, with ``want_filtered``, ``invdepth_filtered`` [H, W] (NaN where nothing was lifted).  A
    ``cam`` or intrinsics that are not finite: ``count`` 0 and bit 0 of the status, never a plausible point."""
    if invdepth.dim() != 2:
        raise RuntimeError("depth_points: invdepth is [height, width]")
    H, W = (int(v) for v in invdepth.shape)
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise RuntimeError("depth_points: at least one pixel and fewer than 2^31")
    for name, m in (("plane", plane), ("confidence", confidence)):
        if m is not None and tuple(m.shape) != (H, W):
            raise RuntimeError("depth_points: %s has the shape of invdepth" % name)
    if not 0 <= int(median_radius) <= 3:
        raise RuntimeError("depth_points: median_radius is 0 .. 3")
    if int(min_support) < 1:
        raise RuntimeError("depth_points: min_support is at least 1")
    if not 0.0 <= float(min_invdepth) < float("inf"):
        raise RuntimeError("depth_points: min_invdepth is finite and not negative")
    if cam.numel() != 7:
        raise RuntimeError("depth_points: cam holds 7 numbers (t, q), camera to world")
    require_cuda(invdepth, cam, plane, confidence)
    dev = invdepth.device
    inv = invdepth.to(torch.float32).contiguous()
    pl = None if plane is None else plane.to(torch.int32).contiguous()
    cf = None if confidence is None else confidence.to(torch.float32).contiguous()
    camf = cam.reshape(7).to(torch.float32).contiguous()
    K = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev).reshape(4).contiguous()
    res = {"points": torch.empty((H * W, 3), dtype=torch.float32, device=dev),
           "conf": torch.empty(H * W, dtype=torch.float32, device=dev),
           "pixel": torch.empty(H * W, dtype=torch.int32, device=dev),
           "count": torch.empty(1, dtype=torch.int32, device=dev),
           "status": torch.empty(8, dtype=torch.int32, device=dev)}
    if want_filtered:
        res["invdepth_filtered"] = torch.empty((H, W), dtype=torch.float32, device=dev)
    ws, nbytes = sized_workspace("ramp_depth_points_ws_bytes", (H, W), dev, "evpts")
    check(lib().ramp_depth_points(ptr(inv), ptr(pl), ptr(cf), ptr(camf), ptr(K), H, W, int(median_radius), int(min_support),
                                  float(min_invdepth), ptr(res["points"]), ptr(res["conf"]), ptr(res["pixel"]),
                                  ptr(res.get("invdepth_filtered")), ptr(res["count"]), ptr(ws), nbytes, ptr(res["status"]),
                                  stream()), "ramp_depth_points")
    return res


def depth_points_status(status):
    """The status words of ``depth_points`` as a dict: the bit of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("depth_points", status)


class PointMap:
    """A persistent map of world points: a voxel hash table on the device (include/ramp_hip.h ``ramp_point_map_*``).  Every
    voxel of edge ``voxel`` that has received a point holds the number of its points, the sum of their positions inside the
    voxel in fixed point (2^-20 voxel), the sum of their confidences (2^-16) and a mask of the views that saw it; ``export``
    returns the mean point of every voxel, sorted by voxel.  All sums are 64-bit integers: the map does not depend on the
    order of the points or on how they are split over calls, and repeats its bits.

    ``capacity``: the slots, a power of two in 2^3 .. 2^30 (64 bytes each).  The table never grows: points whose voxel finds
    no slot are counted (``n_dropped_full``) and dropped -- keep it at most half full.  Coordinates reach +-2^20 voxels from
    the origin; points beyond are counted and dropped."""

    def __init__(self, voxel, capacity=2 ** 20, device="cuda"):
        voxel, capacity = float(voxel), int(capacity)
        if not 0.0 < voxel < float("inf"):
            raise RuntimeError("PointMap: voxel is finite and positive")
        if not (8 <= capacity <= 1 << 30 and capacity & (capacity - 1) == 0):
            raise RuntimeError("PointMap: capacity is a power of two in 2^3 .. 2^30")
        self.voxel, self.capacity, self.device = voxel, capacity, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rampvo_amd operators run on the GPU only (got device %s); there is no CPU fallback" % self.device)
        self.buf = torch.empty(lib().ramp_point_map_bytes(capacity), dtype=torch.uint8, device=self.device)
        self.clear()

    def clear(self):
        """empty the map (one launch on the current stream)"""
        check(lib().ramp_point_map_clear(ptr(self.buf), self.capacity, stream()), "ramp_point_map_clear")

    def insert(self, points, conf=None, count=None, view=0):
        """``points`` [N, 3] (``conf`` [N], None: 1) into the map; ``count``: a device int32 word, the rows that are live
        (``depth_points``' ``count``), read on the device; ``view`` >= 0: the id of the reference view the points come from
        (ids wrap at 64 in the mask of views).  Returns the device status words (``point_map_status``); nothing synchronised."""
        if points.dim() != 2 or points.shape[1] != 3:
            raise RuntimeError("PointMap.insert: points is [N, 3]")
        N = int(points.shape[0])
        if conf is not None and conf.numel() != N:
            raise RuntimeError("PointMap.insert: conf holds one number per point")
        if count is not None and (count.dtype != torch.int32 or count.numel() != 1):
            raise RuntimeError("PointMap.insert: count is one int32 word on the device")
        if int(view) < 0:
            raise RuntimeError("PointMap.insert: view is not negative")
        require_cuda(points, conf, count)
        pts = points.to(torch.float32).contiguous()
        cf = None if conf is None else conf.reshape(-1).to(torch.float32).contiguous()
        status = torch.empty(8, dtype=torch.int32, device=self.device)
        check(lib().ramp_point_map_insert(ptr(self.buf), self.capacity, ptr(pts) if N else None, ptr(cf), N, ptr(count),
                                          self.voxel, int(view), ptr(status), stream()), "ramp_point_map_insert")
        return status

    def export(self, min_points=1, min_views=1, max_out=None):
        """The voxels with at least ``min_points`` points seen from at least ``min_views`` views (of 64: view ids wrap), sorted
        by key, at most ``max_out`` of them (None: all).  Returns a dict of device tensors, nothing synchronised: ``points``
        [R, 3], ``n`` [R] int32, ``conf`` [R] (the summed confidence), ``n_views`` [R] int32, ``key`` [R] int64 with R =
        min(max_out, capacity) rows of which the first ``count`` (int32 [1]) are written, and ``status`` int32 [8]
        (``point_map_export_status``)."""
        if int(min_points) < 0 or int(min_views) < 0 or (max_out is not None and int(max_out) < 0):
            raise RuntimeError("PointMap.export: min_points, min_views and max_out are not negative")
        R = self.capacity if max_out is None else min(int(max_out), self.capacity)
        dev = self.device
        res = {"points": torch.empty((R, 3), dtype=torch.float32, device=dev), "n": torch.empty(R, dtype=torch.int32, device=dev),
               "conf": torch.empty(R, dtype=torch.float32, device=dev), "n_views": torch.empty(R, dtype=torch.int32, device=dev),
               "key": torch.empty(R, dtype=torch.int64, device=dev), "count": torch.empty(1, dtype=torch.int32, device=dev),
               "status": torch.empty(8, dtype=torch.int32, device=dev)}
        ws, nbytes = sized_workspace("ramp_point_map_export_ws_bytes", (self.capacity,), dev, "evmap")
        p = lambda k: ptr(res[k]) if R else None
        check(lib().ramp_point_map_export(ptr(self.buf), self.capacity, self.voxel, int(min_points), int(min_views), R,
                                          p("points"), p("n"), p("conf"), p("n_views"), p("key"), ptr(res["count"]), ptr(ws),
                                          nbytes, ptr(res["status"]), stream()), "ramp_point_map_export")
        return res

    def render(self, cam, intrinsics, height, width, radius=2, footprint=True, min_points=1, min_views=1, fill=None,
               want_key=True, want_n=True, want_conf=True, want_records=False):
        """The map as a camera sees it: a z-buffered [height, width] map of inverse depth (include/ramp_hip.h
        ``ramp_point_map_render``), the map ``event_warp`` samples at an event's pixel.  ``cam`` [7]: the CAMERA-TO-WORLD pose, a
        row of ``trajectory()`` / ``poses_at()``; ``intrinsics`` (fx, fy, cx, cy) at the image's resolution.  Every voxel with at
        least ``min_points`` points from at least ``min_views`` views (``export``'s conditions) is projected with ``export``'s
        mean point and covers the square of radius r_p around its pixel: ``radius`` (0 .. 7) with ``footprint=False``, else half
        the voxel's projected edge, at most ``radius``.  Per pixel the largest inverse depth wins, among equal ones the lowest
        key.  ``fill``: what a pixel no voxel covers gets -- None (NaN), a number, or a one-element device tensor the host never
        reads.  ``radius`` and the footprint rule are defaults nobody has tuned.

        Returns a dict of device tensors, nothing synchronised: ``invdepth`` [H, W], ``status`` int32 [8]
        (``point_map_render_status``) and, as requested, ``key`` [H, W] int64 (-1: nothing rendered), ``n`` [H, W] int32,
        ``conf`` [H, W], ``records`` [capacity, 4] (u, v, inverse depth, r_p per slot that is rendered or outside the image, NaN
        rows else).  A ``cam`` or intrinsics that are not finite: NaN everywhere and bit 0 of the status, never a plausible
        depth."""
        H, W = int(height), int(width)
        if H < 1 or W < 1 or H * W >= 1 << 31:
            raise RuntimeError("PointMap.render: at least one pixel and fewer than 2^31")
        if not 0 <= int(radius) <= 7:
            raise RuntimeError("PointMap.render: radius is 0 .. 7")
        if int(min_points) < 0 or int(min_views) < 0:
            raise RuntimeError("PointMap.render: min_points and min_views are not negative")
        if not isinstance(cam, torch.Tensor) or cam.numel() != 7:
            raise RuntimeError("PointMap.render: cam is a tensor of 7 numbers (t, q), camera to world")
        if isinstance(fill, torch.Tensor) and fill.numel() != 1:
            raise RuntimeError("PointMap.render: fill is None, a number or a one-element device tensor")
        require_cuda(cam, fill if isinstance(fill, torch.Tensor) else None)
        dev = self.device
        camf = cam.reshape(7).to(torch.float32).contiguous()
        K = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev).reshape(4).contiguous()
        if fill is not None:
            fill = (fill.reshape(1).to(torch.float32) if isinstance(fill, torch.Tensor)
                    else torch.full((1,), float(fill), dtype=torch.float32, device=dev))
        res = {"invdepth": torch.empty((H, W), dtype=torch.float32, device=dev), "status": torch.empty(8, dtype=torch.int32, device=dev)}
        for name, want, shape, dtype in (("key", want_key, (H, W), torch.int64), ("n", want_n, (H, W), torch.int32),
                                         ("conf", want_conf, (H, W), torch.float32),
                                         ("records", want_records, (self.capacity, 4), torch.float32)):
            if want:
                res[name] = torch.empty(shape, dtype=dtype, device=dev)
        ws, nbytes = sized_workspace("ramp_point_map_render_ws_bytes", (H, W), dev, "evrender")
        check(lib().ramp_point_map_render(ptr(self.buf), self.capacity, self.voxel, int(min_points), int(min_views), ptr(camf), ptr(K),
                                          H, W, int(radius), 1 if footprint else 0, ptr(fill), ptr(res["invdepth"]), ptr(res.get("key")),
                                          ptr(res.get("n")), ptr(res.get("conf")), ptr(res.get("records")), ptr(ws), nbytes,
                                          ptr(res["status"]), stream()), "ramp_point_map_render")
        return res

    def _localize_arguments(self, name, surface, cam, intrinsics, min_points, min_views, huber):
        """the checks both localisation entries share -> (surface, cam, intrinsics, H, W) as the kernels take them"""
        if not isinstance(surface, torch.Tensor) or surface.dim() != 2 or surface.shape[0] < 2 or surface.shape[1] < 2:
            raise RuntimeError("PointMap.%s: surface is a tensor [H, W] of at least 2 x 2 pixels (ops.time_surface)" % name)
        H, W = int(surface.shape[0]), int(surface.shape[1])
        if H * W >= 1 << 31:
            raise RuntimeError("PointMap.%s: fewer than 2^31 pixels" % name)
        if int(min_points) < 0 or int(min_views) < 0:
            raise RuntimeError("PointMap.%s: min_points and min_views are not negative" % name)
        if not isinstance(cam, torch.Tensor) or cam.numel() != 7:
            raise RuntimeError("PointMap.%s: cam is a tensor of 7 numbers (t, q), camera to world" % name)
        if huber != huber:
            raise RuntimeError("PointMap.%s: huber is a number (<= 0: off)" % name)
        require_cuda(surface, cam)
        return (surface.to(torch.float32).contiguous(), cam.reshape(7).to(torch.float32).contiguous(),
                torch.as_tensor(intrinsics, dtype=torch.float32, device=self.device).reshape(4).contiguous(), H, W)

    def localize_eval(self, surface, cam, intrinsics, min_points=1, min_views=1, huber=0.0, want_records=False):
        """One evaluation of the alignment of the map with a negative time surface (include/ramp_hip.h
        ``ramp_point_map_localize_eval``): every voxel ``render`` would project -- the same conditions, the same u, v in every bit
        -- samples ``surface`` [H, W] (``time_surface``) bilinearly at the CAMERA-TO-WORLD pose ``cam`` [7]; the sample is its
        residual, and a voxel that leaves the image keeps the residual 1.  ``huber``: the threshold of the robust weight (<= 0: off).

        Returns a dict of device tensors, nothing synchronised: ``sums`` float64 [32] and its views ``cost`` (0-d), ``hessian``
        [6, 6] (the Gauss-Newton matrix, symmetric), ``gradient`` [6] -- for the left perturbation of the world-to-camera pose,
        translation then rotation -- and ``in_reach`` (0-d); ``status`` int32 [8] (``point_map_localize_status``); ``records``
        [capacity, 8] (u, v, r, gu, gv, Xc per slot; None unless ``want_records``).  A ``cam`` or intrinsics that are not
        finite: NaN everywhere and bit 0 of the status."""
        S, camf, K, H, W = self._localize_arguments("localize_eval", surface, cam, intrinsics, min_points, min_views, huber)
        dev = self.device
        res = {"sums": torch.empty(32, dtype=torch.float64, device=dev), "status": torch.empty(8, dtype=torch.int32, device=dev),
               "records": torch.empty((self.capacity, 8), dtype=torch.float32, device=dev) if want_records else None}
        ws, nbytes = sized_workspace("ramp_point_map_localize_ws_bytes", (self.capacity, 0), dev, "evlocalize")
        check(lib().ramp_point_map_localize_eval(ptr(self.buf), self.capacity, self.voxel, int(min_points), int(min_views), ptr(camf),
                                                 ptr(K), ptr(S), H, W, float(huber), ptr(res["sums"]), ptr(res["records"]), ptr(ws),
                                                 nbytes, ptr(res["status"]), stream()), "ramp_point_map_localize_eval")
        iu = torch.triu_indices(6, 6, device=dev)
        hess = torch.zeros((6, 6), dtype=torch.float64, device=dev)
        hess[iu[0], iu[1]] = res["sums"][:21]
        hess[iu[1], iu[0]] = res["sums"][:21]
        res.update(cost=res["sums"][27], hessian=hess, gradient=res["sums"][21:27], in_reach=res["sums"][28])
        return res

    def localize(self, surface, cam, intrinsics, min_points=1, min_views=1, huber=0.0, lambda0=1e-3, min_step=1e-6, iters=10,
                 max_evals=None):
        """Where is the camera in this map?  Levenberg-Marquardt over ``localize_eval`` from the start ``cam``, entirely on the
        device (include/ramp_hip.h ``ramp_point_map_localize``: the state machine is written out there): one C call enqueues the
        whole solve, ordered on the current stream, nothing is read back and nothing synchronised.  At most ``iters`` accepted
        steps and ``max_evals`` evaluations (None: ``1 + 9 * iters``); evaluations behind the end of the solve are empty
        launches, which still cost their enqueue.  ``lambda0`` (the first damping), its factors of 10, the 8 rejections that give
        a step up and ``min_step`` (the length of a step that counts as converged) are values nobody has tuned.

        Returns a dict of device tensors: ``pose`` float64 [7] (camera to world), ``pose_f32`` float32 [7] (the bits the
        evaluation at ``pose`` read: pass it to ``localize_eval`` / ``render``), ``cost`` and ``cost0`` (0-d views of ``result``
        float64 [4]: cost, cost0, the final lambda, the voxels in reach), ``hessian`` [6, 6] and ``gradient`` [6] at ``pose``,
        ``history`` float64 [iters] (the accepted costs, NaN behind them), ``status`` int32 [8] (the words of the evaluation
        at ``pose``) and ``info`` int32 [8] (``point_map_localize_info``).  The pose is NaN in every word when fewer than 6
        voxels are in reach at the start, when the first system is singular, or when a camera was not finite."""
        S, camf, K, H, W = self._localize_arguments("localize", surface, cam, intrinsics, min_points, min_views, huber)
        iters = int(iters)
        if iters < 0 or iters > _lib.RAMP_LOCALIZE_MAX_ITERS:
            raise RuntimeError("PointMap.localize: iters is 0 .. %d" % _lib.RAMP_LOCALIZE_MAX_ITERS)
        if not (0.0 <= float(lambda0) < float("inf") and 0.0 <= float(min_step) < float("inf")):
            raise RuntimeError("PointMap.localize: lambda0 and min_step are finite and not negative")
        if max_evals is not None and int(max_evals) < 1:
            raise RuntimeError("PointMap.localize: max_evals is at least 1")
        dev = self.device
        res = {"pose": torch.zeros(7, dtype=torch.float64, device=dev), "pose_f32": torch.zeros(7, dtype=torch.float32, device=dev),
               "result": torch.zeros(4, dtype=torch.float64, device=dev), "hessian": torch.zeros((6, 6), dtype=torch.float64, device=dev),
               "gradient": torch.zeros(6, dtype=torch.float64, device=dev), "history": torch.zeros(iters, dtype=torch.float64, device=dev),
               "status": torch.zeros(8, dtype=torch.int32, device=dev), "info": torch.zeros(8, dtype=torch.int32, device=dev)}
        res["cost"], res["cost0"] = res["result"][0], res["result"][1]
        ws, nbytes = sized_workspace("ramp_point_map_localize_ws_bytes", (self.capacity, iters), dev, "evlocalize")
        check(lib().ramp_point_map_localize(ptr(self.buf), self.capacity, self.voxel, int(min_points), int(min_views), ptr(camf), ptr(K),
                                            ptr(S), H, W, float(huber), float(lambda0), float(min_step), iters,
                                            0 if max_evals is None else int(max_evals), ptr(res["pose"]), ptr(res["pose_f32"]),
                                            ptr(res["result"]), ptr(res["hessian"]), ptr(res["gradient"]),
                                            ptr(res["history"]) if iters else None, ptr(res["status"]), ptr(res["info"]), ptr(ws), nbytes,
                                            stream()), "ramp_point_map_localize")
        return res


LOCALIZE_REASONS = {0: "running", _lib.RAMP_LOCALIZE_ITERS: "iters", _lib.RAMP_LOCALIZE_CONVERGED: "converged",
                    _lib.RAMP_LOCALIZE_STALLED: "stalled", _lib.RAMP_LOCALIZE_SINGULAR: "singular", _lib.RAMP_LOCALIZE_FEW: "few",
                    _lib.RAMP_LOCALIZE_BUDGET: "budget"}


def point_map_localize_status(status):
    """The status words of ``PointMap.localize_eval`` / ``localize`` as a dict: the bit of word 0 by name, then the counters
    (synchronises: one small copy)."""
    return _status("point_map_localize", status)


def point_map_localize_info(info):
    """the info words of ``PointMap.localize`` as a dict (synchronises: one 32-byte copy); ``reason``: ``iters`` (the accepted
    steps asked for), ``converged`` (a step shorter than ``min_step``), ``stalled`` (8 rejections in a row), ``singular`` (the
    damped system has no Cholesky factor), ``few`` (fewer than 6 voxels in reach) or ``budget`` (``max_evals`` ran out)"""
    w = info.detach().cpu()
    return dict(reason=LOCALIZE_REASONS.get(int(w[0]), "unknown"), n_accepted=int(w[1]), n_evals=int(w[2]), rejects=int(w[3]),
                seen=int(w[4]), bad_camera=bool(int(w[4]) & _lib.RAMP_MAP_LOCALIZE_BAD_CAMERA))


def time_surface(x, y, t, t_ref, tau, height, width, smooth=2, last_t=None, negate=True, want_raw=False, want_last_t=False):
    """The time surface of an event list (include/ramp_hip.h ``ramp_time_surface``): per pixel ``exp((last - t_ref) / tau)`` of
    the newest time stamp at or before ``t_ref`` (0 without one), ``negate``: one minus it -- near 0 where events fired just
    before ``t_ref``, 1 where none did, the field ``PointMap.localize`` samples --, smoothed by ``smooth`` (0 .. 8) passes of
    the 5-tap binomial.  ``x, y`` [N] (the pixel is the rounded coordinate), ``t`` [N] float64 in any order; ``last_t``: float64
    [height, width], time stamps from before these events (``event_filter``'s ``last_t`` as it is; NaN: none).  ``smooth=2`` is
    a default nobody has tuned.

    Returns a dict of device tensors, nothing synchronised: ``surface`` [H, W] float32, ``status`` int32 [8]
    (``time_surface_status``), ``raw`` (the surface in front of the smoothing; None unless ``want_raw``) and ``last_t`` (float64
    [H, W], NaN where no event; None unless ``want_last_t``).  A ``t_ref`` or ``tau`` that is not finite, or ``tau <= 0``: NaN
    everywhere and bit 0 of the status."""
    H, W = int(height), int(width)
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise RuntimeError("time_surface: at least one pixel and fewer than 2^31")
    if not 0 <= int(smooth) <= 8:
        raise RuntimeError("time_surface: smooth is 0 .. 8")
    require_cuda(x, y, t, last_t)
    dev = x.device
    xs, ys = x.reshape(-1).to(torch.float32).contiguous(), y.reshape(-1).to(torch.float32).contiguous()
    tf = t.reshape(-1).to(torch.float64).contiguous()
    N = xs.shape[0]
    if not (ys.shape[0] == N and tf.shape[0] == N):
        raise RuntimeError("time_surface: x, y and t differ in length")
    state = None
    if last_t is not None:
        if tuple(last_t.shape) != (H, W) or last_t.dtype != torch.float64:
            raise RuntimeError("time_surface: last_t is float64 [height, width] (event_filter's last_t)")
        state = last_t.contiguous()
    res = {"surface": torch.empty((H, W), dtype=torch.float32, device=dev), "status": torch.empty(8, dtype=torch.int32, device=dev),
           "raw": torch.empty((H, W), dtype=torch.float32, device=dev) if want_raw else None,
           "last_t": torch.empty((H, W), dtype=torch.float64, device=dev) if want_last_t else None}
    ws, nbytes = sized_workspace("ramp_time_surface_ws_bytes", (H, W), dev, "timesurface")
    check(lib().ramp_time_surface(ptr(xs) if N else None, ptr(ys) if N else None, ptr(tf) if N else None, N, ptr(state), float(t_ref),
                                  float(tau), H, W, int(smooth), _lib.RAMP_TIME_SURFACE_NEGATE if negate else 0, ptr(res["surface"]),
                                  ptr(res["raw"]), ptr(res["last_t"]), ptr(ws), nbytes, ptr(res["status"]), stream()),
          "ramp_time_surface")
    return res


def time_surface_status(status):
    """The status words of ``time_surface`` as a dict: the bit of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("time_surface", status)


def point_map_status(status):
    """The status words of ``PointMap.insert`` as a dict (synchronises: one small copy)."""
    return _status("point_map", status)


def point_map_export_status(status):
    """The status words of ``PointMap.export`` as a dict (synchronises: one small copy)."""
    return _status("point_map_export", status)


def point_map_render_status(status):
    """The status words of ``PointMap.render`` as a dict: the bit of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("point_map_render", status)


def event_contrast(x, y, t, p, knots, times, t_ref, intrinsics, invdepth, height, width, correction=None, signed=True,
                   extrapolate=False, want_grad=True, want_iwe=False):
    """The contrast of a motion-compensated event list and its gradient (include/ramp_hip.h ``ramp_event_contrast``): the
    population variance of the image of warped events ``event_warp`` would splat, and its derivative with respect to a small
    correction ``theta = (v[3], w[3], lam)`` -- translation 3, rotation 3, a log depth scale -- that acts in the reference
    camera frame: ``X2 = X1 + tau (v ds + w x X1)``, ``X1 = R_G P + t_G ds``, ``ds = d exp(lam)``, ``tau = t - t_ref``.

    The arguments up to ``width`` are ``event_warp``'s.  ``correction``: None (zero), a sequence of 7 numbers or a device
    tensor [7].  ``signed=False`` scores the count image instead of the polarity-signed one.  Device tensors, ordered on the
    current stream, nothing synchronised.

    Returns a dict of device tensors: ``variance`` (0-d float64 view of ``stats``), ``stats`` float64 [8] (variance, mean,
    sum of I^2, pixel count), ``sums`` int64 [2] (the exact fixed-point sums of the signed and the count accumulators),
    ``status`` int32 [8] (``event_warp_status``; bit 1 of word 0: a correction that is not finite) and, as requested, ``grad``
    float64 [7] and ``iwe`` [2,height,width].  ``stats``, ``sums`` and ``iwe`` are the same bits for any order of the events;
    ``grad`` repeats its bits from call to call.  Time stamps of the knots that decrease, or a correction that is not finite:
    NaN in ``stats``, ``grad`` and ``iwe``, never a plausible number."""
    xf, yf, tf, pi, knots, times, K, d, flags = _event_arguments("event_contrast", x, y, t, p, knots, times, intrinsics,
                                                                 invdepth, height, width, extrapolate)
    dev, N, T = xf.device, xf.shape[0], knots.shape[0]
    if not signed:
        flags |= _lib.RAMP_CONTRAST_UNSIGNED
    cor = _correction("event_contrast", correction, dev)
    res = {"stats": torch.zeros(8, dtype=torch.float64, device=dev), "sums": torch.zeros(2, dtype=torch.int64, device=dev),
           "status": torch.zeros(8, dtype=torch.int32, device=dev)}
    res["variance"] = res["stats"][0]
    if want_grad:
        res["grad"] = torch.zeros(7, dtype=torch.float64, device=dev)
    if want_iwe:
        res["iwe"] = torch.zeros((2, height, width), dtype=torch.float32, device=dev)
    if N == 0:
        res["stats"][3] = float(height * width)
        return res
    ws, nbytes = sized_workspace("ramp_event_contrast_workspace_bytes", (T, height, width), dev, "evcontrast")
    check(lib().ramp_event_contrast(ptr(xf), ptr(yf), ptr(tf), ptr(pi), N, ptr(knots), ptr(times), T, float(t_ref), ptr(K),
                                    ptr(d), ptr(cor), flags, height, width, ptr(res.get("iwe")), ptr(res["sums"]),
                                    ptr(res["stats"]), ptr(res.get("grad")), ptr(ws), nbytes, ptr(res["status"]), stream()),
          "ramp_event_contrast")
    return res


VOXEL_WORKSPACE_CAP = 256 << 20      # bytes: ramp_event_voxel works through more slices than this holds in chunks


def event_slices(n_events, count, device="cuda"):
    """the loader's slicing of an event file (reference evaluate.py:117-135): offsets ``0, count, 2 count, ...`` of the
    ``n_events // count`` full slices as a device int64 tensor -- the last partial slice is dropped, as upstream drops it"""
    if count < 1:
        raise RuntimeError("event_slices: count is positive")
    return torch.arange(0, (n_events // count) * count + 1, count, dtype=torch.int64, device=device)


def event_voxel_grid(x, y, t, p, height, width, num_bins=5, offsets=None, normalize=True, subpixel=False):
    """EventSequenceToVoxelGrid_Pytorch on the device (reference utils/transformers.py:21-125; include/ramp_hip.h
    ``ramp_event_voxel``), for many slices of an event list in one call: every event votes into the two time bins next to its
    normalised time stamp with linear weights, and with ``normalize`` each slice's grid is standardised over its non-zero
    cells (mean, unbiased std).

    ``x, y`` [N] pixel coordinates, ``t`` [N] float64, ``p`` [N] polarity (+-1; 0 is read as -1).  ``offsets``: None -- one
    slice, all events -- or a device int64 tensor [S + 1] (``event_slices``): slice s is the events ``[offsets[s],
    offsets[s + 1])``; the host never reads it.  The pixel is the coordinate truncated toward zero; ``subpixel=True`` splats
    bilinearly instead and skips NaN rows, so the ``xy`` of ``event_warp(want_xy=True)`` can be passed straight in
    (``x=xy[:, 0], y=xy[:, 1]``): a motion-compensated voxel grid.  Unlike the reference, an event outside the image is
    dropped and counted, and an empty slice gives an all-zero grid.

    Returns a dict of device tensors: ``grid`` [S, num_bins, height, width] float32 ([num_bins, height, width] when
    ``offsets`` is None -- the shape the net takes as ``events[None, None]``), ``stats`` float64 [S, 4] (per slice: the number
    of non-zero cells, their mean, their std, their sum) and ``status`` int32 [8] (``event_voxel_status``).  Runs on the
    current stream, nothing is synchronised.  The sums are fixed point over integer atomics: the same bits for any order of
    the events (the first and last of a slice define its time range) and any chunking.  Bad offsets make everything NaN, a
    slice whose first or last time stamp is not finite is NaN: never a plausible number."""
    require_cuda(x, y, t, p, offsets)
    dev = x.device
    xf, yf, tf, pi = _events(x, y, t, p)
    N = xf.shape[0]
    _same_length("event_voxel_grid", "x, y, t and p", N, yf, tf, pi)
    if num_bins < 1 or height < 1 or width < 1:
        raise RuntimeError("event_voxel_grid: num_bins, height and width are positive")
    if offsets is None:
        S, off = 1, None
    else:
        off = offsets.reshape(-1).to(torch.int64).contiguous()
        S = off.shape[0] - 1
        if S < 1:
            raise RuntimeError("event_voxel_grid: offsets holds at least two entries")
    flags = (_lib.RAMP_VOXEL_NORMALIZE if normalize else 0) | (_lib.RAMP_VOXEL_SUBPIXEL if subpixel else 0)
    grid = torch.empty((S, num_bins, height, width), dtype=torch.float32, device=dev)
    res = {"grid": grid if offsets is not None else grid[0], "stats": torch.empty((S, 4), dtype=torch.float64, device=dev),
           "status": torch.empty(8, dtype=torch.int32, device=dev)}
    one = lib().ramp_event_voxel_workspace_bytes(1, num_bins, height, width)
    nbytes = min(lib().ramp_event_voxel_workspace_bytes(S, num_bins, height, width), max(one, VOXEL_WORKSPACE_CAP))
    ws = _lib_workspace(nbytes, dev, "evvoxel")
    check(lib().ramp_event_voxel(ptr(xf), ptr(yf), ptr(tf), ptr(pi), N, ptr(off), S, num_bins, height, width, flags, ptr(grid),
                                 ptr(res["stats"]), ptr(res["status"]), ptr(ws), nbytes, stream()), "ramp_event_voxel")
    return res


def event_voxel_status(status):
    """The status words of ``event_voxel_grid`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_voxel", status)


CAMERA_MODELS = {"pinhole": _lib.RAMP_CAM_PINHOLE, "radtan": _lib.RAMP_CAM_RADTAN, "equidistant": _lib.RAMP_CAM_EQUIDISTANT}
_CAMERA_COEFFS = {_lib.RAMP_CAM_PINHOLE: (0,), _lib.RAMP_CAM_RADTAN: (4, 5), _lib.RAMP_CAM_EQUIDISTANT: (4,)}


def camera_words(model, raw_intrinsics, coeffs=(), rotation=None):
    """the host part of a camera record (include/ramp_hip.h, RAMP_CAMERA_*): a list of RAMP_CAMERA_WORDS floats with the
    rectified intrinsics left at the raw ones"""
    code = CAMERA_MODELS.get(model, model)
    if code not in _CAMERA_COEFFS:
        raise RuntimeError("camera: the model is 'pinhole', 'radtan' or 'equidistant' (got %r)" % (model,))
    k = [float(v) for v in coeffs]
    if code != _lib.RAMP_CAM_PINHOLE and len(k) not in _CAMERA_COEFFS[code]:
        raise RuntimeError("camera: radtan takes (k1, k2, p1, p2[, k3]), equidistant (k1, k2, k3, k4); got %d coefficients" % len(k))
    raw = [float(v) for v in raw_intrinsics]
    if len(raw) != 4:
        raise RuntimeError("camera: intrinsics are (fx, fy, cx, cy)")
    R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if rotation is not None:
        R = [float(v) for v in torch.as_tensor(rotation, dtype=torch.float64).reshape(-1).tolist()]
        if len(R) != 9:
            raise RuntimeError("camera: a rotation is 3 x 3")
    words = [0.0] * _lib.RAMP_CAMERA_WORDS
    words[_lib.RAMP_CAMERA_RAW:_lib.RAMP_CAMERA_RAW + 4] = raw
    words[_lib.RAMP_CAMERA_MODEL] = float(code)
    if code != _lib.RAMP_CAM_PINHOLE:
        words[_lib.RAMP_CAMERA_COEFFS:_lib.RAMP_CAMERA_COEFFS + len(k)] = k
    words[_lib.RAMP_CAMERA_ROTATION:_lib.RAMP_CAMERA_ROTATION + 9] = R
    words[_lib.RAMP_CAMERA_NEW:_lib.RAMP_CAMERA_NEW + 4] = raw
    return words


def camera(model, raw_intrinsics, coeffs=(), new_intrinsics=None, rotation=None, device="cuda"):
    """The device record of a distorting camera (include/ramp_hip.h, "lens distortion"): ``model`` 'pinhole', 'radtan'
    (``coeffs`` k1, k2, p1, p2[, k3]) or 'equidistant' (k1 .. k4: Kalibr's name for OpenCV's fisheye); ``raw_intrinsics``
    (fx, fy, cx, cy) of the sensor; ``rotation`` 3 x 3, raw camera to rectified camera (None: identity); ``new_intrinsics``
    of the rectified pinhole camera (None: the raw ones), a sequence or a DEVICE tensor [4], which is copied on the current
    stream and never read by the host.  Returns a float32 tensor [RAMP_CAMERA_WORDS]."""
    rec = torch.tensor(camera_words(model, raw_intrinsics, coeffs, rotation), dtype=torch.float32, device=device)
    if new_intrinsics is not None:
        rec[_lib.RAMP_CAMERA_NEW:_lib.RAMP_CAMERA_NEW + 4] = torch.as_tensor(new_intrinsics, dtype=torch.float32,
                                                                              device=rec.device).reshape(4)
    return rec


def _camera_record(name, camera, dev):
    require_cuda(camera)
    if camera.dtype != torch.float32 or camera.numel() != _lib.RAMP_CAMERA_WORDS or camera.device != dev:
        raise RuntimeError("%s: the camera is the float32 record ops.camera returns, on the device of the data" % name)
    return camera.reshape(-1).contiguous()


def event_rectify(x, y, camera, height, width, want_valid=False):
    """Raw sensor events to the rectified pinhole camera (include/ramp_hip.h ``ramp_event_rectify``): every event's pixel is
    normalised with the raw intrinsics, the distortion model is inverted with a fixed number of Newton steps, the ray is
    rotated and projected with the rectified intrinsics.  ``x, y`` [N]: integer tensors take the int32 path, floating ones
    fp32 (integer-valued floats give the same bits); ``camera``: ``ops.camera``; ``height, width``: the rectified image, for
    the inside / outside count only.  Device tensors on the current stream, nothing synchronised.

    Returns a dict: ``xy`` [N,2] float32 -- a NaN row for an event that is not finite, not invertible (the solution left the
    branch the model is monotone on, or did not converge to 2^-6 raw pixels) or behind the rectified camera; the format
    ``event_voxel_grid(subpixel=True)``, ``event_warp`` and ``event_contrast`` take -- ``status`` int32 [8]
    (``event_rectify_status``) and ``valid`` uint8 [N] (None unless ``want_valid``)."""
    require_cuda(x, y)
    dev = x.device
    cam = _camera_record("event_rectify", camera, dev)
    if height < 1 or width < 1:
        raise RuntimeError("event_rectify: height and width are positive")
    integer = not (x.is_floating_point() or y.is_floating_point())
    dt = torch.int32 if integer else torch.float32
    xs, ys = x.reshape(-1).to(dt).contiguous(), y.reshape(-1).to(dt).contiguous()
    N = xs.shape[0]
    if ys.shape[0] != N:
        raise RuntimeError("event_rectify: x and y differ in length")
    res = {"xy": torch.empty((N, 2), dtype=torch.float32, device=dev), "status": torch.zeros(8, dtype=torch.int32, device=dev),
           "valid": torch.empty(N, dtype=torch.uint8, device=dev) if want_valid else None}
    if N == 0:
        return res
    check(lib().ramp_event_rectify(ptr(xs), ptr(ys), N, ptr(cam), _lib.RAMP_RECTIFY_XY_I32 if integer else 0, height, width,
                                   ptr(res["xy"]), ptr(res["valid"]), ptr(res["status"]), stream()), "ramp_event_rectify")
    return res


def event_rectify_status(status):
    """The status words of ``event_rectify`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_rectify", status)


_RECTIFY_NORM = {None: _lib.RAMP_RECTIFY_NORM_NONE, "half": _lib.RAMP_RECTIFY_NORM_HALF, "unit": _lib.RAMP_RECTIFY_NORM_UNIT}


def image_rectify(image, camera, height, width, normalize=None, fill=0.0, want_map=False, want_mask=False):
    """A raw frame resampled into the rectified pinhole camera (include/ramp_hip.h ``ramp_image_rectify``): per output pixel
    the ray is rotated back, distorted in closed form and the source sampled bilinearly in fp32.  ``image`` [C,Hs,Ws] or
    [Hs,Ws], uint8 or float32; ``normalize``: None, ``"half"`` (``2 (v / 255) - 0.5``) or ``"unit"`` (``2 (v / 255) - 1``),
    the two branches of the reference's ``normalize_image``; a pixel whose ray is behind the camera, beyond the fold of the
    model or outside the source gets ``fill``.  Device tensors on the current stream, nothing synchronised.

    Returns a dict: ``image`` float32 [C,height,width] ([height,width] for a 2-D source), ``status`` int32 [8]
    (``image_rectify_status``), ``map`` [height,width,2] the source coordinates with NaN where nothing was sampled, and
    ``mask`` uint8 [height,width] (None unless requested)."""
    require_cuda(image)
    dev = image.device
    cam = _camera_record("image_rectify", camera, dev)
    if normalize not in _RECTIFY_NORM:
        raise RuntimeError("image_rectify: normalize is None, 'half' or 'unit'")
    if image.dim() not in (2, 3) or image.numel() == 0 or height < 1 or width < 1:
        raise RuntimeError("image_rectify: an image is [C,Hs,Ws] or [Hs,Ws], not empty; height and width are positive")
    u8 = image.dtype == torch.uint8
    src = (image if u8 else image.to(torch.float32)).contiguous()
    C = 1 if src.dim() == 2 else src.shape[0]
    Hs, Ws = src.shape[-2], src.shape[-1]
    out = torch.empty((C, height, width), dtype=torch.float32, device=dev)
    res = {"image": out if image.dim() == 3 else out[0], "status": torch.zeros(8, dtype=torch.int32, device=dev),
           "map": torch.empty((height, width, 2), dtype=torch.float32, device=dev) if want_map else None,
           "mask": torch.empty((height, width), dtype=torch.uint8, device=dev) if want_mask else None}
    check(lib().ramp_image_rectify(ptr(src), C, Hs, Ws, ptr(cam), _lib.RAMP_RECTIFY_SRC_U8 if u8 else 0, _RECTIFY_NORM[normalize],
                                   float(fill), height, width, ptr(out), ptr(res["map"]), ptr(res["mask"]), ptr(res["status"]),
                                   stream()), "ramp_image_rectify")
    return res


def image_rectify_status(status):
    """The status words of ``image_rectify`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("image_rectify", status)


def event_filter_state(height, width, device="cuda"):
    """the state of ``event_filter`` before the first event: float64 [height, width], all NaN"""
    return torch.full((height, width), float("nan"), dtype=torch.float64, device=device)


def event_filter(x, y, t, height, width, support_dt=None, refractory=0.0, hot_count=0, hot_sigma=0.0, hot_mask=None,
                 last_t=None, want_xy=True, want_index=False):
    """Event denoising on the device (include/ramp_hip.h ``ramp_event_filter``): a hot-pixel mask, a refractory period and the
    8-neighbour background-activity filter, order-independent and bit-exact -- on a time-sorted stream, event for event, the
    textbook sequential filter over a last-time-stamp map.

    ``x, y`` [N]: integer tensors take the int32 path, floating ones fp32 (integer-valued floats give the same bits); ``t`` [N]
    float64, non-decreasing per pixel.  ``support_dt``: an event is kept only when one of its 8 neighbour pixels saw an event at
    most this long before it (None: the test is off).  ``refractory``: an event less than this behind the previous event of its
    own pixel is dropped (0: off).  A pixel is hot with more than ``hot_count`` events (0: off), with more than ``mean +
    hot_sigma * std`` of the counts of the active pixels (0: off), or where ``hot_mask`` [height, width] is not zero.
    ``last_t``: the state of the previous call (``event_filter_state``; None: no event yet); it is not written.

    Returns a dict of device tensors: ``keep`` uint8 [N]; ``xy`` float32 [N, 2], the coordinates of the kept events and a NaN
    row for every other -- the format ``event_rectify`` (as fp32), ``event_voxel_grid(subpixel=True)``, ``event_warp`` and
    ``event_contrast`` skip and count -- (None unless ``want_xy``); ``index`` int32 [N], the kept indices in ascending order,
    then -1, and ``count`` int64 [1], their number (None unless ``want_index``); ``hot`` uint8 [height, width], the final mask;
    ``stats`` float64 [4]: active pixels, mean, std, threshold; ``status`` int32 [8] (``event_filter_status``); ``last_t``, a
    NEW tensor, the state for the next call.  Runs on the current stream, nothing is synchronised; a call repeats its bits.
    Time stamps that decrease within a pixel (or against the state) make every output empty or NaN and set bit 0 of
    ``status[0]``: never a plausible number."""
    require_cuda(x, y, t, hot_mask, last_t)
    dev = x.device
    if height < 1 or width < 1:
        raise RuntimeError("event_filter: height and width are positive")
    integer = not (x.is_floating_point() or y.is_floating_point())
    dt = torch.int32 if integer else torch.float32
    xs, ys = x.reshape(-1).to(dt).contiguous(), y.reshape(-1).to(dt).contiguous()
    tf = t.reshape(-1).to(torch.float64).contiguous()
    N = xs.shape[0]
    if not (ys.shape[0] == N and tf.shape[0] == N):
        raise RuntimeError("event_filter: x, y and t differ in length")
    hot_in = state = None
    if hot_mask is not None:
        if tuple(hot_mask.shape) != (height, width):
            raise RuntimeError("event_filter: hot_mask is [height, width]")
        hot_in = (hot_mask != 0).to(torch.uint8).contiguous()
    if last_t is not None:
        if tuple(last_t.shape) != (height, width) or last_t.dtype != torch.float64:
            raise RuntimeError("event_filter: last_t is float64 [height, width] (event_filter_state)")
        state = last_t.contiguous()
    nan = float("nan")
    res = {"keep": torch.empty(N, dtype=torch.uint8, device=dev),
           "xy": torch.empty((N, 2), dtype=torch.float32, device=dev) if want_xy else None,
           "index": torch.empty(N, dtype=torch.int32, device=dev) if want_index else None,
           "count": torch.zeros(1, dtype=torch.int64, device=dev) if want_index else None,
           "status": torch.zeros(8, dtype=torch.int32, device=dev)}
    if N == 0:                                                # (the entry launches nothing: the empty call's outputs are made here)
        res["hot"] = hot_in.clone() if hot_in is not None else torch.zeros((height, width), dtype=torch.uint8, device=dev)
        res["stats"] = torch.tensor([0.0, nan, nan, nan], dtype=torch.float64, device=dev)
        res["last_t"] = state.clone() if state is not None else event_filter_state(height, width, dev)
        return res
    res["hot"] = torch.empty((height, width), dtype=torch.uint8, device=dev)
    res["stats"] = torch.empty(4, dtype=torch.float64, device=dev)
    res["last_t"] = torch.empty((height, width), dtype=torch.float64, device=dev)
    nbytes = lib().ramp_event_filter_workspace_bytes(N, height, width)
    if nbytes == 0:
        check(_lib.RAMP_EUNSUPPORTED, "ramp_event_filter")
    ws = _lib_workspace(nbytes, dev, "evfilter")
    check(lib().ramp_event_filter(ptr(xs), ptr(ys), ptr(tf), N, height, width, _lib.RAMP_FILTER_XY_I32 if integer else 0,
                                  -1.0 if support_dt is None else float(support_dt), float(refractory), int(hot_count),
                                  float(hot_sigma), ptr(hot_in), ptr(state), ptr(res["last_t"]), ptr(res["keep"]), ptr(res["xy"]),
                                  ptr(res["index"]), ptr(res["count"]), ptr(res["hot"]), ptr(res["stats"]), ptr(res["status"]),
                                  ptr(ws), nbytes, stream()), "ramp_event_filter")
    return res


def event_filter_status(status):
    """The status words of ``event_filter`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_filter", status)


def event_flow(x, y, t, height, width, p=None, radius=2, window_dt=None, min_points=5, refine=1, outlier_dt=None,
               max_speed=float("inf"), last_t=None, want_map=False, want_fit=False):
    """Per-event optical flow on the device (include/ramp_hip.h ``ramp_event_flow``): at every event a plane is fitted to the
    surface of active events -- the last time stamp of each pixel of a ``(2 radius + 1)^2`` window that precedes the event and
    is at most ``window_dt`` older -- and the plane's slope gives the NORMAL flow in pixels per unit of ``t``.  No trajectory,
    no depth.  Order-independent and bit-exact, every rounding fixed by the header.

    ``x, y`` [N]: integer tensors take the int32 path, floating ones fp32; ``t`` [N] float64, non-decreasing per pixel (and
    plane); ``p`` [N]: with it the two polarities have a surface each (``p > 0`` and the rest).  ``radius`` 1 .. 3;
    ``min_points`` 3 .. ``(2 radius + 1)^2`` points a fit needs; ``refine`` 0 .. 2 passes that drop points further than
    ``outlier_dt`` (None: ``window_dt / 4``) from the plane and fit again; flows faster than ``max_speed`` are flat.
    ``last_t``: the state of the previous call, float64 [height, width] without ``p`` (``event_filter``'s ``last_t`` as it
    is), [2, height, width] with it; None: no event yet.  It is not written.

    Returns a dict of device tensors: ``flow`` float32 [N, 2] (NaN rows for every event without a valid flow), ``cls`` uint8
    [N] (2 not finite, 3 outside, 4 too few points, 5 collinear, 6 flat, 7 valid), ``n_used`` uint8 [N], ``status`` int32 [8]
    (``event_flow_status``), ``last_t``, a NEW tensor, the state for the next call; with ``want_fit`` ``fit`` float64 [N, 3]
    (the plane a, b, c); with ``want_map`` ``flow_map`` float32 [2, height, width] and ``map_index`` int32 [height, width]: per
    pixel the valid event with the largest index.  Runs on the current stream, nothing is synchronised; a call repeats its
    bits.  Time stamps that decrease within a pixel (or against the state) make every output NaN, -1 or 0 and set bit 0 of
    ``status[0]``: never a plausible number."""
    dev = x.device
    if height < 1 or width < 1:
        raise RuntimeError("event_flow: height and width are positive")
    if window_dt is None:
        raise RuntimeError("event_flow: window_dt is required (the age, in the unit of t, up to which a neighbour is a point)")
    radius, min_points, refine = int(radius), int(min_points), int(refine)
    window_dt, max_speed = float(window_dt), float(max_speed)
    outlier_dt = window_dt / 4 if outlier_dt is None else float(outlier_dt)
    if not 1 <= radius <= 3:
        raise RuntimeError("event_flow: radius is 1, 2 or 3")
    if not 3 <= min_points <= (2 * radius + 1) ** 2:
        raise RuntimeError("event_flow: min_points is between 3 and (2 radius + 1)^2 = %d" % (2 * radius + 1) ** 2)
    if not 0 <= refine <= 2:
        raise RuntimeError("event_flow: refine is 0, 1 or 2")
    if not window_dt >= 0 or not outlier_dt >= 0:
        raise RuntimeError("event_flow: window_dt and outlier_dt are not negative (and not NaN)")
    if not max_speed > 0:
        raise RuntimeError("event_flow: max_speed is positive (inf: no limit)")
    integer = not (x.is_floating_point() or y.is_floating_point())
    dt = torch.int32 if integer else torch.float32
    xs, ys = x.reshape(-1).to(dt).contiguous(), y.reshape(-1).to(dt).contiguous()
    tf = t.reshape(-1).to(torch.float64).contiguous()
    N = xs.shape[0]
    pd = None if p is None else p.reshape(-1).to(torch.int8).contiguous()
    if not (ys.shape[0] == N and tf.shape[0] == N and (pd is None or pd.shape[0] == N)):
        raise RuntimeError("event_flow: x, y, t and p differ in length")
    planes = 1 if pd is None else 2
    shape = (height, width) if planes == 1 else (2, height, width)
    state = None
    if last_t is not None:
        if tuple(last_t.shape) != shape or last_t.dtype != torch.float64:
            raise RuntimeError("event_flow: last_t is float64 [height, width], or [2, height, width] with p")
        state = last_t.contiguous()
    require_cuda(x, y, t, p, last_t)
    nbytes = lib().ramp_event_flow_ws_bytes(N, height, width, planes)
    if nbytes == 0:
        check(_lib.RAMP_EUNSUPPORTED, "ramp_event_flow")
    res = {"flow": torch.empty((N, 2), dtype=torch.float32, device=dev), "cls": torch.empty(N, dtype=torch.uint8, device=dev),
           "n_used": torch.empty(N, dtype=torch.uint8, device=dev), "status": torch.zeros(8, dtype=torch.int32, device=dev)}
    if want_fit:
        res["fit"] = torch.empty((N, 3), dtype=torch.float64, device=dev)
    if want_map:
        res["flow_map"] = torch.empty((2, height, width), dtype=torch.float32, device=dev)
        res["map_index"] = torch.empty((height, width), dtype=torch.int32, device=dev)
    if N == 0:                                                # (an empty p has no pointer to tell the entry of two planes: the state is made here)
        res["last_t"] = state.clone() if state is not None else torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        state = None
    else:
        res["last_t"] = torch.empty(shape, dtype=torch.float64, device=dev)
    ws = _lib_workspace(nbytes, dev, "evflow")
    check(lib().ramp_event_flow(ptr(xs), ptr(ys), ptr(tf), ptr(pd), N, height, width, _lib.RAMP_FLOW_XY_I32 if integer else 0,
                                radius, window_dt, min_points, refine, outlier_dt, max_speed, ptr(state), ptr(res["last_t"]) if N else None,
                                ptr(res["flow"]), ptr(res["cls"]), ptr(res["n_used"]), ptr(res.get("fit")),
                                ptr(res.get("flow_map")), ptr(res.get("map_index")), ptr(res["status"]), ptr(ws), nbytes,
                                stream()), "ramp_event_flow")
    return res


def event_flow_status(status):
    """The status words of ``event_flow`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_flow", status)


def event_corners(x, y, t, height, width, p=None, inner=(3, 6), outer=(4, 8), wide=False, last_t=None, want_arc=False,
                  want_index=True, want_map=False):
    """Event corner detection on the device (include/ramp_hip.h ``ramp_event_corners``): an event is a corner when, on the
    surface of active events at its own time, both a circle of 16 pixels (radius 3) and one of 20 (radius 4) around it hold a
    contiguous arc of pixels that are all newer than all the rest (Mueggler et al. 2017) -- arcs of ``inner`` = (lo, hi) and
    ``outer`` = (lo, hi) pixels, with ``wide`` also the arcs whose complement has such a length (Arc*, Alzugaray and Chli
    2018).  Time stamps are only compared: order-independent and bit-exact, no tolerance anywhere.

    ``x, y`` [N]: integer tensors take the int32 path, floating ones fp32; ``t`` [N] float64, non-decreasing per pixel (and
    plane); ``p`` [N]: with it the two polarities have a surface each (``p > 0`` and the rest).  ``last_t``: the state of the
    previous call, float64 [height, width] without ``p`` (``event_filter``'s and ``event_flow``'s ``last_t`` as it is),
    [2, height, width] with it; None: no event yet.  It is not written.

    Returns a dict of device tensors: ``cls`` uint8 [N] (2 not finite, 3 outside, 4 border, 5 no inner arc, 6 no outer arc, 7
    corner), ``corner`` bool [N] (``cls == 7``), ``status`` int32 [8] (``event_corners_status``), ``last_t``, a NEW tensor,
    the state for the next call; with ``want_arc`` ``arc`` uint8 [N, 4] (inner start, inner length, outer start, outer length
    of the shortest passing arcs); with ``want_index`` ``index`` int32 [N] (the corners' indices ascending, then -1) and
    ``count`` int32 [1]; with ``want_map`` ``corner_count`` int32 [height, width], the corners per pixel.  Runs on the current
    stream, nothing is synchronised; a call repeats its bits.  Time stamps that decrease within a pixel (or against the state)
    make every output 0, -1 or NaN and set bit 0 of ``status[0]``: never a plausible answer."""
    dev = x.device
    if height < 1 or width < 1:
        raise RuntimeError("event_corners: height and width are positive")
    ranges = []
    for name, n, r in (("inner", 16, inner), ("outer", 20, outer)):
        try:
            lo, hi = (int(v) for v in r)
        except (TypeError, ValueError):
            raise RuntimeError("event_corners: %s is a pair (lo, hi) of arc lengths" % name) from None
        if not 1 <= lo <= hi <= n - 1:
            raise RuntimeError("event_corners: %s is (lo, hi) with 1 <= lo <= hi <= %d" % (name, n - 1))
        ranges += [lo, hi]
    integer = not (x.is_floating_point() or y.is_floating_point())
    dt = torch.int32 if integer else torch.float32
    xs, ys = x.reshape(-1).to(dt).contiguous(), y.reshape(-1).to(dt).contiguous()
    tf = t.reshape(-1).to(torch.float64).contiguous()
    N = xs.shape[0]
    pd = None if p is None else p.reshape(-1).to(torch.int8).contiguous()
    if not (ys.shape[0] == N and tf.shape[0] == N and (pd is None or pd.shape[0] == N)):
        raise RuntimeError("event_corners: x, y, t and p differ in length")
    planes = 1 if pd is None else 2
    shape = (height, width) if planes == 1 else (2, height, width)
    state = None
    if last_t is not None:
        if tuple(last_t.shape) != shape or last_t.dtype != torch.float64:
            raise RuntimeError("event_corners: last_t is float64 [height, width], or [2, height, width] with p")
        state = last_t.contiguous()
    require_cuda(x, y, t, p, last_t)
    nbytes = lib().ramp_event_corners_ws_bytes(N, height, width, planes)
    if nbytes == 0:
        check(_lib.RAMP_EUNSUPPORTED, "ramp_event_corners")
    res = {"cls": torch.empty(N, dtype=torch.uint8, device=dev), "status": torch.zeros(8, dtype=torch.int32, device=dev)}
    if want_arc:
        res["arc"] = torch.empty((N, 4), dtype=torch.uint8, device=dev)
    if want_index:
        res["index"] = torch.empty(N, dtype=torch.int32, device=dev)
        res["count"] = torch.zeros(1, dtype=torch.int32, device=dev)
    if want_map:
        res["corner_count"] = torch.empty((height, width), dtype=torch.int32, device=dev)
    if N == 0:                                                # (an empty p has no pointer to tell the entry of two planes: the state is made here;
        # an empty index has none to pair with count: count, zeroed above, stays here too)
        res["last_t"] = state.clone() if state is not None else torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        state = None
    else:
        res["last_t"] = torch.empty(shape, dtype=torch.float64, device=dev)
    ws = _lib_workspace(nbytes, dev, "evcorners")
    flags = (_lib.RAMP_CORNER_XY_I32 if integer else 0) | (_lib.RAMP_CORNER_WIDE if wide else 0)
    check(lib().ramp_event_corners(ptr(xs), ptr(ys), ptr(tf), ptr(pd), N, height, width, flags, *ranges, ptr(state),
                                   ptr(res["last_t"]) if N else None, ptr(res["cls"]), ptr(res.get("arc")), ptr(res.get("index")),
                                   ptr(res.get("count")) if N else None, ptr(res.get("corner_count")), ptr(res["status"]), ptr(ws), nbytes,
                                   stream()), "ramp_event_corners")
    res["corner"] = res["cls"] == 7
    return res


def event_corners_status(status):
    """The status words of ``event_corners`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_corners", status)


def event_corner_tracks(x, y, t, height, width, corner=None, p=None, radius=3, max_dt=None, state=None, next_id=None,
                        want_parent=True, want_birth=False, want_velocity=True):
    """Event corner tracks on the device (include/ramp_hip.h ``ramp_event_corner_tracks``): every candidate event is linked to
    the newest candidate in the (2 ``radius`` + 1)^2 window around it -- its own pixel included -- that precedes it by at most
    ``max_dt`` (required, in the unit of ``t``; ``float("inf")`` is allowed); without one a track is born.  A track has an id
    (the global number of the event it was born with), a birth (t0, x0, y0) and a length, and each of its events the mean
    image velocity since the birth, both components.  Order-independent and bit-exact.  ``radius`` = 3 is a default nobody
    has tuned.

    ``x, y`` [N]: integer tensors take the int32 path, floating ones fp32; ``t`` [N] float64, non-decreasing per pixel (and
    plane); ``corner`` [N]: nonzero marks the candidates (``event_corners``' ``corner`` as it is), None: every valid event is
    one; ``p`` [N]: with it the two polarities are linked apart.  ``state`` and ``next_id``: those of the previous call (both or
    neither; None: no track yet, ids from 0), int64 [height, width, 4] without ``p``, [2, height, width, 4] with it
    (``corner_track_state`` unpacks it), and int64 [1].  Neither is written.

    Returns a dict of device tensors: ``cls`` uint8 [N] (2 not finite, 3 outside, 4 not a candidate, 5 born, 6 carried on from
    the state, 7 linked to an event of this call), ``track`` int64 [N] (-1 for an event that is no candidate), ``length`` int32
    [N] (the events of the track so far, 0), ``status`` int32 [8] (``event_corner_tracks_status``), ``state`` and ``next_id``,
    NEW tensors, for the next call: a stream fed in pieces gets the tracks and ids of the stream fed whole; with
    ``want_parent`` ``parent`` int32 [N] (the event linked to, -1 a birth or no candidate, -2 the state); with ``want_birth``
    ``birth`` float64 [N, 3] (t0, x0, y0; NaN); with ``want_velocity`` ``velocity`` float32 [N, 2] in pixels per unit of ``t``
    (NaN at a birth and for an event that is no candidate).  Runs on the current stream, nothing is synchronised; a call
    repeats its bits.  Time stamps that decrease within a pixel (or against the state) make every output 0, -1 or NaN, empty
    the state and set bit 0 of ``status[0]``: never a plausible answer."""
    dev = x.device
    if height < 1 or width < 1:
        raise RuntimeError("event_corner_tracks: height and width are positive")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= 5:
        raise RuntimeError("event_corner_tracks: radius is an integer in 0 .. 5")
    if max_dt is None:
        raise RuntimeError("event_corner_tracks: max_dt is required (the longest gap a link may span, in the unit of t)")
    max_dt = float(max_dt)
    if not max_dt >= 0.0:
        raise RuntimeError("event_corner_tracks: max_dt is not negative and not NaN")
    integer = not (x.is_floating_point() or y.is_floating_point())
    dt = torch.int32 if integer else torch.float32
    xs, ys = x.reshape(-1).to(dt).contiguous(), y.reshape(-1).to(dt).contiguous()
    tf = t.reshape(-1).to(torch.float64).contiguous()
    N = xs.shape[0]
    pd = None if p is None else p.reshape(-1).to(torch.int8).contiguous()
    cd = None if corner is None else (corner.reshape(-1) != 0).to(torch.uint8).contiguous()
    if not (ys.shape[0] == N and tf.shape[0] == N and (pd is None or pd.shape[0] == N) and (cd is None or cd.shape[0] == N)):
        raise RuntimeError("event_corner_tracks: x, y, t, corner and p differ in length")
    planes = 1 if pd is None else 2
    shape = (height, width, 4) if planes == 1 else (2, height, width, 4)
    if (state is None) != (next_id is None):
        raise RuntimeError("event_corner_tracks: state and next_id go together (both of the previous call, or neither)")
    if state is not None:
        if tuple(state.shape) != shape or state.dtype != torch.int64:
            raise RuntimeError("event_corner_tracks: state is int64 [height, width, 4], or [2, height, width, 4] with p")
        if next_id.numel() != 1 or next_id.dtype != torch.int64:
            raise RuntimeError("event_corner_tracks: next_id is int64 [1]")
        state, next_id = state.contiguous(), next_id.reshape(1)
    require_cuda(x, y, t, corner, p, state, next_id)
    nbytes = lib().ramp_event_corner_tracks_ws_bytes(N, height, width, planes)
    if nbytes == 0:
        check(_lib.RAMP_EUNSUPPORTED, "ramp_event_corner_tracks")
    res = {"cls": torch.empty(N, dtype=torch.uint8, device=dev), "track": torch.empty(N, dtype=torch.int64, device=dev),
           "length": torch.empty(N, dtype=torch.int32, device=dev), "status": torch.zeros(8, dtype=torch.int32, device=dev)}
    if want_parent:
        res["parent"] = torch.empty(N, dtype=torch.int32, device=dev)
    if want_birth:
        res["birth"] = torch.empty((N, 3), dtype=torch.float64, device=dev)
    if want_velocity:
        res["velocity"] = torch.empty((N, 2), dtype=torch.float32, device=dev)
    if N == 0:                                                # (an empty p has no pointer to tell the entry of two planes: the state is made here)
        res["state"] = state.clone() if state is not None else _empty_track_state(shape, dev)
        res["next_id"] = next_id.clone() if next_id is not None else torch.zeros(1, dtype=torch.int64, device=dev)
        state = next_id = None
    else:
        res["state"] = torch.empty(shape, dtype=torch.int64, device=dev)
        res["next_id"] = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _lib_workspace(nbytes, dev, "evtracks")
    check(lib().ramp_event_corner_tracks(ptr(xs), ptr(ys), ptr(tf), ptr(pd), ptr(cd), N, height, width,
                                         _lib.RAMP_CORNER_TRACK_XY_I32 if integer else 0, radius, max_dt, ptr(state), ptr(next_id),
                                         ptr(res["state"]) if N else None, ptr(res["next_id"]) if N else None, ptr(res["cls"]),
                                         ptr(res.get("parent")), ptr(res["track"]), ptr(res["length"]), ptr(res.get("birth")),
                                         ptr(res.get("velocity")), ptr(res["status"]), ptr(ws), nbytes, stream()),
          "ramp_event_corner_tracks")
    return res


def _empty_track_state(shape, dev):
    """no track yet: every cell's t is NaN, its other words 0"""
    s = torch.zeros(shape, dtype=torch.int64, device=dev)
    s[..., 0] = torch.tensor(float("nan"), dtype=torch.float64).view(torch.int64).item()
    return s


def event_corner_tracks_status(status):
    """The status words of ``event_corner_tracks`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_corner_tracks", status)


def corner_track_state(state):
    """The state of ``event_corner_tracks`` (int64 [..., height, width, 4]) unpacked with plain torch, on the state's device: a
    dict ``t`` float64 (NaN: the cell holds no corner), ``track`` int64, ``t0`` float64, ``x0``, ``y0`` int64 (the birth) and
    ``length`` int32, each [..., height, width].  The state is also the live-track map: ``t >= now - max_dt`` marks the cells
    that hold a live track's newest corner."""
    if state.dtype != torch.int64 or state.dim() < 3 or state.shape[-1] != 4:
        raise RuntimeError("corner_track_state: state is int64 [..., height, width, 4]")
    width = state.shape[-2]
    pix = state[..., 3] & 0xFFFFFFFF
    return {"t": state[..., 0].contiguous().view(torch.float64), "track": state[..., 1].clone(),
            "t0": state[..., 2].contiguous().view(torch.float64), "x0": pix % width, "y0": torch.div(pix, width, rounding_mode="floor"),
            "length": (state[..., 3] >> 32).to(torch.int32)}


def event_landmarks(x, y, t, track, knots, times, intrinsics, min_obs=3, refine=2, min_parallax=0.02, max_rms=2.0, sigma_px=1.0,
                    max_landmarks=None, extrapolate=False, want_index=False, want_residual=False, want_rays=False):
    """Event landmarks on the device (include/ramp_hip.h ``ramp_event_landmarks``): every corner track, seen from the camera
    poses at its own events' time stamps, is triangulated into one 3-D point -- a midpoint solve, ``refine`` (0 .. 4)
    Gauss-Newton steps on the reprojection error in pixels, the covariance ``sigma_px``^2 H^-1 and a class.

    ``x, y`` [N] pixel coordinates of the pinhole camera ``intrinsics`` (fx, fy, cx, cy) -- rectify raw pixels first; ``t`` [N]
    float64; ``track`` [N] int64, ``event_corner_tracks``' ``track`` (negative: the event observes nothing); ``knots`` [T,7]
    CAMERA-TO-WORLD with ``times`` [T] float64, as ``Ramp_vo.trajectory()`` returns them.  An event outside the knots' range
    observes nothing unless ``extrapolate``.  ``max_landmarks=None``: min(N, 2**20), at least 1; the tracks with the highest
    ids are cut off and counted.  ``min_obs`` = 3, ``refine`` = 2, ``min_parallax`` = 0.02 rad, ``max_rms`` = 2 pixels and
    ``sigma_px`` = 1 are defaults nobody has tuned.

    Returns a dict of device tensors, nothing synchronised: ``count`` int32 [1] and, over ``max_landmarks`` rows of which the
    first ``count`` are written, in ascending id: ``track`` int64, ``point`` [.,3] and ``cov`` [.,6] (xx, xy, xz, yy, yz, zz;
    both NaN unless ``cls`` is 7, so ``PointMap.insert(point, count=count)`` drops the rest by itself), ``n_obs`` int32, ``cls``
    uint8 (1 fewer than ``min_obs`` observations, 2 parallax below ``min_parallax``, 3 the midpoint system is singular, 4 the
    point lies behind or too near a camera, 5 rms above ``max_rms``, 6 not finite, 7 valid), ``rms`` in pixels, ``parallax`` in
    radians, ``span`` float64 [.,2] (first and last time stamp); ``status`` int32 [8] (``event_landmarks_status``); with
    ``want_index`` ``index`` int32 [N] (the event's landmark number, -1), with ``want_residual`` ``residual`` [N,2] (pixels;
    NaN), with ``want_rays`` ``rays`` [N,6] (camera centre and world direction; NaN).  Only the observations of this call are
    triangulated.  A call repeats its bits; time stamps of the knots that decrease or are not finite give ``count`` = 0 and
    set bit 0 of ``status[0]``: never a plausible answer."""
    name = "event_landmarks"
    if isinstance(min_obs, bool) or not isinstance(min_obs, int) or min_obs < 2:
        raise RuntimeError(name + ": min_obs is an integer, at least 2")
    if isinstance(refine, bool) or not isinstance(refine, int) or not 0 <= refine <= 4:
        raise RuntimeError(name + ": refine is an integer in 0 .. 4")
    for k, v in (("min_parallax", min_parallax), ("max_rms", max_rms), ("sigma_px", sigma_px)):
        if not 0.0 <= float(v) <= 3.4028234663852886e38:
            raise RuntimeError(name + ": %s is finite and not negative" % k)
    if max_landmarks is not None and (isinstance(max_landmarks, bool) or not isinstance(max_landmarks, int) or max_landmarks < 1):
        raise RuntimeError(name + ": max_landmarks is a positive integer or None")
    xf, yf, tf, _ = _events(x, y, t, None)
    N = xf.shape[0]
    if track.dtype != torch.int64:
        raise RuntimeError(name + ": track is int64 (event_corner_tracks' track)")
    tr = track.reshape(-1).contiguous()
    _same_length(name, "x, y, t and track", N, yf, tf, tr)
    knots = knots.reshape(-1, 7).contiguous().float()
    times = times.reshape(-1).contiguous().double()
    T = knots.shape[0]
    if T < 1 or times.shape[0] != T:
        raise RuntimeError("%s: %d knots but %d time stamps (at least one knot)" % (name, T, times.shape[0]))
    if N >= 2 ** 31:
        check(_lib.RAMP_EUNSUPPORTED, "ramp_event_landmarks")
    require_cuda(x, y, t, track, knots, times)
    dev = xf.device
    K = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev).reshape(4).contiguous()
    L = max(1, min(N, 2 ** 20)) if max_landmarks is None else max_landmarks
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    res = {"track": e(L, torch.int64), "point": e((L, 3), torch.float32), "cov": e((L, 6), torch.float32), "n_obs": e(L, torch.int32),
           "cls": e(L, torch.uint8), "rms": e(L, torch.float32), "parallax": e(L, torch.float32), "span": e((L, 2), torch.float64),
           "count": e(1, torch.int32), "status": e(8, torch.int32)}
    if want_index:
        res["index"] = e(N, torch.int32)
    if want_residual:
        res["residual"] = e((N, 2), torch.float32)
    if want_rays:
        res["rays"] = e((N, 6), torch.float32)
    ws, nbytes = sized_workspace("ramp_event_landmarks_ws_bytes", (N, T, L), dev, "evlandmarks")
    opt = lambda k: ptr(res[k]) if k in res and N else None
    check(lib().ramp_event_landmarks(ptr(xf), ptr(yf), ptr(tf), ptr(tr), N, ptr(knots), ptr(times), T, ptr(K),
                                     _lib.RAMP_INTERP_EXTRAPOLATE if extrapolate else 0, min_obs, refine, float(min_parallax),
                                     float(max_rms), float(sigma_px), L, ptr(res["track"]), ptr(res["point"]), ptr(res["cov"]),
                                     ptr(res["n_obs"]), ptr(res["cls"]), ptr(res["rms"]), ptr(res["parallax"]), ptr(res["span"]),
                                     ptr(res["count"]), opt("index"), opt("residual"), opt("rays"), ptr(res["status"]), ptr(ws),
                                     nbytes, stream()), "ramp_event_landmarks")
    return res


def event_landmarks_status(status):
    """The status words of ``event_landmarks`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("event_landmarks", status)


# ------------------------------------------------------------------- IMU
def _host_value(name, v):
    """``v`` as nested lists; a device tensor is refused: reading it back would synchronise, which these wrappers never do"""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise RuntimeError(name + " is a host value (a list, an array, a CPU tensor): a device tensor would have to be "
                               "read back, and this call synchronises nothing")
        return v.detach().tolist()
    return v


def _host3(name, v, n=3):
    """a host float64 array of n words for a C entry that reads it before it returns (None: NULL)"""
    if v is None:
        return None, None
    v = _host_value(name, v)
    flat = [float(c) for row in v for c in (row if hasattr(row, "__len__") else [row])]
    if len(flat) != n:
        raise RuntimeError("%s holds %d numbers" % (name, n))
    arr = (ctypes.c_double * n)(*flat)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _imu_samples(name, tau, gyro, accel, times):
    require_cuda(tau, gyro, accel, times)
    tf, tt = tau.reshape(-1).to(torch.float64).contiguous(), times.reshape(-1).to(torch.float64).contiguous()
    f64 = gyro.dtype == torch.float64 or accel.dtype == torch.float64
    dt = torch.float64 if f64 else torch.float32
    g, a = gyro.to(dt).reshape(-1, 3).contiguous(), accel.to(dt).reshape(-1, 3).contiguous()
    N = tf.shape[0]
    if N < 1 or g.shape[0] != N or a.shape[0] != N:
        raise RuntimeError(name + ": tau [N], gyro [N,3] and accel [N,3] hold the same N >= 1 samples")
    return tf, g, a, tt, N, (_lib.RAMP_IMU_F64 if f64 else 0)


def imu_preintegrate(tau, gyro, accel, times, bias_g=None, bias_a=None, stride=1, max_gap=float("inf")):
    """Forster's on-manifold IMU preintegrals between consecutive time stamps ``times[0], times[stride], ...`` (include/
    ramp_hip.h ``ramp_imu_preintegrate``; one wave per interval, float64): ``tau`` [N] float64 sample times, ``gyro``, ``accel``
    [N,3] float32 or float64 device tensors, the biases HOST triples (lists, arrays, CPU tensors; a device tensor is refused, it
    would have to be read back).  Returns ``(preint, status)``: ``preint`` float64
    [K - 1, 24] -- dt, the sub-interval count, dR as qx qy qz qw, dv, dp, d dR / d bias_g row-major, three zeros; NaN for an
    interval the samples do not cover -- and ``status`` int32 [8] (``imu_status``).  Runs on the current stream, nothing is
    synchronised.  A record's bits depend on its own interval's samples and the biases alone."""
    tf, g, a, tt, N, flags = _imu_samples("imu_preintegrate", tau, gyro, accel, times)
    T = tt.shape[0]
    K = (T - 1) // max(int(stride), 1) + 1
    if T < 2 or stride < 1 or K < 2:
        raise RuntimeError("imu_preintegrate: at least two of the time stamps are used (stride >= 1)")
    (_, bg), (_, ba) = keep = _host3("imu_preintegrate: bias_g", bias_g), _host3("imu_preintegrate: bias_a", bias_a)
    preint = torch.empty((K - 1, _lib.RAMP_IMU_PREINT_WORDS), dtype=torch.float64, device=tf.device)
    status = torch.empty(8, dtype=torch.int32, device=tf.device)
    check(lib().ramp_imu_preintegrate(ptr(tf), ptr(g), ptr(a), N, ptr(tt), T, int(stride), bg, ba, float(max_gap), flags,
                                      ptr(preint), ptr(status), stream()), "ramp_imu_preintegrate")
    del keep
    return preint, status


def imu_align(tau, gyro, accel, knots, times, R_bc=None, p_bc=None, bias_g=None, bias_a=None, stride=1, max_gap=float("inf"),
              gravity_norm=None, gyro_steps=1, want_preint=False):
    """Metric scale, gravity and gyro bias of a monocular trajectory from raw IMU samples, on the device (include/ramp_hip.h
    ``ramp_imu_align``): ONE C call enqueues the preintegration between the knots used (``0, stride, ...``), ``gyro_steps``
    Gauss-Newton steps of the gyro bias, the integration again with the corrected bias, the linear solve for ``(s, g)`` over
    all triples of knots, and the velocities.  Nothing is read back, nothing synchronised.

    ``knots`` [T,7] camera-to-world rows (``trajectory(as_tensor=True)``), ``times`` [T] float64.  ``R_bc`` [3,3], ``p_bc`` [3]:
    the camera in the IMU frame (None: identity, zero); ``R_bc`` has to be a rotation.  ``bias_g``, ``bias_a``: the start gyro
    bias and the accelerometer bias (not estimated).  These four are HOST values (lists, arrays, CPU tensors); a device tensor
    is refused, since reading it back would synchronise.  ``gravity_norm``: None or 0 leaves the norm free; a value fixes ``|g|``.

    Returns a dict of device tensors: ``result`` float64 [16] with the views ``scale`` [1], ``gravity`` [3], ``bias_g`` [3],
    ``rms`` [1], ``cond`` [1]; ``normal`` float64 [32] (N, y, H, b); ``velocity`` [K,3]; ``residual`` [K-2]; ``status`` int32
    [8] (``imu_status``); with ``want_preint`` the records of the final integration.  A stage that fails sets its status bit
    and leaves NaN, never a plausible number."""
    tf, g, a, tt, N, flags = _imu_samples("imu_align", tau, gyro, accel, times)
    require_cuda(knots)
    kn = knots.reshape(-1, 7).to(torch.float32).contiguous()
    T = tt.shape[0]
    K = (T - 1) // max(int(stride), 1) + 1
    if kn.shape[0] != T:
        raise RuntimeError("imu_align: knots [T,7] and times [T] differ in length")
    if T < 2 or stride < 1 or K < 2:
        raise RuntimeError("imu_align: at least two of the knots are used (stride >= 1)")
    ext = _imu_extrinsics("imu_align", R_bc, p_bc)
    (_, ex), (_, bg), (_, ba) = keep = (_host3("imu_align: R_bc and p_bc", ext, 12), _host3("imu_align: bias_g", bias_g),
                                        _host3("imu_align: bias_a", bias_a))
    dev = tf.device
    f64 = dict(dtype=torch.float64, device=dev)
    res = {"result": torch.empty(16, **f64), "normal": torch.empty(32, **f64), "velocity": torch.empty((K, 3), **f64),
           "residual": torch.empty(max(K - 2, 0), **f64), "status": torch.empty(8, dtype=torch.int32, device=dev)}
    if want_preint:
        res["preint"] = torch.empty((K - 1, _lib.RAMP_IMU_PREINT_WORDS), **f64)
    ws, nbytes = sized_workspace("ramp_imu_workspace_bytes", (N, K), dev, "imu")
    check(lib().ramp_imu_align(ptr(tf), ptr(g), ptr(a), N, ptr(kn), ptr(tt), T, int(stride), ex, bg, ba, float(max_gap),
                               float(gravity_norm or 0.0), int(gyro_steps), flags, ptr(res["result"]), ptr(res["normal"]),
                               ptr(res["velocity"]), ptr(res["residual"]) if K > 2 else None, ptr(res.get("preint")),
                               ptr(res["status"]), ptr(ws), nbytes, stream()), "ramp_imu_align")
    del keep
    r = res["result"]
    res.update(scale=r[0:1], gravity=r[1:4], bias_g=r[4:7], rms=r[7:8], cond=r[8:9])
    return res


def imu_status(status):
    """The status words of ``imu_preintegrate`` / ``imu_align`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("imu", status)


def _imu_extrinsics(name, R_bc, p_bc):
    """R_bc [3,3] and p_bc [3] (host values; None: identity, zero) as the 12 host words the C entries take, or None for both"""
    if R_bc is None and p_bc is None:
        return None
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]] if R_bc is None else R_bc
    R = [list(r) for r in _host_value(name + ": R_bc", R)]
    p = [0.0, 0.0, 0.0] if p_bc is None else list(_host_value(name + ": p_bc", p_bc))
    return list(R) + [p]


def imu_anchor(align, knots, times, stride=1):
    """The anchor of ``imu_propagate`` from the dict of ``imu_align`` and the last knot it used (``knots`` [T,7], ``times`` [T],
    ``stride`` as given there): device float64 [24] -- t0, the knot's translation, its quaternion, the knot's velocity, ``s``,
    ``g``, ``bias_g``, six zeros (include/ramp_hip.h ``ramp_imu_propagate``).  Torch ops on the current stream: nothing is read
    back, nothing synchronised; a failed alignment's NaNs simply arrive in it, and the propagation answers ``bad_anchor``."""
    require_cuda(knots, times, align["result"], align["velocity"])
    kn, tt = knots.reshape(-1, 7), times.reshape(-1)
    T = kn.shape[0]
    K = (T - 1) // max(int(stride), 1) + 1
    if stride < 1 or tt.shape[0] != T or align["velocity"].shape[0] != K:
        raise RuntimeError("imu_anchor: the alignment holds %d knots, knots [T,7] / times [T] at this stride hold %d"
                           % (align["velocity"].shape[0], K))
    last = (K - 1) * int(stride)
    r = align["result"]
    return torch.cat([tt[last:last + 1].to(torch.float64), kn[last].to(torch.float64), align["velocity"][K - 1], r[0:7],
                      torch.zeros(6, dtype=torch.float64, device=r.device)])


def imu_propagate(tau, gyro, accel, anchor, R_bc=None, p_bc=None, bias_a=None, max_gap=float("inf"), horizon=float("inf"),
                  want_state=False):
    """Poses at the IMU's rate ahead of a knot (include/ramp_hip.h ``ramp_imu_propagate``): from ``anchor`` (``imu_anchor``)
    forward through every sample behind it -- a device-wide ordered float64 scan of the preintegration elements.  ``tau`` [N],
    ``gyro``, ``accel`` [N,3], ``R_bc``, ``p_bc``, ``bias_a``, ``max_gap`` as in ``imu_align``; ``horizon``: rows further than this
    many seconds from the anchor are NaN.  Returns a dict of device tensors: ``poses`` [N,7] fp32 camera-to-world rows in the
    tracker's unit and ``times`` [N] float64 ``max(tau, t0)`` -- together the ``knots, times`` of ``se3_interp`` /
    ``event_warp`` --, ``status`` int32 [8] (``imu_propagate_status``), with ``want_state`` ``state`` [N,16] float64 (dt, q_wb,
    v, p_wb, zeros).  Rows at or before the anchor hold its pose; rows behind a sample that is not finite or a gap above
    ``max_gap`` are NaN; a status bit makes everything NaN, never a plausible number.  One C call on the current stream,
    nothing read back, nothing synchronised.  Row i's bits depend on samples 0 .. i and the arguments alone."""
    tf, g, a, an, N, flags = _imu_samples("imu_propagate", tau, gyro, accel, anchor)
    if an.shape[0] != _lib.RAMP_IMU_ANCHOR_WORDS:
        raise RuntimeError("imu_propagate: anchor holds %d float64 words (imu_anchor)" % _lib.RAMP_IMU_ANCHOR_WORDS)
    (_, ex), (_, ba) = keep = (_host3("imu_propagate: R_bc and p_bc", _imu_extrinsics("imu_propagate", R_bc, p_bc), 12),
                               _host3("imu_propagate: bias_a", bias_a))
    dev = tf.device
    res = {"poses": torch.empty((N, 7), dtype=torch.float32, device=dev), "times": torch.empty(N, dtype=torch.float64, device=dev),
           "status": torch.empty(8, dtype=torch.int32, device=dev)}
    if want_state:
        res["state"] = torch.empty((N, 16), dtype=torch.float64, device=dev)
    ws, nbytes = sized_workspace("ramp_imu_propagate_workspace_bytes", (N,), dev, "imu_propagate")
    check(lib().ramp_imu_propagate(ptr(tf), ptr(g), ptr(a), N, ptr(an), ex, ba, float(max_gap), float(horizon), flags,
                                   ptr(res["poses"]), ptr(res["times"]), ptr(res.get("state")), ptr(res["status"]), ptr(ws),
                                   nbytes, stream()), "ramp_imu_propagate")
    del keep
    return res


def imu_propagate_status(status):
    """The status words of ``imu_propagate`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("imu_propagate", status)


def align_loop(evaluate, correction, free, step, iters):
    """the line search of ``event_align`` over ``evaluate(theta) -> (variance, grad)``: normalised gradient ascent with
    backtracking.  The direction is the gradient masked by ``free``, divided by its norm; the step length starts at ``step``,
    doubles after an accepted step and halves, up to 8 times, while the contrast does not rise; the loop stops after ``iters``
    accepted steps, when a step fails 8 halvings, or when the masked gradient is zero or not finite."""
    theta = [float(c) for c in correction]
    mask = [1.0 if f else 0.0 for f in free]
    f, g = evaluate(theta)
    f0, history, length = f, [], float(step)
    while len(history) < iters:
        gm = [gi * mi for gi, mi in zip(g, mask)]
        norm = sum(gi * gi for gi in gm) ** 0.5
        if not (norm > 0.0 and norm < float("inf")):
            break
        accepted = False
        for _ in range(9):                                    # the first trial and up to 8 halvings
            trial = [ti + length * gi / norm for ti, gi in zip(theta, gm)]
            ft, gt = evaluate(trial)
            if ft > f:
                theta, f, g, accepted = trial, ft, gt, True
                break
            length *= 0.5
        if not accepted:
            break
        history.append(f)
        length *= 2.0
    return dict(correction=theta, variance=f, variance0=f0, history=history)


ALIGN_REASONS = {0: "running", _lib.RAMP_ALIGN_ITERS: "iters", _lib.RAMP_ALIGN_STALLED: "stalled", _lib.RAMP_ALIGN_FLAT: "flat",
                 _lib.RAMP_ALIGN_BUDGET: "budget"}


def event_align(x, y, t, p, knots, times, t_ref, intrinsics, invdepth, height, width, correction=None,
                free=(0, 0, 0, 1, 1, 1, 0), step=0.05, iters=20, signed=True, extrapolate=False, resident=False, max_evals=None):
    """Refine a correction by contrast maximisation: normalised gradient ascent with backtracking over ``event_contrast``, over
    the components ``free`` marks (the default frees the rotation rate).  ``step``: the first step length, in the units of
    ``theta`` (a rate per unit of the time stamps).

    ``resident=False``: a HOST loop (``align_loop``).  Every evaluation reads 8 + 7 doubles back (the statistics and the
    gradient: one synchronisation each), so this form is a convenience for a few dozen evaluations, not a hot path.  Returns
    a dict: ``correction`` (list of 7 floats), ``variance``, ``variance0`` (at the start) and ``history`` (the accepted
    variances, strictly rising).

    ``resident=True``: the same loop on the device (include/ramp_hip.h ``ramp_event_align``): one C call enqueues the whole
    alignment, ordered on the current stream, nothing is read back and nothing synchronised.  The arguments are checked as
    ``event_contrast`` checks them; the start is read as float32, as every evaluation reads its correction.  ``max_evals``:
    the evaluations enqueued; None means ``1 + 9 * iters``, with which the answer is the host loop's bit for bit; a smaller
    budget ends with reason ``budget`` at the last accepted point.  Nobody has tuned this default: evaluations behind the
    end of the search are empty launches, which still cost their enqueue.  Returns a dict of device tensors: ``correction``
    float64 [7], ``correction_f32`` float32 [7] (the bits the evaluation at ``correction`` read: pass it to
    ``event_contrast(correction=...)``), ``variance`` and ``variance0`` (0-d views of ``result`` float64 [4]: variance,
    variance0, the final step length, 0), ``grad`` float64 [7] at ``correction``, ``history`` float64 [iters] (NaN behind the
    accepted steps), ``status`` int32 [8] (the words of the evaluation at ``correction``) and ``info`` int32 [8]
    (``event_align_info``)."""
    if len(free) != 7:
        raise RuntimeError("event_align: free marks the 7 components of (v[3], w[3], lam)")
    if not resident:
        if max_evals is not None:
            raise RuntimeError("event_align: max_evals belongs to resident=True")

        def evaluate(theta):
            r = event_contrast(x, y, t, p, knots, times, t_ref, intrinsics, invdepth, height, width, correction=theta,
                               signed=signed, extrapolate=extrapolate)
            both = torch.cat([r["stats"], r["grad"]]).cpu().tolist()           # (the 8 + 7 doubles)
            return both[0], both[8:]

        return align_loop(evaluate, [0.0] * 7 if correction is None else torch.as_tensor(correction).reshape(-1).tolist(), free,
                          step, iters)
    xf, yf, tf, pi, knots, times, K, d, flags = _event_arguments("event_align", x, y, t, p, knots, times, intrinsics,
                                                                 invdepth, height, width, extrapolate)
    dev, N, T = xf.device, xf.shape[0], knots.shape[0]
    if not signed:
        flags |= _lib.RAMP_CONTRAST_UNSIGNED
    cor = _correction("event_align", correction, dev)
    iters = int(iters)
    if iters < 0 or iters > _lib.RAMP_ALIGN_MAX_ITERS:
        raise RuntimeError("event_align: iters is 0 .. %d" % _lib.RAMP_ALIGN_MAX_ITERS)
    need = 1 + _lib.RAMP_ALIGN_TRIALS * iters
    max_evals = need if max_evals is None else int(max_evals)
    if max_evals < 1:
        raise RuntimeError("event_align: max_evals is at least 1")
    res = {"correction": torch.zeros(7, dtype=torch.float64, device=dev),
           "correction_f32": torch.zeros(7, dtype=torch.float32, device=dev),
           "result": torch.zeros(4, dtype=torch.float64, device=dev), "grad": torch.zeros(7, dtype=torch.float64, device=dev),
           "history": torch.zeros(iters, dtype=torch.float64, device=dev),
           "status": torch.zeros(8, dtype=torch.int32, device=dev), "info": torch.zeros(8, dtype=torch.int32, device=dev)}
    res["variance"], res["variance0"] = res["result"][0], res["result"][1]
    ws, nbytes = sized_workspace("ramp_event_align_workspace_bytes", (T, height, width), dev, "evcontrast")
    check(lib().ramp_event_align(ptr(xf), ptr(yf), ptr(tf), ptr(pi), N, ptr(knots), ptr(times), T, float(t_ref), ptr(K), ptr(d),
                                 ptr(cor), flags, height, width, sum(1 << i for i, f in enumerate(free) if f), float(step),
                                 iters, min(max_evals, need), ptr(res["correction"]), ptr(res["correction_f32"]),
                                 ptr(res["result"]), ptr(res["grad"]), ptr(res["history"]) if iters else None,
                                 ptr(res["status"]), ptr(res["info"]), ptr(ws), nbytes, stream()), "ramp_event_align")
    return res


def event_align_info(info):
    """the info words of ramp_event_align as a dict (synchronises: one 32-byte copy); ``reason``: ``iters`` (the accepted
    steps asked for), ``stalled`` (a direction failed its 9 trials), ``flat`` (a masked gradient that is zero or not finite)
    or ``budget`` (``max_evals`` ran out)"""
    w = info.detach().cpu()
    return dict(reason=ALIGN_REASONS.get(int(w[0]), "unknown"), n_accepted=int(w[1]), n_evals=int(w[2]), halvings=int(w[3]),
                seen=int(w[4]), bad_times=bool(int(w[4]) & _lib.RAMP_INTERP_BAD_TIMES),
                bad_correction=bool(int(w[4]) & _lib.RAMP_CONTRAST_BAD_CORRECTION))


def invdepth_map(poses, patches, intrinsics, cam, height, width, radius, scale=1, index=None, count=None, conf=None,
                 conf_is_variance=False, prior=None, prior_weight=0.0, prior_relative=False, dyn_rows=None, per_row=0,
                 last_rows=0, want_weight=True, want_records=False):
    """Dense inverse-depth map from patches (include/ramp_hip.h ``ramp_invdepth_map``): the selected patches are projected
    into the pose ``cam`` and regressed with a biweight kernel of support ``radius`` (image pixels) -- the [height, width]
    map ``event_warp`` takes as ``invdepth``.

    ``poses`` [n,7] world-to-camera, ``patches`` [n*M,3,P,P] (or [n,M,3,P,P]; M = patches per pose row), ``intrinsics`` row 0
    (fx, fy, cx, cy) at patch resolution, image pixel = ``scale`` x patch coordinate; ``cam`` [7] a device CAMERA-TO-WORLD
    pose, a row of ``Ramp_vo.trajectory()`` / ``poses_at()``.  ``index`` / ``count``: the selection as ``map_select`` returns
    it (device int32 list and device count; ``count=None``: the whole list), or None for all patches -- with ``last_rows``
    the newest ``last_rows * per_row`` of them.  ``dyn_rows``: a device int32 word that clips the patches to ``dyn_rows *
    per_row`` on the device.  ``conf`` [n*M]: per-patch confidence, or variance with ``conf_is_variance`` (c = 1 / conf).
    ``prior``: a float or a one-element device tensor, weighted ``prior_weight``, or ``prior_weight / prior**2`` with
    ``prior_relative``.  Device tensors, ordered on the current stream, nothing synchronised.

    Returns a dict of device tensors: ``invdepth`` [height, width] (NaN where neither a patch nor a prior reaches),
    ``status`` int32 [8] (``invdepth_map_status``) and, as requested, ``weight`` [height, width] (the summed kernel weight)
    and ``records`` [K,4] (u, v, d', c per slot of the selection; weight 0: rejected)."""
    require_cuda(poses, patches, cam, index, count, conf, dyn_rows)
    dev = cam.device
    P = patches.shape[-1]
    poses = poses.reshape(-1, 7)
    n = patches.numel() // (3 * P * P)
    if poses.dtype != torch.float32 or patches.dtype != torch.float32 or not (poses.is_contiguous() and patches.is_contiguous()):
        raise RuntimeError("invdepth_map: poses and patches are contiguous float32")
    if n and (poses.shape[0] == 0 or n % poses.shape[0]):
        raise RuntimeError("invdepth_map: %d patches do not divide into %d pose rows" % (n, poses.shape[0]))
    M = max(n // max(poses.shape[0], 1), 1)
    K4 = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev).reshape(-1)[:4].contiguous()
    camf = cam.reshape(7).to(torch.float32).contiguous()
    for name, x in (("index", index), ("count", count), ("dyn_rows", dyn_rows)):
        if x is not None and (x.dtype != torch.int32 or not x.is_contiguous()):
            raise RuntimeError("invdepth_map: %s is a contiguous int32 tensor" % name)
    if count is not None and index is None:
        raise RuntimeError("invdepth_map: a count needs an index")
    if conf is not None:
        conf = conf.reshape(-1)
        if conf.dtype != torch.float32 or not conf.is_contiguous() or conf.numel() < n:
            raise RuntimeError("invdepth_map: conf is contiguous float32, one entry per patch")
    if isinstance(prior, torch.Tensor):
        require_cuda(prior)
        pr = prior.reshape(-1)[:1].to(torch.float32).contiguous()
    elif prior is not None:
        pr = torch.full((1,), float(prior), dtype=torch.float32, device=dev)
    else:
        pr = None
    Ki = int(index.numel()) if index is not None else 0
    Kc = Ki if index is not None else (min(n, int(last_rows) * int(per_row)) if last_rows > 0 else n)
    flags = (_lib.RAMP_DEPTHMAP_CONF_IS_VARIANCE if conf_is_variance else 0) | (_lib.RAMP_DEPTHMAP_PRIOR_RELATIVE if prior_relative else 0)
    res = {"status": torch.zeros(8, dtype=torch.int32, device=dev),
           "invdepth": torch.empty((height, width), dtype=torch.float32, device=dev)}
    if want_weight:
        res["weight"] = torch.empty((height, width), dtype=torch.float32, device=dev)
    if want_records:
        res["records"] = torch.empty((Kc, 4), dtype=torch.float32, device=dev)
    ws, nbytes = sized_workspace("ramp_invdepth_map_workspace_bytes", (Kc,), dev, "depthmap")
    check(lib().ramp_invdepth_map(ptr(poses), ptr(patches), ptr(K4), ptr(camf), n, M, P, float(scale), ptr(index), ptr(count),
                                  Ki, ptr(dyn_rows), int(per_row), int(last_rows), ptr(conf), ptr(pr), float(prior_weight),
                                  float(radius), flags, int(height), int(width), ptr(res["invdepth"]), ptr(res.get("weight")),
                                  ptr(res.get("records")), ptr(ws), nbytes, ptr(res["status"]), stream()), "ramp_invdepth_map")
    return res


def invdepth_map_status(status):
    """The status words of ``invdepth_map`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("invdepth_map", status)


def depth_median_fill(patches_state, n, F, patches_new):
    """patches_new[:, 2] = median of patches_state[n-F:n, :, 2] (reference Ramp_vo.py:370-371), one launch.
    patches_state [N,M,3,P,P], patches_new [M,3,P,P] (both contiguous fp32)"""
    require_cuda(patches_state, patches_new)
    _, M, _, P, _ = patches_state.shape
    assert patches_state.is_contiguous() and patches_new.is_contiguous() and n - F >= 0
    check(lib().ramp_depth_median_fill(ptr(patches_state[n - F]), F, M, P, ptr(patches_new), stream()),
          "ramp_depth_median_fill")


def depth_median_supported(F, M, P):
    return F * M * P * P <= 8192


def event_topk(events, k, nms_kernel_size=11, want_indices=False, out=None):
    """patch centres of one frame: events [bins,H,W] float32 -> coords [k,2] float32 (x + y/h, y) at the
    top-k cells of the NMS'ed mean |event| map (reference utils.py:186-226), one score kernel + one NMS
    kernel + a one-workgroup radix select"""
    require_cuda(events)
    bins, H, W = events.shape
    events = events.contiguous().float()
    coords = out if out is not None else torch.empty((k, 2), dtype=torch.float32, device=events.device)
    assert coords.shape == (k, 2) and coords.dtype == torch.float32 and coords.is_contiguous()
    idx = torch.empty(k, dtype=torch.int64, device=events.device) if want_indices else None
    ws, nbytes = sized_workspace("ramp_event_topk_workspace_bytes", (H, W), events.device, "topk")
    check(lib().ramp_event_topk(ptr(events), bins, H, W, int(k), int(nms_kernel_size), ptr(coords),
                                ptr(idx) if idx is not None else None, ptr(ws), nbytes, stream()),
          "ramp_event_topk")
    return (coords, idx) if want_indices else coords


def event_topk_supported(events, k, nms_kernel_size):
    return (events.dim() == 3 and events.shape[2] % 4 == 0 and events.shape[1] >= 4 and k <= 512
            and k <= (events.shape[1] // 4) * (events.shape[2] // 4) and (nms_kernel_size == 0 or (nms_kernel_size % 2 == 1 and nms_kernel_size <= 17)))


def pyramid_pack(fmap, out1=None, out4=None, split=None):
    """NHWC map [H,W,128] -> (level1 [H,4,W,32], level4 [H/4,4,W/4,32]) (fp16) or ([H,8,W,16], [H/4,8,W/4,16]) (fp32) in the
    correlation kernel's packed target layout (RAMP_NHWC32: 64 bytes per pixel and plane); level4 is the 4x4 mean
    (Ramp_vo.py:378-381; fp32: torch's avg_pool2d to the bit).  fp32 with ``split`` (default: corr_f32_mode() == 2): the two
    float32 containers hold split fp16 parts [H,4,2,W,32] (x = hi + lo 2^-11; unpack_split() decodes them) for
    corr(..., fast_f32=2)"""
    require_cuda(fmap)
    H, W, C = fmap.shape
    assert fmap.dtype in (torch.float16, torch.float32) and fmap.is_contiguous()
    if split is None:
        split = _lib.corr_f32_mode() == 2
    split = bool(split) and fmap.dtype == torch.float32
    kp = kplane(fmap.dtype)
    if out1 is None:
        out1 = torch.empty((H, C // kp, W, kp), dtype=fmap.dtype, device=fmap.device)
    if out4 is None:
        out4 = torch.empty((H // 4, C // kp, W // 4, kp), dtype=fmap.dtype, device=fmap.device)
    check(lib().ramp_pyramid_pack(ptr(fmap), ptr(out1), ptr(out4), H, W, C,
                                  dtype_code(fmap) | (_LIB_CORR_X2 if split else 0), stream()), "ramp_pyramid_pack")
    return out1, out4


def pack_split(rows):
    """float32 rows [..., H, W, 128] -> the float32 container [..., H, 8, W, 16] of split fp16 pairs, in torch (the
    arithmetic of csrc/altcorr.hip::corr_split2: load_state_dict, tests); pyramid_pack(split=True) is the kernel"""
    assert rows.dtype == torch.float32 and rows.shape[-1] == 128
    lead, (H, W) = rows.shape[:-3], rows.shape[-3:-1]
    hi = torch.where(rows.abs() < 6.103515625e-5, torch.zeros_like(rows), rows.half().float())
    lo = ((rows - hi) * 2048.0).half()
    v = torch.stack((hi.half(), lo), -2)                                  # [.., H, W, 2, 128]
    n = len(lead)
    v = v.view(*lead, H, W, 2, 4, 32).permute(*range(n), n, n + 3, n + 2, n + 1, n + 4).contiguous()   # [.., H, 4, 2, W, 32]
    return v.view(torch.float32).view(*lead, H, 8, W, 16)


def unpack_split(planes):
    """float32 container [..., H, 8, W, 16] of split fp16 pairs (pyramid_pack(split=True)) -> (hi, lo) fp16 tensors
    [..., H, W, 128]: the value is hi + lo * 2**-11 (tests, debugging)"""
    lead, (H, _, W, _) = planes.shape[:-4], planes.shape[-4:]
    v = planes.contiguous().view(torch.float16).view(*lead, H, 4, 2, W, 32)
    n = len(lead)
    perm = tuple(range(n)) + (n + 2, n, n + 3, n + 1, n + 4)          # [.., 2, H, W, 4, 32]
    v = v.permute(*perm).reshape(*lead, 2, H, W, 128)
    return v.select(n, 0), v.select(n, 1)


def pyramid_pack_supported(H, W, C=128):
    return C == 128 and W % 16 == 0 and H % 4 == 0


# ------------------------------------------------------------------ lietorch
def _flat(x, dim):
    return x.reshape(-1, dim).contiguous().float()


def se3_unary(name, x, din, dout):
    require_cuda(x)
    shp = x.shape[:-1]
    x2 = _flat(x, din)
    out = torch.empty((x2.shape[0], dout), dtype=torch.float32, device=x.device)
    check(getattr(lib(), name)(ptr(x2), ptr(out), x2.shape[0], stream()), name)
    return out.view(shp + (dout,))


def se3_binary(name, x, y, dx, dy, dout):
    require_cuda(x, y)
    bs = torch.broadcast_shapes(x.shape[:-1], y.shape[:-1])
    x2 = x.float().expand(bs + (dx,)).reshape(-1, dx).contiguous()
    y2 = y.float().expand(bs + (dy,)).reshape(-1, dy).contiguous()
    out = torch.empty((x2.shape[0], dout), dtype=torch.float32, device=x.device)
    check(getattr(lib(), name)(ptr(x2), ptr(y2), ptr(out), x2.shape[0], stream()), name)
    return out.view(bs + (dout,))


# ---------------------------------------------------------------- poses at any time
def se3_interp(knots, times, query, extrapolate=False, twist=False, row_stores=False):
    """The SE(3) geodesic through ``knots`` [T,7] at time stamps ``times`` [T] (float64, non-decreasing), evaluated at ``query``
    [Q] (float64): ``X(t) = Exp(alpha * Log(X[s+1] X[s]^-1)) X[s]`` (include/ramp_hip.h ``ramp_se3_interp``, two launches).
    Device tensors in and out, ordered on the current stream, nothing synchronised.

    Returns ``(poses [Q,7], twist [Q,6] or None, status int32 [4])``; status: bits (bit 0: ``times`` decreases or is not
    finite -- every row is NaN then), queries below the range, above it, NaN queries.  Outside the range alpha is clamped,
    or with ``extrapolate`` the end segment's screw motion is continued.  ``row_stores``: the other store form of the query
    launch (same bits; tools/pose_query_cost.py)."""
    require_cuda(knots, times, query)
    knots = knots.reshape(-1, 7).contiguous().float()
    times = times.reshape(-1).contiguous().double()
    query = query.reshape(-1).contiguous().double()
    T, Q = knots.shape[0], query.shape[0]
    if times.shape[0] != T:
        raise RuntimeError("se3_interp: %d knots but %d time stamps" % (T, times.shape[0]))
    dev = knots.device
    out = torch.empty((Q, 7), dtype=torch.float32, device=dev)
    tw = torch.empty((Q, 6), dtype=torch.float32, device=dev) if twist else None
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    nbytes = lib().ramp_se3_interp_workspace_bytes(T)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    flags = (_lib.RAMP_INTERP_EXTRAPOLATE if extrapolate else 0) | (_lib.RAMP_INTERP_ROW_STORES if row_stores else 0)
    check(lib().ramp_se3_interp(ptr(knots), ptr(times), T, ptr(query), Q, flags, ptr(out), ptr(tw), ptr(ws), nbytes,
                                ptr(status), stream()), "ramp_se3_interp")
    return out, tw, status


def se3_interp_status(status):
    """The status words of ``se3_interp`` as a dict: the bits of word 0 by name, then the counters (synchronises: one small copy)."""
    return _status("se3_interp", status)


# ----------------------------------------------------------- projective ops
def _idx(t):
    assert t.dtype == torch.int64
    return t.contiguous()


def _geometry(poses, patches, intrinsics):
    """poses [..,7], patches [..,3,P,P], intrinsics [..,4] as the flat contiguous fp32 tensors the kernels read, and P"""
    P = patches.shape[-1]
    return (poses.reshape(-1, 7).contiguous().float(), patches.reshape(-1, 3, P, P).contiguous().float(),
            intrinsics.reshape(-1, 4).contiguous().float(), P)


def transform(poses, patches, intrinsics, ii, jj, kk, tonly=False):
    """Ramp_vo.reproject: poses [..,7], patches [..,3,P,P], intrinsics [..,4] -> [1,E,2,P,P]"""
    require_cuda(poses, patches, intrinsics, ii, jj, kk)
    P = patches.shape[-1]
    f32 = torch.float32
    if not (poses.dtype == f32 and patches.dtype == f32 and intrinsics.dtype == f32 and poses.is_contiguous()
            and patches.is_contiguous() and intrinsics.is_contiguous()):        # (the tracker's buffers are)
        poses, patches, intrinsics, P = _geometry(poses, patches, intrinsics)
    E = ii.shape[0]
    out = torch.empty((1, E, 2, P, P), dtype=torch.float32, device=poses.device)
    check(lib().ramp_transform(ptr(poses), ptr(patches), ptr(intrinsics), ptr(_idx(ii)),
                               ptr(_idx(jj)), ptr(_idx(kk)), ptr(out), E, P, int(bool(tonly)),
                               stream()), "ramp_transform")
    return out


def reproject(poses, patches, intrinsics, ii, jj, kk):
    """cuda_ba.reproject -> [1,E,2,P,P]"""
    require_cuda(poses, patches, intrinsics, ii, jj, kk)
    poses, patches, intrinsics, P = _geometry(poses, patches, intrinsics)
    E = ii.shape[0]
    out = torch.empty((1, E, 2, P, P), dtype=torch.float32, device=poses.device)
    check(lib().ramp_reproject(ptr(poses), ptr(patches), ptr(intrinsics), ptr(_idx(ii)),
                               ptr(_idx(jj)), ptr(_idx(kk)), ptr(out), E, P, stream()),
          "ramp_reproject")
    return out


def point_cloud(poses, patches, intrinsics, ix):
    """3-D point of every patch centre: patches [m,3,P,P] (or [1,m,..]), ix [m] -> [m,3]"""
    require_cuda(poses, patches, intrinsics, ix)
    poses, patches, intrinsics, P = _geometry(poses, patches, intrinsics)
    m = ix.shape[0]
    assert patches.shape[0] >= m
    out = torch.empty((m, 3), dtype=torch.float32, device=poses.device)
    check(lib().ramp_point_cloud(ptr(poses), ptr(patches), ptr(intrinsics), ptr(_idx(ix)),
                                 ptr(out), m, P, stream()), "ramp_point_cloud")
    return out


def motionmag(poses, patches, intrinsics, ii, jj, kk, pair_groups, key_ij, key_ji, beta=0.5):
    """[mean flow i->j, mean flow j->i] (device tensor [2]); pair_groups: the (ii, jj) grouping"""
    require_cuda(poses, patches, intrinsics, ii, jj, kk)
    poses, patches, intrinsics, P = _geometry(poses, patches, intrinsics)
    out = torch.empty(2, dtype=torch.float32, device=poses.device)
    g = pair_groups
    check(lib().ramp_motionmag(ptr(poses), ptr(patches), ptr(intrinsics), ptr(_idx(ii)), ptr(_idx(jj)),
                               ptr(_idx(kk)), ptr(g.order), ptr(g.seg_start), ptr(g.ukeys), ptr(g.ngroups),
                               int(key_ij), int(key_ji), float(beta), ptr(out), P, stream()), "ramp_motionmag")
    return out


def multi_copy(pairs):
    """pairs: list of (src_tensor, dst_tensor) with equal byte sizes, both contiguous; one launch"""
    n = len(pairs)
    src = (ctypes.c_void_p * n)(*[s.data_ptr() for s, _ in pairs])
    dst = (ctypes.c_void_p * n)(*[d.data_ptr() for _, d in pairs])
    nbytes = (ctypes.c_long * n)(*[s.numel() * s.element_size() for s, _ in pairs])
    for s, d in pairs:
        assert s.is_contiguous() and d.is_contiguous() and s.numel() * s.element_size() == d.numel() * d.element_size()
    check(lib().ramp_multi_copy(src, dst, nbytes, n, stream()), "ramp_multi_copy")


def _row_copies(srcs, bufs, rows=None):
    """descriptor arrays (src, dst, row_bytes) and the row sizes in bytes for: contiguous tensor srcs[i] -> one row of the
    contiguous buffer bufs[i]; row rows[i], or with rows=None dst is left for the caller to fill"""
    n = len(srcs)
    rb = [b.stride(0) * b.element_size() for b in bufs]
    for s_, b, nb in zip(srcs, bufs, rb):
        assert s_.numel() * s_.element_size() == nb and s_.is_contiguous() and b.is_contiguous()
    src = (ctypes.c_void_p * n)(*[s_.data_ptr() for s_ in srcs])
    dst = (ctypes.c_void_p * n)(*([] if rows is None else [b.data_ptr() + int(r) * nb for b, r, nb in zip(bufs, rows, rb)]))
    return src, dst, (ctypes.c_long * n)(*rb), rb


def store_rows(srcs, rows):
    """one launch: contiguous tensor srcs[i] -> row rows[i][1] of the contiguous buffer rows[i][0] (no view tensors)"""
    src, dst, rbc, _ = _row_copies(srcs, [b for b, _ in rows], [r for _, r in rows])
    check(lib().ramp_multi_copy(src, dst, rbc, len(srcs), stream()), "ramp_multi_copy")


def depth_median(patches_state, n, frames, out):
    """median depth of patches_state[n - frames : n] into the device scalar ``out`` (ramp_depth_median)"""
    _, M, _, P, _ = patches_state.shape
    check(lib().ramp_depth_median(ptr(patches_state[n - frames]), int(frames), M, P, ptr(out), stream()),
          "ramp_depth_median")


def depth_median_rows(patches_state, n_dev, frames, out):
    """the same with the row count read on the device: the median of rows n - frames .. n - 1, n = ``n_dev[0]`` (int32)"""
    _, M, _, P, _ = patches_state.shape
    check(lib().ramp_depth_median_rows(ptr(patches_state), ptr(n_dev), int(frames), M, P, ptr(out), stream()),
          "ramp_depth_median_rows")


def frame_commit(poses, n, motion, damping, tstamps, counter, index_map, index_val, intrinsics, copy_k, patches_state,
                 median_frames, patches_new, srcs, rows, median_dev=None):
    """ramp_frame_commit: frame_begin + depth_median_fill + the state stores of one frame in one launch;
    srcs[i] -> row rows[i][1] of buffer rows[i][0] (like store_rows), patches_new -> patches_state[n];
    median_dev: the median of the last ``median_frames`` frames if the caller computed it ahead (depth_median)"""
    src, dst, rbc, _ = _row_copies(srcs, [b for b, _ in rows], [r for _, r in rows])
    _, M, _, P, _ = patches_state.shape
    check(lib().ramp_frame_commit(ptr(poses), int(n), int(motion), float(damping), ptr(tstamps), int(counter),
                                  ptr(index_map), int(index_val), ptr(intrinsics), int(bool(copy_k)), ptr(patches_state),
                                  int(median_frames), M, P, ptr(patches_new), len(srcs), src, dst, rbc,
                                  ptr(median_dev), stream()), "ramp_frame_commit")


class FrameCommitPlan:
    """ramp_frame_commit for a fixed set of sources / destination buffers: the descriptor arrays are built once, a
    call only fills in the destination rows (this launch sits between the keyframe read-back and the correlation
    kernel, where the host is the limiter)"""

    def __init__(self, srcs, bufs, patches_state):
        self.n_copy = len(srcs)
        self.keep = (list(srcs), list(bufs), patches_state)
        self.src, self.dst, self.rbc, self.rb = _row_copies(srcs, bufs)
        self.base = [b.data_ptr() for b in bufs]
        _, self.M, _, self.P, _ = patches_state.shape
        self.src_ptrs = tuple(s_.data_ptr() for s_ in srcs)

    def run(self, poses, n, motion, damping, tstamps, counter, index_map, index_val, intrinsics, copy_k, patches_state,
            median_frames, patches_new, rows, median_dev=None):
        for i in range(self.n_copy):
            self.dst[i] = self.base[i] + int(rows[i]) * self.rb[i]
        check(lib().ramp_frame_commit(ptr(poses), int(n), int(motion), float(damping), ptr(tstamps), int(counter),
                                      ptr(index_map), int(index_val), ptr(intrinsics), int(bool(copy_k)),
                                      ptr(patches_state), int(median_frames), self.M, self.P, ptr(patches_new),
                                      self.n_copy, self.src, self.dst, self.rbc, ptr(median_dev), stream()),
              "ramp_frame_commit")


class ShiftPlan:
    """ramp_shift_rows for a fixed set of buffers -- bufs: list of (tensor [rows, ...], ring_modulus or 0) -- whose
    descriptor arrays are built once; run(k, nrows): rows k+1..nrows-1 move down by one"""

    def __init__(self, bufs):
        n = self.n = len(bufs)
        for t, _ in bufs:
            assert t.is_contiguous()
        self.keep = [t for t, _ in bufs]
        self.base = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in bufs])
        self.rb = (ctypes.c_long * n)(*[t[0].numel() * t.element_size() for t, _ in bufs])
        self.mod = (ctypes.c_int * n)(*[int(m) for _, m in bufs])

    def run(self, k, nrows):
        check(lib().ramp_shift_rows(self.base, self.rb, self.mod, self.n, int(k), int(nrows), stream()),
              "ramp_shift_rows")


def motion_model(poses, n, damping):
    """in place: poses[n] = Exp(damping * Log(poses[n-1] * poses[n-2]^-1)) * poses[n-1]"""
    require_cuda(poses)
    assert poses.dtype == torch.float32 and poses.is_contiguous()
    check(lib().ramp_motion_model(ptr(poses), int(n), float(damping), stream()), "ramp_motion_model")


def frame_begin(poses, n, motion, damping, tstamps, counter, index_map, index_val, intrinsics, copy_k):
    """one launch for the per-frame bookkeeping (reference Ramp_vo.py:345-363); see include/ramp_hip.h"""
    require_cuda(poses, tstamps, index_map, intrinsics)
    assert poses.dtype == torch.float32 and poses.is_contiguous() and intrinsics.is_contiguous()
    assert tstamps.dtype == torch.long and index_map.dtype == torch.long
    check(lib().ramp_frame_begin(ptr(poses), int(n), int(motion), float(damping), ptr(tstamps), int(counter),
                                 ptr(index_map), int(index_val), ptr(intrinsics), int(bool(copy_k)), stream()),
          "ramp_frame_begin")


# --------------------------------------------------------------------- graph
class Groups:
    """result of group_by: order/gid/seg_start/ukeys/ngroups (device tensors)"""
    __slots__ = ("order", "gid", "seg_start", "ukeys", "ngroups", "E")


def _new_groups(E, dev):
    g = Groups()
    g.E = E
    g.order = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    g.gid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    g.seg_start = torch.empty(E + 1, dtype=torch.int32, device=dev)
    g.ukeys = torch.empty(max(E, 1), dtype=torch.int64, device=dev)
    g.ngroups = torch.empty(1, dtype=torch.int32, device=dev)
    return g


def group_by(keys, key_bound=0):
    require_cuda(keys)
    keys = _idx(keys)
    E = keys.shape[0]
    dev = keys.device
    g = _new_groups(E, dev)
    ws, nbytes = sized_workspace("ramp_group_by_workspace_bytes", (E,), dev, "graph")
    check(lib().ramp_group_by(ptr(keys), E, int(key_bound), ptr(g.order), ptr(g.gid),
                              ptr(g.seg_start), ptr(g.ukeys), ptr(g.ngroups), ptr(ws),
                              ws.numel(), stream()), "ramp_group_by")
    return g


def group_by_small(a, b, mul, sub, K, max_groups=0):
    """group_by for keys a*mul + b - sub known to lie in [0, K) (counting sort, 5 short kernels); a key outside the
    range gives the empty grouping (ngroups 0).  max_groups: an upper bound on the number of groups, 0 = min(K, E)"""
    require_cuda(a)
    a = _idx(a)
    b = _idx(b) if b is not None else None
    E = a.shape[0]
    dev = a.device
    g = _new_groups(E, dev)
    ws, nbytes = sized_workspace("ramp_group_by_small_workspace_bytes", (E, int(K)), dev, "graph")
    check(lib().ramp_group_by_small(ptr(a), ptr(b), int(mul), int(sub), int(K), E, ptr(g.order), ptr(g.gid),
                                    ptr(g.seg_start), ptr(g.ukeys), ptr(g.ngroups), int(max_groups), ptr(ws),
                                    ws.numel(), stream()), "ramp_group_by_small")
    return g


def neighbors_from_groups(groups, jj, max_groups, want_kj=False):
    """cuda_ba.neighbors(kk, jj) from the per-kk groups (no extra sort); want_kj: also the factors in (kk, jj) order"""
    require_cuda(jj)
    jj = _idx(jj)
    E = jj.shape[0]
    ix = torch.empty(E, dtype=torch.int64, device=jj.device)
    jx = torch.empty(E, dtype=torch.int64, device=jj.device)
    kj = torch.empty(E, dtype=torch.int32, device=jj.device) if want_kj else None
    check(lib().ramp_neighbors_from_groups(ptr(groups.order), ptr(groups.seg_start), ptr(groups.ngroups), ptr(jj),
                                           ptr(ix), ptr(jx), ptr(kj), E, int(max_groups), stream()),
          "ramp_neighbors_from_groups")
    return (ix, jx, kj) if want_kj else (ix, jx)


def neighbors(kk, jj, kk_bound=0, jj_bound=0):
    require_cuda(kk, jj)
    kk, jj = _idx(kk), _idx(jj)
    E = kk.shape[0]
    ix = torch.empty(E, dtype=torch.int64, device=kk.device)
    jx = torch.empty(E, dtype=torch.int64, device=kk.device)
    if E == 0:
        return ix, jx
    ws, nbytes = sized_workspace("ramp_neighbors_workspace_bytes", (E,), kk.device, "graph")
    check(lib().ramp_neighbors(ptr(kk), ptr(jj), ptr(ix), ptr(jx), E, int(kk_bound),
                               int(jj_bound), ptr(ws), ws.numel(), stream()), "ramp_neighbors")
    return ix, jx


def segment_softmax_sum(fx, gx, groups, max_groups):
    """y[g] = sum_{e in g} softmax_e(gx[e]) * fx[e];  fx,gx [E,C] -> y [max_groups,C]"""
    require_cuda(fx, gx)
    fx = fx.contiguous()
    gx = gx.contiguous()
    assert fx.dtype == gx.dtype and fx.shape == gx.shape
    E, C = fx.shape
    y = torch.zeros((max_groups, C), dtype=fx.dtype, device=fx.device)
    check(lib().ramp_segment_softmax_sum(ptr(fx), ptr(gx), ptr(groups.order),
                                         ptr(groups.seg_start), ptr(groups.ngroups), ptr(y), E, C,
                                         int(max_groups), dtype_code(fx), stream()),
          "ramp_segment_softmax_sum")
    return y


# -------------------------------------------------------------------- fastba
def _ba_problem(what, poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, plan):
    """what ba and ba_covariance share: the checks, then ``head`` (every C entry's arguments up to t1), ``sizes`` (the
    workspace queries' arguments), the plan's ``groups`` (None without one: the planned entries' group arguments, and the
    two bounds of their workspace queries) and the converted tensors behind the pointers, to be kept until the call"""
    require_cuda(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk)
    for t in (poses, patches):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(what + " poses/patches in place: contiguous float32 required")
    P = patches.shape[-1]
    n_poses = poses.numel() // 7
    n_patches = patches.numel() // (3 * P * P)
    intrinsics = intrinsics.reshape(-1, 4).contiguous().float()
    target = target.reshape(-1, 2).contiguous().float()
    weight = weight.reshape(-1, 2).contiguous().float()
    lmbda = lmbda.reshape(-1).contiguous().float()
    E = ii.shape[0]
    assert target.shape[0] == E and weight.shape[0] == E
    keep = (intrinsics, target, weight, lmbda, _idx(ii), _idx(jj), _idx(kk))
    sizes = (E, n_poses, n_patches, int(t0), int(t1))
    head = (ptr(poses), ptr(patches), *(ptr(t) for t in keep), E, P, n_poses, n_patches, int(t0), int(t1))
    groups = None
    if plan is not None:
        # groupings shared with the update operator (GraphPlan): no sort inside BA
        gk, gp = plan.g_kk, plan.g_ij
        mk, mp = max(int(plan.max_kk), 1), max(int(plan.max_ij), 1)
        groups = ((ptr(gk.order), ptr(gk.seg_start), ptr(gk.ngroups), ptr(gk.ukeys), mk, ptr(gp.order), ptr(gp.seg_start),
                   ptr(gp.ngroups), mp), (mk, mp))
    return head, sizes, groups, keep


def ba(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, iterations=2,
       info=None, plan=None):
    """in-place bundle adjustment (cuda_ba.forward).  poses [..,7] and patches
    [..,3,P,P] must be contiguous float32 views of the caller's storage."""
    head, sizes, groups, _keep = _ba_problem("BA mutates", poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk,
                                             t0, t1, plan)
    if groups is not None:
        ws = _lib.workspace(lib().ramp_ba_planned_workspace_bytes(*sizes, *groups[1]), poses.device, "ba")
        check(lib().ramp_ba_forward_planned(*head, int(iterations), *groups[0], ptr(ws), ws.numel(), ptr(info), stream()),
              "ramp_ba_forward_planned")
        return
    ws = _lib.workspace(lib().ramp_ba_workspace_bytes(*sizes), poses.device, "ba")
    check(lib().ramp_ba_forward(*head, int(iterations), ptr(ws), ws.numel(), ptr(info), stream()), "ramp_ba_forward")


def _ba_covariance(entry, poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, info, plan, extra=()):
    """ramp_ba_covariance / ramp_ba_map_covariance (``entry``), self-grouped or planned; ``extra``: the output tensors behind
    stats"""
    head, sizes, groups, _keep = _ba_problem(entry[5:] + " reads", poses, patches, intrinsics, target, weight, lmbda, ii,
                                             jj, kk, t0, t1, plan)
    n_patches, n6 = sizes[2], 6 * max(sizes[4] - sizes[3], 0)
    dev = poses.device
    cov = torch.empty((n6, n6), dtype=torch.float32, device=dev)
    depth_var = torch.full((n_patches,), float("inf"), dtype=torch.float32, device=dev)
    stats = torch.zeros(8, dtype=torch.float32, device=dev)
    outs = (ptr(cov), ptr(depth_var), ptr(stats)) + tuple(ptr(x) for x in extra)
    if groups is not None:
        ws = _lib.workspace(getattr(lib(), entry + "_planned_workspace_bytes")(*sizes, *groups[1]), dev, "ba")
        check(getattr(lib(), entry + "_planned")(*head, *outs, *groups[0], ptr(ws), ws.numel(), ptr(info), stream()),
              entry + "_planned")
    else:
        ws = _lib.workspace(getattr(lib(), entry + "_workspace_bytes")(*sizes), dev, "ba")
        check(getattr(lib(), entry)(*head, *outs, ptr(ws), ws.numel(), ptr(info), stream()), entry)
    return cov, depth_var, stats


def ba_covariance(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, info=None, plan=None):
    """marginal covariance of the free poses and marginal depth variances of the window (include/ramp_hip.h
    ``ramp_ba_covariance``): returns (cov [6N, 6N], depth_var [n_patches] pre-filled with inf, stats [8] raw words).
    The inputs are only read."""
    return _ba_covariance("ramp_ba_covariance", poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, info,
                          plan)


def map_outputs(n_patches, device):
    """the four map outputs of ramp_ba_map_covariance / ramp_track_map as the caller fills them: point [n, 3], point_cov
    [n, 6] and pose_depth_cov [n, 6] NaN (a patch without a factor is never a finite point), n_obs [n] zero"""
    nan = float("nan")
    return (torch.full((n_patches, 3), nan, dtype=torch.float32, device=device),
            torch.full((n_patches, 6), nan, dtype=torch.float32, device=device),
            torch.full((n_patches, 6), nan, dtype=torch.float32, device=device),
            torch.zeros(n_patches, dtype=torch.int32, device=device))


def ba_map_covariance(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, info=None, plan=None, out=None):
    """ba_covariance plus the map (include/ramp_hip.h ``ramp_ba_map_covariance``): returns (cov, depth_var, stats, point
    [n_patches, 3], point_cov [n_patches, 6] (xx, xy, xz, yy, yz, zz), pose_depth_cov [n_patches, 6], n_obs [n_patches]
    int32).  ``out``: the caller's four map tensors (contiguous; ``map_outputs`` otherwise) -- entries of patches without a
    factor are left as they are."""
    P = patches.shape[-1]
    n_patches = patches.numel() // (3 * P * P)
    if out is None:
        out = map_outputs(n_patches, poses.device)
    point, point_cov, pdc, n_obs = out
    require_cuda(*out)
    for x, shape, dt in ((point, (n_patches, 3), torch.float32), (point_cov, (n_patches, 6), torch.float32),
                         (pdc, (n_patches, 6), torch.float32), (n_obs, (n_patches,), torch.int32)):
        if tuple(x.shape) != shape or x.dtype != dt or not x.is_contiguous():
            raise RuntimeError("ba_map_covariance: a map output must be contiguous %s %s" % (dt, shape))
    cov, depth_var, stats = _ba_covariance("ramp_ba_map_covariance", poses, patches, intrinsics, target, weight, lmbda, ii,
                                           jj, kk, t0, t1, info, plan, extra=out)
    return cov, depth_var, stats, point, point_cov, pdc, n_obs


def map_select(point_cov, depth_var, patches, n_obs, max_sigma=None, max_rel_depth_sigma=None, min_obs=0, n=None,
               dyn_rows=None, per_row=0):
    """stable compaction of the map (include/ramp_hip.h ``ramp_map_select``): returns (index [n] int32 -- the selected patch
    ids ascending in its first ``count`` entries, -1 behind them -- and count [1] int32), device tensors; nothing is
    synchronised.  A threshold of None (or +inf / min_obs 0) switches its criterion off.  ``dyn_rows``: a device int32 word
    that clips n to ``dyn_rows * per_row`` on the device."""
    require_cuda(point_cov, depth_var, patches, n_obs)
    P = patches.shape[-1]
    n = int(point_cov.shape[0] if n is None else n)
    assert point_cov.dtype == torch.float32 and depth_var.dtype == torch.float32 and n_obs.dtype == torch.int32
    assert patches.dtype == torch.float32 and patches.is_contiguous() and point_cov.is_contiguous()
    assert depth_var.is_contiguous() and n_obs.is_contiguous()
    assert point_cov.numel() >= 6 * n and depth_var.numel() >= n and n_obs.numel() >= n and patches.numel() >= 3 * P * P * n
    inf = float("inf")
    index = torch.full((max(n, 1),), -1, dtype=torch.int32, device=point_cov.device)
    count = torch.zeros(1, dtype=torch.int32, device=point_cov.device)
    check(lib().ramp_map_select(ptr(point_cov), ptr(depth_var), ptr(patches), ptr(n_obs), n, P, ptr(dyn_rows), int(per_row),
                                inf if max_sigma is None else float(max_sigma),
                                inf if max_rel_depth_sigma is None else float(max_rel_depth_sigma), int(min_obs or 0),
                                ptr(index), ptr(count), stream()), "ramp_map_select")
    return index[:n], count


def ba_covariance_stats(stats):
    """the stats words of ramp_ba_covariance as a dict (synchronises: one 32-byte copy)"""
    w = stats.detach().cpu()
    i = w.view(torch.int32)
    return dict(chi2=float(w[0]), n_valid=int(i[1]), Mu=int(i[2]), N=int(i[3]), t0=int(i[4]), failed=bool(i[5]))
