"""fastba operator surface (reference: ramp/fastba/ba.py:1-8, ba.cpp:183-189)."""
import torch

from . import ops


def BA(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, M=None,
       iterations=2, eff_impl=False, info=None, plan=None):
    """cuda_ba.forward: in-place GN bundle adjustment (reference ba_cuda.cu:433-582).

    ``M`` (patches per frame, the reference's PPF) and ``eff_impl`` select the reference's storage of the pose-depth
    coupling E: a dense [6N x Mu] matrix, or ``EfficentE``'s per-(i, j)-block lookup (fastba/block_e.cu).  Both are the
    same algebra (oracle: ``orc.ba(eff_ppf=M)`` restates the lookup kernels and agrees with the dense restatement to
    rounding).  This implementation has ONE storage and serves both settings with it: one row of 6N values per
    patch that actually occurs in the graph (``Erow [Mu][6N]``, 8.3 MB at configs[4]: Mu = 10,752, 6N = 192), formed
    by an ordered segment sum over the patch's edges and consumed by a split-K SYRK -- neither the dense matrix's
    atomic scatter nor the lookup's (frames x frames) index tensor exists here, so there is nothing for the flag to
    switch.  tests/test_ops_gpu.py::test_ba_eff_impl_at_config5_size pins it against the oracle's lookup path."""
    p = poses.data if hasattr(poses, "data") and not isinstance(poses, torch.Tensor) else poses
    if eff_impl and not M:
        raise ValueError("eff_impl=True needs M (patches per frame), as cuda_ba.forward's PPF")
    if plan is not None:
        ops.ba(p, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, iterations, info, plan=plan)
    else:
        ops.ba(p, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, iterations, info)
    return []


def covariance(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, M=0, info=None, plan=None):
    """Uncertainty of the window: ``(cov [6N, 6N], depth_var [n_patches], stats)`` with N = t1 - t0 free poses.

    The system is the one ``BA`` builds in one iteration, linearised at the state passed in -- same per-factor terms, same
    validity gate, intrinsics row 0, poses outside [t0, t1) fixed -- and no step is taken: the inputs are untouched.
    ``Q = 1 / (C + lmbda)``, ``S = B - E Q E'`` INCLUDING the solver's own diagonal damping ``S_dd += 1e-4 S_dd + 1``: the
    covariance is that of the system the step is actually solved with, not of the undamped normal equations.

    * ``cov = S^-1``, symmetric bit for bit.  Tangent order as the step's (translation 3, rotation 3 per pose); the
      perturbation is the left one of the retraction ``T <- Exp(xi) T`` on the world-to-camera poses.
    * ``depth_var[k] = Q_k + Q_k^2 e_k' S^-1 e_k`` at index ``kk`` for every patch with a factor; the others stay ``inf``.
    * ``stats``: dict(chi2 = sum over valid factors of w0 rx^2 + w1 ry^2, n_valid, Mu, N, t0, failed).  Reading it
      synchronises; ``cov`` / ``depth_var`` are device tensors ordered on the current stream.

    t1 == t0: ``cov`` is empty and ``depth_var = Q_k``.  A failed factorisation (or an inverse that is not finite) sets bit
    0 of ``info`` as ``BA`` does and fills ``cov`` and the written ``depth_var`` entries with NaN.  ``M`` is accepted for
    symmetry with ``BA`` (one storage serves both of the reference's settings).  No autograd."""
    p = poses.data if hasattr(poses, "data") and not isinstance(poses, torch.Tensor) else poses
    cov, depth_var, raw = ops.ba_covariance(p, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, info, plan=plan)
    return cov, depth_var, ops.ba_covariance_stats(raw)


def map_covariance(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, M=0, info=None, plan=None, out=None):
    """The map with its uncertainty: ``(cov, depth_var, stats, point, point_cov, pose_depth_cov, n_obs)``.

    ``cov``, ``depth_var`` and ``stats`` are ``covariance``'s, the same bits.  For every patch k with a factor (the other
    entries keep their fill: NaN / 0, or what the caller's ``out`` tensors held):

    * ``point [n_patches, 3]``: the world point of the patch centre, ``projective_ops.point_cloud``'s (intrinsics row 0, as
      the system uses; the same bits where every row is equal).
    * ``point_cov [n_patches, 6]``: its 3 x 3 covariance as xx, xy, xz, yy, yz, zz, propagated from the joint inverse of the
      damped system: the source pose's block of ``cov``, ``depth_var[k]`` and the pose-depth cross term.  Left perturbation
      ``T <- Exp(xi) T`` of the world-to-camera pose (translation 3, rotation 3), ``d <- d + z``.
    * ``pose_depth_cov [n_patches, 6]``: ``cov(xi_i, z_k) = -Q_k (S^-1 e_k)`` restricted to the patch's source frame i; zeros
      where that frame is not a free pose -- ``point_cov`` is then the rank-one ``depth_var[k] J_d J_d'``.
    * ``n_obs [n_patches]`` int32: the patch's factors that pass the validity gate.

    A failed factorisation (``stats["failed"]``, bit 0 of ``info``) gives NaN ``point_cov`` / ``pose_depth_cov``; ``point``
    stays finite.  No autograd."""
    p = poses.data if hasattr(poses, "data") and not isinstance(poses, torch.Tensor) else poses
    cov, depth_var, raw, point, point_cov, pdc, n_obs = ops.ba_map_covariance(p, patches, intrinsics, target, weight, lmbda,
                                                                              ii, jj, kk, t0, t1, info, plan=plan, out=out)
    return cov, depth_var, ops.ba_covariance_stats(raw), point, point_cov, pdc, n_obs


def neighbors(ii, jj, ii_bound=0, jj_bound=0):
    """cuda_ba.neighbors(kk, jj) -> (ix, jx), computed on the device."""
    return ops.neighbors(ii, jj, ii_bound, jj_bound)


def reproject(poses, patches, intrinsics, ii, jj, kk):
    return ops.reproject(poses, patches, intrinsics, ii, jj, kk)
