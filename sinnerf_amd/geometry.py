"""Density gradients and normal maps: the derivative of the raw sigma with respect to a POSITION.

The reference has no such function; autograd through ``Embedding`` + ``NeRF.forward`` (``models/nerf.py:36-41, 122-148``) would give
it.  Here it is the stored-state path of training, run for one fixed upstream gradient:

    sn_mlp_forward_train  ->  sn_mlp_backward_chain with g_raw = (0, 0, 0, 1) per point  ->  sn_point_grads  [->  sn_point_grads_wsum]

sigma always means the RAW sigma column of the network output (``nerf.py:136``: before the compositor's ReLU, without noise) -- the
quantity ``eval_points`` returns.  Every output is a label: it carries no gradient, no weight-gradient kernel runs and no ``.grad``
is touched.  ``NeRF.forward`` itself still refuses ``x.requires_grad``.  ``compute_dtype`` 'fp32', 'bf16' (bf16 state) and 'bf16x3'
are supported; 'fp16' is an inference arithmetic and raises.  There is no CPU fallback: CPU tensors raise.
"""
import torch

from . import _lib
from .nerf import NeRF, dtype_code

__all__ = ["density_gradients", "ray_density_gradients", "render_normals"]


def _check_model(model, what):
    if not isinstance(model, NeRF):
        raise TypeError(f"sinnerf_amd.{what} needs a sinnerf_amd.NeRF model")
    if dtype_code(model.compute_dtype) == _lib.SN_DTYPE_F16:
        raise NotImplementedError("sinnerf_amd: compute_dtype='fp16' is an INFERENCE arithmetic (sn_mlp_forward only); density gradients "
                                  "need the training state of 'fp32', 'bf16' or 'bf16x3'")


def _check_cuda(t, what, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"sinnerf_amd.{what}: {name} must be a CUDA/ROCm tensor (there is no CPU fallback)")


def _sigma_grads(model, rays, z_vals, weights):
    """(raw (N, S, 4), g_xyz (N S, 4), g_sum (N, 4) or None) of one pass; rays (N, 8), z_vals / weights (N, S): contiguous fp32 on one
    device, N >= 1.  The caller holds ``torch.no_grad()`` and the device."""
    from .autograd import _chain_state
    n, s = z_vals.shape
    dev = rays.device
    g_raw = torch.zeros((n * s, 4), dtype=torch.float32, device=dev)
    g_raw[:, 3] = 1.0                                                    # d(raw sigma): the rgb columns get no gradient
    raw, G, rows, code = _chain_state(model, rays, z_vals, g_raw)
    raws = model.raw_tensors()
    w1, w5 = (raws[i].detach().contiguous().float() for i in (0, 8))     # xyz_encoding_1 / _5 weights
    g_xyz = torch.empty((n * s, 4), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib.sn_point_grads(_lib.ptr(w1), _lib.ptr(w5), code, _lib.ptr(G), rows, _lib.ptr(rays), _lib.ptr(z_vals), n, s,
                                       _lib.ptr(g_xyz), _lib.stream_ptr()), "sn_point_grads")
    g_sum = None
    if weights is not None:
        g_sum = torch.empty((n, 4), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib.sn_point_grads_wsum(_lib.ptr(g_xyz), _lib.ptr(weights), n, s, _lib.ptr(g_sum), _lib.stream_ptr()),
                   "sn_point_grads_wsum")
    return raw, g_xyz, g_sum


def ray_density_gradients(model, rays, z_vals, weights=None):
    """d(raw sigma)/d(xyz) at the sample points ``xyz = o + d z`` of ``rays`` (N, 8) = [o, d, near, far] and ``z_vals`` (N, S), S <= 1024.

    Returns ``grad`` (N, S, 3); with ``weights`` (N, S) -- e.g. a pass's ``opacity_*`` -- also ``grad_sum`` (N, 3) =
    ``sum_s weights[:, s] grad[:, s]`` (fp64 sums in a fixed order, rounded once).  The position is the fp32 value the network
    embeds, ``fl(o + fl(d z))``.  Labels: no output requires grad, no parameter ``.grad`` is written."""
    what = "ray_density_gradients"
    _check_model(model, what)
    _check_cuda(rays, what, "rays")
    _check_cuda(z_vals, what, "z_vals")
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise RuntimeError(f"rays must have shape (N_rays, 8), got {tuple(rays.shape)}")
    if z_vals.dim() != 2 or z_vals.shape[0] != rays.shape[0] or z_vals.shape[1] < 1:
        raise RuntimeError(f"z_vals must have shape (N_rays, S >= 1), got {tuple(z_vals.shape)}")
    if weights is not None:
        _check_cuda(weights, what, "weights")
        if tuple(weights.shape) != tuple(z_vals.shape):
            raise RuntimeError(f"weights must have the shape of z_vals {tuple(z_vals.shape)}, got {tuple(weights.shape)}")
    n, s = z_vals.shape
    with torch.no_grad(), torch.cuda.device(rays.device):
        if n == 0:
            e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=rays.device)
            return e(0, s, 3) if weights is None else (e(0, s, 3), e(0, 3))
        rays, z_vals = rays.detach().contiguous().float(), z_vals.detach().contiguous().float()
        if weights is not None:
            weights = weights.detach().contiguous().float()
        _, g_xyz, g_sum = _sigma_grads(model, rays, z_vals, weights)
    grad = g_xyz.view(n, s, 4)[..., :3]
    return grad if weights is None else (grad, g_sum[:, :3])


def density_gradients(points, model):
    """Raw sigma and its gradient at free points: points (B, 3) -> ``(sigma (B, 1), grad (B, 3))``.

    The same path with one ray ``[p, 0, 0, 0, 0, 0]`` and one sample ``z = 0`` per point: the embedded position is ``p`` exactly and a
    zero direction cannot reach sigma (``nerf.py:136``).  ``sigma`` is the value ``eval_points`` evaluates, from the training forward."""
    what = "density_gradients"
    _check_model(model, what)
    _check_cuda(points, what, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"density_gradients: points must be (B, 3), got {tuple(points.shape)}")
    b = points.shape[0]
    dev = points.device
    with torch.no_grad(), torch.cuda.device(dev):
        if b == 0:
            return torch.empty((0, 1), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev)
        rays = torch.zeros((b, 8), dtype=torch.float32, device=dev)
        rays[:, :3] = points.detach().float()
        z = torch.zeros((b, 1), dtype=torch.float32, device=dev)
        raw, g_xyz, _ = _sigma_grads(model, rays, z, None)
    return raw[:, 0, 3:4], g_xyz[:, :3]


def render_normals(models, embeddings, rays, N_samples=64, use_disp=False, N_importance=0, white_back=False, max_points=1 << 18,
                   keep=None):
    """``render_rays(models, embeddings, rays, N_samples, use_disp, perturb=0, noise_std=0, N_importance, white_back=white_back)`` under
    ``torch.no_grad()`` -- the same dict, bit for bit -- plus a normal map of the last pass:

        grad_fine    (N, 3)   sum_i w_i grad sigma_i over the samples of the pass that produced ``opacity_fine`` (the fine pass and
                              ``models[1]``; with ``N_importance == 0`` the coarse pass and ``models[0]``), w = ``opacity_fine``
        normal_fine  (N, 3)   -grad_fine / max(||grad_fine||, 1e-12): density grows into the surface, the normal points out of it

    The training state behind the gradient costs about 20 KB per point in fp32 (activations plus their gradients), so that part runs
    in chunks of whole rays holding at most ``max_points`` points (at least one ray); rays are independent, the result does not
    depend on the chunk size.  ``keep`` (a dict) receives ``z_vals`` (N, S) and ``grad_samples`` (N, S, 3), the per-sample depths and
    gradients of that pass.  Labels: nothing here requires grad or writes a ``.grad``."""
    from . import rendering as R
    what = "render_normals"
    _check_cuda(rays, what, "rays")
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise RuntimeError(f"rays must have shape (N_rays, 8), got {tuple(rays.shape)}")
    if N_importance > 0 and len(models) < 2:
        raise IndexError("list index out of range")
    model = models[1] if N_importance > 0 else models[0]
    for m in models:
        _check_model(m, what)
    if int(max_points) < 1:
        raise ValueError("render_normals: max_points must be positive")
    n = rays.shape[0]
    s = N_samples + N_importance
    dev = rays.device
    R._check_embeddings(embeddings)
    if s > R.MAX_FUSED_SAMPLES:
        raise NotImplementedError("sinnerf_amd.render_normals: %d + %d samples per ray; the per-ray kernels hold at most %d in one wave.  "
                                  "Supported: %s" % (N_samples, N_importance, R.MAX_FUSED_SAMPLES, R.SUPPORTED))
    rays = rays.detach().contiguous().float()
    with torch.no_grad(), torch.cuda.device(dev):
        # the no-grad path of render_rays itself (perturb = 0, noise_std = 0), which also hands out the depths of each pass
        passes = {}
        res = R._forward_core(models, rays, N_samples, use_disp, 0, 0, N_importance, white_back, False, keep=passes)
        if n == 0:
            res.update(grad_fine=torch.empty((0, 3), dtype=torch.float32, device=dev),
                       normal_fine=torch.empty((0, 3), dtype=torch.float32, device=dev))
            if keep is not None:
                keep.update(z_vals=torch.empty((0, s), dtype=torch.float32, device=dev),
                            grad_samples=torch.empty((0, s, 3), dtype=torch.float32, device=dev))
            return res
        z = passes["z_fine"] if N_importance > 0 else passes["z_coarse"]
        weights = res["opacity_fine"]
        per = max(1, int(max_points) // s)
        g_sum = torch.empty((n, 4), dtype=torch.float32, device=dev)
        g_all = torch.empty((n, s, 4), dtype=torch.float32, device=dev) if keep is not None else None
        for r0 in range(0, n, per):
            r1 = min(n, r0 + per)
            _, g_xyz, gs = _sigma_grads(model, rays[r0:r1], z[r0:r1], weights[r0:r1])
            g_sum[r0:r1] = gs
            if g_all is not None:
                g_all[r0:r1] = g_xyz.view(r1 - r0, s, 4)
        grad = g_sum[:, :3]
        g64 = grad.double()
        normal = (-g64 / g64.norm(dim=1, keepdim=True).clamp_min(1e-12)).float()
        res.update(grad_fine=grad, normal_fine=normal)
        if keep is not None:
            keep.update(z_vals=z, grad_samples=g_all[..., :3])
    return res
