"""Regularisers on the distribution of the compositing weights along a ray, computed by the two-launch HIP kernel pair
``sn_ray_regularizers`` (value AND the gradient w.r.t. the weights in one go; csrc/sn_ray_reg.hip):

* ``distortion_loss``   Mip-NeRF 360, eq. 15: pulls a ray's weight into one compact interval
* ``ray_entropy_loss``  InfoNeRF, eqs. 5-7: the entropy of the normalised weights, over the rays whose opacity exceeds a threshold
* ``ray_regularizers``  both at once, ``w_dist * mean(dist) + w_ent * mean(ent)``

All take ``(weights, z_vals, rays)``: the ``opacity_coarse`` / ``opacity_fine`` of ``render_rays``, the depths of that pass
(``render_rays(..., keep=d)`` hands them out as ``d['z_vals_coarse']`` / ``d['z_vals_fine']``) and the rays, whose columns 6, 7 give
near and far.  include/sinnerf_hip.h states the definitions.  The gradient goes to ``weights``; ``z_vals``, near and far are data.

No CPU fallback: CUDA (ROCm) tensors only.
"""
import torch

from . import _lib

__all__ = ["ray_regularizers", "distortion_loss", "ray_entropy_loss"]

SHAPES = "weights (N, S), z_vals (N, S), rays (N, 8) with 1 <= S <= 1024"


def _check(weights, z_vals, rays):
    named = (("weights", weights), ("z_vals", z_vals), ("rays", rays))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"sinnerf_amd.ray_regularizers: {name} must be a tensor; expected {SHAPES}")
    ok = (weights.dim() == 2 and z_vals.dim() == 2 and rays.dim() == 2 and tuple(z_vals.shape) == tuple(weights.shape)
          and tuple(rays.shape) == (weights.shape[0], 8) and 1 <= weights.shape[1] <= 1024)
    if not ok:
        raise RuntimeError(f"sinnerf_amd.ray_regularizers: expected {SHAPES}; got weights {tuple(weights.shape)}, "
                           f"z_vals {tuple(z_vals.shape)}, rays {tuple(rays.shape)}")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"sinnerf_amd.ray_regularizers: {name} must be a CUDA/ROCm tensor (there is no CPU fallback); "
                               f"expected {SHAPES}")


class _RayRegFn(torch.autograd.Function):
    """(weights, z_vals, rays) -> (total, out[4] = mean dist, mean ent, total, rays with the mask set, per_ray (N, 2)); only ``total``
    carries a gradient, and only to ``weights``"""

    @staticmethod
    def forward(ctx, weights, z_vals, rays, w_dist, w_ent, ent_threshold):
        ctx.set_materialize_grads(False)
        n, s = weights.shape
        dev = weights.device
        prep = lambda t: t.detach().to(torch.float32).contiguous()
        w, z, r = prep(weights), prep(z_vals), prep(rays)
        g_w = torch.empty_like(w) if weights.requires_grad else None
        out = torch.empty(4, dtype=torch.float32, device=dev)
        per_ray = torch.empty((n, 2), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if n == 0:                              # empty batch: the entry's own answer for n_rays <= 0, without its null pointers
                out.zero_()
            else:
                ws = _lib.workspace(_lib.lib.sn_ray_regularizers_workspace_bytes(n), "sn_ray_regularizers_workspace_bytes", dev)
                _lib.check(_lib.lib.sn_ray_regularizers(_lib.ptr(w), _lib.ptr(z), _lib.ptr(r), n, s, float(w_dist), float(w_ent),
                                                        float(ent_threshold), _lib.ptr(g_w), _lib.ptr(per_ray), _lib.ptr(ws),
                                                        _lib.ptr(out), _lib.stream_ptr()), "sn_ray_regularizers")
        ctx.save_for_backward(*([g_w] if g_w is not None else []))
        ctx.mark_non_differentiable(out, per_ray)
        return out[2].clone(), out, per_ray

    @staticmethod
    def backward(ctx, g_total, _g_out, _g_per_ray):
        saved = ctx.saved_tensors
        if g_total is None or not saved:
            return (None,) * 6
        return saved[0] * g_total, None, None, None, None, None


def ray_regularizers(weights, z_vals, rays, w_dist=1.0, w_ent=0.0, ent_threshold=0.1):
    """``w_dist * mean(dist) + w_ent * mean(ent)`` over all rays -> ``(total, stats)``.  ``stats``: ``distortion``, ``entropy`` (the two
    means), ``n_masked`` (rays with ``sum(w) > ent_threshold``) as 0-d device tensors and ``per_ray`` (N, 2) = (dist, ent) of each ray,
    all detached.  ``total`` is differentiable in ``weights``."""
    _check(weights, z_vals, rays)
    total, out, per_ray = _RayRegFn.apply(weights, z_vals, rays, w_dist, w_ent, ent_threshold)
    return total, {"distortion": out[0], "entropy": out[1], "n_masked": out[3], "per_ray": per_ray}


def distortion_loss(weights, z_vals, rays):
    """the mean distortion loss of the rays (Mip-NeRF 360, eq. 15)"""
    return ray_regularizers(weights, z_vals, rays, 1.0, 0.0)[0]


def ray_entropy_loss(weights, z_vals, rays, ent_threshold=0.1):
    """``mean(mask * H)`` over all rays (InfoNeRF, eqs. 5-7), mask = ``sum(w) > ent_threshold``"""
    return ray_regularizers(weights, z_vals, rays, 0.0, 1.0, ent_threshold)[0]
