"""The unseen-view reprojection loss: the inverse warp of a render into the reference camera, computed by the two-launch HIP kernel pair
``sn_reproject_loss`` (value AND the gradients w.r.t. the rendered depth and colour in one go; csrc/sn_reproject.hip).

Every pixel of the unseen-view render is lifted along its own ray by the depth the network rendered, projected into the reference camera,
and compared there with the bilinearly sampled reference image and depth:

* the photometric term: the Charbonnier distance of the rendered colour to the sampled one, over the pixels the reference camera sees
  (``|z - D| <= occ_tol D``) -- the view-synthesis loss of SfMLearner / MonoDepth2 with an occlusion test;
* the free-space term: ``max(0, (D - z) / D - occ_tol)`` -- a rendered surface in front of what the reference camera saw is a floater.

include/sinnerf_hip.h states the definitions.  The gradient goes to ``depth`` (through the sampling coordinates) and to ``rgb``; the rays,
the reference frame and the projection matrix are data.  The rays must be in WORLD space (not NDC).

No CPU fallback: CUDA (ROCm) tensors only.
"""
import torch

from . import _lib

__all__ = ["reprojection_loss"]

SHAPES = ("rays (N, 8), depth (N,), rgb (N, C) with 1 <= C <= 4, ref_image (H, W, C) channel-last over ref_depth (H, W) with H, W >= 2, "
          "ref_proj (4, 4) float64")
OUT_KEYS = ("photo", "free", "total", "n_vis", "n_geo", "n_front")


def _check(rays, depth, rgb, ref_image, ref_depth, ref_proj, opacity):
    named = (("rays", rays), ("depth", depth), ("rgb", rgb), ("ref_image", ref_image), ("ref_depth", ref_depth), ("ref_proj", ref_proj))
    if opacity is not None:
        named += (("opacity", opacity),)
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"sinnerf_amd.reprojection_loss: {name} must be a tensor; expected {SHAPES}")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"sinnerf_amd.reprojection_loss: {name} must be a CUDA/ROCm tensor (there is no CPU fallback); "
                               f"expected {SHAPES}")
    n = rays.shape[0] if rays.dim() == 2 else -1
    ok = (rays.dim() == 2 and rays.shape[1] == 8 and depth.numel() == n and depth.dim() <= 2 and rgb.dim() == 2 and rgb.shape[0] == n
          and 1 <= rgb.shape[1] <= 4 and (opacity is None or (opacity.numel() == n and opacity.dim() <= 2)))
    if not ok:
        raise RuntimeError(f"sinnerf_amd.reprojection_loss: expected {SHAPES}; got rays {tuple(rays.shape)}, depth {tuple(depth.shape)}, "
                           f"rgb {tuple(rgb.shape)}" + ("" if opacity is None else f", opacity {tuple(opacity.shape)}"))
    if (ref_depth.dim() != 2 or ref_image.dim() != 3 or tuple(ref_image.shape[:2]) != tuple(ref_depth.shape)
            or ref_image.shape[2] != rgb.shape[1] or min(ref_depth.shape) < 2):
        raise RuntimeError(f"sinnerf_amd.reprojection_loss: ref_image must be (H, W, C) channel-last over ref_depth's (H, W) frame with "
                           f"rgb's C and H, W >= 2; got ref_image {tuple(ref_image.shape)}, ref_depth {tuple(ref_depth.shape)}, "
                           f"rgb {tuple(rgb.shape)}")
    if tuple(ref_proj.shape) != (4, 4) or ref_proj.dtype != torch.float64:
        raise RuntimeError(f"sinnerf_amd.reprojection_loss: ref_proj must be a (4, 4) float64 tensor on the device "
                           f"(warp.projection_matrix); got {tuple(ref_proj.shape)} {ref_proj.dtype}")


class _ReprojectFn(torch.autograd.Function):
    """(depth, rgb | rays, opacity, ref_image, ref_depth, ref_proj) -> (total, out[6], per_pixel (N, 2), flags (N,) uint8); only
    ``total`` carries a gradient, and only to ``depth`` and ``rgb``"""

    @staticmethod
    def forward(ctx, depth, rgb, rays, opacity, ref_image, ref_depth, ref_proj, w_photo, w_free, occ_tol, charb_eps, z_min,
                opacity_threshold):
        ctx.set_materialize_grads(False)
        n, C = rgb.shape
        H, W = ref_depth.shape
        dev = rgb.device
        prep = lambda t: t.detach().to(torch.float32).contiguous()
        r, d, c = prep(rays), prep(depth).reshape(-1), prep(rgb)
        o = None if opacity is None else prep(opacity).reshape(-1)
        img, dep, P = prep(ref_image), prep(ref_depth), ref_proj.detach().contiguous()
        ctx.depth_shape = tuple(depth.shape)
        need_d, need_c = depth.requires_grad, rgb.requires_grad
        g_d = torch.empty_like(d) if need_d else None
        g_c = torch.empty_like(c) if need_c else None
        out = torch.empty(6, dtype=torch.float32, device=dev)
        per_pixel = torch.empty((n, 2), dtype=torch.float32, device=dev)
        flags = torch.empty((n,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            if n == 0:                              # empty batch: the entry's own answer for n <= 0, without its null pointers
                out.zero_()
            else:
                ws = _lib.workspace(_lib.lib.sn_reproject_loss_workspace_bytes(n), "sn_reproject_loss_workspace_bytes", dev)
                _lib.check(_lib.lib.sn_reproject_loss(_lib.ptr(r), _lib.ptr(d), _lib.ptr(c), _lib.ptr(o), n, C, _lib.ptr(img),
                                                      _lib.ptr(dep), H, W, _lib.ptr(P), float(occ_tol), float(charb_eps), float(z_min),
                                                      float(opacity_threshold), float(w_photo), float(w_free), _lib.ptr(g_d),
                                                      _lib.ptr(g_c), _lib.ptr(per_pixel), _lib.ptr(flags), _lib.ptr(ws), _lib.ptr(out),
                                                      _lib.stream_ptr()), "sn_reproject_loss")
        ctx.have = (need_d, need_c)
        ctx.save_for_backward(*[g for g in (g_d, g_c) if g is not None])
        ctx.mark_non_differentiable(out, per_pixel, flags)
        return out[2].clone(), out, per_pixel, flags

    @staticmethod
    def backward(ctx, g_total, _g_out, _g_per_pixel, _g_flags):
        none = (None,) * 13
        if g_total is None:
            return none
        saved = list(ctx.saved_tensors)
        g_d = saved.pop(0) if ctx.have[0] else None
        g_c = saved.pop(0) if ctx.have[1] else None
        return (None if g_d is None else (g_d * g_total).reshape(ctx.depth_shape), None if g_c is None else g_c * g_total) + none[2:]


def reprojection_loss(rays, depth, rgb, ref_image, ref_depth, ref_proj, *, opacity=None, w_photo=1.0, w_free=1.0, occ_tol=0.05,
                      charb_eps=1e-3, z_min=1e-6, opacity_threshold=0.5):
    """``w_photo * photo + w_free * free`` of the render ``(rays, depth, rgb)`` seen from the reference camera -> ``(total, stats)``.

    ``rays`` (N, 8) in WORLD space, ``depth`` (N,) the rendered depth along each ray (``depth_fine``), ``rgb`` (N, C) the rendered colour,
    ``ref_image`` (H, W, C) channel-last and ``ref_depth`` (H, W) the reference view, ``ref_proj`` (4, 4) float64 its
    ``warp.projection_matrix(K, extrinsics)``; ``opacity`` (N,): pixels at or below ``opacity_threshold`` take no part.

    ``stats``: ``photo``, ``free`` (the two means), ``total``, ``n_vis``, ``n_geo``, ``n_front`` (pixels the reference camera sees / that project
    onto its foreground / that lie in front of its surface) as 0-d device tensors, ``flags`` (N,) uint8 (bit 0 geometric validity, bit 1
    visible, bit 2 in front) and ``per_pixel`` (N, 2) = (photo_i, free_i), all detached.  ``total`` is differentiable in ``depth`` and
    ``rgb``; the rays, the reference and the pose are data."""
    _check(rays, depth, rgb, ref_image, ref_depth, ref_proj, opacity)
    total, out, per_pixel, flags = _ReprojectFn.apply(depth, rgb, rays, opacity, ref_image, ref_depth, ref_proj, w_photo, w_free, occ_tol,
                                                      charb_eps, z_min, opacity_threshold)
    stats = {k: out[i] for i, k in enumerate(OUT_KEYS)}
    stats.update(flags=flags, per_pixel=per_pixel)
    return total, stats
