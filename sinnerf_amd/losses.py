"""Losses on the rendered rays -- the step right after the hot path, same call surface as the
reference's loss objects, computed by the two-launch HIP kernel pair ``sn_render_loss`` (forward value AND the
gradients w.r.t. the rendered tensors in one go; csrc/sn_next.hip):

* ``MSELoss``        losses.py:12-22         ``forward(inputs, targets) -> {'tot', 'l2'}``
* ``SL1Loss``        models/sinnerf.py:32-42 ``forward(depth_pred, depth_gt, mask=None, useMask=True)``
* ``psnr``           metrics.py:14-15
* ``render_loss``    the fused form the system uses: MSE coarse+fine + w_depth * (SL1 coarse + SL1 fine) + PSNR stats

and the losses on the rendered PATCHES, by ``sn_patch_loss`` / ``sn_depth_smoothness`` (csrc/sn_patch_loss.hip):

* ``L2_SSIM_Loss``   losses.py:94-109        ``forward(inputs, targets) -> {'tot', 'l2', 'ssim'}``
* ``ssim_loss``      kornia 0.6.3 ``kornia.losses.ssim_loss(img1, img2, window_size)``, gradient to ``img1``
* ``inverse_depth_smoothness_loss``  kornia 0.6.3, gradients to ``idepth`` and ``image``
* ``loss_dict``      losses.py:152-153 without ``'l2_vgg'`` (pretrained VGG weights are not available offline)

The patch losses take NCHW tensors as kornia's do.  The kernels read channel-last memory: an NCHW view that is a permute of a
contiguous (B, H, W, C) buffer -- ``rearrange(rgb, '(b p q) c -> b c p q')`` of a render result -- is used in place, anything else is
copied once.

No CPU fallback: CUDA (ROCm) fp32 tensors only.
"""
import torch

from . import _lib

def _workspace(device):
    # ~10 KB of per-block partial sums, allocated per call from torch's caching allocator (stream-ordered: two streams
    # computing losses concurrently never share it)
    return _lib.workspace(_lib.lib.sn_render_loss_workspace_bytes(), "sn_render_loss_workspace_bytes", device)


def _prep(t, n, width, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError(f"{name}: CUDA tensor required (the HIP path has no CPU fallback)")
    t = t.detach().to(torch.float32).reshape(n, width) if width else t.detach().to(torch.float32).reshape(n)
    return t.contiguous()


class _RenderLossFn(torch.autograd.Function):
    """inputs in ABI order; returns (total, stats[8]); stats carries no gradient."""

    @staticmethod
    def forward(ctx, rgb_c, rgb_f, depth_c, depth_f, rgb_gt, depth_gt, mask, mask_mode, w_rgb, w_depth):
        ctx.set_materialize_grads(False)
        preds = (rgb_c, rgb_f, depth_c, depth_f)
        ref = next(t for t in preds if t is not None)
        n = ref.numel() // 3 if ref is rgb_c or ref is rgb_f else ref.numel()
        dev = ref.device
        p = [_prep(rgb_c, n, 3, "rgb_coarse"), _prep(rgb_f, n, 3, "rgb_fine"), _prep(depth_c, n, 0, "depth_coarse"),
             _prep(depth_f, n, 0, "depth_fine")]
        gt_rgb, gt_d = _prep(rgb_gt, n, 3, "rgb_gt"), _prep(depth_gt, n, 0, "depth_gt")
        m = None
        if mask_mode == 2:
            m = mask.detach().reshape(n).to(torch.uint8).contiguous()
        grads = [torch.empty_like(t) if (t is not None and orig.requires_grad) else None
                 for t, orig in zip(p, preds)]
        out = torch.empty(8, dtype=torch.float32, device=dev)
        if n == 0:                                  # empty batch: the reference's 'mean' reductions return NaN (0/0), no raise
            out.fill_(float("nan"))
            out[7] = 0.0
            ctx.shapes = [None if t is None else t.shape for t in preds]
            ctx.save_for_backward(*[g for g in grads if g is not None])
            ctx.have = [g is not None for g in grads]
            ctx.mark_non_differentiable(out)
            return out[4].clone(), out
        with torch.cuda.device(dev):
            ws = _workspace(dev)
            _lib.check(_lib.lib.sn_render_loss(_lib.ptr(p[0]), _lib.ptr(p[1]), _lib.ptr(p[2]), _lib.ptr(p[3]),
                                               _lib.ptr(gt_rgb),
                                               _lib.ptr(gt_d), _lib.ptr(m), int(mask_mode), n, float(w_rgb), float(w_depth),
                                               _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(grads[2]), _lib.ptr(grads[3]),
                                               _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr()), "sn_render_loss")
        ctx.shapes = [None if t is None else t.shape for t in preds]
        ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.have = [g is not None for g in grads]
        ctx.mark_non_differentiable(out)
        return out[4].clone(), out

    @staticmethod
    def backward(ctx, g_total, _g_stats):
        saved = list(ctx.saved_tensors)
        if g_total is None:
            return (None,) * 10
        scaled = list(torch._foreach_mul(saved, g_total)) if saved else []      # one launch for all four gradients
        res = []
        for have, shape in zip(ctx.have, ctx.shapes):
            res.append(scaled.pop(0).reshape(shape) if have else None)
        return (*res, None, None, None, None, None, None)


def render_loss(results, rgbs=None, depths=None, w_rgb=1.0, w_depth=1.0, mask=None, useMask=False):
    """MSE(rgb_coarse) + MSE(rgb_fine) (losses.py:12-22) + w_depth * (SL1(depth_coarse) + SL1(depth_fine))
    (models/sinnerf.py:310-319, which calls SL1Loss with useMask=False).  Missing keys / targets drop their terms.
    Returns (total, stats) with stats = dict(mse_coarse, mse_fine, sl1_coarse, sl1_fine, psnr_coarse, psnr_fine, n_depth)."""
    mode = 2 if mask is not None else (1 if useMask else 0)
    total, out = _RenderLossFn.apply(results.get("rgb_coarse") if rgbs is not None else None,
                                     results.get("rgb_fine") if rgbs is not None else None,
                                     results.get("depth_coarse") if depths is not None else None,
                                     results.get("depth_fine") if depths is not None else None,
                                     rgbs, depths, mask, mode, w_rgb, w_depth)
    names = ("mse_coarse", "mse_fine", "sl1_coarse", "sl1_fine", "total", "psnr_coarse", "psnr_fine", "n_depth")
    return total, {k: out[i] for i, k in enumerate(names)}


class MSELoss(torch.nn.Module):
    """losses.py:12-22; (B, C, H, W) patches too, as the reference's ``patch_loss`` feeds them (models/sinnerf.py:348, 367-368)."""

    def forward(self, inputs, targets):
        if targets.dim() == 4:
            loss, _ = _PatchLossFn.apply(inputs.get("rgb_coarse"), inputs.get("rgb_fine"), targets, 0, 0, 1.0, 0.0)
            return {"tot": loss, "l2": loss}
        loss, _ = render_loss(inputs, rgbs=targets)
        return {"tot": loss, "l2": loss}


class SL1Loss(torch.nn.Module):
    """models/sinnerf.py:32-42 (``levels`` is accepted and unused, as there)."""

    def __init__(self, levels=3):
        super().__init__()
        self.levels = levels

    def forward(self, depth_pred, depth_gt, mask=None, useMask=True):
        loss, _ = render_loss({"depth_fine": depth_pred}, depths=depth_gt, mask=mask, useMask=useMask)
        return loss


def psnr(image_pred, image_gt):
    """metrics.py:14-15 (no valid_mask, reduction='mean')."""
    with torch.no_grad():
        _, stats = render_loss({"rgb_fine": image_pred}, rgbs=image_gt)
    return stats["psnr_fine"]


# ---- losses on the rendered patches (csrc/sn_patch_loss.hip) ------------------------------------------------------------------------
SSIM_WEIGHT = 2.8333                                # losses.py:109 "ratio from MonoDepth"


def _channel_last(t, name):
    """(B, C, H, W) -> ((B, H, W, C) contiguous fp32 tensor, in_place): the memory under a permuted channel-last buffer as it is, one
    copy of anything else"""
    if t is None:
        return None, True
    if not t.is_cuda:
        raise ValueError(f"{name}: CUDA tensor required (the HIP path has no CPU fallback)")
    if t.dim() != 4:
        raise ValueError(f"{name}: (B, C, H, W) expected, got {tuple(t.shape)}")
    v = t.detach().permute(0, 2, 3, 1)
    in_place = v.is_contiguous() and v.dtype == torch.float32
    return (v if in_place else v.to(torch.float32).contiguous()), in_place


def _nchw_grad(g, in_place):
    """a channel-last gradient buffer in the caller's layout"""
    g = g.permute(0, 3, 1, 2)
    return g if in_place else g.contiguous()


class _PatchLossFn(torch.autograd.Function):
    """(coarse, fine, target) NCHW -> (total, out[4] = mse_coarse, mse_fine, ssim_loss, total); out carries no gradient"""

    @staticmethod
    def forward(ctx, coarse, fine, target, use_ssim, window, w_mse, w_ssim):
        ctx.set_materialize_grads(False)
        ref = fine if fine is not None else coarse
        if ref is None:
            raise ValueError("patch loss: neither 'rgb_coarse' nor 'rgb_fine'")
        (c, c_in), (f, f_in), (t, _) = _channel_last(coarse, "coarse"), _channel_last(fine, "fine"), _channel_last(target, "target")
        B, H, W, C = (f if f is not None else c).shape
        for name, x in (("coarse", c), ("target", t)):
            if x is not None and tuple(x.shape) != (B, H, W, C):
                raise ValueError(f"patch loss: {name} {tuple(x.permute(0, 3, 1, 2).shape)} != {(B, C, H, W)}")
        dev = ref.device
        g_c = torch.empty_like(c) if (c is not None and coarse.requires_grad) else None
        g_f = torch.empty_like(f) if (f is not None and fine.requires_grad) else None
        out = torch.empty(4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = _lib.workspace(_lib.lib.sn_patch_loss_workspace_bytes(B, H, W, C, int(use_ssim)), "sn_patch_loss_workspace_bytes", dev)
            _lib.check(_lib.lib.sn_patch_loss(_lib.ptr(c), _lib.ptr(f), _lib.ptr(t), B, H, W, C, int(use_ssim), int(window),
                                              float(w_mse), float(w_ssim), _lib.ptr(g_c), _lib.ptr(g_f), _lib.ptr(ws), _lib.ptr(out),
                                              _lib.stream_ptr()), "sn_patch_loss")
        ctx.save_for_backward(*[g for g in (g_c, g_f) if g is not None])
        ctx.have, ctx.in_place = (g_c is not None, g_f is not None), (c_in, f_in)
        ctx.mark_non_differentiable(out)
        return out[3].clone(), out

    @staticmethod
    def backward(ctx, g_total, _g_out):
        if g_total is None:
            return (None,) * 7
        saved = list(ctx.saved_tensors)
        scaled = list(torch._foreach_mul(saved, g_total)) if saved else []
        res = [_nchw_grad(scaled.pop(0), in_place) if have else None for have, in_place in zip(ctx.have, ctx.in_place)]
        return (*res, None, None, None, None, None)


class _DepthSmoothnessFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idepth, image):
        ctx.set_materialize_grads(False)
        (d, d_in), (im, im_in) = _channel_last(idepth, "idepth"), _channel_last(image, "image")
        B, H, W, C = im.shape
        if tuple(d.shape) != (B, H, W, 1):
            raise ValueError(f"inverse_depth_smoothness_loss: idepth {tuple(idepth.shape)} and image {tuple(image.shape)} must be "
                             "(B, 1, H, W) and (B, C, H, W)")
        dev = idepth.device
        g_d = torch.empty_like(d) if idepth.requires_grad else None
        g_i = torch.empty_like(im) if image.requires_grad else None
        out = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = _lib.workspace(_lib.lib.sn_depth_smoothness_workspace_bytes(), "sn_depth_smoothness_workspace_bytes", dev)
            _lib.check(_lib.lib.sn_depth_smoothness(_lib.ptr(d), _lib.ptr(im), B, H, W, C, _lib.ptr(g_d), _lib.ptr(g_i), _lib.ptr(ws),
                                                    _lib.ptr(out), _lib.stream_ptr()), "sn_depth_smoothness")
        ctx.save_for_backward(*[g for g in (g_d, g_i) if g is not None])
        ctx.have, ctx.in_place = (g_d is not None, g_i is not None), (d_in, im_in)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g_total):
        if g_total is None:
            return None, None
        saved = list(ctx.saved_tensors)
        scaled = list(torch._foreach_mul(saved, g_total)) if saved else []
        return tuple(_nchw_grad(scaled.pop(0), in_place) if have else None for have, in_place in zip(ctx.have, ctx.in_place))


def ssim_loss(img1, img2, window_size):
    """kornia 0.6.3 ``ssim_loss`` (``max_val`` 1, ``eps`` 1e-12, reduction 'mean'): (B, C, H, W) with C in {1, 3}; the gradient goes to
    ``img1``"""
    total, _ = _PatchLossFn.apply(None, img1, img2, 1, window_size, 0.0, 1.0)
    return total


def inverse_depth_smoothness_loss(idepth, image):
    """kornia 0.6.3: ``idepth`` (B, 1, H, W), ``image`` (B, C, H, W); gradients go to both"""
    return _DepthSmoothnessFn.apply(idepth, image)


class L2_SSIM_Loss(torch.nn.Module):
    """losses.py:94-109 on (B, C, H, W) patches, C in {1, 3}.  'tot' carries the gradient; 'l2' and 'ssim' are its two parts as values."""

    def forward(self, inputs, targets):
        if "rgb_fine" not in inputs:        # the reference fails here with an unbound local `ssim`
            raise KeyError("L2_SSIM_Loss needs inputs['rgb_fine']: the SSIM term is taken on the fine render (losses.py:103-105)")
        total, out = _PatchLossFn.apply(inputs.get("rgb_coarse"), inputs["rgb_fine"], targets, 1, 11, 1.0, SSIM_WEIGHT)
        return {"tot": total, "l2": out[0] + out[1], "ssim": out[2]}


class _LossDict(dict):
    def __getitem__(self, key):
        if key == "l2_vgg":
            raise NotImplementedError("patch_loss 'l2_vgg' (losses.py:135-149) needs torchvision's pretrained VGG16 weights, which "
                                      "cannot be downloaded here; use 'mse' or 'l2_ssim'")
        return super().__getitem__(key)


loss_dict = _LossDict({"mse": MSELoss, "l2_ssim": L2_SSIM_Loss})                     # losses.py:152-153
