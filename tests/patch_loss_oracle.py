"""The yardstick of the patch-loss tests: kornia 0.6.3's ``ssim_loss`` and ``inverse_depth_smoothness_loss`` (the version the reference's
requirements.txt pins; kornia itself is not installed) and the reference's ``L2_SSIM_Loss`` (losses.py:94-109), restated in plain torch
ops on NCHW tensors.  Evaluated in fp64 it is the reference value; evaluated in fp32 on the same inputs it gives ``e32``, the error a
correct fp32 implementation has, from which the tests' bars are formed (``bar``)."""
import torch
import torch.nn.functional as F

SSIM_WEIGHT = 2.8333


def gaussian(window_size, dtype, device):
    k = torch.arange(window_size, dtype=dtype, device=device) - window_size // 2
    g = torch.exp(-k ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def filter2d(x, window_size):
    """per-channel correlation with g (x) g after reflect padding by window_size // 2"""
    C = x.shape[1]
    g = gaussian(window_size, x.dtype, x.device)
    w = (g[:, None] * g[None, :]).expand(C, 1, window_size, window_size).contiguous()
    p = window_size // 2
    return F.conv2d(F.pad(x, (p, p, p, p), mode="reflect"), w, groups=C)


def ssim_loss(a, b, window_size):
    C1, C2, eps = 0.01 ** 2, 0.03 ** 2, 1e-12
    mu1, mu2 = filter2d(a, window_size), filter2d(b, window_size)
    s11 = filter2d(a * a, window_size) - mu1 * mu1
    s22 = filter2d(b * b, window_size) - mu2 * mu2
    s12 = filter2d(a * b, window_size) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2) + eps)
    return torch.clamp((1 - ssim) / 2, 0, 1).mean()


def inverse_depth_smoothness_loss(idepth, image):
    dx = lambda t: t[:, :, :, :-1] - t[:, :, :, 1:]
    dy = lambda t: t[:, :, :-1, :] - t[:, :, 1:, :]
    wx = torch.exp(-dx(image).abs().mean(1, keepdim=True))
    wy = torch.exp(-dy(image).abs().mean(1, keepdim=True))
    return (dx(idepth) * wx).abs().mean() + (dy(idepth) * wy).abs().mean()


def mse(a, b):
    return ((a - b) ** 2).mean()


def sl1(pred, gt, mask=None):
    """models/sinnerf.py:32-42 with a boolean mask (None: every element)"""
    d = (pred - gt).abs()
    l = torch.where(d < 1, 0.5 * d * d, d - 0.5)
    return l.mean() if mask is None else l[mask].mean()


def l2_ssim(coarse, fine, target, window_size=11):
    """losses.py:94-109 -> (tot, l2, ssim)"""
    l2 = mse(coarse, target) + mse(fine, target)
    s = ssim_loss(fine, target, window_size)
    return l2 + s * SSIM_WEIGHT, l2, s


def evaluate(fn, inputs, wrt, dtype):
    """value and gradients of fn(*inputs) w.r.t. the inputs listed in `wrt` (indices), computed in `dtype` on the CPU; all as fp64"""
    xs = [x.detach().cpu().to(dtype).requires_grad_(i in wrt) for i, x in enumerate(inputs)]
    val = fn(*xs)
    if not wrt:
        return val.detach().double(), []
    grads = torch.autograd.grad(val, [xs[i] for i in wrt], allow_unused=True)
    return val.detach().double(), [torch.zeros_like(xs[i]).double() if g is None else g.double() for i, g in zip(wrt, grads)]


def rel(got, want):
    """relative L2 distance (a scalar: relative error); 0 when both are exactly zero"""
    got, want = got.detach().double().cpu(), want.double()
    n = want.norm().item()
    d = (got - want).norm().item()
    return d / n if n > 0 else d


def bar(e32):
    """the kernel must be within max(4 e32, 1e-6) of fp64: 4 for a different summation order, the floor for quantities whose e32 is at
    rounding level"""
    return max(4.0 * e32, 1e-6)


def reference(fn, inputs, wrt):
    """-> (value64, grads64, e32 of the value, [e32 of each gradient])"""
    v64, g64 = evaluate(fn, inputs, wrt, torch.float64)
    v32, g32 = evaluate(fn, inputs, wrt, torch.float32)
    return v64, g64, rel(v32, v64), [rel(a, b) for a, b in zip(g32, g64)]
