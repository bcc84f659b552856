"""On-GPU ray generation -- SURVEY.md §8f rank 1, the step immediately before the hot path.

Reference: ``datasets/ray_utils.py:86-133`` (``get_ray_directions`` + ``get_rays``; directions are NOT normalised,
``:110`` is commented out) and the ``[rays_o, rays_d, near, far]`` packing the datasets do (blender:
``blender_ray_patch_1image_rot3d.py:201-211``; strided patches ``:487-498``).  The reference builds the (H*W, 8) array on
the CPU in the DataLoader and copies it to the device (``eval.py:155``); here ``sn_generate_rays`` writes it directly in
HBM from the 12 floats of ``c2w``.

The reference's other two cameras go through ``sn_generate_rays_cam``: llff, whose rays pass ``get_ndc_rays``
(``datasets/ray_utils.py:123-164``; ``llff_ray_patch_1image_proj.py:473-483, :541-545, :676-682``), and dtu, with two focal
lengths, a principal point and the OpenCV signs (``get_ray_directions_dtu``, ``datasets/dtu_proj.py:17-35``).  ``get_ndc_rays``
is the reference's function of that name over rays that exist already (``sn_ndc_rays``).

The intrinsics may be device tensors (a focal length that is being learnt): ``sn_generate_rays_cam_dev`` / ``sn_ndc_rays_dev`` read them
on the device -- nothing is pulled to the host, so the call neither synchronises nor breaks a stream capture -- and their backwards
form ``dL/d(fx, fy, cx, cy)`` next to the pose gradient (the reference's functions are torch ops and differentiate through them).
"""
import torch

from . import _lib


def _generate(c2w, H, W, focal, near, far, win):
    x0, y0, sx, sy, pw, ph = win
    rays = torch.empty((pw * ph, 8), dtype=torch.float32, device=c2w.device)
    with torch.cuda.device(c2w.device):
        _lib.check(_lib.lib.sn_generate_rays(_lib.ptr(c2w), H, W, float(focal), float(near), float(far), x0, y0, sx, sy, pw,
                                             ph, _lib.ptr(rays), _lib.stream_ptr()), "sn_generate_rays")
    return rays


class _GetRaysFn(torch.autograd.Function):
    """``get_rays`` under autograd (ray_utils.py:109, :112 are ordinary differentiable torch ops in the reference):
    rays_d = directions @ c2w[:, :3].T, rays_o = c2w[:, 3]  ->  g_c2w[:, :3] = g_d^T directions, g_c2w[:, 3] = sum g_o."""

    @staticmethod
    def forward(ctx, c2w, H, W, focal, near, far, win):
        ctx.args = (H, W, float(focal), win)
        return _generate(c2w, H, W, focal, near, far, win)

    @staticmethod
    def backward(ctx, g_rays):
        H, W, focal, (x0, y0, sx, sy, pw, ph) = ctx.args
        g_rays = g_rays.contiguous().float()
        dev = g_rays.device
        ws = _lib.workspace(_lib.lib.sn_generate_rays_backward_workspace_bytes(), "sn_generate_rays_backward_workspace_bytes", dev)
        g_c2w = torch.empty((3, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.sn_generate_rays_backward(_lib.ptr(g_rays), H, W, focal, x0, y0, sx, sy, pw, ph, _lib.ptr(ws),
                                                          _lib.ptr(g_c2w), _lib.stream_ptr()), "sn_generate_rays_backward")
        return g_c2w, None, None, None, None, None, None


CONVENTIONS = {"opengl": 0, "opencv": 1}


def _camera_args(H, W, cam):
    """the arguments sn_generate_rays_cam and its backward share, between c2w and the window"""
    fx, fy, cx, cy, convention, ndc_near = cam
    ndc = ndc_near is not None
    return (H, W, fx, fy, cx, cy, convention, int(ndc), fx, float(ndc_near) if ndc else 0.0)      # ndc_focal = fx (= fy with NDC)


def _generate_cam(c2w, H, W, cam, near, far, win):
    rays = torch.empty((win[4] * win[5], 8), dtype=torch.float32, device=c2w.device)
    with torch.cuda.device(c2w.device):
        _lib.check(_lib.lib.sn_generate_rays_cam(_lib.ptr(c2w), *_camera_args(H, W, cam), float(near), float(far), *win,
                                                 _lib.ptr(rays), _lib.stream_ptr()), "sn_generate_rays_cam")
    return rays


class _GetRaysCamFn(torch.autograd.Function):
    """``get_rays`` for the llff / dtu cameras under autograd: the direction stack (ray_utils.py:89-91 or dtu_proj.py:31-33),
    ray_utils.py:109-114 and, with NDC, get_ndc_rays (:144-162) are ordinary differentiable torch ops in the reference."""

    @staticmethod
    def forward(ctx, c2w, H, W, cam, near, far, win):
        ctx.args = (H, W, cam, win)
        ctx.save_for_backward(c2w)
        return _generate_cam(c2w, H, W, cam, near, far, win)

    @staticmethod
    def backward(ctx, g_rays):
        H, W, cam, win = ctx.args
        c2w, = ctx.saved_tensors
        g_rays = g_rays.contiguous().float()
        dev = g_rays.device
        ws = _lib.workspace(_lib.lib.sn_generate_rays_backward_workspace_bytes(), "sn_generate_rays_backward_workspace_bytes", dev)
        g_c2w = torch.empty((3, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.sn_generate_rays_cam_backward(_lib.ptr(g_rays), _lib.ptr(c2w), *_camera_args(H, W, cam), *win,
                                                              _lib.ptr(ws), _lib.ptr(g_c2w), _lib.stream_ptr()),
                       "sn_generate_rays_cam_backward")
        return g_c2w, None, None, None, None, None, None


def _generate_cam_dev(c2w, intr, H, W, convention, ndc_near, near, far, win):
    ndc = ndc_near is not None
    rays = torch.empty((win[4] * win[5], 8), dtype=torch.float32, device=c2w.device)
    with torch.cuda.device(c2w.device):
        _lib.check(_lib.lib.sn_generate_rays_cam_dev(_lib.ptr(c2w), _lib.ptr(intr), H, W, convention, int(ndc),
                                                     float(ndc_near) if ndc else 0.0, float(near), float(far), *win, _lib.ptr(rays),
                                                     _lib.stream_ptr()), "sn_generate_rays_cam_dev")
    return rays


class _GetRaysDevFn(torch.autograd.Function):
    """``get_rays`` with the intrinsics ``intr = (fx, fy, cx, cy)`` in a device tensor, under autograd in ``c2w`` and ``intr``:
    ``sn_generate_rays_cam_dev_backward`` forms what ``needs_input_grad`` asks for in one pass over the rays."""

    @staticmethod
    def forward(ctx, c2w, intr, H, W, convention, ndc_near, near, far, win):
        ctx.args = (H, W, convention, ndc_near, win)
        ctx.save_for_backward(c2w, intr)
        return _generate_cam_dev(c2w, intr, H, W, convention, ndc_near, near, far, win)

    @staticmethod
    def backward(ctx, g_rays):
        H, W, convention, ndc_near, win = ctx.args
        c2w, intr = ctx.saved_tensors
        ndc = ndc_near is not None
        g_rays = g_rays.contiguous().float()
        dev = g_rays.device
        ws = _lib.workspace(_lib.lib.sn_camera_backward_workspace_bytes(), "sn_camera_backward_workspace_bytes", dev)
        g_c2w = torch.empty((3, 4), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        g_intr = torch.empty((4,), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.sn_generate_rays_cam_dev_backward(_lib.ptr(g_rays), _lib.ptr(c2w), _lib.ptr(intr), H, W, convention, int(ndc),
                                                                  float(ndc_near) if ndc else 0.0, *win, _lib.ptr(ws), _lib.ptr(g_c2w),
                                                                  _lib.ptr(g_intr), _lib.stream_ptr()),
                       "sn_generate_rays_cam_dev_backward")
        return g_c2w, g_intr, None, None, None, None, None, None, None


def _on_device(name, v):
    """True: ``v`` is a device tensor (the device path); False: a number, a pair or a CPU tensor without grad (the host path)"""
    if not torch.is_tensor(v):
        return False
    if not v.is_cuda and v.requires_grad:
        raise RuntimeError(f"sinnerf_amd.ray_utils: {name} requires grad but is a CPU tensor: keep it on the ROCm device (its gradient "
                           "is formed there; no CPU fallback)")
    return v.is_cuda


def _intrinsics(H, W, focal, center, ndc, dev):
    """(4,) fp32 (fx, fy, cx, cy) on ``dev`` by torch ops only: autograd routes its gradient back to ``focal`` / ``center``; numbers are
    placed by fill kernels (no host-to-device copy), nothing is read back"""
    fill = lambda v: torch.full((1,), float(v), dtype=torch.float32, device=dev)
    if torch.is_tensor(focal) and focal.is_cuda:
        if focal.numel() == 1:
            fx = fy = focal.reshape(1)
        elif tuple(focal.shape) == (2,):
            if ndc:
                raise ValueError("the NDC map has one focal length (get_ndc_rays(H, W, focal, ...)): pass a one-element focal tensor")
            fx, fy = focal[0:1], focal[1:2]
        else:
            raise RuntimeError(f"a focal tensor must have one element or be (2,), got {tuple(focal.shape)}")
    else:
        pair = isinstance(focal, (tuple, list)) or getattr(focal, "ndim", 0) > 0
        fx, fy = (float(focal[0]), float(focal[1])) if pair else (float(focal), float(focal))
        if ndc and fx != fy:
            raise ValueError("the NDC map has one focal length (get_ndc_rays(H, W, focal, ...)): fx must equal fy")
        fx, fy = fill(fx), fill(fy)
    if torch.is_tensor(center) and center.is_cuda:
        if tuple(center.shape) != (2,):
            raise RuntimeError(f"a center tensor must be (2,), got {tuple(center.shape)}")
        cxy = [center]
    else:
        cxy = [fill(W / 2), fill(H / 2)] if center is None else [fill(center[0]), fill(center[1])]
    return torch.cat([v.to(device=dev, dtype=torch.float32) for v in (fx, fy, *cxy)])


def get_rays(H, W, focal, c2w, near, far, window=None, *, center=None, convention="opengl", ndc_near=None):
    """(n, 8) fp32 rays ``[o(3), d(3), near, far]`` on ``c2w``'s device, row-major over pixels.

    ``c2w``: (3,4) camera-to-world tensor on the ROCm device.  ``window = (x0, y0, stride_x, stride_y, patch_w, patch_h)``
    selects a strided patch; default = the full frame.  When ``c2w.requires_grad`` (under grad mode) the result carries the
    pose gradient (``sn_generate_rays_backward`` / ``sn_generate_rays_cam_backward``): optimise ``c2w`` through ``render_rays``.

    The camera: ``focal`` is one focal length or an ``(fx, fy)`` pair, ``center = (cx, cy)`` the principal point (default
    ``(W/2, H/2)``), ``convention`` ``"opengl"`` (``((i-cx)/fx, -(j-cy)/fy, -1)``: blender, llff) or ``"opencv"``
    (``((i-cx)/fx, (j-cy)/fy, +1)``: dtu, ``dtu_proj.py:17-35``).  ``ndc_near`` (llff: 1.0) sends every ray through the reference's
    ``get_ndc_rays(H, W, focal, ndc_near, ...)``; ``near`` / ``far`` are then the NDC bounds the dataset packs (0, 1).  With the
    keyword defaults and one focal length this is ``sn_generate_rays`` as before; anything else is ``sn_generate_rays_cam``.

    ``focal`` may also be a device tensor with one element or of shape ``(2,)`` (``fx, fy``; not with ``ndc_near``, whose map has one
    focal length), ``center`` a device tensor of shape ``(2,)``.  If either is, the call reads the intrinsics on the device
    (``sn_generate_rays_cam_dev``: no host sync, capturable; the bits of the call with the same values as numbers) and the rays carry the
    gradient with respect to whichever of ``focal``, ``center`` and ``c2w`` require it (``sn_generate_rays_cam_dev_backward``).  The values
    of device intrinsics cannot be checked without a sync: a focal length <= 0 gives inf / NaN rays, not an error.  A CPU tensor
    that requires grad is refused; a CPU tensor or a number without grad goes the host path."""
    if not c2w.is_cuda:
        raise RuntimeError("sinnerf_amd.ray_utils.get_rays: c2w must be a CUDA/ROCm tensor (no CPU fallback)")
    if convention not in CONVENTIONS:
        raise ValueError(f"convention must be one of {sorted(CONVENTIONS)}, got {convention!r}")
    pose_grad = torch.is_grad_enabled() and c2w.requires_grad
    c2w = c2w.contiguous().float()
    if tuple(c2w.shape) != (3, 4):
        raise RuntimeError(f"c2w must be (3, 4), got {tuple(c2w.shape)}")
    win = tuple(window) if window is not None else (0, 0, 1, 1, W, H)
    if _on_device("focal", focal) | _on_device("center", center):
        intr = _intrinsics(H, W, focal, center, ndc_near is not None, c2w.device)
        ndc_near = None if ndc_near is None else float(ndc_near)
        if pose_grad or (torch.is_grad_enabled() and intr.requires_grad):
            return _GetRaysDevFn.apply(c2w, intr, H, W, CONVENTIONS[convention], ndc_near, near, far, win)
        return _generate_cam_dev(c2w, intr, H, W, CONVENTIONS[convention], ndc_near, near, far, win)
    pair = isinstance(focal, (tuple, list)) or getattr(focal, "ndim", 0) > 0
    if not pair and center is None and convention == "opengl" and ndc_near is None:
        if pose_grad:
            return _GetRaysFn.apply(c2w, H, W, focal, near, far, win)
        return _generate(c2w, H, W, focal, near, far, win)
    fx, fy = (float(focal[0]), float(focal[1])) if pair else (float(focal), float(focal))
    if ndc_near is not None and fx != fy:
        raise ValueError("the NDC map has one focal length (get_ndc_rays(H, W, focal, ...)): fx must equal fy")
    cx, cy = (W / 2, H / 2) if center is None else (float(center[0]), float(center[1]))
    cam = (fx, fy, cx, cy, CONVENTIONS[convention], None if ndc_near is None else float(ndc_near))
    if pose_grad:
        return _GetRaysCamFn.apply(c2w, H, W, cam, near, far, win)
    return _generate_cam(c2w, H, W, cam, near, far, win)


class _NdcRaysFn(torch.autograd.Function):
    """get_ndc_rays on (n, 8) rays; backward = sn_ndc_rays_backward at the saved world rays"""

    @staticmethod
    def forward(ctx, rays, H, W, focal, near):
        ctx.args = (H, W, focal, near)
        ctx.save_for_backward(rays)
        out = torch.empty_like(rays)
        with torch.cuda.device(rays.device):
            _lib.check(_lib.lib.sn_ndc_rays(_lib.ptr(rays), rays.shape[0], H, W, focal, near, _lib.ptr(out), _lib.stream_ptr()),
                       "sn_ndc_rays")
        return out

    @staticmethod
    def backward(ctx, g_out):
        H, W, focal, near = ctx.args
        rays, = ctx.saved_tensors
        g_out = g_out.contiguous().float()
        g_in = torch.empty_like(rays)
        with torch.cuda.device(rays.device):
            _lib.check(_lib.lib.sn_ndc_rays_backward(_lib.ptr(rays), _lib.ptr(g_out), rays.shape[0], H, W, focal, near, _lib.ptr(g_in),
                                                     _lib.stream_ptr()), "sn_ndc_rays_backward")
        return g_in, None, None, None, None


class _NdcRaysDevFn(torch.autograd.Function):
    """get_ndc_rays with the focal length in a one-element device tensor, differentiable in it too (sn_ndc_rays_dev_backward)"""

    @staticmethod
    def forward(ctx, rays, focal, H, W, near):
        ctx.args = (H, W, near)
        ctx.save_for_backward(rays, focal)
        out = torch.empty_like(rays)
        with torch.cuda.device(rays.device):
            _lib.check(_lib.lib.sn_ndc_rays_dev(_lib.ptr(rays), rays.shape[0], H, W, _lib.ptr(focal), near, _lib.ptr(out),
                                                _lib.stream_ptr()), "sn_ndc_rays_dev")
        return out

    @staticmethod
    def backward(ctx, g_out):
        H, W, near = ctx.args
        rays, focal = ctx.saved_tensors
        g_out = g_out.contiguous().float()
        ws = _lib.workspace(_lib.lib.sn_camera_backward_workspace_bytes(), "sn_camera_backward_workspace_bytes", rays.device)
        g_in, g_focal = torch.empty_like(rays), torch.empty_like(focal)
        with torch.cuda.device(rays.device):
            _lib.check(_lib.lib.sn_ndc_rays_dev_backward(_lib.ptr(rays), _lib.ptr(g_out), rays.shape[0], H, W, _lib.ptr(focal), near,
                                                         _lib.ptr(ws), _lib.ptr(g_in), _lib.ptr(g_focal), _lib.stream_ptr()),
                       "sn_ndc_rays_dev_backward")
        return g_in, g_focal, None, None, None


def get_ndc_rays(H, W, focal, near, rays_o, rays_d):
    """The reference's ``get_ndc_rays`` (``datasets/ray_utils.py:123-164``) for callers that hold world-space rays already:
    ``rays_o``, ``rays_d`` (N_rays, 3) on the ROCm device -> ``(rays_o, rays_d)`` in NDC, fp32.  ``near``: a float (the depth of the
    near plane; llff: 1.0).  Differentiable in ``rays_o`` and ``rays_d`` (``sn_ndc_rays_backward``).  ``focal``: a number, or a
    one-element device tensor: then it is read on the device (no sync; the bits of the float path) and the result is differentiable in
    it as well (``sn_ndc_rays_dev``, ``sn_ndc_rays_dev_backward``)."""
    if not (rays_o.is_cuda and rays_d.is_cuda):
        raise RuntimeError("sinnerf_amd.ray_utils.get_ndc_rays: rays_o and rays_d must be CUDA/ROCm tensors (no CPU fallback)")
    if rays_o.shape != rays_d.shape or rays_o.shape[-1] != 3:
        raise RuntimeError(f"rays_o and rays_d must both be (N_rays, 3), got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
    shape = rays_o.shape
    o, d = rays_o.reshape(-1, 3).float(), rays_d.reshape(-1, 3).float()
    rays = torch.cat([o, d, o.new_zeros((o.shape[0], 2))], 1)
    if _on_device("focal", focal):
        if focal.numel() != 1:
            raise RuntimeError(f"a focal tensor must have one element (the NDC map has one focal length), got {tuple(focal.shape)}")
        out = _NdcRaysDevFn.apply(rays, focal.reshape(1).to(device=rays.device, dtype=torch.float32), int(H), int(W), float(near))
    else:
        out = _NdcRaysFn.apply(rays, int(H), int(W), float(focal), float(near))
    return out[:, 0:3].reshape(shape), out[:, 3:6].reshape(shape)
