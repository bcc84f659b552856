"""The unseen view's geometry pseudo-labels on the GPU: the forward warp of the reference view and its depth into a new pose.

Reference: ``project_with_depth`` + ``forward_warp`` of ``datasets/blender_ray_patch_1image_rot3d.py:103-150`` (run on the CPU for
every training sample, ``:464-499``), ``blender_ray_patch_1image_proj.py:93-138`` (with ``depth_mask``),
``llff_ray_patch_1image_proj.py:117-166`` and ``warp_img_proj_numpy`` of ``dtu_proj.py:236-273`` (painter's loop).  Here one rule
(``include/sinnerf_hip.h``: ``sn_forward_warp``) covers the four, in fp64 on the device, with deterministic collisions; the projected
rays are drawn among the landed pixels by ``sn_select_landed`` instead of a boolean compaction.  Nothing in this module moves a value
to the host: the matrices are composed by a few fp64 torch ops on the device, and every entry can be captured in a graph.

The outputs are labels: they carry no gradient.
"""
import torch

from . import _lib
from .ray_utils import get_rays

COLLIDE = {"last": 0, "nearest": 1}


def _need_cuda(what, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"sinnerf_amd.warp.{what}: every tensor must be a CUDA/ROCm tensor (no CPU fallback)")


def _pose44(c2w):
    """(3, 4) or (4, 4) -> (4, 4) fp64 with the last row 0 0 0 1"""
    if tuple(c2w.shape) not in ((3, 4), (4, 4)):
        raise RuntimeError(f"a pose must be (3, 4) or (4, 4), got {tuple(c2w.shape)}")
    bottom = torch.zeros((1, 4), dtype=torch.float64, device=c2w.device)      # built by fills: a literal is copied from the host, which a
    bottom[:, 3:] = 1.0                                                       # stream under capture refuses (so it does `bottom[0, 3] = 1.0`)
    return torch.cat([c2w[:3].double(), bottom], 0)


def extrinsics_from_c2w(c2w, convention="opengl"):
    """World-to-camera (4, 4) fp64 of a camera-to-world pose, on its device.

    ``"opengl"``: ``[F R^T | -F R^T T]`` with ``F = diag(1, -1, -1)``, the y/z flip into the projective camera that ``convert`` of the
    blender and llff datasets produces (``blender_ray_patch_1image_rot3d.py:85-100``; it takes R as a rotation).  ``"opencv"``: the
    plain inverse of the pose, as ``dtu_proj.py:180-181``."""
    if convention not in ("opengl", "opencv"):
        raise ValueError(f"convention must be 'opengl' or 'opencv', got {convention!r}")
    p = _pose44(c2w)
    R, T = p[:3, :3], p[:3, 3:]
    if convention == "opengl":
        flip = torch.ones((3, 1), dtype=torch.float64, device=p.device)
        flip[1:] = -1.0
        Ri = flip * R.t()
    else:                                                   # rows of the inverse: cross products of the columns over the determinant
        c0, c1, c2 = R[:, 0], R[:, 1], R[:, 2]
        cr = torch.stack([torch.linalg.cross(c1, c2), torch.linalg.cross(c2, c0), torch.linalg.cross(c0, c1)])
        Ri = cr / (c0 * cr[0]).sum()
    return torch.cat([torch.cat([Ri, -(Ri @ T)], 1), p[3:]], 0)


def rotate_3d(c2w, x, y, z):
    """The pose ``c2w`` ((3, 4) or (4, 4)) turned about the world origin by ``x``, ``y``, ``z`` degrees (numbers or device scalars):
    ``Rx(x) Ry(y) Rz(z) c2w`` with ``Ry = [[c, 0, -s], [0, 1, 0], [s, 0, c]]``, the interface and the sign conventions of the
    reference's ``rotate_3d`` (``blender_ray_patch_1image_rot3d.py:80-82``).  Formed in fp64 on the device, returned in ``c2w``'s dtype
    and shape."""
    _need_cuda("rotate_3d", c2w)
    a = torch.deg2rad(torch.stack([torch.as_tensor(v, dtype=torch.float64, device=c2w.device) for v in (x, y, z)]))
    c, s = torch.cos(a), torch.sin(a)
    one, zero = torch.ones_like(c[0]), torch.zeros_like(c[0])
    rows = lambda *v: torch.stack(v).reshape(3, 3)
    Rx = rows(one, zero, zero, zero, c[0], -s[0], zero, s[0], c[0])
    Ry = rows(c[1], zero, -s[1], zero, one, zero, s[1], zero, c[1])
    Rz = rows(c[2], -s[2], zero, s[2], c[2], zero, zero, zero, one)
    out = c2w.double().clone()
    out[:3] = (Rx @ Ry @ Rz) @ c2w[:3].double()
    return out.to(c2w.dtype)


def projection_matrix(intrinsics, extrinsics):
    """``[K E[:3]; 0 0 0 1]`` (4, 4) fp64 on the device"""
    P = torch.zeros((4, 4), dtype=torch.float64, device=intrinsics.device)
    P[:3] = intrinsics.double() @ extrinsics.double()[:3]
    P[3:, 3:] = 1.0                                         # a slice: `P[3, 3] = 1.0` is refused by a stream under capture
    return P


def _warp(data, ref_depth, ref_proj, src_proj, mode, eps, window, want_new=True, want_depth=True, want_mask=True, want_winner=False):
    """one sn_forward_warp call -> (new, new_depth, mask uint8, winner), each (out_h * out_w[, C]) or None"""
    H, W = ref_depth.shape
    dev = ref_depth.device
    x0, y0, sx, sy, ow, oh = (0, 0, 1, 1, W, H) if window is None else tuple(int(v) for v in window)
    n_out = max(ow, 0) * max(oh, 0)
    C = data.shape[-1] if data is not None else 0
    new = torch.empty((n_out, C), dtype=torch.float32, device=dev) if (want_new and data is not None) else None
    new_depth = torch.empty((n_out,), dtype=torch.float32, device=dev) if want_depth else None
    mask = torch.empty((n_out,), dtype=torch.uint8, device=dev) if want_mask else None
    winner = torch.empty((n_out,), dtype=torch.int32, device=dev) if want_winner else None
    ws = _lib.workspace(_lib.lib.sn_forward_warp_workspace_bytes(H, W), "sn_forward_warp_workspace_bytes", dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.sn_forward_warp(_lib.ptr(ref_depth), _lib.ptr(data), H, W, C, _lib.ptr(ref_proj), _lib.ptr(src_proj),
                                            float(eps), mode, x0, y0, sx, sy, ow, oh, _lib.ptr(new), _lib.ptr(new_depth),
                                            _lib.ptr(mask), _lib.ptr(winner), _lib.ptr(ws), _lib.stream_ptr()), "sn_forward_warp")
    return new, new_depth, mask, winner, (oh, ow)


def _prepare(what, data, ref_depth, collide):
    if collide not in COLLIDE:
        raise ValueError(f"collide must be 'last' or 'nearest', got {collide!r}")
    _need_cuda(what, data, ref_depth)
    ref_depth = ref_depth.detach()
    if ref_depth.ndim == 3 and ref_depth.shape[0] == 1:
        ref_depth = ref_depth[0]
    if ref_depth.ndim != 2:
        raise RuntimeError(f"ref_depth must be (H, W) or (1, H, W), got {tuple(ref_depth.shape)}")
    ref_depth = ref_depth.contiguous().float()
    if data is not None:
        data = data.detach()
        if data.ndim == 4 and data.shape[0] == 1:
            data = data[0].permute(1, 2, 0)                 # (1, C, H, W), as the reference passes it
        if data.ndim != 3 or tuple(data.shape[:2]) != tuple(ref_depth.shape):
            raise RuntimeError(f"data must be (1, C, H, W) or (H, W, C) over ref_depth's frame, got {tuple(data.shape)}")
        data = data.contiguous().float()
    return data, ref_depth


def forward_warp_proj(data, ref_depth, ref_proj_mat, src_proj_mat, *, collide="last", eps=0.0, window=None, return_winner=False):
    """``forward_warp`` from the two (4, 4) projection matrices ``[K E[:3]; 0 0 0 1]``, the form ``warp_img_proj_numpy`` takes
    (``dtu_proj.py:236-273``; its painter's loop is ``collide="nearest"``).  Keywords and results as for ``forward_warp``."""
    data, ref_depth = _prepare("forward_warp_proj", data, ref_depth, collide)
    _need_cuda("forward_warp_proj", ref_proj_mat, src_proj_mat)
    ref_P, src_P = ref_proj_mat.detach().double().contiguous(), src_proj_mat.detach().double().contiguous()
    if tuple(ref_P.shape) != (4, 4) or tuple(src_P.shape) != (4, 4):
        raise RuntimeError("the projection matrices must be (4, 4)")
    new, new_depth, mask, winner, (oh, ow) = _warp(data, ref_depth, ref_P, src_P, COLLIDE[collide], eps, window,
                                                   want_winner=return_winner)
    out = (None if new is None else new.reshape(oh, ow, -1), new_depth.reshape(oh, ow), mask.view(torch.bool).reshape(oh, ow))
    return out + (winner.reshape(oh, ow),) if return_winner else out


def forward_warp(data, ref_depth, ref_intrinsics, ref_extrinsics, src_intrinsics, src_extrinsics, *, collide="last", eps=0.0,
                 window=None, return_winner=False):
    """The reference's ``forward_warp(data, ref_depth, ref_intrinsics, ref_extrinsics, src_intrinsics, src_extrinsics)`` on the device.

    ``data``: (1, C, H, W) as the reference passes it, or channel-last (H, W, C); ``ref_depth``: (H, W) or (1, H, W); intrinsics (3, 3),
    extrinsics (4, 4) world-to-camera (``extrinsics_from_c2w``).  ``collide``: ``"last"`` -- the last source pixel in raster order wins a
    target (the blender datasets) -- or ``"nearest"`` -- the smallest projected depth wins (llff, dtu).  ``eps`` is added to the
    divisor (llff: 1e-9).  ``window = (x0, y0, stride_x, stride_y, out_w, out_h)`` as for ``get_rays`` restricts what is written; the
    scatter always covers the frame.

    Returns ``new`` (out_h, out_w, C), ``new_depth`` (out_h, out_w), ``depth_mask`` (out_h, out_w) bool and, with ``return_winner``,
    the source raster index per pixel (int32, -1 where nothing landed).  A source pixel whose projection is NaN is dropped."""
    if collide not in COLLIDE:
        raise ValueError(f"collide must be 'last' or 'nearest', got {collide!r}")
    _need_cuda("forward_warp", data, ref_depth, ref_intrinsics, ref_extrinsics, src_intrinsics, src_extrinsics)
    return forward_warp_proj(data, ref_depth, projection_matrix(ref_intrinsics, ref_extrinsics),
                             projection_matrix(src_intrinsics, src_extrinsics), collide=collide, eps=eps, window=window,
                             return_winner=return_winner)


def select_landed(mask, u):
    """``idx`` (m,) int32 and ``n_landed`` (0-d int32) on the device: with N set elements in ``mask`` (any shape, bool or uint8),
    ``idx[j]`` is the raster index of the ``min(floor(u[j] N), N - 1)``-th of them; -1 everywhere when N = 0.  ``u``: (m,) in [0, 1).
    The device form of ``np.random.choice(N, m)`` over ``rays_full[depth_mask]`` (``blender_ray_patch_1image_proj.py:390-394``)."""
    _need_cuda("select_landed", mask, u)
    mask = mask.detach().contiguous()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise RuntimeError(f"mask must be bool or uint8, got {mask.dtype}")
    u = u.detach().reshape(-1).contiguous().float()
    n, m, dev = mask.numel(), u.numel(), mask.device
    idx = torch.empty((m,), dtype=torch.int32, device=dev)
    n_landed = torch.empty((), dtype=torch.int32, device=dev)
    ws = _lib.workspace(_lib.lib.sn_select_landed_workspace_bytes(n), "sn_select_landed_workspace_bytes", dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.sn_select_landed(_lib.ptr(mask), n, _lib.ptr(u), m, _lib.ptr(idx), _lib.ptr(n_landed), _lib.ptr(ws),
                                             _lib.stream_ptr()), "sn_select_landed")
    return idx, n_landed


def unseen_view_batch(ref_view, ref_depth, K, ref_c2w, side_c2w, near, far, window, u_proj, collide="last", *, focal, eps=0.0,
                      center=None, convention="opengl", ndc_near=None):
    """The unseen-view part of a training sample (``blender_ray_patch_1image_rot3d.py:473-515``,
    ``blender_ray_patch_1image_proj.py:376-394, 472-478``) with no host sync, as a dict with the reference's keys:

    * ``rays_full`` (ph * pw, 8): the window's rays from ``side_c2w`` (``get_rays``; the reference's ``fake_patch``);
    * ``warp_patch`` (C, ph, pw), ``warp_patch_depth`` (ph, pw): the reference view and its depth warped into ``side_c2w``, at the window;
    * ``rays_proj`` (m, 8), ``depth_proj`` (m,): the rays of ``side_c2w`` and the warped depths at the pixels ``select_landed`` draws
      with ``u_proj`` (m,) among those of the full frame where a pixel landed; zero rows when none landed;
    * ``side_coord``: the window's row coordinates and column coordinates (stacked (2, ps) when the window is square, else a pair);
    * ``n_landed``: 0-d int32 device tensor, the number of landed pixels of the full frame.

    ``ref_view`` (H, W, C) channel-last or (1, C, H, W); ``ref_depth`` (H, W); ``K`` (3, 3); the poses (3, 4) or (4, 4) camera-to-world;
    ``focal``, ``center``, ``convention``, ``ndc_near``, ``near``, ``far``: the camera of ``get_rays``; the extrinsics of the warp follow
    ``convention`` (``extrinsics_from_c2w``).

    The window is ``(x0, y0, stride_x, stride_y, pw, ph)`` in pixel coordinates (x = column).  The reference slices
    ``depth[ll:ll + (ps - 1) sW + 1:sW, up:up + (ps - 1) sH + 1:sH]``: its ``ll`` indexes ROWS and its ``up`` COLUMNS, so the same
    patch is ``window = (up, ll, sH, sW, ps, ps)``.  Whether the window is all holes (the reference redraws it, ``rot3d:486-499``) is the
    caller's to decide from ``warp_patch_depth`` and ``n_landed``."""
    data, depth = _prepare("unseen_view_batch", ref_view, ref_depth, collide)
    _need_cuda("unseen_view_batch", K, ref_c2w, side_c2w, u_proj)
    H, W = depth.shape
    x0, y0, sx, sy, pw, ph = (int(v) for v in window)
    ref_P = projection_matrix(K, extrinsics_from_c2w(ref_c2w, convention)).contiguous()
    src_P = projection_matrix(K, extrinsics_from_c2w(side_c2w, convention)).contiguous()
    mode = COLLIDE[collide]
    new, new_depth, _, _, _ = _warp(data, depth, ref_P, src_P, mode, eps, (x0, y0, sx, sy, pw, ph), want_mask=False)
    _, depth_full, mask_full, _, _ = _warp(None, depth, ref_P, src_P, mode, eps, None)
    idx, n_landed = select_landed(mask_full, u_proj)
    focal, center = (v.detach() if torch.is_tensor(v) else v for v in (focal, center))       # labels: no gradient, device tensors stay there
    cam = dict(center=center, convention=convention, ndc_near=ndc_near)
    side_pose = side_c2w[:3].detach().float()
    rays_full = get_rays(H, W, focal, side_pose, near, far, (x0, y0, sx, sy, pw, ph), **cam)
    rays_all = get_rays(H, W, focal, side_pose, near, far, None, **cam)
    valid = idx >= 0
    at = idx.clamp(min=0).long()
    rows = torch.arange(ph, device=depth.device) * sy + y0
    cols = torch.arange(pw, device=depth.device) * sx + x0
    return {"rays_full": rays_full,
            "warp_patch": new.reshape(ph, pw, -1).permute(2, 0, 1),
            "warp_patch_depth": new_depth.reshape(ph, pw),
            "rays_proj": rays_all[at] * valid[:, None],
            "depth_proj": depth_full[at] * valid,
            "side_coord": torch.stack([rows, cols]) if ph == pw else (rows, cols),
            "n_landed": n_landed}


def unseen_view_full(ref_view, ref_depth, K, ref_c2w, side_c2w, near, far, collide="last", *, focal, eps=0.0, center=None,
                     convention="opengl", ndc_near=None, ref_proj=None):
    """The FULL frame of the unseen view, for a caller that picks its window on the device afterwards (``sinnerf_amd.sampler``): the
    reference view and its depth warped into ``side_c2w`` by ONE ``sn_forward_warp`` (``blender_ray_patch_1image_rot3d.py:481-484``) and
    the rays of ``side_c2w`` by one ``get_rays`` (``:476-479``).  Arguments as for ``unseen_view_batch``, without a window and ``u_proj``;
    ``ref_proj``: the (4, 4) fp64 projection matrix of the reference pose where the caller keeps it (it does not change between draws).

    Returns a dict: ``out`` (H, W, C), ``depth`` (H, W), ``mask`` (H, W) uint8 -- 1 where a pixel landed -- and ``rays`` (H * W, 8).
    No value moves to the host and nothing is built from host literals, so the call can be captured in a graph."""
    data, depth = _prepare("unseen_view_full", ref_view, ref_depth, collide)
    _need_cuda("unseen_view_full", K, ref_c2w, side_c2w, ref_proj)
    if data is None:
        raise RuntimeError("unseen_view_full: ref_view is required")
    H, W = depth.shape
    ref_P = projection_matrix(K, extrinsics_from_c2w(ref_c2w, convention)) if ref_proj is None else ref_proj.detach().double()
    src_P = projection_matrix(K, extrinsics_from_c2w(side_c2w, convention))
    new, new_depth, mask, _, _ = _warp(data, depth, ref_P.contiguous(), src_P.contiguous(), COLLIDE[collide], eps, None)
    focal, center = (v.detach() if torch.is_tensor(v) else v for v in (focal, center))       # labels: no gradient
    rays = get_rays(H, W, focal, side_c2w[:3].detach().float(), near, far, None, center=center, convention=convention, ndc_near=ndc_near)
    return {"out": new.reshape(H, W, -1), "depth": new_depth.reshape(H, W), "mask": mask.reshape(H, W), "rays": rays}
