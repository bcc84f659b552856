"""One-image training batches drawn on the device: what the reference's train split builds per sample on the CPU
(``datasets/blender_ray_patch_1image_rot3d.py:443-528``; without the rejection loops ``llff_ray_patch_1image_proj.py:619-669``), with
every random choice made on the device, nothing read back and every launch capturable in a graph.

``OneImageSampler`` holds on the device what the dataset's ``__init__`` holds on the host (``rot3d:253-363``) and ``draw()`` returns the
dict ``SinNeRFSystem._training_step_patches`` consumes.  The two rejection loops -- redraw a uniform window origin until the window has
content (``rot3d:451-460``, ``:486-499``) -- accept an origin uniform over the origins WITH content, so each is one
``sn_valid_windows`` (the map of such origins) and one ``sn_select_landed`` (its ``floor(u N)``-th set element); the strided slices are
``sn_gather_windows`` at an origin the kernel reads from device memory.  The outputs are labels: they carry no gradient.

Names.  The reference's ``ll`` indexes ROWS with stride ``sW`` and its ``up`` COLUMNS with stride ``sH`` (``rot3d:456-457``); in the
llff file ``patch_size_x`` goes with ``ll`` and ``patch_size_y`` with ``up`` (``llff:625-630``).  In pixel coordinates (x = column) a
window is therefore ``(x0, y0, stride_x, stride_y, pw, ph) = (up, ll, sH, sW, patch_size_y, patch_size_x)``; origins are ``(x0, y0)``.
"""
import ctypes

import torch

from . import _lib, warp
from .ray_utils import get_rays

MAX_SOURCES = 8                                  # SN_GATHER_MAX_SOURCES of include/sinnerf_hip.h
CHOICES = ("origin_real", "origin_side", "ray_idx", "ray_idx2", "angles", "u_proj")


def _need_cuda(what, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"sinnerf_amd.sampler.{what}: every tensor must be a CUDA/ROCm tensor (no CPU fallback)")


def _as_mask(what, mask):
    _need_cuda(what, mask)
    mask = mask.detach().contiguous()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8 or mask.ndim != 2:
        raise RuntimeError(f"mask must be (H, W) bool or uint8, got {tuple(mask.shape)} {mask.dtype}")
    return mask


def reference_counts(H, W, stride_x, stride_y, pw, ph):
    """``(nx, ny)``: the candidate origins of ``np.random.randint(0, w - (ps - 1) * sW - 1)`` (``rot3d:452-455``): one fewer per axis
    than would fit"""
    return W - (pw - 1) * stride_x - 1, H - (ph - 1) * stride_y - 1


def valid_windows(mask, stride_x, stride_y, pw, ph, nx=None, ny=None):
    """``valid`` (ny, nx) uint8 and ``n_valid`` (0-d int32) on the device: ``valid[y0, x0]`` is 1 where any
    ``mask[y0 + j stride_y, x0 + i stride_x]``, ``j < ph``, ``i < pw``, is set (``sn_valid_windows``).  ``mask``: (H, W) bool or uint8.
    ``nx``, ``ny`` default to the reference's candidate counts (``reference_counts``)."""
    mask = _as_mask("valid_windows", mask)
    H, W = mask.shape
    rx, ry = reference_counts(H, W, stride_x, stride_y, pw, ph)
    nx, ny = rx if nx is None else int(nx), ry if ny is None else int(ny)
    dev = mask.device
    valid = torch.empty((max(ny, 0), max(nx, 0)), dtype=torch.uint8, device=dev)
    n_valid = torch.empty((), dtype=torch.int32, device=dev)
    ws = _lib.workspace(_lib.lib.sn_valid_windows_workspace_bytes(H, nx), "sn_valid_windows_workspace_bytes", dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.sn_valid_windows(_lib.ptr(mask), H, W, int(stride_x), int(stride_y), int(pw), int(ph), nx, ny,
                                             _lib.ptr(valid), _lib.ptr(n_valid), _lib.ptr(ws), _lib.stream_ptr()), "sn_valid_windows")
    return valid, n_valid


def gather_windows(sources, origin, stride_x, stride_y, pw, ph, planar=None):
    """The strided window at ``origin`` -- (2,) int32 ON THE DEVICE, ``(x0, y0)``, clamped into the frame by the kernel -- out of each of
    up to 8 channel-last ``(H, W, C_k)`` (or ``(H, W)``) fp32 / int32 tensors over one frame, in one launch (``sn_gather_windows``).
    Returns a list: ``(ph, pw, C_k)`` per source, or ``(C_k, ph, pw)`` where ``planar[k]`` is true; values bit for bit."""
    _need_cuda("gather_windows", origin, *sources)
    n = len(sources)
    if not 1 <= n <= MAX_SOURCES:
        raise RuntimeError(f"gather_windows takes 1..{MAX_SOURCES} sources, got {n}")
    planar = [False] * n if planar is None else [bool(p) for p in planar]
    if len(planar) != n:
        raise RuntimeError("planar must name a layout per source")
    if origin.dtype != torch.int32 or origin.numel() != 2:
        raise RuntimeError(f"origin must be two int32 on the device, got {tuple(origin.shape)} {origin.dtype}")
    H, W = sources[0].shape[:2]
    srcs, dsts, chans = [], [], []
    for s, p in zip(sources, planar):
        s = s.detach()
        if s.ndim == 2:
            s = s[..., None]
        if s.ndim != 3 or tuple(s.shape[:2]) != (H, W) or s.element_size() != 4:
            raise RuntimeError(f"a source must be (H, W[, C]) over one frame with 4-byte elements, got {tuple(s.shape)} {s.dtype}")
        C = s.shape[2]
        srcs.append(s.contiguous())
        dsts.append(torch.empty((C, ph, pw) if p else (ph, pw, C), dtype=s.dtype, device=s.device))
        chans.append(C)
    origin = origin.detach().reshape(2).contiguous()
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    mask = sum(1 << k for k, p in enumerate(planar) if p)
    with torch.cuda.device(origin.device):
        _lib.check(_lib.lib.sn_gather_windows(ptrs(srcs), ptrs(dsts), (ctypes.c_int * n)(*chans), n, mask, H, W, _lib.ptr(origin),
                                              int(stride_x), int(stride_y), int(pw), int(ph), _lib.stream_ptr()), "sn_gather_windows")
    return dsts


class OneImageSampler:
    """The train split of the reference's one-image datasets, resident on the device.

    ``ref_view`` (H, W, 3) channel-last or (1, 3, H, W), ``ref_depth`` (H, W), ``ref_c2w`` (3, 4) or (4, 4), ``K`` (3, 3): the reference
    view, its depth, its pose and the intrinsics of the warp.  ``focal``, ``center``, ``convention``, ``ndc_near``, ``near``, ``far``: the
    camera of ``ray_utils.get_rays``.  ``patch_size`` (or ``patch_size_x`` -- rows -- and ``patch_size_y`` -- columns), ``sW`` (row
    stride), ``sH`` (column stride), ``angle``, ``num`` (4096 at ``rot3d:464``): the reference's.  ``collide``, ``eps``: the warp's
    (``warp.forward_warp``; rot3d: ``"last"``, 1e-9).  Held from construction on (``rot3d:253-363``): ``all_rays`` (H W, 8) of the
    reference pose, ``all_rgbs`` (H W, 3), ``all_depth`` (H W, 1), ``nonwhite`` (H, W) uint8 = ``rgb.sum(-1) != 3`` with its count
    ``rgb_num`` (row k of the reference's ``nonzero_*`` tables is the k-th set pixel of that mask), ``content`` (H, W) uint8 = a pixel
    with a non-zero channel, and -- the image does not change -- the real window's valid map.  Construction may synchronise; ``draw``
    never does.  An image without a non-white pixel is refused (the reference's ``np.random.choice(0, n)`` raises too).

    ``require_content=False``: no rejection loops, as in the llff file (``llff:625-645``): both origins are uniform over all candidates
    and no valid map is formed.  ``candidates="all"`` admits every origin that fits instead of the reference's one-fewer count.
    ``ref_patch_origin``: the rot3d file slices the reference-view patch (``depth_ray``, ``depth_gt``, ``depth_ray_rgb``, ``:523-528``)
    with the ``ll, up`` the UNSEEN-view loop left behind, not those of ``real_patch``; ``"side"`` (default) mirrors that, ``"real"``
    uses the real window's origin.

    ``generator``: a ``torch.Generator`` of the device; default: the device's default generator.  With several ranks each rank's sampler
    draws from its own generator: seed them differently (the reference's DataLoader workers do), or every rank draws the same batch.

    Differences from the reference, on purpose: (1) ``rays_proj`` / ``depth_proj`` are drawn among the landed pixels of THIS draw's
    pose, as ``warp.unseen_view_batch`` does; the table of 125 pre-warped poses of ``rot3d:365-410`` is not reproduced.  (2) Where no
    origin has content the reference loops forever; here the window falls back to origin (0, 0) and ``n_valid_real`` / ``n_valid_side``
    say 0 (the step's ``n_depth > 0`` guard keeps its loss finite).  (3) The pose is composed in fp64 on the device
    (``warp.rotate_3d``) and rounded once.
    """

    def __init__(self, ref_view, ref_depth, ref_c2w, K, *, focal, near, far, patch_size=None, patch_size_x=None, patch_size_y=None,
                 sW=1, sH=1, angle=30, num=4096, collide="last", eps=0.0, center=None, convention="opengl", ndc_near=None,
                 require_content=True, candidates="reference", ref_patch_origin="side", generator=None):
        if candidates not in ("reference", "all"):
            raise ValueError(f"candidates must be 'reference' or 'all', got {candidates!r}")
        if ref_patch_origin not in ("side", "real"):
            raise ValueError(f"ref_patch_origin must be 'side' or 'real', got {ref_patch_origin!r}")
        _need_cuda("OneImageSampler", ref_view, ref_depth, ref_c2w, K)
        data, depth = warp._prepare("OneImageSampler", ref_view, ref_depth, collide)
        if data is None or data.shape[-1] != 3:
            raise RuntimeError("ref_view must have three channels")
        self.ref_view, self.ref_depth = data, depth
        self.H, self.W = H, W = depth.shape
        self.device = depth.device
        ph = patch_size if patch_size_x is None else patch_size_x
        pw = patch_size if patch_size_y is None else patch_size_y
        if ph is None or pw is None:
            raise ValueError("give patch_size, or patch_size_x and patch_size_y")
        self.ph, self.pw, self.sy, self.sx = int(ph), int(pw), int(sW), int(sH)
        self.window = (self.sx, self.sy, self.pw, self.ph)
        fit = (W - (self.pw - 1) * self.sx, H - (self.ph - 1) * self.sy)
        self.nx, self.ny = fit if candidates == "all" else (fit[0] - 1, fit[1] - 1)
        if min(self.ph, self.pw, self.sx, self.sy) <= 0 or self.nx <= 0 or self.ny <= 0:
            raise ValueError(f"a {self.ph} x {self.pw} window of strides ({self.sy}, {self.sx}) has no candidate origin in {H} x {W}")
        self.num, self.angle = int(num), angle
        self.collide, self.eps = collide, float(eps)
        self.near, self.far = near, far
        self.require_content, self.ref_patch_origin, self.generator = bool(require_content), ref_patch_origin, generator
        self.cam = dict(focal=focal.detach() if torch.is_tensor(focal) else focal, center=center.detach() if torch.is_tensor(center) else center,
                        convention=convention, ndc_near=ndc_near)
        self.ref_c2w = ref_c2w.detach().float().contiguous()
        self.K = K.detach().double().contiguous()
        self.ref_proj = warp.projection_matrix(self.K, warp.extrinsics_from_c2w(self.ref_c2w, convention)).contiguous()
        f, cam = self.cam["focal"], {k: v for k, v in self.cam.items() if k != "focal"}
        self.all_rays = get_rays(H, W, f, self.ref_c2w[:3].contiguous(), near, far, None, **cam)       # rot3d:336-345
        self.all_rgbs = data.reshape(-1, 3)
        self.all_depth = depth.reshape(-1, 1)
        self.nonwhite = (self.all_rgbs.sum(-1) != 3).reshape(H, W).to(torch.uint8)                   # rot3d:347-351
        self.rgb_num = int(self.nonwhite.sum().item())
        if self.rgb_num == 0:
            raise ValueError("the reference view has no non-white pixel to draw rays from")
        if self.rgb_num > 1 << 23:
            raise ValueError("more than 2^23 non-white pixels: the fp32 u of sn_select_landed no longer names every one of them")
        # rot3d:459 tests patch.max() != 0 over the window's channels; the image is non-negative, so that is "a non-zero channel"
        self.content = (data != 0).any(-1).to(torch.uint8)
        self._count = torch.full((), self.nx * self.ny, dtype=torch.int32, device=self.device)
        if self.require_content:
            self.valid_real, self.n_valid_real = valid_windows(self.content, *self.window, self.nx, self.ny)
        else:
            self.valid_real, self.n_valid_real = None, self._count
        max_x0, max_y0 = W - 1 - (self.pw - 1) * self.sx, H - 1 - (self.ph - 1) * self.sy
        self._origin_max = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._origin_max[0], self._origin_max[1] = max_x0, max_y0
        self._origin_min = torch.zeros(2, dtype=torch.int32, device=self.device)

    def signature(self):
        """what a captured ``draw`` bakes in besides the tensors it reads: shapes and the host-side numbers of every launch"""
        return (self.H, self.W, self.window, self.nx, self.ny, self.num, self.angle, self.collide, self.eps, self.near, self.far,
                self.require_content, self.ref_patch_origin, self.rgb_num, self.cam["convention"], self.cam["ndc_near"],
                tuple((k, v.data_ptr() if torch.is_tensor(v) else v) for k, v in self.cam.items() if k in ("focal", "center")))

    # ---- the pieces of a draw ------------------------------------------------------------------------------------------------------
    def _rand(self, n):
        return torch.rand(n, device=self.device, generator=self.generator)

    def _origin(self, valid):
        """(x0, y0) int32 (2,): uniform over the set elements of ``valid``; over all candidates when it is None; (0, 0) when none is set"""
        if valid is None:
            idx = torch.randint(0, self.nx * self.ny, (1,), device=self.device, generator=self.generator)
        else:
            idx, _ = warp.select_landed(valid, self._rand(1))
            idx = idx.clamp(min=0)                                           # -1: nothing valid
        y0 = torch.div(idx, self.nx, rounding_mode="floor")
        return torch.cat([idx - y0 * self.nx, y0]).to(torch.int32)

    def _clamped(self, origin):
        """the clamp of sn_gather_windows, so that ``side_coord`` names the pixels the kernel read"""
        origin = origin.detach().reshape(2).to(torch.int32)
        return torch.minimum(torch.maximum(origin, self._origin_min), self._origin_max).contiguous()

    def unseen_view(self, angles):
        """the drawn pose ``rotate_3d(ref_c2w, x, y, z)`` (``rot3d:473-475``) and the full frame seen from it (``warp.unseen_view_full``):
        a dict with ``c2w`` (3, 4), ``out`` (H, W, 3), ``depth`` (H, W), ``mask`` (H, W) uint8, ``rays`` (H W, 8).  ``angles``: (3,)
        degrees on the device."""
        _need_cuda("unseen_view", angles)
        a = angles.detach().double().reshape(3)
        c2w = warp.rotate_3d(self.ref_c2w, a[0], a[1], a[2])[:3].contiguous()
        full = warp.unseen_view_full(self.ref_view, self.ref_depth, self.K, self.ref_c2w, c2w, self.near, self.far, self.collide,
                                     eps=self.eps, ref_proj=self.ref_proj, **self.cam)
        full["c2w"] = c2w
        return full

    def side_valid(self, depth_full):
        """``(valid, n_valid)`` of the unseen view's window.  ``rot3d:493`` tests ``warp_patch_depth.sum() != 0``; the map here is "any
        pixel of the window != 0".  The two agree wherever the depths are non-negative -- the warp writes the depth of a surface in front
        of the camera, or 0 where nothing landed -- because a sum of non-negative terms is zero only if every term is."""
        return valid_windows((depth_full != 0).to(torch.uint8), *self.window, self.nx, self.ny)

    def draw(self, choices=None):
        """One training batch, every tensor on the device, under the keys ``SinNeRFSystem`` reads:

            reference key (rot3d:503-528)             key here        shape
            ``depth_ray``                             ``rays_full``   (ph pw, 8)   rays of the reference-view patch
            ``depth_ray_rgb``                         ``rgbs_full``   (ph pw, 3)
            ``rays_full`` (the ``fake_patch``)        ``rays_side``   (ph pw, 8)   the unseen view's window
            ``rays``, ``rgbs``, ``depth``             unchanged       (num, 8 / 3 / 1): ``num - num // 10`` rows of non-white pixels,
                                                                      then ``num // 10`` of all pixels (``:464-466``, ``:503-505``)
            ``depth_gt``                              unchanged       (ph pw, 1)
            ``real_patch``                            unchanged       (1, 3, ph, pw): collated, as a discriminator takes it
            ``warp_patch``, ``warp_patch_depth``      unchanged       (3, ph, pw), (ph, pw)
            ``rays_proj``, ``depth_proj``             unchanged       (num, 8), (num, 1); zero rows when nothing landed
            ``side_coord``                            unchanged       (2, ps) int64 rows, columns (a pair when ph != pw) (``:515``)

        and ``side_rgb`` (ph pw, 3): the warped patch with white where nothing landed (``models/sinnerf.py:300-302``); ``n_landed``,
        ``n_valid_real``, ``n_valid_side`` (0-d int32; the latter two 0 when no origin had content: the window is then at (0, 0));
        ``origin_real``, ``origin_side`` ((2,) int32, ``(x0, y0)`` = ``(up, ll)``), ``angles`` ((3,) fp64 degrees), ``c2w_side`` (3, 4).

        ``choices``: a dict of DEVICE tensors that replace draws -- ``origin_real``, ``origin_side`` ((2,) int32 ``(x0, y0)``, clamped into
        the frame), ``ray_idx`` (``num // 10`` raster indices, ``:465``), ``ray_idx2`` (``num - num // 10`` indices into the non-white
        pixels, ``:466``), ``angles`` ((3,) degrees, ``:468-472``), ``u_proj`` ((num,) in [0, 1)).  What is not given comes from the
        generator in the reference's order: the u of the real origin (one ``rand(1)``; ``randint`` with ``require_content=False``);
        ``ray_idx`` (``randint``); ``ray_idx2`` (``randint``); ``angles`` (``randn(3)`` fp64, times ``angle // 2``); the u of the unseen
        origin; ``u_proj`` (``rand(num)``).  Nothing is read back: the call can be captured in a graph, and each replay draws afresh."""
        ch = {} if choices is None else dict(choices)
        unknown = set(ch) - set(CHOICES)
        if unknown:
            raise KeyError(f"unknown choices {sorted(unknown)}; known: {CHOICES}")
        _need_cuda("draw", *ch.values())
        dev, g = self.device, self.generator
        n_all = self.num // 10
        n_nonwhite = self.num - n_all
        with torch.no_grad():
            # rot3d:451-460: the real patch's window
            origin_real = self._clamped(ch["origin_real"] if "origin_real" in ch else self._origin(self.valid_real))
            # :465-466: ray_idx over all pixels, ray_idx2 over the non-white ones
            ray_idx = ch["ray_idx"] if "ray_idx" in ch else torch.randint(0, self.H * self.W, (n_all,), device=dev, generator=g)
            ray_idx2 = ch["ray_idx2"] if "ray_idx2" in ch else torch.randint(0, self.rgb_num, (n_nonwhite,), device=dev, generator=g)
            # row k of nonzero_rays = the k-th set pixel of the mask: u = (k + 1/2) / N has floor(u N) = k in fp32 for N <= 2^23
            u2 = ((ray_idx2.double() + 0.5) / self.rgb_num).float()
            at2, _ = warp.select_landed(self.nonwhite, u2)
            pick = torch.cat([at2.long(), ray_idx.long()])                  # :503-505: the non-white rows first
            # :468-473: the unseen pose
            if "angles" in ch:
                angles = ch["angles"].detach().double().reshape(3)
            else:
                angles = torch.randn(3, dtype=torch.float64, device=dev, generator=g) * float(self.angle // 2)
            full = self.unseen_view(angles)                                 # :476-484: ONE full-frame warp, one full-frame get_rays
            # :486-499: the unseen view's window, among the origins whose window is not all holes
            if self.require_content:
                valid_side, n_valid_side = self.side_valid(full["depth"])
            else:
                valid_side, n_valid_side = None, self._count
            origin_side = self._clamped(ch["origin_side"] if "origin_side" in ch else self._origin(valid_side))
            u_proj = ch["u_proj"].detach().reshape(-1).float() if "u_proj" in ch else self._rand(self.num)
            idx, n_landed = warp.select_landed(full["mask"], u_proj)
            landed = idx >= 0
            at = idx.clamp(min=0).long()

            ref_rays = self.all_rays.reshape(self.H, self.W, 8)              # rot3d:363 ref_rays
            side_rays = full["rays"].reshape(self.H, self.W, 8)              # :479 rays_full.view(w, h, 8)
            at_side = [full["out"], full["depth"], side_rays]               # :491-497
            ref_patch = [ref_rays, self.ref_depth, self.ref_view]           # :523-528
            at_real = [self.ref_view]                                       # :456-457
            if self.ref_patch_origin == "side":
                at_side += ref_patch
            else:
                at_real += ref_patch
            got_side = gather_windows(at_side, origin_side, *self.window, planar=[True] + [False] * (len(at_side) - 1))
            got_real = gather_windows(at_real, origin_real, *self.window, planar=[True] + [False] * (len(at_real) - 1))
            warp_patch, warp_patch_depth, rays_side = got_side[:3]
            real_patch = got_real[0]
            rays_full, depth_gt, rgbs_full = got_side[3:] if self.ref_patch_origin == "side" else got_real[1:]
            # :515: side_coord is the unseen window's, whichever origin the reference-view patch took
            rows =torch.arange(self.ph, device=dev) * self.sy + origin_side[1]
            cols = torch.arange(self.pw, device=dev) * self.sx + origin_side[0]
            # models/sinnerf.py:300-302: white where the warped patch is empty
            lit = warp_patch.sum(0, keepdim=True) > 0
            side_rgb = torch.where(lit, warp_patch, torch.ones_like(warp_patch))
            n = self.ph * self.pw
            return {"rays": self.all_rays[pick], "rgbs": self.all_rgbs[pick], "depth": self.all_depth[pick],
                    "rays_full": rays_full.reshape(n, 8), "rgbs_full": rgbs_full.reshape(n, 3), "depth_gt": depth_gt.reshape(n, 1),
                    "rays_side": rays_side.reshape(n, 8), "real_patch": real_patch[None],
                    "warp_patch": warp_patch, "warp_patch_depth": warp_patch_depth.reshape(self.ph, self.pw),
                    "rays_proj": full["rays"][at] * landed[:, None], "depth_proj": (full["depth"].reshape(-1)[at] * landed)[:, None],
                    "side_coord": torch.stack([rows, cols]) if self.ph == self.pw else (rows, cols),
                    "side_rgb": side_rgb.permute(1, 2, 0).reshape(n, 3),
                    "n_landed": n_landed, "n_valid_real": self.n_valid_real, "n_valid_side": n_valid_side,
                    "origin_real": origin_real, "origin_side": origin_side, "angles": angles, "c2w_side": full["c2w"]}
