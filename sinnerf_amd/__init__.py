"""sinnerf_amd -- MI355X-native (gfx950) volume-rendering hot path behind SinNeRF's own Python surface.

Drop-in names (reference: VITA-Group/SinNeRF):
  sinnerf_amd.rendering.render_rays / sample_pdf   <->  models/rendering.py
  sinnerf_amd.nerf.Embedding / NeRF                <->  models/nerf.py
"""
from .nerf import Embedding, NeRF                      # noqa: F401
from .rendering import eval_points, render_rays, sample_pdf   # noqa: F401
from .geometry import density_gradients, ray_density_gradients, render_normals   # noqa: F401
from .warp import (extrinsics_from_c2w, forward_warp, forward_warp_proj, rotate_3d, select_landed,   # noqa: F401
                   unseen_view_batch, unseen_view_full)
from .sampler import OneImageSampler, gather_windows, valid_windows   # noqa: F401
from .regularizers import distortion_loss, ray_entropy_loss, ray_regularizers   # noqa: F401
from .reprojection import reprojection_loss   # noqa: F401

__all__ = ["Embedding", "NeRF", "render_rays", "sample_pdf", "eval_points", "forward_warp", "forward_warp_proj",
           "extrinsics_from_c2w", "rotate_3d", "select_landed", "unseen_view_batch", "unseen_view_full", "OneImageSampler",
           "valid_windows", "gather_windows", "density_gradients", "ray_density_gradients",
           "render_normals", "ray_regularizers", "distortion_loss", "ray_entropy_loss", "reprojection_loss"]
