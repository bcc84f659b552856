"""NumPy restatement of the slicing and gathering of one training sample of the one-image datasets (the train branch of ``__getitem__``,
``datasets/blender_ray_patch_1image_rot3d.py:443-528``), of the map of window origins with content (include/sinnerf_hip.h:
sn_valid_windows) and of the window gather (sn_gather_windows).  The fixture (tests/golden/sampler.npz, tools/gen_golden_sampler.py) holds
it to the unmodified reference in tests/test_sampler_cpu.py.

The reference's ``ll`` indexes rows with stride ``sW`` and ``up`` columns with stride ``sH`` (``rot3d:456-457``); in pixel coordinates
(x = column) the window is ``(x0, y0, stride_x, stride_y, pw, ph) = (up, ll, sH, sW, ps, ps)``."""
import numpy as np

from tests import warp_oracle as WO


def reference_counts(H, W, sx, sy, pw, ph):
    """(nx, ny) of ``np.random.randint(0, w - (ps - 1) * sW - 1)`` (rot3d:452-455): one candidate fewer per axis than would fit"""
    return W - (pw - 1) * sx - 1, H - (ph - 1) * sy - 1


def window(a, x0, y0, sx, sy, pw, ph):
    """``a[ll:ll + (ps - 1) sW + 1:sW, up:up + (ps - 1) sH + 1:sH]`` (rot3d:456-457, :491-497, :523-528) of an (H, W[, C]) array"""
    return a[y0:y0 + (ph - 1) * sy + 1:sy, x0:x0 + (pw - 1) * sx + 1:sx]


def clamp_origin(x0, y0, H, W, sx, sy, pw, ph):
    """the clamp of sn_gather_windows: into [0, W - (pw - 1) sx) x [0, H - (ph - 1) sy)"""
    return int(min(max(x0, 0), W - 1 - (pw - 1) * sx)), int(min(max(y0, 0), H - 1 - (ph - 1) * sy))


def gather(a, x0, y0, sx, sy, pw, ph, planar=False):
    """sn_gather_windows on one (H, W[, C]) source: (ph, pw, C), or (C, ph, pw) when planar; the origin clamped"""
    a = a if a.ndim == 3 else a[..., None]
    x0, y0 = clamp_origin(x0, y0, a.shape[0], a.shape[1], sx, sy, pw, ph)
    out = window(a, x0, y0, sx, sy, pw, ph)
    return np.ascontiguousarray(out.transpose(2, 0, 1) if planar else out)


def valid_windows(mask, sx, sy, pw, ph, nx, ny):
    """valid (ny, nx) uint8: any set pixel in the window at (x0, y0) -- rows first, then columns"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    assert 0 < nx <= W - (pw - 1) * sx and 0 < ny <= H - (ph - 1) * sy
    rows = np.zeros((H, nx), bool)
    for i in range(pw):
        rows |= m[:, i * sx:i * sx + nx]
    valid = np.zeros((ny, nx), bool)
    for j in range(ph):
        valid |= rows[j * sy:j * sy + ny]
    return valid.astype(np.uint8)


def valid_windows_brute(mask, sx, sy, pw, ph, nx, ny):
    m = np.asarray(mask) != 0
    valid = np.zeros((ny, nx), np.uint8)
    for y0 in range(ny):
        for x0 in range(nx):
            valid[y0, x0] = any(m[y0 + j * sy, x0 + i * sx] for j in range(ph) for i in range(pw))
    return valid


def kth_valid(valid, u):
    """(x0, y0) of the floor(u N)-th valid origin in raster order (sn_select_landed over the map); (0, 0) when there is none; and N"""
    idx, N = WO.select_landed(valid, np.asarray([u], np.float32))
    i = max(int(idx[0]), 0)
    return (i % valid.shape[1], i // valid.shape[1]), N


def sample(tables, full, draws, sx, sy, pw, ph, mirror_quirk=True):
    """The sample under the REFERENCE's keys and shapes (rot3d:503-528), from

    tables: ``all_rays`` (H W, 8), ``rgb`` (H, W, 3), ``depth`` (H, W) of the reference view;
    full:   ``out`` (H, W, 3), ``depth`` (H, W), ``rays`` (H W, 8) of the unseen view (forward_warp and get_rays of the drawn pose);
    draws:  ``origin_real``, ``origin_side`` as (x0, y0) = (up, ll); ``ray_idx`` (:465), ``ray_idx2`` (:466).

    ``mirror_quirk``: the reference-view patch takes the UNSEEN view's origin (:523-528 reuse the ``ll, up`` of :487-490)."""
    rgb, depth, all_rays = tables["rgb"], tables["depth"], tables["all_rays"]
    H, W = depth.shape
    all_rgbs, all_depth = rgb.reshape(-1, 3), depth.reshape(-1, 1)                    # rot3d:338-345
    nonwhite = np.flatnonzero(all_rgbs.sum(-1) != 3)                                  # :347-351: the rows of the nonzero_* tables
    pick = np.r_[nonwhite[np.asarray(draws["ray_idx2"], np.int64)], np.asarray(draws["ray_idx"], np.int64)]      # :503-505
    win = (sx, sy, pw, ph)
    xr, yr = clamp_origin(*draws["origin_real"], H, W, *win)
    xs, ys = clamp_origin(*draws["origin_side"], H, W, *win)
    xq, yq = (xs, ys) if mirror_quirk else (xr, yr)
    n = ph * pw
    return {"rays": all_rays[pick], "rgbs": all_rgbs[pick], "depth": all_depth[pick], "pick": pick,
            "real_patch": gather(rgb, xr, yr, *win, planar=True),                                                 # :456-457 (3, ps, ps)
            "rays_full": gather(full["rays"].reshape(H, W, 8), xs, ys, *win).reshape(n, 8),                      # :496-498 fake_patch
            "warp_patch": gather(full["out"], xs, ys, *win, planar=True),                                         # :494-495
            "warp_patch_depth": gather(full["depth"], xs, ys, *win).reshape(ph, pw),                              # :491-492
            "side_coord": np.stack([np.arange(ph) * sy + ys, np.arange(pw) * sx + xs]) if ph == pw
            else (np.arange(ph) * sy + ys, np.arange(pw) * sx + xs),                                              # :515
            "depth_ray": gather(all_rays.reshape(H, W, 8), xq, yq, *win).reshape(n, 8),                           # :523-524
            "depth_gt": gather(depth, xq, yq, *win).reshape(n, 1),                                                # :525-526
            "depth_ray_rgb": gather(rgb, xq, yq, *win).reshape(n, 3)}                                             # :527-528


def projected(full, u_proj):
    """``rays_proj`` (m, 8), ``depth_proj`` (m, 1), ``n_landed``: drawn among the landed pixels of the unseen view (its ``mask``), zero rows
    when nothing landed -- warp.unseen_view_batch's rule"""
    idx, N = WO.select_landed(full["mask"], np.asarray(u_proj, np.float32))
    ok = idx >= 0
    at = np.maximum(idx, 0)
    return full["rays"][at] * ok[:, None], (full["depth"].reshape(-1)[at] * ok)[:, None], N


def to_system(s, full=None, u_proj=None):
    """the keys and shapes of ``OneImageSampler.draw`` from a reference-keyed sample (the table of its docstring)"""
    wp = s["warp_patch"]
    lit = wp.sum(0, keepdims=True) > 0                                                 # models/sinnerf.py:300-302
    out = {"rays": s["rays"], "rgbs": s["rgbs"], "depth": s["depth"], "rays_full": s["depth_ray"], "rgbs_full": s["depth_ray_rgb"],
           "depth_gt": s["depth_gt"], "rays_side": s["rays_full"], "real_patch": s["real_patch"][None], "warp_patch": wp,
           "warp_patch_depth": s["warp_patch_depth"], "side_coord": s["side_coord"],
           "side_rgb": np.where(lit, wp, np.float32(1.0)).transpose(1, 2, 0).reshape(-1, 3)}
    if full is not None:
        out["rays_proj"], out["depth_proj"], out["n_landed"] = projected(full, u_proj)
    return out
