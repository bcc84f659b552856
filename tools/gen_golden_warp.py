#!/usr/bin/env python3
"""Golden forward warps of the reference's four dataset variants, from the UNMODIFIED reference (run in the build container only, like
tools/gen_golden_cameras.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_warp.py

The dataset modules need cv2 and torchvision and cannot be imported whole: the function nodes ``project_with_depth``, ``forward_warp``,
``convert``, ``rotate_3d`` with its ``rot_*`` helpers and ``warp_img_proj_numpy`` are compiled out of the mounted files (ast) at
generation time; nothing of them is re-typed here.  ``warp_img_proj_numpy`` keeps its projected coordinates to itself: it runs with an
``np`` that records the first argument of ``np.clip`` (the fp32 coordinates) and of ``np.zeros_like`` (depth_src).

The scene is a sphere in front of a background; the unseen pose is the reference pose rotated by (9, -14, 5) degrees.  The data image
has four channels: three colours and the source raster index + 1, so the reference's ``new`` names its winner (0 = nothing landed).

``tests/golden/warp.npz`` holds, per case prefix ``rot3d_ / proj_ / llff_ / dtu_``:

    H, W, mode, eps                     the frame, the collision rule (0 last / 1 nearest) and the eps of the variant's division
    data (H, W, 4), depth (H, W)        the inputs, fp32
    K, E_ref, E_src                     intrinsics and the 4x4 extrinsics given to forward_warp (rot3d, proj, llff)
    P_ref, P_src                        the 4x4 projection matrices [K E[:3]; 0 0 0 1] (dtu: what warp_img_proj_numpy was given)
    new (H, W, 4), new_depth (H, W)     the reference's outputs;  mask (proj) its depth_mask
    x_src, y_src, depth_src (H, W)      the reference's fp32 coordinates and depth
    e_xy, e_d                           max |fp32 - tests/warp_oracle.py fp64| of the coordinates over the source pixels that land inside
                                        the frame unclamped, and of depth_src over the same pixels
"""
import ast
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import warp_oracle as WO                                    # noqa: E402

REF = os.environ.get("SINNERF_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "warp.npz")
HELPERS = ("rot_phi", "rot_theta", "rot_z", "rotate_3d", "convert", "project_with_depth", "forward_warp", "warp_img_proj_numpy")


def ref_functions(filename, np_module=np, torch_module=torch):
    """the reference's warp functions compiled from their own nodes in the mounted file"""
    path = os.path.join(REF, "datasets", filename)
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in HELPERS]
    ns = {"torch": torch_module, "np": np_module}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return types.SimpleNamespace(**{n.name: ns[n.name] for n in nodes})


class NpSpy:
    """numpy, with the first arguments of clip and zeros_like recorded"""

    def __init__(self):
        self.clipped, self.zeros_like_of = [], []

    def __getattr__(self, name):
        return getattr(np, name)

    def clip(self, a, *args, **kw):
        self.clipped.append(np.array(a))
        return np.clip(a, *args, **kw)

    def zeros_like(self, a, *args, **kw):
        self.zeros_like_of.append(np.array(a))
        return np.zeros_like(a, *args, **kw)


class TorchOnArrays:
    """torch, with ``ones_like`` / ``zeros_like`` that take an ndarray: blender_ray_patch_1image_proj.py:135-136 hands them
    ``new_depth = np.zeros_like(tensor)``, which is an ndarray with today's numpy and makes those two lines raise.  The images stay NumPy
    arrays, so duplicates are resolved by NumPy's fancy-index assignment as in the rot3d file."""

    def __getattr__(self, name):
        return getattr(torch, name)

    def ones_like(self, a, *args, **kw):
        return torch.ones_like(a, *args, **kw) if torch.is_tensor(a) else np.ones_like(a)

    def zeros_like(self, a, *args, **kw):
        return torch.zeros_like(a, *args, **kw) if torch.is_tensor(a) else np.zeros_like(a)


def scene(H, W, focal, background):
    """depth along the camera axis of a sphere of radius 1 at distance 4 (pinhole at the reference pose), over `background`"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = (x - (W - 1) / 2) / focal, (y - (H - 1) / 2) / focal
    a, b = dx * dx + dy * dy + 1.0, -8.0
    disc = b * b - 4 * a * 15.0
    z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), background)
    rgb = np.stack([0.5 + 0.5 * np.sin(0.37 * x), 0.5 + 0.5 * np.cos(0.23 * y), np.where(disc > 0, 0.9, 0.2)], -1)
    index = (np.arange(H * W).reshape(H, W, 1) + 1).astype(np.float64)
    return np.concatenate([rgb, index], -1).astype(np.float32), z.astype(np.float32)


def ref_c2w():
    """a camera 4 units up the z axis looking at the origin (the blender layout), float32 as the datasets hold it"""
    c2w = np.eye(4, dtype=np.float32)
    c2w[2, 3] = 4.0
    return torch.from_numpy(c2w)


def errors(x32, y32, d32, res, H, W):
    xs, ys = res["xs"], res["ys"]
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    e_xy = max(np.abs(x32.reshape(-1).astype(np.float64) - xs)[inside].max(), np.abs(y32.reshape(-1).astype(np.float64) - ys)[inside].max())
    e_d = np.abs(d32.reshape(-1).astype(np.float64) - res["p2"])[inside].max()
    return float(e_xy), float(e_d), int(inside.sum())


def torch_case(name, filename, H, W, focal, background, mode, eps):
    R = ref_functions(filename, torch_module=TorchOnArrays() if name == "proj" else torch)
    data, depth = scene(H, W, focal, background)
    if name == "llff":
        K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]])
    else:
        K = np.array([[focal, 0, (W - 1) / 2], [0, focal, (H - 1) / 2], [0, 0, 1]])     # the reference's (n - 1) / 2 centre
    K = torch.from_numpy(K).float()
    c2w_ref = ref_c2w()
    rotate_3d = ref_functions("blender_ray_patch_1image_rot3d.py").rotate_3d          # the llff file has none
    c2w_src = torch.FloatTensor(rotate_3d(c2w_ref, 9.0, -14.0, 5.0))[:3, :4]
    E_ref = torch.FloatTensor(R.convert(c2w_ref.numpy()))
    E_src = torch.FloatTensor(R.convert(c2w_src.numpy()))
    args = (torch.from_numpy(depth).unsqueeze(0), K, E_ref, K, E_src)
    x32, y32, d32 = R.project_with_depth(*args)
    out = R.forward_warp(torch.from_numpy(data).permute(2, 0, 1).unsqueeze(0), *args)
    case = dict(H=H, W=W, mode=mode, eps=eps, data=data, depth=depth, K=K.numpy(), E_ref=E_ref.numpy(), E_src=E_src.numpy(),
                P_ref=WO.proj_matrix(K.numpy(), E_ref.numpy()), P_src=WO.proj_matrix(K.numpy(), E_src.numpy()),
                new=np.asarray(out[0], np.float32), new_depth=np.asarray(out[1], np.float32).reshape(H, W),
                x_src=x32.numpy().reshape(H, W), y_src=y32.numpy().reshape(H, W), depth_src=d32.numpy().reshape(H, W))
    if len(out) > 2:
        case["mask"] = np.asarray(out[2], np.float32).reshape(H, W) != 0
    return case


def dtu_case(H, W, focal):
    spy = NpSpy()
    R = ref_functions("dtu_proj.py", spy)
    data, depth = scene(H, W, focal, 6.0)
    K = np.array([[focal, 0, 19.3], [0, focal * 0.97, 16.4], [0, 0, 1]])
    blender = ref_functions("blender_ray_patch_1image_rot3d.py")
    c2w_ref = np.eye(4)
    c2w_ref[:3, :3] = np.diag([1.0, -1.0, -1.0])                          # OpenCV axes: looking down -z of the world from z = 4
    c2w_ref[2, 3] = 4.0
    c2w_src = blender.rotate_3d(torch.from_numpy(c2w_ref).float(), 9.0, -14.0, 5.0).numpy().astype(np.float64)
    P_ref = WO.proj_matrix(K, R.convert(c2w_ref))
    P_src = WO.proj_matrix(K, R.convert(c2w_src))
    new, new_depth = R.warp_img_proj_numpy(data, depth, P_ref, P_src)
    x32, y32 = spy.clipped[0], spy.clipped[1]                              # dtu_proj.py:261-262: X[0] against width, X[1] against height
    d32 = spy.zeros_like_of[1]
    return dict(H=H, W=W, mode=1, eps=0.0, data=data, depth=depth, P_ref=P_ref, P_src=P_src, new=new, new_depth=new_depth,
                x_src=x32.reshape(H, W), y_src=y32.reshape(H, W), depth_src=d32.reshape(H, W))


def main():
    cases = {
        "rot3d": torch_case("rot3d", "blender_ray_patch_1image_rot3d.py", 48, 48, 66.0, 0.0, 0, 1e-9),
        "proj": torch_case("proj", "blender_ray_patch_1image_proj.py", 48, 48, 66.0, 0.0, 0, 0.0),
        "llff": torch_case("llff", "llff_ray_patch_1image_proj.py", 40, 56, 60.0, 6.0, 1, 1e-9),
        "dtu": dtu_case(32, 40, 44.0),
    }
    arrays = {}
    for name, c in cases.items():
        H, W = c["H"], c["W"]
        res = WO.forward_warp(c["data"], c["depth"], c["P_ref"], c["P_src"], c["eps"], c["mode"])
        c["e_xy"], c["e_d"], inside = errors(c["x_src"], c["y_src"], c["depth_src"], res, H, W)
        ref_win = c["new"].reshape(H * W, 4)[:, 3].astype(np.int64) - 1
        print(f"{name}: {H}x{W}, {inside} of {H * W} land inside, e_xy {c['e_xy']:.3e}, e_d {c['e_d']:.3e}, landed "
              f"{(ref_win >= 0).sum()}, oracle winners differing {(ref_win != res['winner']).sum()}")
        arrays.update({f"{name}_{k}": np.asarray(v) for k, v in c.items()})
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
