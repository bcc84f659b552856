#!/usr/bin/env python3
"""Golden rays and pose gradients of the reference's llff (NDC) and dtu cameras, from the UNMODIFIED reference (run in the build
container only, like oracle/gen_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_cameras.py

``datasets/ray_utils.py`` is imported from the reference as it is (it needs nothing but torch).  ``datasets/dtu_proj.py`` cannot
be imported without cv2, so ``get_ray_directions_dtu`` alone is compiled from its own function node in the mounted file (ast) at
generation time; nothing of it is re-typed here.

Two cases go into ``tests/golden/rays_cameras.npz``, every key prefixed ``llff_`` / ``dtu_``:

    H, W, focal, center (dtu), c2w, near, far, ndc_near (llff)     the inputs
    rays32, rays64       (H*W, 8) [o, d, near, far] by the reference's functions in fp32 / by the same functions in fp64
    e_ref                max |rays32 - rays64|: the reference's own fp32 error, the yardstick of the forward tests
    world32 (llff)       the fp32 world-space rays that went into get_ndc_rays
    g                    (H*W, 8) fixed upstream gradient, RandomState(seed); L = sum(rays * g), columns 6:8 do not reach c2w
    g_c2w64              fp64 autograd dL/dc2w
    err32_c2w            ||fp32 autograd - g_c2w64|| / ||g_c2w64||: the reference's own fp32 error of that gradient
    g_world64 (llff)     (H*W, 6) fp64 dL/d(rays_o, rays_d) of get_ndc_rays alone at world32, L = sum(ndc rays * g[:, :6])
    err32_world (llff)   the fp32 autograd error of that, norm-wise as above
"""
import ast
import functools
import importlib.util
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SINNERF_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "rays_cameras.npz")

spec = importlib.util.spec_from_file_location("ref_ray_utils", os.path.join(REF, "datasets", "ray_utils.py"))
RU = importlib.util.module_from_spec(spec)
spec.loader.exec_module(RU)


def ref_dtu_directions():
    """get_ray_directions_dtu compiled from the reference file, in a namespace that sees the reference's ray_utils (its star import)"""
    path = os.path.join(REF, "datasets", "dtu_proj.py")
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_ray_directions_dtu")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["get_ray_directions_dtu"], ns


DTU_DIRS, DTU_NS = ref_dtu_directions()


class Meshgrid:
    """the reference's create_meshgrid with its dtype argument set, where the reference's callers leave the fp32 default"""

    def __init__(self, dtype):
        self.fn = functools.partial(RU.create_meshgrid, dtype=dtype)

    def __enter__(self):
        self.saved = RU.create_meshgrid
        RU.create_meshgrid = DTU_NS["create_meshgrid"] = self.fn

    def __exit__(self, *exc):
        RU.create_meshgrid = DTU_NS["create_meshgrid"] = self.saved


def rays_of(case, dtype, c2w):
    """the dataset's chain on the reference's own functions -> (rays_o, rays_d) and, for llff, the world rays before NDC"""
    H, W = case["H"], case["W"]
    with Meshgrid(dtype):
        if case["kind"] == "llff":
            directions = RU.get_ray_directions(H, W, case["focal"])
        else:
            directions = DTU_DIRS(H, W, case["focal"], case["center"])
    assert directions.dtype == dtype
    o, d = RU.get_rays(directions, c2w)
    world = (o, d)
    if case["kind"] == "llff":
        o, d = RU.get_ndc_rays(H, W, case["focal"], case["ndc_near"], o, d)
    return o, d, world


def norm_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run_case(case, seed):
    H, W = case["H"], case["W"]
    n = H * W
    g = np.random.RandomState(seed).standard_normal((n, 8)).astype(np.float32)
    out, res = {}, {}
    for dtype in (torch.float32, torch.float64):
        c2w = torch.from_numpy(case["c2w"]).to(dtype).requires_grad_(True)
        o, d, world = rays_of(case, dtype, c2w)
        nf = torch.tensor([case["near"], case["far"]], dtype=dtype).expand(n, 2)
        rays = torch.cat([o, d, nf], 1)
        (rays * torch.from_numpy(g).to(dtype)).sum().backward()
        res[dtype] = (rays.detach().numpy(), c2w.grad.numpy(), torch.cat(world, 1).detach().numpy())
    rays32, gc32, world32 = res[torch.float32]
    rays64, gc64, _ = res[torch.float64]
    out.update(H=H, W=W, focal=np.asarray(case["focal"], np.float64), c2w=case["c2w"], near=case["near"], far=case["far"],
               rays32=rays32, rays64=rays64, e_ref=np.abs(rays32.astype(np.float64) - rays64).max(), g=g, g_c2w64=gc64,
               err32_c2w=norm_err(gc32, gc64))
    if case["kind"] == "dtu":
        out["center"] = np.asarray(case["center"], np.float64)
    else:
        out.update(ndc_near=case["ndc_near"], world32=world32)
        gw = {}
        for dtype in (torch.float32, torch.float64):                    # get_ndc_rays alone, at the fp32 world rays
            wo = torch.from_numpy(world32[:, 0:3].copy()).to(dtype).requires_grad_(True)
            wd = torch.from_numpy(world32[:, 3:6].copy()).to(dtype).requires_grad_(True)
            o, d = RU.get_ndc_rays(H, W, case["focal"], case["ndc_near"], wo, wd)
            (torch.cat([o, d], 1) * torch.from_numpy(g[:, :6]).to(dtype)).sum().backward()
            gw[dtype] = torch.cat([wo.grad, wd.grad], 1).numpy()
        out.update(g_world64=gw[torch.float64], err32_world=norm_err(gw[torch.float32], gw[torch.float64]))
    print(f"{case['kind']}: {n} rays, max |rays| {np.abs(rays64[:, :6]).max():.3f}, e_ref {out['e_ref']:.3e}, "
          f"err32_c2w {out['err32_c2w']:.3e}" + (f", err32_world {out['err32_world']:.3e}" if "err32_world" in out else ""))
    return {f"{case['kind']}_{k}": np.asarray(v) for k, v in out.items()}


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def main():
    # llff: a forward-facing camera near the origin looking down -z, tilted about all three axes (d_z < 0 for every pixel)
    llff = dict(kind="llff", H=29, W=37, focal=41.5, ndc_near=1.0, near=0.0, far=1.0,
                c2w=np.concatenate([rotation(0.12, -0.17, 0.08), [[0.13], [-0.21], [0.37]]], 1).astype(np.float32))
    # dtu: OpenCV axes (x right, y down, z forward), two focal lengths, an off-centre principal point
    dtu = dict(kind="dtu", H=23, W=31, focal=(38.0, 36.5), center=(14.2, 12.7), near=0.5, far=3.5,
               c2w=np.concatenate([rotation(2.3, 0.4, -0.9), [[0.9], [-1.4], [1.1]]], 1).astype(np.float32))
    arrays = {}
    arrays.update(run_case(llff, 101))
    arrays.update(run_case(dtu, 102))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
