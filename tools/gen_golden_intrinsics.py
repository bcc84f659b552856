#!/usr/bin/env python3
"""Golden gradients with respect to the camera INTRINSICS (focal lengths, principal point) of the reference's three cameras, from
the UNMODIFIED reference (run in the build container only, like tools/gen_golden_cameras.py, whose loaders this script imports: the
reference's ``datasets/ray_utils.py`` as it is, ``get_ray_directions_dtu`` compiled from its own function node; nothing re-typed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_intrinsics.py

The reference's functions are ordinary torch ops: with ``focal`` (and, for dtu, ``center``) as leaf tensors they differentiate through
them.  Three cases go into ``tests/golden/rays_intrinsics.npz``, every key prefixed ``llff_`` / ``blender_`` / ``dtu_``; sizes and
poses are those of tests/golden/rays_cameras.npz:

    H, W, focal, center (dtu), c2w, near, far, ndc_near (llff)     the inputs; blender = the llff frame without NDC
    seeds                (K,) = 8 seeds; upstream k is g_k = RandomState(seed_k).standard_normal((H*W, 8)).astype(float32),
                         L_k = sum(rays * g_k) over the (H*W, 8) [o, d, near, far] rays
    G64                  (K, c) fp64 autograd dL_k/d(focal[, fy][, cx, cy]): c = 1 (llff, blender) or 4 (dtu: fx, fy, cx, cy)
    G32                  the same by the reference's fp32 autograd (float32)
    err32_focal          ||fp32 autograd - G64|| / ||G64|| (Frobenius, over the K rows) of the focal columns: the reference's own fp32
    err32_center (dtu)   error, the yardstick of the GPU tests; the same for the centre columns
    llff_ndc_G64         (K,) fp64 dL_k/dfocal of get_ndc_rays ALONE at the fp32 world rays (rays_cameras.npz llff_world32),
    llff_ndc_G32,        L_k = sum(ndc rays * g_k[:, :6]); the same in fp32, and the yardstick from the two
    llff_ndc_err32
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_cameras as C                                                        # noqa: E402  (loads the reference)

OUT = os.path.join(C.REPO, "tests", "golden", "rays_intrinsics.npz")
K = 8


def frob_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rays_of(case, dtype, focal, center):
    """the dataset's chain on the reference's own functions with tensor intrinsics -> (n, 8) rays"""
    H, W = case["H"], case["W"]
    c2w = torch.from_numpy(case["c2w"]).to(dtype)
    with C.Meshgrid(dtype):
        if case["kind"] == "dtu":
            directions = C.DTU_DIRS(H, W, focal, center)
        else:
            directions = C.RU.get_ray_directions(H, W, focal)
    assert directions.dtype == dtype
    o, d = C.RU.get_rays(directions, c2w)
    if case["kind"] == "llff":
        o, d = C.RU.get_ndc_rays(H, W, focal, case["ndc_near"], o, d)
    nf = torch.tensor([case["near"], case["far"]], dtype=dtype).expand(H * W, 2)
    return torch.cat([o, d, nf], 1)


def run_case(case, seeds):
    n = case["H"] * case["W"]
    dtu = case["kind"] == "dtu"
    G = {}
    for dtype in (torch.float32, torch.float64):
        rows = []
        for seed in seeds:
            g = torch.from_numpy(np.random.RandomState(seed).standard_normal((n, 8)).astype(np.float32)).to(dtype)
            focal = torch.tensor(case["focal"], dtype=dtype, requires_grad=True)
            center = torch.tensor(case["center"], dtype=dtype, requires_grad=True) if dtu else None
            (rays_of(case, dtype, focal, center) * g).sum().backward()
            rows.append(torch.cat([focal.grad.reshape(-1)] + ([center.grad] if dtu else [])).numpy())
        G[dtype] = np.stack(rows)
    G32, G64 = G[torch.float32], G[torch.float64]
    nf = 2 if dtu else 1
    out = dict(H=case["H"], W=case["W"], focal=np.asarray(case["focal"], np.float64), c2w=case["c2w"], near=case["near"], far=case["far"],
               seeds=np.asarray(seeds, np.int64), G64=G64, G32=G32, err32_focal=frob_err(G32[:, :nf], G64[:, :nf]))
    msg = f"{case['kind']}: {n} rays, K = {len(seeds)}, err32 focal {out['err32_focal']:.3e}"
    if dtu:
        out.update(center=np.asarray(case["center"], np.float64), err32_center=frob_err(G32[:, 2:], G64[:, 2:]))
        msg += f", centre {out['err32_center']:.3e}"
    if case["kind"] == "llff":
        out["ndc_near"] = case["ndc_near"]
        world32 = case["world32"]
        N = {}
        for dtype in (torch.float32, torch.float64):                    # get_ndc_rays alone, at the fp32 world rays
            rows = []
            for seed in seeds:
                g = torch.from_numpy(np.random.RandomState(seed).standard_normal((n, 8)).astype(np.float32)[:, :6].copy()).to(dtype)
                focal = torch.tensor(case["focal"], dtype=dtype, requires_grad=True)
                wo, wd = (torch.from_numpy(world32[:, a:a + 3].copy()).to(dtype) for a in (0, 3))
                o, d = C.RU.get_ndc_rays(case["H"], case["W"], focal, case["ndc_near"], wo, wd)
                (torch.cat([o, d], 1) * g).sum().backward()
                rows.append(focal.grad.item())
            N[dtype] = np.asarray(rows, np.float32 if dtype == torch.float32 else np.float64)
        out.update(ndc_G64=N[torch.float64], ndc_G32=N[torch.float32], ndc_err32=frob_err(N[torch.float32], N[torch.float64]))
        msg += f", get_ndc_rays alone {out['ndc_err32']:.3e}"
    print(msg)
    return {f"{case['kind']}_{k}": np.asarray(v) for k, v in out.items()}


def main():
    z = np.load(os.path.join(C.REPO, "tests", "golden", "rays_cameras.npz"))
    llff = dict(kind="llff", H=int(z["llff_H"]), W=int(z["llff_W"]), focal=float(z["llff_focal"]), ndc_near=float(z["llff_ndc_near"]),
                near=float(z["llff_near"]), far=float(z["llff_far"]), c2w=z["llff_c2w"], world32=z["llff_world32"])
    blender = dict(llff, kind="blender", near=2.0, far=6.0)
    dtu = dict(kind="dtu", H=int(z["dtu_H"]), W=int(z["dtu_W"]), focal=tuple(z["dtu_focal"]), center=tuple(z["dtu_center"]),
               near=float(z["dtu_near"]), far=float(z["dtu_far"]), c2w=z["dtu_c2w"])
    assert (llff["H"], llff["W"], llff["focal"]) == (29, 37, 41.5) and (dtu["H"], dtu["W"]) == (23, 31)
    arrays = {}
    arrays.update(run_case(llff, list(range(201, 201 + K))))
    arrays.update(run_case(blender, list(range(301, 301 + K))))
    arrays.update(run_case(dtu, list(range(401, 401 + K))))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
