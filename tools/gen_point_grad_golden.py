#!/usr/bin/env python3
"""Golden DENSITY gradients from the UNMODIFIED reference (run in the build container only, like tools/gen_ray_grad_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_point_grad_golden.py

300 points (no multiple of 128 or 256) on lego rays at depths z in [2, 6] go through the reference's ``Embedding(3, 10)`` and
``NeRF(..., sigma_only=True)`` as an fp32 leaf that requires grad; torch autograd gives d(sum sigma_raw)/d(points), which is the
per-point gradient because the points are independent.  Stored per case (``tests/golden/grad_points_*.npz``):

    points (300, 3) fp32, sigma (300, 1)      the positions and the reference's fp32 raw sigma
    g32, g64                                  the fp32 autograd result / the same run with model and points cast to float64
    e_p (300)                                 ||g32_p - g64_p|| / (||g64_p|| + 1e-3 max_p ||g64_p||)  (the per-row quantity of
                                              ray_grad_oracle.median_ray_err): the reference's own fp32-vs-fp64 disagreement
    spread_median, spread_max, spread_share   median and maximum of e_p, share of points with e_p > 1e-3
    meta_weights, meta_seed, meta_draw        "init" (oracle_np.init_params(seed, teacher=True)) or "trained_student" (fine model);
                                              the RandomState seed that drew the points

A point whose ReLU mask flips between fp32 and float64 lands far above 1e-3; the generator ASSERTS that the reference alone leaves at
most 0.5 % of the points there and otherwise redraws the points with the next seed, so the tests' cap on excluded points is room for
the implementation under test and not for the fixture.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as G                                 # noqa: E402  (importing it runs nothing)
from oracle import oracle_np as O                                  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
N_POINTS = 300
MAX_SHARE = 0.005


def draw_points(seed):
    lego = O.lego_rays(400, 400, seed=0)
    r = np.random.RandomState(seed)
    rays = lego[r.choice(lego.shape[0], N_POINTS, replace=False)]
    z = r.uniform(2, 6, (N_POINTS, 1)).astype(np.float32)
    return np.ascontiguousarray(O._points(rays, z).reshape(-1, 3).astype(np.float32))


def run(model, points, dtype):
    p = torch.from_numpy(points.copy()).to(dtype).requires_grad_(True)
    sigma = model(G.Embedding(3, 10)(p), sigma_only=True)
    sigma.sum().backward()
    return sigma.detach().numpy(), p.grad.numpy()


def spread(g32, g64):
    g32, g64 = g32.astype(np.float64), g64.astype(np.float64)
    nr = np.linalg.norm(g64, axis=1)
    return np.linalg.norm(g32 - g64, axis=1) / (nr + 1e-3 * nr.max())


def case(name, seed, weights, first_draw):
    model, _ = G.ref_model(seed, True)
    for draw in range(first_draw, first_draw + 16):
        points = draw_points(draw)
        sigma, g32 = run(model.float(), points, torch.float32)
        _, g64 = run(model.double(), points, torch.float64)
        e_p = spread(g32, g64)
        share = float((e_p > 1e-3).mean())
        print(f"{name}: draw {draw}  e_p median {np.median(e_p):.2e} max {e_p.max():.2e} share > 1e-3 {share:.4f}")
        if share <= MAX_SHARE:
            break
    assert share <= MAX_SHARE, (name, share)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), points=points, sigma=sigma.astype(np.float32), g32=g32, g64=g64, e_p=e_p,
                        spread_median=np.asarray(np.median(e_p)), spread_max=np.asarray(e_p.max()), spread_share=np.asarray(share),
                        meta_weights=np.asarray(weights), meta_seed=np.asarray(seed if isinstance(seed, int) else -1),
                        meta_draw=np.asarray(draw))


def main():
    case("grad_points_init", 3, "init", 41)
    case("grad_points_trained", "trained:fine", "trained_student", 43)


if __name__ == "__main__":
    main()
