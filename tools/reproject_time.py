#!/usr/bin/env python3
"""What the unseen-view reprojection loss costs, on one MI355X.

    python tools/reproject_time.py [--steps 40] [--warmup 5] [--out profiles/reprojection_time.txt]

* the call alone -- ``sn_reproject_loss`` with every output, both launches -- between two device events, eager and replayed from a
  captured graph, at the lego side patch: 4096 pixels x 3 channels over the 400 x 400 reference frame.  Beside it a torch-op formulation
  of the same loss (fp32 projection, two ``grid_sample`` calls for the image and the depth, one for the corner test, autograd backward)
  on the same inputs;
* one bf16 ``train_step_sampled(sampler, graph=True)`` step between two device synchronises (host clock), with the terms on
  (reproj_weight 0.1, freespace_weight 0.1) and off, the two alternating step by step.

Medians with (p10, p90) after warm-up.  The last line is the record as JSON."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinnerf_amd import _lib                          # noqa: E402
from sinnerf_amd.sampler import OneImageSampler       # noqa: E402
from sinnerf_amd.system import SinNeRFSystem          # noqa: E402
from ray_reg_time import between_events               # noqa: E402
from sampler_time import H, W, NUM, PS, STRIDE, quantiles, scene      # noqa: E402

OCC_TOL, CHARB_EPS, Z_MIN, OPACITY_THRESHOLD = 0.05, 1e-3, 1e-6, 0.5
W_PHOTO = W_FREE = 0.1


def inputs(sampler):
    """the unseen-view patch of one draw: its rays, the warped depth moved by up to +-10 % (4 where nothing landed) as the rendered
    depth, the warped colours as the rendered colours, opacities in [0.3, 1]"""
    dev = sampler.device
    g = torch.Generator(device=dev).manual_seed(1)
    b = sampler.draw()
    n = b["rays_side"].shape[0]
    d = b["warp_patch_depth"].reshape(-1)
    depth = torch.where(d > 0, d * (0.9 + 0.2 * torch.rand(n, generator=g, device=dev)), torch.full_like(d, 4.0)).contiguous()
    opacity = (0.3 + 0.7 * torch.rand(n, generator=g, device=dev)).contiguous()
    return b["rays_side"].contiguous(), depth, b["side_rgb"].contiguous(), opacity


def torch_formulation(rays, depth, rgb, opacity, image, ref_depth, P):
    """the same loss in torch ops, fp32; image (1, C, H, W), ref_depth (1, 1, H, W), P (4, 4) fp32"""
    fh, fw = ref_depth.shape[-2:]
    X = rays[:, 0:3] + depth[:, None] * rays[:, 3:6]
    q = X @ P[:3, :3].T + P[:3, 3]
    z = q[:, 2]
    u, v = q[:, 0] / z, q[:, 1] / z
    grid = torch.stack([2 * u / (fw - 1) - 1, 2 * v / (fh - 1) - 1], -1)[None, None]
    sample = lambda a: F.grid_sample(a, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0]
    D, c = sample(ref_depth)[0], sample(image).T
    corners = sample((ref_depth > 0).float())[0] > 0.999                    # every corner that carries weight is foreground
    G = ((depth > 0) & (z >= Z_MIN) & (opacity > OPACITY_THRESHOLD) & (u >= 0) & (u <= fw - 1) & (v >= 0) & (v <= fh - 1) & corners).detach()
    r = (z - D) / torch.where(G, D, torch.ones_like(D))
    V = (G & (r.abs() <= OCC_TOL)).detach()
    zero = torch.zeros_like(r)
    photo_i = torch.sqrt((rgb - c) ** 2 + CHARB_EPS ** 2).mean(-1)
    photo = torch.where(V, photo_i, zero).sum() / V.sum().clamp(min=1)
    free = torch.where(G, torch.relu(-r - OCC_TOL), zero).sum() / G.sum().clamp(min=1)
    return W_PHOTO * photo + W_FREE * free


def time_calls(sampler, steps, warmup):
    dev = sampler.device
    rays, depth, rgb, opacity = inputs(sampler)
    n, C = rgb.shape
    fh, fw = sampler.ref_depth.shape
    g_depth, g_rgb, per_pixel = torch.empty_like(depth), torch.empty_like(rgb), torch.empty((n, 2), device=dev)
    flags, out = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(6, device=dev)
    ws = torch.empty(_lib.lib.sn_reproject_loss_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def kernel():
        _lib.check(_lib.lib.sn_reproject_loss(_lib.ptr(rays), _lib.ptr(depth), _lib.ptr(rgb), _lib.ptr(opacity), n, C,
                                              _lib.ptr(sampler.ref_view), _lib.ptr(sampler.ref_depth), fh, fw, _lib.ptr(sampler.ref_proj),
                                              OCC_TOL, CHARB_EPS, Z_MIN, OPACITY_THRESHOLD, W_PHOTO, W_FREE, _lib.ptr(g_depth),
                                              _lib.ptr(g_rgb), _lib.ptr(per_pixel), _lib.ptr(flags), _lib.ptr(ws), _lib.ptr(out),
                                              _lib.stream_ptr()), "sn_reproject_loss")

    image = sampler.ref_view.permute(2, 0, 1)[None].contiguous()
    ref_depth, P = sampler.ref_depth[None, None].contiguous(), sampler.ref_proj.float()
    d_leaf, c_leaf = depth.clone().requires_grad_(True), rgb.clone().requires_grad_(True)

    def torch_ops():
        d_leaf.grad = c_leaf.grad = None
        torch_formulation(rays, d_leaf, c_leaf, opacity, image, ref_depth, P).backward()

    r = {"reproject_loss": between_events(kernel, steps, warmup), "torch_ops": between_events(torch_ops, steps, warmup)}
    kernel()
    total = torch_formulation(rays, depth, rgb, opacity, image, ref_depth, P)
    torch.cuda.synchronize()
    counts = {"n": n, "n_vis": int(out[3].item()), "n_geo": int(out[4].item()), "n_front": int(out[5].item()),
              "total_kernel": out[2].item(), "total_torch_fp32": total.item()}
    return r, counts


def time_steps(sampler, steps, warmup):
    """ms per synchronised bf16 step, the terms on and off, alternating, on two systems of the same seed"""
    dev = sampler.device
    systems = {}
    for name, hp in (("off", {}), ("on", dict(reproj_weight=W_PHOTO, freespace_weight=W_FREE))):
        torch.manual_seed(7)
        s = SinNeRFSystem(N_importance=64, compute_dtype="bf16", perturb=1.0, noise_std=1.0, white_back=True, depth_weight=1.0, **hp).to(dev)
        s.configure_optimizers()
        systems[name] = s
    times = {k: [] for k in systems}
    for i in range(warmup + steps):
        for k, s in systems.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = s.train_step_sampled(sampler, graph=True)
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(out["loss"]).item()
    return {k: quantiles(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/reproject_time.py measures on the MI355X; there is no CPU path"
    dev = torch.device("cuda:0")
    fmt = lambda q: f"{1e3 * q['median']:.1f} us ({1e3 * q['p10']:.1f}, {1e3 * q['p90']:.1f})"
    t = lambda a: torch.from_numpy(a).to(dev)
    rgb, depth, c2w, K, focal = scene()
    torch.manual_seed(0)
    sampler = OneImageSampler(t(rgb), t(depth), t(c2w), t(K), focal=focal, near=2.0, far=6.0, patch_size=PS, sW=STRIDE, sH=STRIDE, num=NUM,
                              eps=1e-9)
    lines = [f"# tools/reproject_time.py --steps {args.steps} --warmup {args.warmup} on one MI355X, world size 1; medians (p10, p90)"]
    rec = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup}
    r, counts = time_calls(sampler, args.steps, args.warmup)
    rec["calls_ms"], rec["inputs"] = r, counts
    lines.append(f"inputs: {counts['n']} pixels x 3 over {H} x {W}: {counts['n_geo']} geometrically valid, {counts['n_vis']} visible, "
                 f"{counts['n_front']} in front; total {counts['total_kernel']:.9g} (torch ops, fp32: {counts['total_torch_fp32']:.9g})")
    for name, q in r.items():
        lines.append(f"{counts['n']} x 3 {name:15s} between device events: eager {fmt(q['eager'])}; replayed from a graph {fmt(q['graph'])}")
    k, o = r["reproject_loss"]["graph"]["median"], r["torch_ops"]["graph"]["median"]
    lines.append(f"{counts['n']} x 3 replayed: torch ops / reproject_loss = {o / k:.1f}")
    r = time_steps(sampler, args.steps, args.warmup)
    rec["step_ms"] = r
    on, off = r["on"], r["off"]
    lines.append(f"bf16 train_step_sampled(graph=True), {H} x {W} frame, patch {PS} x {PS} stride {STRIDE}, num {NUM}, 64 + 64 samples: terms on "
                 f"{on['median']:.3f} ms ({on['p10']:.3f}, {on['p90']:.3f})   off {off['median']:.3f} ms ({off['p10']:.3f}, {off['p90']:.3f})   "
                 f"difference {on['median'] - off['median']:+.3f} ms = {100 * (on['median'] - off['median']) / off['median']:+.2f} %")
    lines.append(json.dumps(rec))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
