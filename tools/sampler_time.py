#!/usr/bin/env python3
"""What drawing the batch on the device costs next to the training step it feeds, on one MI355X.

    python tools/sampler_time.py [--steps 40] [--warmup 5] [--out profiles/sampler_time.txt]

The lego patch shapes of bench.py's train_cfg2: a 400 x 400 frame, patch_size 64 with sW = sH = 5, num = 4096, 64 + 64 samples; the scene
is a shaded sphere with depth on a white, zero-depth background.  Two figures per compute dtype (bf16, fp32):

* ``draw()`` alone: the time between two device events around one call, median of --steps calls (eager: it includes the launch gaps of
  its ~60 small launches), and the same draw replayed from a captured graph;
* one step between two device synchronises (host clock), median of --steps steps after --warmup: ``train_step_sampled(sampler,
  graph=True)`` -- the draw inside the captured region -- against ``train_step(batch, graph=True)`` fed ONE prebuilt batch of the same
  shapes and keys (the step as it was before the sampler: the batch arrives from elsewhere), the two alternating step by step.

The last line is the record as JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinnerf_amd.sampler import OneImageSampler       # noqa: E402
from sinnerf_amd.system import SinNeRFSystem          # noqa: E402

H = W = 400
PS, STRIDE, NUM = 64, 5, 4096


def scene():
    """a sphere of radius 1 at the origin seen from z = 4 (pinhole, the blender layout), shaded, over white at depth 0"""
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = (x - W / 2) / focal, (y - H / 2) / focal
    a = dx * dx + dy * dy + 1.0
    disc = 64.0 - 4 * a * 15.0
    hit = disc > 0
    z = np.where(hit, (8.0 - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
    shade = np.stack([0.5 + 0.4 * np.sin(0.07 * x), 0.5 + 0.4 * np.cos(0.05 * y), 0.7 + 0 * x], -1)
    rgb = np.where(hit[..., None], shade, 1.0)
    c2w = np.eye(4, dtype=np.float32)
    c2w[2, 3] = 4.0
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], np.float32)
    return rgb.astype(np.float32), z.astype(np.float32), c2w, K, float(focal)


def quantiles(samples):
    s = np.sort(np.asarray(samples))
    return {"median": float(np.median(s)), "p10": float(s[int(0.1 * (len(s) - 1))]), "p90": float(s[int(0.9 * (len(s) - 1))])}


def time_draw(sampler, steps, warmup):
    """ms per draw between device events: eager, and replayed from a graph"""
    for _ in range(warmup):
        sampler.draw()
    torch.cuda.synchronize()
    eager = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sampler.draw()
        e1.record()
        torch.cuda.synchronize()
        eager.append(e0.elapsed_time(e1))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sampler.draw()
    replay = []
    for _ in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        replay.append(e0.elapsed_time(e1))
    return quantiles(eager), quantiles(replay[warmup:])


def time_steps(dtype, sampler, steps, warmup):
    """ms per synchronised step: the sampled step and the prebuilt-batch step, alternating, on two systems of the same seed"""
    dev = sampler.device
    systems = []
    for _ in range(2):
        torch.manual_seed(7)
        s = SinNeRFSystem(N_importance=64, compute_dtype=dtype, perturb=1.0, noise_std=1.0, white_back=True, depth_weight=1.0).to(dev)
        s.configure_optimizers()
        systems.append(s)
    sampled, prebuilt = systems
    reads = ("rays", "rgbs", "depth", "rays_full", "rgbs_full", "depth_gt", "rays_side", "real_patch", "warp_patch", "warp_patch_depth",
             "rays_proj", "depth_proj", "side_rgb", "side_coord")       # what a DataLoader would deliver: no bookkeeping tensors to copy
    batch = {k: v for k, v in sampler.draw().items() if k in reads}
    run = {"sampled": lambda: sampled.train_step_sampled(sampler, graph=True), "prebuilt": lambda: prebuilt.train_step(batch, graph=True)}
    times = {k: [] for k in run}
    for i in range(warmup + steps):
        for k, fn in run.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
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
    assert torch.cuda.is_available(), "tools/sampler_time.py measures on the MI355X; there is no CPU path"
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)
    rgb, depth, c2w, K, focal = scene()
    torch.manual_seed(0)
    sampler = OneImageSampler(t(rgb), t(depth), t(c2w), t(K), focal=focal, near=2.0, far=6.0, patch_size=PS, sW=STRIDE, sH=STRIDE, num=NUM,
                              eps=1e-9)
    lines = [f"# tools/sampler_time.py --steps {args.steps} --warmup {args.warmup} on one MI355X, world size 1: {H} x {W} frame, patch "
             f"{PS} x {PS} stride {STRIDE}, num {NUM}, 64 + 64 samples; medians (p10, p90)"]
    eager, replay = time_draw(sampler, args.steps, args.warmup)
    lines.append(f"draw() between device events: eager {eager['median']:.3f} ms ({eager['p10']:.3f}, {eager['p90']:.3f}); replayed from a "
                 f"graph {replay['median']:.3f} ms ({replay['p10']:.3f}, {replay['p90']:.3f})")
    rec = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "draw_eager_ms": eager, "draw_graph_ms": replay,
           "step_ms": {}}
    for dtype in ("bf16", "fp32"):
        r = time_steps(dtype, sampler, args.steps, args.warmup)
        rec["step_ms"][dtype] = r
        s, p = r["sampled"], r["prebuilt"]
        lines.append(f"{dtype:5s} step, graph: drawn inside {s['median']:.3f} ms ({s['p10']:.3f}, {s['p90']:.3f})   prebuilt batch "
                     f"{p['median']:.3f} ms ({p['p10']:.3f}, {p['p90']:.3f})   difference {s['median'] - p['median']:+.3f} ms = "
                     f"{100 * (s['median'] - p['median']) / p['median']:+.1f} %; the replayed draw alone is "
                     f"{100 * replay['median'] / s['median']:.1f} % of the sampled step")
    lines.append(json.dumps(rec))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
