#!/usr/bin/env python3
"""What the ray regularisers cost, on one MI355X.

    python tools/ray_reg_time.py [--steps 40] [--warmup 5] [--out profiles/ray_regularizers_time.txt]

* the call alone -- ``sn_ray_regularizers`` with all outputs, both launches -- between two device events, eager and replayed from a
  captured graph, at the lego side patch (4096 rays x 128 samples) and at 4096 x 64.  Beside it at the same shapes:
  ``sn_composite_forward`` (the kernel whose layout it shares) and a torch-op formulation of the same loss (value and gradient through
  ``cumsum`` / ``cat``, autograd backward) on the same device;
* one bf16 ``train_step_sampled(sampler, graph=True)`` step between two device synchronises (host clock), with the terms on
  (distortion_weight 0.01, entropy_weight 0.001) and off, the two alternating step by step.

Medians with (p10, p90) after warm-up.  The last line is the record as JSON."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinnerf_amd import _lib                          # noqa: E402
from sinnerf_amd.sampler import OneImageSampler       # noqa: E402
from sinnerf_amd.system import SinNeRFSystem          # noqa: E402
from sampler_time import H, W, NUM, PS, STRIDE, quantiles, scene      # noqa: E402

N_RAYS = 4096


def inputs(S, dev):
    """weights from random alphas, sorted depths in [near, far], raw (rgb, sigma) for the compositor"""
    g = torch.Generator(device=dev).manual_seed(S)
    alpha = torch.rand((N_RAYS, S), generator=g, device=dev) ** 3
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha[:, :-1]], 1), 1)
    rays = torch.zeros((N_RAYS, 8), device=dev)
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn((N_RAYS, 3), generator=g, device=dev), dim=1)
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    z = torch.sort(2.0 + 4.0 * torch.rand((N_RAYS, S), generator=g, device=dev), 1)[0]
    raw = torch.rand((N_RAYS, S, 4), generator=g, device=dev)
    return (alpha * T).contiguous(), z.contiguous(), rays, raw


def torch_formulation(w, z, rays, w_dist, w_ent, thr):
    """the same loss in torch ops, O(S) through cumsum; the gradient by autograd"""
    near, far = rays[:, 6:7], rays[:, 7:8]
    s = (z - near) / (far - near)
    m = torch.cat([(s[:, :-1] + s[:, 1:]) / 2, s[:, -1:]], 1)
    d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, -1:])], 1)
    wm = w * m
    W_lt, M_lt = torch.cumsum(w, 1) - w, torch.cumsum(wm, 1) - wm
    W_gt, M_gt = w.sum(1, keepdim=True) - W_lt - w, wm.sum(1, keepdim=True) - M_lt - wm
    dist = (w * (m * (W_lt - W_gt) - (M_lt - M_gt))).sum(1) + (w * w * d).sum(1) / 3
    o = w.sum(1)
    p = w / (o + 1e-10)[:, None]
    ent = torch.where(o > thr, -(p * torch.log(p + 1e-10)).sum(1), torch.zeros_like(o))
    return w_dist * dist.mean() + w_ent * ent.mean()


def between_events(fn, steps, warmup):
    """ms per call between device events: eager, and replayed from a graph"""
    side = torch.cuda.Stream()                   # warm-up on a side stream, as before every capture in sinnerf_amd/system.py
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(warmup, 3)):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    def timed(run, count):
        out = []
        for _ in range(count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    eager = timed(fn, steps)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    replay = timed(g.replay, warmup + steps)[warmup:]
    return {"eager": quantiles(eager), "graph": quantiles(replay)}


def time_calls(S, dev, steps, warmup):
    w, z, rays, raw = inputs(S, dev)
    g_w, per_ray, out = torch.empty_like(w), torch.empty((N_RAYS, 2), device=dev), torch.empty(4, device=dev)
    ws = torch.empty(_lib.lib.sn_ray_regularizers_workspace_bytes(N_RAYS), dtype=torch.uint8, device=dev)
    rgb, depth, weights = torch.empty((N_RAYS, 3), device=dev), torch.empty(N_RAYS, device=dev), torch.empty_like(w)

    def reg():
        _lib.check(_lib.lib.sn_ray_regularizers(_lib.ptr(w), _lib.ptr(z), _lib.ptr(rays), N_RAYS, S, 0.01, 0.001, 0.1, _lib.ptr(g_w),
                                                _lib.ptr(per_ray), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr()), "sn_ray_regularizers")

    def composite():
        _lib.check(_lib.lib.sn_composite_forward(_lib.ptr(raw), 1, _lib.ptr(z), _lib.ptr(rays), None, 0.0, N_RAYS, S, 1, _lib.ptr(rgb),
                                                 _lib.ptr(depth), _lib.ptr(weights), _lib.stream_ptr()), "sn_composite_forward")

    w_leaf = w.clone().requires_grad_(True)

    def torch_ops():
        w_leaf.grad = None
        torch_formulation(w_leaf, z, rays, 0.01, 0.001, 0.1).backward()

    return {"ray_regularizers": between_events(reg, steps, warmup), "composite_forward": between_events(composite, steps, warmup),
            "torch_ops": between_events(torch_ops, steps, warmup)}


def time_steps(sampler, steps, warmup):
    """ms per synchronised bf16 step, the terms on and off, alternating, on two systems of the same seed"""
    dev = sampler.device
    systems = {}
    for name, hp in (("off", {}), ("on", dict(distortion_weight=0.01, entropy_weight=0.001))):
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
    assert torch.cuda.is_available(), "tools/ray_reg_time.py measures on the MI355X; there is no CPU path"
    dev = torch.device("cuda:0")
    fmt = lambda q: f"{1e3 * q['median']:.1f} us ({1e3 * q['p10']:.1f}, {1e3 * q['p90']:.1f})"
    lines = [f"# tools/ray_reg_time.py --steps {args.steps} --warmup {args.warmup} on one MI355X, world size 1; medians (p10, p90)"]
    rec = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "calls_ms": {}}
    for S in (128, 64):
        r = time_calls(S, dev, args.steps, args.warmup)
        rec["calls_ms"][f"{N_RAYS}x{S}"] = r
        for name, q in r.items():
            lines.append(f"{N_RAYS} x {S:3d} {name:17s} between device events: eager {fmt(q['eager'])}; replayed from a graph {fmt(q['graph'])}")
        k, c, o = (r[n]["graph"]["median"] for n in ("ray_regularizers", "composite_forward", "torch_ops"))
        lines.append(f"{N_RAYS} x {S:3d} replayed: ray_regularizers / composite_forward = {k / c:.2f}; torch ops / ray_regularizers = {o / k:.1f}")
    t = lambda a: torch.from_numpy(a).to(dev)
    rgb, depth, c2w, K, focal = scene()
    torch.manual_seed(0)
    sampler = OneImageSampler(t(rgb), t(depth), t(c2w), t(K), focal=focal, near=2.0, far=6.0, patch_size=PS, sW=STRIDE, sH=STRIDE, num=NUM,
                              eps=1e-9)
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
