#!/usr/bin/env python3
"""Times the camera kernels: for each of the three cameras (blender, llff with NDC, dtu), on a 400 x 400 frame and
on a 64 x 64 strided window of it,

    host    sn_generate_rays_cam          the intrinsics as host floats
    dev     sn_generate_rays_cam_dev      the intrinsics read from device memory
    fwdbwd  sn_generate_rays_cam_dev + sn_generate_rays_cam_dev_backward with g_c2w and g_intr

Each sample is one call between two stream synchronisations (wall clock, so launch overhead is in it: these are 32 B/ray kernels and
launches dominate).  The three variants alternate within the one run, sample by sample, so drift hits them alike; the median, min and
max of --calls samples after --warmup rounds are printed as one JSON line per (camera, shape).

    python tools/camera_time.py [--calls 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinnerf_amd import _lib as L                                                   # noqa: E402

H = W = 400
SHAPES = {"frame_400x400": (0, 0, 1, 1, W, H), "window_64x64_stride6": (5, 7, 6, 6, 64, 64)}
# (fx, fy, cx, cy, convention, ndc, ndc_near)
CAMERAS = {"blender": (555.5, 555.5, W / 2, H / 2, 0, 0, 0.0), "llff": (555.5, 555.5, W / 2, H / 2, 0, 1, 1.0),
           "dtu": (540.0, 530.5, 203.2, 195.7, 1, 0, 0.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert args.calls >= 200, "medians of at least 200 calls"
    dev = torch.device("cuda:0")
    c2w = torch.tensor([[0.99, -0.08, -0.11, 0.13], [0.09, 0.99, 0.05, -0.21], [0.10, -0.06, 0.99, 0.37]], device=dev)
    ws = torch.empty(int(L.lib.sn_camera_backward_workspace_bytes()), dtype=torch.uint8, device=dev)
    g_c2w, g_intr = torch.empty((3, 4), device=dev), torch.empty(4, device=dev)
    stream = L.stream_ptr()
    for cam_name, (fx, fy, cx, cy, conv, ndc, ndc_near) in CAMERAS.items():
        intr = torch.tensor([fx, fy, cx, cy], dtype=torch.float32).to(dev)
        for shape_name, win in SHAPES.items():
            n = win[4] * win[5]
            rays = torch.empty((n, 8), device=dev)
            g = torch.randn((n, 8), generator=torch.Generator().manual_seed(1)).to(dev)

            def host():
                L.check(L.lib.sn_generate_rays_cam(L.ptr(c2w), H, W, fx, fy, cx, cy, conv, ndc, fx, ndc_near, 0.0, 1.0, *win, L.ptr(rays),
                                                   stream), "sn_generate_rays_cam")

            def device():
                L.check(L.lib.sn_generate_rays_cam_dev(L.ptr(c2w), L.ptr(intr), H, W, conv, ndc, ndc_near, 0.0, 1.0, *win, L.ptr(rays), stream),
                        "sn_generate_rays_cam_dev")

            def fwdbwd():
                device()
                L.check(L.lib.sn_generate_rays_cam_dev_backward(L.ptr(g), L.ptr(c2w), L.ptr(intr), H, W, conv, ndc, ndc_near, *win, L.ptr(ws),
                                                                L.ptr(g_c2w), L.ptr(g_intr), stream), "sn_generate_rays_cam_dev_backward")

            variants = {"host": host, "dev": device, "fwdbwd": fwdbwd}
            samples = {k: [] for k in variants}
            for it in range(args.warmup + args.calls):
                for name, fn in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        samples[name].append((time.perf_counter() - t0) * 1e6)
            out = {"camera": cam_name, "shape": shape_name, "rays": n, "calls": args.calls, "unit": "us"}
            for name, v in samples.items():
                out[name] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
