"""Time the patch losses at the lego patch size (64 x 64 x 3): the HIP entries behind sinnerf_amd.losses against the same formulas spelled
in torch ops (tests/patch_loss_oracle.py) on the same device, forward + backward, median of synchronised calls.

    python tools/patch_loss_time.py [--iters 200]

The inputs are NCHW views of channel-last buffers, as a rearranged render result is.  No bar is attached to the numbers."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sinnerf_amd import losses as SL                                                   # noqa: E402
from tests import patch_loss_oracle as PO                                              # noqa: E402


def median_ms(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = lambda c: torch.rand(1, 64, 64, c, generator=g).to(dev)
    coarse, fine, depth = rows(3).requires_grad_(True), rows(3).requires_grad_(True), rows(1).requires_grad_(True)
    target = rows(3)
    v = lambda t: t.permute(0, 3, 1, 2)
    leaves = (coarse, fine, depth)

    def step(loss_fn):
        def run():
            for l in leaves:
                l.grad = None
            loss_fn().backward()
        return run

    cases = {
        "l2_ssim": (lambda: SL.L2_SSIM_Loss()({"rgb_coarse": v(coarse), "rgb_fine": v(fine)}, v(target))["tot"],
                    lambda: PO.l2_ssim(v(coarse), v(fine), v(target))[0]),
        "inverse_depth_smoothness": (lambda: SL.inverse_depth_smoothness_loss(v(depth), v(fine)),
                                     lambda: PO.inverse_depth_smoothness_loss(v(depth), v(fine))),
    }
    for name, (hip, ops) in cases.items():
        a, b = hip().item(), ops().item()
        t_hip, t_ops = median_ms(step(hip), args.iters), median_ms(step(ops), args.iters)
        print("%-26s 64x64x3 fwd+bwd: HIP %.3f ms, torch ops %.3f ms (%.1fx); values %.7f / %.7f" % (name, t_hip, t_ops, t_ops / t_hip, a, b))


if __name__ == "__main__":
    main()
