"""cost of the pose gradient: the 4096-ray 64+64 forward + backward of render_rays with and without rays.requires_grad

    python tools/ray_grad_time.py [fp32 bf16 bf16x3]

Every step is timed on its own between two device synchronisations (host clock); the median of the steps after the warm-up is
printed, with the run-to-run spread (min / max), per arithmetic:  (a) rays.requires_grad  (b) parameters only.  The same
script run on the parent commit prints only (b)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_np as O                                   # noqa: E402
import sinnerf_amd                                                  # noqa: E402

dev = torch.device("cuda:0")
HAVE_RAY_GRADS = hasattr(sinnerf_amd._lib.lib, "sn_ray_grads")


def step_times(dtype, rays_grad, steps=20, warmup=5):
    models = []
    for seed in (0, 1):
        m = sinnerf_amd.NeRF(use_new_activation=True, compute_dtype=dtype)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in O.init_params(seed, True).items()})
        models.append(m.to(dev).train())
    emb = [sinnerf_amd.Embedding(3, 10), sinnerf_amd.Embedding(3, 4)]
    base = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::39][:4096].copy()).to(dev)
    torch.manual_seed(0)
    out = []
    for i in range(warmup + steps):
        for m in models:
            m.zero_grad(set_to_none=True)
        rays = base.clone().requires_grad_(rays_grad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sinnerf_amd.render_rays(models, emb, rays, 64, False, 1.0, 1.0, 64, 32768, True)
        (res["rgb_fine"].sum() + res["rgb_coarse"].sum() + res["depth_fine"].sum()).backward()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
        if rays_grad:
            assert rays.grad is not None
    return np.array(out)


for dtype in (sys.argv[1:] or ["fp32", "bf16", "bf16x3"]):
    line = f"{dtype:7s}"
    med = {}
    for tag, rg in (("a rays+params", True), ("b params only", False)):
        if rg and not HAVE_RAY_GRADS:
            continue
        ts = step_times(dtype, rg)
        med[tag[0]] = float(np.median(ts))
        line += f"  ({tag}) median {np.median(ts):7.3f} ms  min {ts.min():7.3f}  max {ts.max():7.3f}"
    if "a" in med:
        line += f"  a/b {med['a'] / med['b']:.3f}"
    print(line, flush=True)
