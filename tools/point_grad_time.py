"""cost of the density gradients at P = 4096 rays x 192 samples (64 + 128)

    python tools/point_grad_time.py [out.txt]

(1) sn_point_grads, sn_ray_grads and sn_point_grads_wsum alone, on ONE random training state per layout (fp32 rows, bf16 rows, bf16x3
    pairs): device events around each launch, the kernels alternating call by call in one process, median / min / max of 20 after 5
    warm-up rounds.  sn_ray_grads runs the same 512-deep contraction plus the 128-deep direction block and its reduction.
(2) end to end, fp32, trained-size networks: render_rays under no_grad, render_normals (the same render + the gradient part in
    chunks of max_points), and ray_density_gradients on all 4096 x 192 points at once; host clock between two device synchronisations."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_np as O                                   # noqa: E402
import sinnerf_amd                                                  # noqa: E402
from sinnerf_amd import _lib as L                                   # noqa: E402

dev = torch.device("cuda:0")
N, S = 4096, 192
P = N * S
ROUNDS, WARM = 20, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stats(ts):
    ts = np.array(ts[WARM:])
    return f"median {np.median(ts):8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernels():
    r = np.random.RandomState(0)
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::39][:N].copy()).to(dev)
    z = torch.sort(torch.rand((N, S), device=dev) * 4 + 2, -1)[0].contiguous()
    w = torch.rand((N, S), device=dev)
    w1, w5, wd = (torch.from_numpy(r.uniform(-0.1, 0.1, s).astype(np.float32)).to(dev) for s in ((256, 63), (256, 319), (128, 283)))
    g_xyz = torch.empty((P, 4), device=dev)
    g_sum = torch.empty((N, 4), device=dev)
    g_rays = torch.empty((N, 8), device=dev)
    ws = torch.empty(int(L.lib.sn_ray_grads_workspace_bytes(N, S)), dtype=torch.uint8, device=dev)
    G32 = torch.randn((10, P, 256), device=dev)
    for tag, code, G in (("fp32 rows", L.SN_DTYPE_F32, G32), ("bf16 rows", L.SN_DTYPE_BF16_STATE, None), ("bf16x3 pairs", L.SN_DTYPE_BF16X3, None)):
        if tag == "bf16 rows":
            G = G32.to(torch.bfloat16)
        elif tag == "bf16x3 pairs":                                  # the same bytes read as bf16 halves; top exponent bit of every
            G = G32                                                  # half cleared (0xBFFFBFFF), so each half is finite, |v| < 2
            G.view(torch.int32).bitwise_and_(-1073758209)
        sp = lambda: L.check(L.lib.sn_point_grads(L.ptr(w1), L.ptr(w5), code, L.ptr(G), P, L.ptr(rays), L.ptr(z), N, S, L.ptr(g_xyz),
                                                  L.stream_ptr()), "sn_point_grads")
        sr = lambda: L.check(L.lib.sn_ray_grads(L.ptr(w1), L.ptr(w5), L.ptr(wd), code, L.ptr(G), P, L.ptr(rays), L.ptr(z), N, S, L.ptr(ws),
                                                L.ptr(g_rays), L.stream_ptr()), "sn_ray_grads")
        sw = lambda: L.check(L.lib.sn_point_grads_wsum(L.ptr(g_xyz), L.ptr(w), N, S, L.ptr(g_sum), L.stream_ptr()), "sn_point_grads_wsum")
        tp, tr, tw = [], [], []
        for _ in range(WARM + ROUNDS):
            tp.append(timed(sp)); tr.append(timed(sr)); tw.append(timed(sw))
        assert torch.isfinite(g_xyz).all() and torch.isfinite(g_sum).all()
        row_bytes = 512 if code == L.SN_DTYPE_BF16_STATE else 1024
        gb = (2 * P * row_bytes + P * 16) / 1e9
        say(f"{tag:13s} sn_point_grads      {stats(tp)}   ({gb:.2f} GB of state read + written: {gb / np.median(tp[WARM:]) * 1e3:.0f} GB/s)")
        say(f"{tag:13s} sn_ray_grads        {stats(tr)}")
        say(f"{tag:13s} sn_point_grads_wsum {stats(tw)}")
        del G
    del G32


def end_to_end():
    models = []
    for tag in ("coarse", "fine"):
        m = sinnerf_amd.NeRF(use_new_activation=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in O.trained_params(tag).items()})
        models.append(m.to(dev).eval())
    emb = [sinnerf_amd.Embedding(3, 10), sinnerf_amd.Embedding(3, 4)]
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::39][:N].copy()).to(dev)
    keep = {}
    res = sinnerf_amd.render_normals(models, emb, rays, 64, False, 128, True, keep=keep)
    z, w = keep["z_vals"], res["opacity_fine"]
    del keep

    def host(fn):
        ts = []
        for _ in range(WARM + ROUNDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def plain():
        with torch.no_grad():
            sinnerf_amd.render_rays(models, emb, rays, 64, False, 0, 0, 128, 32768, True)
    t_r = host(plain)
    t_n = host(lambda: sinnerf_amd.render_normals(models, emb, rays, 64, False, 128, True))
    t_g = host(lambda: sinnerf_amd.ray_density_gradients(models[1], rays, z, w))
    say(f"fp32 end to end, {N} rays x (64 + 128): render_rays (no_grad)            {stats(t_r)}")
    say(f"fp32 end to end, {N} rays x (64 + 128): render_normals (max_points 2^18) {stats(t_n)}")
    say(f"fp32 end to end, {N} x {S} points at once: ray_density_gradients + wsum    {stats(t_g)}")
    say(f"gradient part of render_normals (difference of the medians): "
        f"{np.median(t_n[WARM:]) - np.median(t_r[WARM:]):.3f} ms")


say(f"device: {torch.cuda.get_device_name(0)}   P = {N} x {S} = {P} points")
kernels()
torch.cuda.empty_cache()
end_to_end()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
