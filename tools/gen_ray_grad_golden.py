#!/usr/bin/env python3
"""Golden RAY gradients from the UNMODIFIED reference (run in the build container only, like oracle/gen_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_ray_grad_golden.py

``rays = cat([o, d, near_far])`` with ``o`` and ``d`` as fp32 leaves that require grad go through the reference's
``render_rays`` in train mode; the loss is the seeded linear loss of ``oracle/gen_golden.py::case_grad`` (coefficients from
``RandomState(99)``).  Stored per case (``tests/golden/grad_rays_*.npz``):

    rays, rng_* (the reference's torch.rand / torch.randn draws in call order), coef_*, loss, meta_*
    g_o, g_d                      the reference's fp32 autograd result
    g_o64, g_d64                  the same run with models and inputs cast to float64 and the SAME recorded draws replayed
    spread_o, spread_d            ||g - g64|| / ||g64||: the reference's own fp32-vs-fp64 disagreement on these inputs
    spread_med_o, spread_med_d    median over rays of ||g_r - g64_r|| / (||g64_r|| + 1e-3 max_r ||g64_r||)

The spreads are the yardstick of tests/test_ray_grads_gpu.py: ReLU masks and sample bins flip on last-bit differences (the
effect tests/test_grads_gpu.py::test_mlp_backward_vs_oracle documents), so any two correct implementations differ by about
as much as the reference differs from its own float64 evaluation.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as G                                 # noqa: E402  (importing it runs nothing)
from oracle import oracle_np as O                                  # noqa: E402

ref_model, RngTap, ref_rendering = G.ref_model, G.RngTap, G.ref_rendering
OUT = os.path.join(REPO, "tests", "golden")


class Replay:
    """torch.rand / torch.randn return the recorded draws (cast to ``dtype``); torch.linspace returns ``dtype`` holding the fp32
    values, so the float64 run sees the very same sample positions and noise."""

    def __init__(self, draws, dtype):
        self.q, self.dtype = list(draws), dtype

    def __enter__(self):
        self._saved = torch.rand, torch.randn, torch.linspace

        def take(kind):
            k, arr = self.q.pop(0)
            assert k == kind, (k, kind)
            return torch.from_numpy(arr.copy()).to(self.dtype)
        lin = torch.linspace
        torch.rand = lambda *a, **k: take("rand")
        torch.randn = lambda *a, **k: take("randn")
        torch.linspace = lambda *a, **k: lin(*a, **k).to(self.dtype)
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randn, torch.linspace = self._saved
        assert not self.q or exc[0] is not None


def run(models, rays, coef, kw, dtype, draws=None):
    emb = [G.Embedding(3, 10), G.Embedding(3, 4)]
    o = torch.from_numpy(rays[:, 0:3].copy()).to(dtype).requires_grad_(True)
    d = torch.from_numpy(rays[:, 3:6].copy()).to(dtype).requires_grad_(True)
    r = torch.cat([o, d, torch.from_numpy(rays[:, 6:8].copy()).to(dtype)], 1)
    ctx = RngTap() if draws is None else Replay(draws, dtype)
    with ctx as tap:
        res = ref_rendering.render_rays(models, emb, r, kw["N_samples"], False, kw["perturb"], kw["noise_std"],
                                        kw["N_importance"], 32768, kw["white_back"])
        loss = sum((res[k] * torch.from_numpy(v).to(dtype)).sum() for k, v in coef.items())
    loss.backward()
    return loss.item(), o.grad.numpy(), d.grad.numpy(), (tap.draws if draws is None else None)


def spreads(g, g64):
    g, g64 = g.astype(np.float64), g64.astype(np.float64)
    nr = np.linalg.norm(g64, axis=1)
    per_ray = np.linalg.norm(g - g64, axis=1) / (nr + 1e-3 * nr.max())
    return np.linalg.norm(g - g64) / np.linalg.norm(g64), float(np.median(per_ray)), float(per_ray.max())


def case(name, rays, seeds, **kw):
    mc, _ = ref_model(seeds[0], True)
    mf, _ = ref_model(seeds[1], True)
    mc.train(); mf.train()
    n = rays.shape[0]
    r = np.random.RandomState(99)                                  # the coefficients of case_grad
    coef = {"rgb_coarse": r.standard_normal((n, 3)), "depth_coarse": r.standard_normal(n) * 0.3,
            "rgb_fine": r.standard_normal((n, 3)), "depth_fine": r.standard_normal(n) * 0.3}
    coef = {k: v.astype(np.float32) for k, v in coef.items()}
    torch.manual_seed(4321)
    loss, g_o, g_d, draws = run([mc, mf], rays, coef, kw, torch.float32)
    _, g_o64, g_d64, _ = run([mc.double(), mf.double()], rays, coef, kw, torch.float64, draws)
    names = ["perturb", "noise_coarse", "u", "noise_fine"] if kw["perturb"] > 0 else ["noise_coarse", "noise_fine"]
    assert len(draws) == len(names)
    so, smo, mxo = spreads(g_o, g_o64)
    sd, smd, mxd = spreads(g_d, g_d64)
    trained = isinstance(seeds[0], str)
    arrays = {"rays": rays, "loss": np.asarray(loss), "g_o": g_o, "g_d": g_d, "g_o64": g_o64, "g_d64": g_d64,
              "spread_o": np.asarray(so), "spread_d": np.asarray(sd), "spread_med_o": np.asarray(smo), "spread_med_d": np.asarray(smd)}
    arrays.update({"rng_" + k: v for k, (_, v) in zip(names, draws)})
    arrays.update({"coef_" + k: v for k, v in coef.items()})
    arrays.update({"meta_" + k: np.asarray(v) for k, v in dict(seed_coarse=-1 if trained else seeds[0], seed_fine=-1 if trained else seeds[1],
                                                               weights="trained_student" if trained else "init", **kw).items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
    print(f"{name}: loss {loss:.6f}  spread o {so:.2e} d {sd:.2e}  per-ray median o {smo:.2e} d {smd:.2e}  per-ray max o {mxo:.2e} d {mxd:.2e}")


def main():
    lego = O.lego_rays(400, 400, seed=0)
    sel = np.random.RandomState(17).choice(lego.shape[0], 96, replace=False)          # the selection of gen_golden.main_grads
    case("grad_rays_lego_train", np.ascontiguousarray(lego[sel]), (0, 1), N_samples=64, perturb=1.0, noise_std=1.0,
         N_importance=64, white_back=True)
    case("grad_rays_lego_det", np.ascontiguousarray(lego[sel[:48]]), (2, 3), N_samples=64, perturb=0, noise_std=0,
         N_importance=64, white_back=False)
    sel0 = np.random.RandomState(29).choice(lego.shape[0], 96, replace=False)         # ... of gen_golden.main_trained
    case("grad_rays_trained_det", np.ascontiguousarray(lego[sel0[:48]]), ("trained:coarse", "trained:fine"), N_samples=64,
         perturb=0, noise_std=0, N_importance=64, white_back=True)


if __name__ == "__main__":
    main()
