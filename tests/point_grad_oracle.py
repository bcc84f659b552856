"""float64 restatement of the density gradient d(raw sigma)/d(xyz) (helper of tests/test_point_grads_{cpu,gpu}.py).

What autograd derives from the reference for ``sigma = NeRF(Embedding(xyz), sigma_only=True)`` (models/nerf.py:36-41, :122-138):

    G_l       = pre-activation gradients of the chain for the upstream gradient (0, 0, 0, 1) of [rgb, sigma]
    g_emb_xyz = G0 . W1 + G4 . W5[:, 0:63]            G0 / G4 of xyz_encoding_1 / _5 (the skip input is cat([input_xyz, h]), nerf.py:133)
    g_x       = ge[0:3] + sum_k 2^k (cos(2^k x) ge[3+6k : 6+6k] - sin(2^k x) ge[6+6k : 9+6k])

built from the pieces that exist: ``oracle_np.nerf_forward(cache=)``, ``oracle_np.nerf_backward(gy_out=)`` and
``ray_grad_oracle.embed_grad``.
"""
import numpy as np

from oracle import oracle_np as O
from tests.ray_grad_oracle import embed_grad

F, f8 = np.float32, np.float64


def point_grads_mlp(G0, G4, w1, w5, rays, z, abs_bound=False):
    """What ``sn_point_grads`` computes: (n, S, 3) float64.

    G0, G4 (P, 256): decoded pre-activation gradients, P = n * S rows in (ray, sample) order; w1 (256, 63), w5 (256, 319); rays (n, 8),
    z (n, S) fp32.  The position is the fp32 value the network embedded, xyz = fl(o + fl(d z)); everything after that is float64.
    ``abs_bound``: the same computation with every factor replaced by its absolute value (the quantity A of the error bounds)."""
    a = np.abs if abs_bound else (lambda v: v)
    rays, z = np.asarray(rays, F), np.asarray(z, F)
    n, S = z.shape
    ge = a(np.asarray(G0, f8)) @ a(np.asarray(w1, f8)) + a(np.asarray(G4, f8)) @ a(np.asarray(w5, f8)[:, :63])
    xyz = O._points(rays, z).reshape(-1, 3)
    return embed_grad(xyz, ge, 10, abs_bound).reshape(n, S, 3)


def embedding64(x, n_freqs):
    """Embedding (nerf.py:36-41) of fp32 positions evaluated in float64"""
    x = np.asarray(x, f8)
    out = [x]
    for k in range(n_freqs):
        out += [np.sin(2.0 ** k * x), np.cos(2.0 ** k * x)]
    return np.concatenate(out, -1)


def sigma_grads(params, points, wide=True):
    """(sigma (B, 1), d sigma / d points (B, 3) float64) of the raw sigma at fp32 ``points`` (B, 3).

    ``oracle_np.nerf_forward`` evaluates the network in fp32 and fills the cache, ``oracle_np.nerf_backward`` runs the chain in
    float64 for the upstream gradient (0, 0, 0, 1) and hands out the pre-activation gradients, the formulas above do the rest.
    ``wide=True``: the trunk activations of the cache -- the ReLU masks of the backward -- are recomputed in float64 first, so the
    result is the float64 evaluation of the reference; ``wide=False`` keeps the masks of the fp32 forward (what an fp32
    implementation sees: a pre-activation within rounding of zero may flip one)."""
    points = np.ascontiguousarray(points, F)
    B = points.shape[0]
    xin = np.concatenate([O.embedding(points, 10), np.repeat(O.embedding(np.zeros((1, 3), F), 4), B, 0)], 1)
    cache = {}
    out = O.nerf_forward(params, xin, cache=cache)
    sigma = out[:, 3:4]
    if wide:
        ex = embedding64(points, 10)
        h = ex
        for i in range(8):
            if i == 4:
                h = np.concatenate([ex, h], -1)
            h = np.maximum(h @ params[f"xyz_encoding_{i+1}.0.weight"].astype(f8).T + params[f"xyz_encoding_{i+1}.0.bias"].astype(f8), 0.0)
            cache[f"h{i+1}"] = h
        sigma = h @ params["sigma.weight"].astype(f8).T + params["sigma.bias"].astype(f8)
    g_out = np.zeros((B, 4), f8)
    g_out[:, 3] = 1.0
    gy = {}
    O.nerf_backward(params, cache, g_out, gy_out=gy)
    ge = gy["l1"] @ params["xyz_encoding_1.0.weight"].astype(f8) + gy["l5"] @ params["xyz_encoding_5.0.weight"].astype(f8)[:, :63]
    return sigma, embed_grad(points, ge, 10)


def point_err(got, ref):
    """per point ||g_p - ref_p|| / (||ref_p|| + 1e-3 max_p ||ref_p||): the per-row quantity of ``ray_grad_oracle.median_ray_err``"""
    got, ref = np.asarray(got, f8), np.asarray(ref, f8)
    nr = np.linalg.norm(ref, axis=1)
    return np.linalg.norm(got - ref, axis=1) / (nr + 1e-3 * nr.max())
