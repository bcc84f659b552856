"""float64 restatement of the ray gradient of one render pass (helper of tests/test_ray_grads_{cpu,gpu}.py).

What autograd derives from the reference for ``rays = [o, d, near, far]`` with the sample depths z held constant
(models/rendering.py:284-285, :187-190, :215-228; models/nerf.py:36-41, :122-148):

    g_emb_xyz = G0 . W1 + G4 . W5[:, 0:63]            G0 / G4 / G9 = pre-activation gradients of xyz_encoding_1 / _5 / dir_encoding
    g_emb_dir = G9[:, 0:128] . Wdir[:, 256:283]
    g_x       = ge[0:3] + sum_k 2^k (cos(2^k x) ge[3+6k : 6+6k] - sin(2^k x) ge[6+6k : 9+6k])
    g_o       = sum_s g_xyz            g_d = sum_s z g_xyz + sum_s g_dirvec + dL/d||d|| . d / ||d||
"""
import numpy as np

from oracle import oracle_np as O

F, f8 = np.float32, np.float64


def embed_grad(x, ge, n_freqs, abs_bound=False):
    """backward of Embedding (nerf.py:36-41) at x (..., 3) for upstream ge (..., 3 + 6 n_freqs).  ``abs_bound``: every factor
    replaced by its absolute value (ge is expected to be non-negative already)."""
    x = np.asarray(x, f8)
    g = np.array(ge[..., 0:3], f8)
    for k in range(n_freqs):
        f = 2.0 ** k
        s, c = np.sin(f * x), np.cos(f * x)
        gs, gc = ge[..., 3 + 6 * k:6 + 6 * k], ge[..., 6 + 6 * k:9 + 6 * k]
        g = g + (f * (np.abs(c) * gs + np.abs(s) * gc) if abs_bound else f * (c * gs - s * gc))
    return g


def ray_grads_mlp(G0, G4, G9, w1, w5, wdir, rays, z, abs_bound=False):
    """The MLP part of dL/d(rays) -- what ``sn_ray_grads`` computes: (n, 8) float64, columns 6, 7 zero.

    G0, G4 (P, 256), G9 (P, >= 128): decoded pre-activation gradients, P = n * S rows in (ray, sample) order; w1 (256, 63),
    w5 (256, 319), wdir (128, 283); rays (n, 8), z (n, S) fp32.  The sample position is the fp32 value the network embedded,
    xyz = fl(o + fl(d z)) (rendering.py:284-285); everything after that is float64.
    ``abs_bound``: the same computation with every factor replaced by its absolute value (the quantity A of the error bounds)."""
    a = np.abs if abs_bound else (lambda v: v)
    rays, z = np.asarray(rays, F), np.asarray(z, F)
    n, S = z.shape
    G0, G4, G9 = a(np.asarray(G0, f8)), a(np.asarray(G4, f8)), a(np.asarray(G9, f8)[:, :128])
    w1, w5, wdir = a(np.asarray(w1, f8)), a(np.asarray(w5, f8)[:, :63]), a(np.asarray(wdir, f8)[:, 256:283])
    ge_xyz = G0 @ w1 + G4 @ w5
    ge_dir = G9 @ wdir
    xyz = O._points(rays, z).reshape(-1, 3)
    d = np.repeat(rays[:, 3:6], S, 0)
    g_xyz = embed_grad(xyz, ge_xyz, 10, abs_bound).reshape(n, S, 3)
    g_dv = embed_grad(d, ge_dir, 4, abs_bound).reshape(n, S, 3)
    out = np.zeros((n, 8), f8)
    out[:, 0:3] = g_xyz.sum(1)
    out[:, 3:6] = (a(z.astype(f8))[:, :, None] * g_xyz).sum(1) + g_dv.sum(1)
    return out


def composite_torch64(raw, z, d, noise, noise_std, white_back):
    """rendering.py:215-246 in torch float64; ``d`` (n, 3) may require grad (deltas = dz * ||d||)."""
    import torch
    dz = torch.cat([z[:, 1:] - z[:, :-1], 1e10 * torch.ones_like(z[:, :1])], -1)
    deltas = dz * torch.norm(d.unsqueeze(1), dim=-1)
    sig = raw[..., 3] if noise is None else raw[..., 3] + noise * noise_std
    alphas = 1 - torch.exp(-deltas * torch.relu(sig))
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-10], -1)
    w = alphas * torch.cumprod(shifted, -1)[:, :-1]
    rgb = (w.unsqueeze(-1) * raw[..., :3]).sum(-2)
    if white_back:
        rgb = rgb + 1 - w.sum(1).unsqueeze(-1)
    return rgb, (w * z).sum(-1), w


def composite_dir_grad(raw, z, d, noise, noise_std, white_back, g_rgb, g_depth, g_w=None):
    """dL/dd through ||d|| of one compositing pass (torch-float64 autograd): (n, 3) float64."""
    import torch
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).double()
    dt = t(d).requires_grad_(True)
    if noise is not None:                                    # the fp32 product the reference forms (rendering.py:224)
        noise, noise_std = (np.asarray(noise, F) * F(noise_std)).astype(F), 1.0
    rgb, depth, w = composite_torch64(t(raw), t(z), dt, t(noise), noise_std, white_back)
    loss = (rgb * t(g_rgb)).sum() + (depth * t(g_depth)).sum()
    if g_w is not None:
        loss = loss + (w * t(g_w)).sum()
    loss.backward()
    return dt.grad.numpy()


def render_rays_ray_grads(models, rays, upstream, N_samples, perturb, noise_std, N_importance, white_back, rng):
    """dL/do, dL/dd of the whole ``render_rays`` (coarse + fine pass, sample_pdf detached) from the oracle's pieces, per pass:
    nerf_forward -> composite_backward -> nerf_backward(gy_out=...) -> ray_grads_mlp + composite_dir_grad.  (n, 3), (n, 3)."""
    rays = np.asarray(rays, F)
    n = rays.shape[0]
    rays_d = rays[:, 3:6]
    dir_emb = O.embedding(rays_d, 4)
    total = np.zeros((n, 8), f8)

    def one(params, z, noise, tag):
        s = z.shape[1]
        xin = np.concatenate([O.embedding(O._points(rays, z).reshape(-1, 3), 10), np.repeat(dir_emb, s, 0)], 1)
        cache = {}
        raw = O.nerf_forward(params, xin, cache=cache).reshape(n, s, 4)
        g_rgb, g_depth = upstream.get("rgb_" + tag, np.zeros((n, 3))), upstream.get("depth_" + tag, np.zeros((n,)))
        g_raw = O.composite_backward(raw, z, rays_d, noise, noise_std, white_back, g_rgb, g_depth, upstream.get("opacity_" + tag))
        gy = {}
        O.nerf_backward(params, cache, g_raw.reshape(-1, 4), gy_out=gy)
        g = ray_grads_mlp(gy["l1"], gy["l5"], gy["dir"], params["xyz_encoding_1.0.weight"], params["xyz_encoding_5.0.weight"],
                          params["dir_encoding.0.weight"], rays, z)
        g[:, 3:6] += composite_dir_grad(raw, z, rays_d, noise, noise_std, white_back, g_rgb, g_depth, upstream.get("opacity_" + tag))
        return raw, g

    z = O.coarse_z_vals(rays, N_samples, False, perturb, rng.get("perturb"))
    raw_c, g = one(models[0], z, rng.get("noise_coarse"), "coarse")
    total += g
    if N_importance > 0:
        _, _, w_c = O.composite(raw_c, z, rays_d, rng.get("noise_coarse"), noise_std, white_back)
        mid = (F(0.5) * (z[:, :-1] + z[:, 1:]).astype(F)).astype(F)
        z_f = O.sample_pdf(mid, w_c[:, 1:-1], N_importance, det=(perturb == 0), u=rng.get("u"))
        z_all = np.sort(np.concatenate([z, z_f], -1), -1)
        _, g = one(models[1], z_all, rng.get("noise_fine"), "fine")
        total += g
    return total[:, 0:3], total[:, 3:6]


def norm_err(got, ref):
    got, ref = np.asarray(got, f8), np.asarray(ref, f8)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def median_ray_err(got, ref):
    """median over rays of ||g_r - ref_r|| / (||ref_r|| + 1e-3 max_r ||ref_r||): the fixture's spread_med_* quantity"""
    got, ref = np.asarray(got, f8), np.asarray(ref, f8)
    nr = np.linalg.norm(ref, axis=1)
    return float(np.median(np.linalg.norm(got - ref, axis=1) / (nr + 1e-3 * nr.max())))
