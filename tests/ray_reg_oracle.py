"""The yardstick of the ray-regulariser tests: the distortion loss of Mip-NeRF 360 (eq. 15) as its plain O(S^2) double sum and the ray
entropy of InfoNeRF (eqs. 5-7), with their analytic gradients, in numpy -- the definitions of include/sinnerf_hip.h restated without the
prefix-sum form the kernel uses.  Evaluated in fp64 it is the reference value; evaluated in fp32 on the same inputs it gives ``e32``, the
error a correct fp32 implementation has, from which the tests' bars are formed (``bar``)."""
import numpy as np

THRESHOLD = 0.1
MARGIN = 1e-6            # every ray of `cases` has |sum(w) - threshold| > MARGIN (the generator keeps 1e-3)


def evaluate(weights, z_vals, rays, w_dist=1.0, w_ent=0.0, threshold=THRESHOLD, dtype=np.float64):
    """every quantity of sn_ray_regularizers, all arithmetic in `dtype` -> dict(dist (n,), ent (n,), o (n,), mask (n,), out (4,),
    per_ray (n, 2), g_weights (n, S), g_cancel (n, S))"""
    t = dtype
    w, z = np.asarray(weights).astype(t), np.asarray(z_vals).astype(t)
    near, far = np.asarray(rays)[:, 6].astype(t), np.asarray(rays)[:, 7].astype(t)
    n, S = w.shape
    span = far - near
    inv = np.where(far > near, t(1) / np.where(far > near, span, t(1)), t(0)).astype(t)
    s = (z - near[:, None]) * inv[:, None]
    m, d = s.copy(), np.zeros_like(s)
    if S > 1:
        m[:, :-1] = (s[:, :-1] + s[:, 1:]) / t(2)
        d[:, :-1] = s[:, 1:] - s[:, :-1]
    gap = np.abs(m[:, :, None] - m[:, None, :])                         # (n, S, S)
    A = (w[:, None, :] * gap).sum(-1, dtype=t)                          # A_k = sum_j w_j |m_k - m_j|
    dist = (w * A).sum(-1, dtype=t) + (w * w * d).sum(-1, dtype=t) / t(3)
    g_dist = t(2) * A + t(2) / t(3) * w * d
    o = w.sum(-1, dtype=t)
    q = o + t(1e-10)
    p = w / q[:, None]
    lg = np.log(p + t(1e-10))
    H = -(p * lg).sum(-1, dtype=t)
    h = -(lg + p / (p + t(1e-10)))
    g_H = (h - (h * p).sum(-1, dtype=t)[:, None]) / q[:, None]
    mask = o > t(threshold)
    ent = np.where(mask, H, t(0)).astype(t)
    md, me = dist.sum(dtype=t) / t(n), ent.sum(dtype=t) / t(n)
    out = np.array([md, me, t(w_dist) * md + t(w_ent) * me, t(mask.sum())], dtype=t)
    g = (t(w_dist) * g_dist + t(w_ent) * np.where(mask[:, None], g_H, t(0))) / t(n)
    # the size of the two operands of the entropy gradient's subtraction, h_k and sum_i h_i p_i, scaled like the gradient: where one
    # sample holds (nearly) all the weight they cancel, and a rounding of p shows in the difference at eps x this size
    cancel = t(w_ent) * np.where(mask[:, None], (np.abs(h) + np.abs((h * p).sum(-1, dtype=t))[:, None]) / q[:, None], t(0)) / t(n)
    return dict(dist=dist, ent=ent, o=o, mask=mask, out=out, per_ray=np.stack([dist, ent], 1), g_weights=g.astype(t),
                g_cancel=cancel.astype(t))


def rel(got, want):
    """relative L2 distance (a scalar: relative error); the absolute one where the reference is exactly zero"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nrm = float(np.linalg.norm(want.ravel()))
    dif = float(np.linalg.norm((got - want).ravel()))
    return dif / nrm if nrm > 0 else dif


def bar(x64, x32):
    """the kernel must be within max(4 e32, 1e-6) of fp64, e32 = the error of this oracle's own fp32 evaluation: 4 for a different
    summation order, the floor for quantities whose e32 is at rounding level"""
    return max(4.0 * rel(x32, x64), 1e-6)


KINDS = ("dense", "faint", "zero", "onehot", "flat", "last", "sparse", "faint")


def cases(n, S, seed=0, threshold=THRESHOLD):
    """-> (weights (n, S), z_vals (n, S), rays (n, 8)) fp32.  Weights from random alphas, w_i = a_i prod_{j<i} (1 - a_j), so sum w <= 1;
    depths a sorted uniform draw in [near, far] with a run of exact ties.  Ray r is of kind KINDS[r % 8]: dense (opaque), faint (sum w
    below the threshold), all zero, one-hot, far == near, all weight on the last sample, sparse (a few large alphas).  Every ray ends
    with |sum w - threshold| > 1e-3 in fp64 (a ray that lands closer is halved)."""
    r = np.random.RandomState(1000 * seed + 7 * n + S)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, :3] = r.uniform(-1, 1, (n, 3))
    dirs = r.normal(size=(n, 3))
    rays[:, 3:6] = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    rays[:, 6] = r.uniform(1.5, 2.5, n)
    rays[:, 7] = rays[:, 6] + r.uniform(3.0, 5.0, n).astype(np.float32)
    w = np.zeros((n, S), dtype=np.float32)
    z = np.zeros((n, S), dtype=np.float32)
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        near, far = float(rays[i, 6]), float(rays[i, 7])
        zi = np.sort(r.uniform(near, far, S)).astype(np.float32)
        if S >= 4:
            a0 = r.randint(0, S - 2)
            zi[a0:a0 + 3] = zi[a0]                                      # a run of exact ties (zi stays ascending: the run's minimum)
        u = r.uniform(0, 1, S)
        if kind == "dense":
            alpha = u ** 3
        elif kind == "faint":
            alpha = u * (0.1 / S)
        elif kind == "sparse":
            alpha = np.where(r.uniform(0, 1, S) < 4.0 / S, 0.3 + 0.6 * u, 0.0)
            alpha[r.randint(0, S)] = 0.5
        else:
            alpha = np.zeros(S)
        wi = alpha * np.concatenate([[1.0], np.cumprod(1.0 - alpha)[:-1]])
        if kind == "onehot":
            wi[r.randint(0, S)] = 1.0
        elif kind == "last":
            wi[S - 1] = 0.9
        elif kind == "flat":
            rays[i, 7] = rays[i, 6]
            zi[:] = rays[i, 6]
            wi = u ** 2 * np.concatenate([[1.0], np.cumprod(1.0 - u ** 2)[:-1]])
        wi = wi.astype(np.float32)
        while abs(float(wi.astype(np.float64).sum()) - threshold) <= 1e-3:
            wi = (wi * np.float32(0.5)).astype(np.float32)
        w[i], z[i] = wi, zi
    return w, z, rays
