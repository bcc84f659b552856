"""The yardstick of the reprojection-loss tests: every quantity of ``sn_reproject_loss`` (include/sinnerf_hip.h) in numpy, with the analytic
gradients written out, all arithmetic in a chosen dtype.  Evaluated in fp64 it is the reference value; evaluated in fp32 on the same
inputs it gives ``e32``, the error a correct fp32 implementation has, from which the tests' bars are formed (``bar``).

It also reports how far every pixel is from the decision boundaries of the definition (``margins``): a comparison of values or gradients
runs only on inputs where NO pixel is closer than ``MARGIN`` to one (``assert_margins``; nothing is filtered out), and ``recipe`` builds
inputs that keep 0.025 from the occlusion boundary and 0.1 from the lattice by construction."""
import numpy as np

OCC_TOL, CHARB_EPS, Z_MIN, OPACITY_THRESHOLD = 0.05, 1e-3, 1e-6, 0.5
MARGIN = 1e-3
SHAPES = [(1, 2, 2, 1), (65, 5, 7, 3), (257, 33, 17, 4), (4096, 40, 40, 3)]          # (n, H, W, C)
ORIGIN = (0.5, -0.2, -0.3)


def bilinear(img, x0, y0, fx, fy, t):
    """img (H, W[, C]) sampled at corners (y0, x0) with fractions (fx, fy) -> (sample, d/du, d/dv), in dtype t"""
    s00, s10, s01, s11 = (img[y0, x0].astype(t), img[y0, x0 + 1].astype(t), img[y0 + 1, x0].astype(t), img[y0 + 1, x0 + 1].astype(t))
    if img.ndim == 3:
        fx, fy = fx[:, None], fy[:, None]
    one = t(1)
    s = (one - fy) * ((one - fx) * s00 + fx * s10) + fy * ((one - fx) * s01 + fx * s11)
    s_u = (one - fy) * (s10 - s00) + fy * (s11 - s01)
    s_v = (one - fx) * (s01 - s00) + fx * (s11 - s10)
    return s, s_u, s_v, (s00, s10, s01, s11)


def evaluate(rays, depth, rgb, opacity, ref_image, ref_depth, ref_proj, w_photo=1.0, w_free=1.0, occ_tol=OCC_TOL, charb_eps=CHARB_EPS,
             z_min=Z_MIN, opacity_threshold=OPACITY_THRESHOLD, dtype=np.float64):
    """-> dict: G, V, front (n,) bool; flags (n,) uint8; photo_i, free_i, per_pixel (n, 2); out (6,); g_depth (n,), g_rgb (n, C);
    u, v, z, r; margins: dict of (n,) distances to the decision boundaries.  The float parameters are taken as the entry takes them:
    rounded to fp32 first."""
    t = dtype
    old = np.seterr(all="ignore")
    try:
        rays, ref_image, ref_depth = np.asarray(rays), np.asarray(ref_image), np.asarray(ref_depth)
        n, C = rgb.shape
        H, W = ref_depth.shape
        tol, eps, zmin, thr = (t(np.float32(x)) for x in (occ_tol, charb_eps, z_min, opacity_threshold))
        wp, wf = t(np.float32(w_photo)), t(np.float32(w_free))
        P = np.asarray(ref_proj).astype(t)
        o, d, td = rays[:, 0:3].astype(t), rays[:, 3:6].astype(t), np.asarray(depth).reshape(-1).astype(t)
        X = o + td[:, None] * d
        q = X @ P[:3, :3].T + P[:3, 3]
        z = q[:, 2]
        u, v = q[:, 0] / z, q[:, 1] / z
        ok_t = np.isfinite(td) & (td > 0)
        ok_z = z >= zmin
        ok_o = np.ones(n, bool) if opacity is None else (np.asarray(opacity).reshape(-1).astype(t) > thr)
        ok_uv = (u >= 0) & (u <= t(W - 1)) & (v >= 0) & (v <= t(H - 1))
        pre = ok_t & ok_z & ok_o & ok_uv
        us, vs = np.where(pre, u, t(0)), np.where(pre, v, t(0))              # a safe position for the pixels that are out already
        x0 = np.minimum(np.floor(us).astype(np.int64), W - 2)
        y0 = np.minimum(np.floor(vs).astype(np.int64), H - 2)
        fx, fy = us - x0.astype(t), vs - y0.astype(t)
        D, D_u, D_v, corners = bilinear(ref_depth, x0, y0, fx, fy, t)
        G = pre & (corners[0] > 0) & (corners[1] > 0) & (corners[2] > 0) & (corners[3] > 0)
        c, c_u, c_v, _ = bilinear(ref_image, x0, y0, fx, fy, t)
        Ds = np.where(G, D, t(1))
        r = np.where(G, (z - Ds) / Ds, t(0))
        V = G & (np.abs(r) <= tol)
        fr = -r - tol
        front = G & (fr > 0)
        e = rgb.astype(t) - c
        h = np.sqrt(e * e + eps * eps)
        photo_i = np.where(V, h.sum(-1, dtype=t) / t(C), t(0)).astype(t)
        free_i = np.where(front, fr, t(0)).astype(t)
        n_vis, n_geo, n_front = int(V.sum()), int(G.sum()), int(front.sum())
        photo = photo_i.sum(dtype=t) / t(n_vis) if n_vis else t(0)
        free = free_i.sum(dtype=t) / t(n_geo) if n_geo else t(0)
        out = np.array([photo, free, wp * photo + wf * free, n_vis, n_geo, n_front], dtype=t)
        # the gradient chain
        a = d @ P[:3, :3].T
        zs = np.where(pre, z, t(1))
        u_t, v_t = (a[:, 0] - us * a[:, 2]) / zs, (a[:, 1] - vs * a[:, 2]) / zs
        s = e / h
        k_photo = wp / (t(n_vis) * t(C)) if n_vis else t(0)
        k_free = wf / t(n_geo) if n_geo else t(0)
        g_rgb = np.where(V[:, None], k_photo * s, t(0)).astype(t)
        g_photo = -k_photo * (s * (c_u * u_t[:, None] + c_v * v_t[:, None])).sum(-1, dtype=t)
        r_t = a[:, 2] / Ds - zs * (D_u * u_t + D_v * v_t) / (Ds * Ds)
        g_depth = (np.where(V, g_photo, t(0)) + np.where(front, k_free * -r_t, t(0))).astype(t)
        flags = (G.astype(np.uint8) | (V.astype(np.uint8) << 1) | (front.astype(np.uint8) << 2)).astype(np.uint8)
        far = np.float64(np.inf)
        fin = lambda x: np.where(np.isfinite(x), np.abs(x).astype(np.float64), far)
        margins = dict(occlusion=np.where(G, fin(np.abs(r) - tol), far),
                       lattice=np.where(pre, np.minimum(fin(us - np.round(us)), fin(vs - np.round(vs))), far),
                       edge=np.where(ok_t & ok_z & ok_o, np.minimum(np.minimum(fin(u), fin(u - t(W - 1))),
                                                                    np.minimum(fin(v), fin(v - t(H - 1)))), far),
                       opacity=np.full(n, far) if opacity is None else fin(np.asarray(opacity).reshape(-1).astype(t) - thr))
        return dict(G=G, V=V, front=front, flags=flags, photo_i=photo_i, free_i=free_i, per_pixel=np.stack([photo_i, free_i], 1), out=out,
                    g_depth=g_depth, g_rgb=g_rgb, u=u, v=v, z=z, r=r, margins=margins)
    finally:
        np.seterr(**old)


def assert_margins(res, margin=MARGIN):
    """the condition of every comparison of values and gradients: no pixel within `margin` of a decision boundary"""
    for name, m in res["margins"].items():
        assert m.size == 0 or float(m.min()) >= margin, (name, float(m.min()), int(m.argmin()))


def rel(got, want):
    """relative L2 distance (a scalar: relative error); the absolute one where the reference is exactly zero"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nrm = float(np.linalg.norm(want.ravel()))
    dif = float(np.linalg.norm((got - want).ravel()))
    return dif / nrm if nrm > 0 else dif


def bar(x64, x32):
    """the kernel must be within max(4 e32, 1e-6) of fp64, e32 = the error of this oracle's own fp32 evaluation (the rule of
    tests/ray_reg_oracle.py)"""
    return max(4.0 * rel(x32, x64), 1e-6)


def frame(H, W, C):
    """depth 2 + 0.3 sin(0.7 x) cos(0.5 y), image 0.5 + 0.4 sin(0.9 x + 0.6 y + c): (ref_image (H, W, C), ref_depth (H, W)) fp32"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 2.0 + 0.3 * np.sin(0.7 * x) * np.cos(0.5 * y)
    image = np.stack([0.5 + 0.4 * np.sin(0.9 * x + 0.6 * y + c) for c in range(C)], -1)
    return image.astype(np.float32), depth.astype(np.float32)


def intrinsics(H, W):
    K = np.eye(3)
    K[0, 0] = K[1, 1] = 1.2 * W
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return K


def projection(K, E=None):
    """[K E[:3]; 0 0 0 1] fp64; E = None: the camera at the world origin"""
    P = np.eye(4)
    P[:3] = K @ (np.eye(4) if E is None else E)[:3]
    return P


def recipe(n, H, W, C, seed=0, occ_tol=OCC_TOL, t=None):
    """-> dict(rays (n, 8), depth (n,), rgb (n, C), opacity (n,), ref_image, ref_depth: fp32; ref_proj (4, 4) fp64; family (n,)).
    ``t`` (n,): depths to use instead of the drawn ones (a render's: the rays are then aimed so that THOSE depths reach the targets).
    Pixel i is aimed at a target (u*, v*) of the reference frame whose fractional parts lie in [0.1, 0.9], at the residual r* of its
    family -- i % 3 = 0 visible (|r*| <= tol / 2), 1 in front (r* in [-4 tol, -2 tol]), 2 behind (r* in [2 tol, 4 tol]) -- from the
    origin (0.5, -0.2, -0.3) with t in [1, 3] and an opacity in [0.6, 1]."""
    rs = np.random.RandomState(1000 * seed + 31 * n + 7 * H + W + C)
    image, depth_map = frame(H, W, C)
    K = intrinsics(H, W)
    xi, yi = rs.randint(0, W - 1, n), rs.randint(0, H - 1, n)
    fx, fy = rs.uniform(0.1, 0.9, n), rs.uniform(0.1, 0.9, n)
    us, vs = xi + fx, yi + fy
    family = np.arange(n) % 3
    lo = np.array([-0.5, -4.0, 2.0])[family] * occ_tol
    hi = np.array([0.5, -2.0, 4.0])[family] * occ_tol
    r_star = rs.uniform(lo, hi)
    D = bilinear(depth_map, xi, yi, fx, fy, np.float64)[0]
    z = D * (1.0 + r_star)
    X = np.stack([us * z, vs * z, z], 1) @ np.linalg.inv(K).T
    drawn = rs.uniform(1.0, 3.0, n).astype(np.float32)
    t = drawn if t is None else np.asarray(t, dtype=np.float32).reshape(n)
    o = np.broadcast_to(np.array(ORIGIN), (n, 3))
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = o
    rays[:, 3:6] = (X - o) / t.astype(np.float64)[:, None]
    rays[:, 6], rays[:, 7] = 0.5, 6.0
    return dict(rays=rays, depth=t, rgb=rs.uniform(0, 1, (n, C)).astype(np.float32), opacity=rs.uniform(0.6, 1.0, n).astype(np.float32),
                ref_image=image, ref_depth=depth_map, ref_proj=projection(K), family=family)


def call_args(inp):
    """the recipe's arrays in the order evaluate() takes them"""
    return tuple(inp[k] for k in ("rays", "depth", "rgb", "opacity", "ref_image", "ref_depth", "ref_proj"))


def lattice(H, W, C, dtype=np.float32):
    """The lattice camera: P = [I | 0], o = 0, d = (x, y, 1), depth t = 1 at every pixel (x, y) of the frame in raster order, rgb = the
    image -- there u = x and v = y exactly, z = 1; with ref_depth = 1 everywhere r = 0 exactly and photo = charb_eps.  -> the dict of
    recipe() (opacity 1)."""
    image, _ = frame(H, W, C)
    y, x = np.mgrid[0:H, 0:W]
    n = H * W
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 3], rays[:, 4], rays[:, 5] = x.reshape(-1), y.reshape(-1), 1.0
    rays[:, 6], rays[:, 7] = 0.5, 6.0
    return dict(rays=rays, depth=np.ones(n, dtype=np.float32), rgb=image.reshape(n, C).copy(), opacity=np.ones(n, dtype=np.float32),
                ref_image=image, ref_depth=np.ones((H, W), dtype=np.float32), ref_proj=np.eye(4))
