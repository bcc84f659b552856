"""fp64 numpy restatement of the intrinsics sums of ``sn_generate_rays_cam_dev_backward`` / ``sn_ndc_rays_dev_backward``
(include/sinnerf_hip.h), shared by tests/test_intrinsics_cpu.py (which holds it to the reference's fp64 autograd) and the GPU tests."""
import numpy as np


def upstream(n, seed):
    """g_k of tools/gen_golden_intrinsics.py"""
    return np.random.RandomState(int(seed)).standard_normal((n, 8)).astype(np.float32)


def camera_dirs(H, W, fx, fy, cx, cy, s):
    """(n, 3) camera-space directions, row-major over pixels; s = -1 (opengl) or +1 (opencv)"""
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    c = np.stack([(i - cx) / fx, s * (j - cy) / fy, np.full_like(i, s)], -1)
    return c.reshape(-1, 3)


def ndc_quotients(o, d, near):
    t = -(near + o[:, 2]) / d[:, 2]
    p = o + t[:, None] * d
    return t, p, p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], d[:, 0] / d[:, 2], d[:, 1] / d[:, 2]


def ndc_scale_sums(o, d, near, go, gd):
    """(g_ax, g_ay) from the gradient (go, gd) of the map's OUTPUT"""
    _, _, ox_oz, oy_oz, u, v = ndc_quotients(o, d, near)
    return ((go[:, 0] * ox_oz + gd[:, 0] * (u - ox_oz)).sum(), (go[:, 1] * oy_oz + gd[:, 1] * (v - oy_oz)).sum())


def ndc_adjoint(o, d, near, ax, ay, go, gd):
    """gradient of the map's INPUT (o, d) from that of its output: autograd of get_ndc_rays written out"""
    t, p, ox_oz, oy_oz, u, v = ndc_quotients(o, d, near)
    pz, dz = p[:, 2], d[:, 2]
    g_rz = (go[:, 2] - gd[:, 2]) * 2.0 * near
    g_u, g_v = ax * gd[:, 0], ay * gd[:, 1]
    g_a, g_b = ax * go[:, 0] - g_u, ay * go[:, 1] - g_v
    g_p = np.stack([g_a / pz, g_b / pz, -g_rz / pz ** 2 - g_a * ox_oz / pz - g_b * oy_oz / pz], -1)
    g_d = np.stack([g_u / dz, g_v / dz, -g_u * u / dz - g_v * v / dz], -1) + t[:, None] * g_p
    g_t = (g_p * d).sum(-1)
    g_d[:, 2] -= g_t * t / dz
    g_o = g_p.copy()
    g_o[:, 2] -= g_t / dz
    return g_o, g_d


def intrinsics_grad(H, W, fx, fy, cx, cy, s, c2w, g, ndc_near=None):
    """(dL/dfx, dL/dfy, dL/dcx, dL/dcy) of L = sum(rays * g) by the formulas of the header, all in fp64; with NDC the map's focal
    length is fx and its share is in dL/dfx"""
    c2w, g = np.asarray(c2w, np.float64), np.asarray(g, np.float64)
    R = c2w[:, :3]
    c = camera_dirs(H, W, fx, fy, cx, cy, s)
    go, gd = g[:, 0:3], g[:, 3:6]
    g_ax = g_ay = 0.0
    if ndc_near is not None:
        o, d = np.broadcast_to(c2w[:, 3], c.shape), c @ R.T
        g_ax, g_ay = ndc_scale_sums(o, d, ndc_near, go, gd)
        go, gd = ndc_adjoint(o, d, ndc_near, -2.0 * fx / W, -2.0 * fx / H, go, gd)
    gc = gd @ R                                                         # gc_k = sum_r gd[r] R[r][k]
    g_fx = (gc[:, 0] * (-c[:, 0] / fx)).sum() + g_ax * (-2.0 / W) + g_ay * (-2.0 / H)
    return np.array([g_fx, (gc[:, 1] * (-c[:, 1] / fy)).sum(), (gc[:, 0] * (-1.0 / fx)).sum(), (gc[:, 1] * (-s / fy)).sum()])


def ndc_focal_grad(H, W, world, near, g):
    """dL/dfocal of get_ndc_rays alone at the world rays (n, 6), L = sum(ndc rays * g[:, :6])"""
    world, g = np.asarray(world, np.float64), np.asarray(g, np.float64)
    g_ax, g_ay = ndc_scale_sums(world[:, 0:3], world[:, 3:6], near, g[:, 0:3], g[:, 3:6])
    return g_ax * (-2.0 / W) + g_ay * (-2.0 / H)


def case_camera(z, case):
    """(H, W, fx, fy, cx, cy, s, ndc_near) of a case of tests/golden/rays_intrinsics.npz, as Python floats"""
    H, W = int(z[f"{case}_H"]), int(z[f"{case}_W"])
    if case == "dtu":
        (fx, fy), (cx, cy) = (float(v) for v in z["dtu_focal"]), (float(v) for v in z["dtu_center"])
        return H, W, fx, fy, cx, cy, 1.0, None
    f = float(z[f"{case}_focal"])
    return H, W, f, f, W / 2, H / 2, -1.0, float(z["llff_ndc_near"]) if case == "llff" else None
