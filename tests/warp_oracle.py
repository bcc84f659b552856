"""NumPy fp64 restatement of the unseen-view forward warp (include/sinnerf_hip.h: sn_forward_warp, sn_select_landed): the projection,
both collision rules and the k-th-set-element selection.  Written from the header's rule, not from the reference's code; the fixture
(tests/golden/warp.npz, tools/gen_golden_warp.py) holds it to the unmodified reference in tests/test_warp_cpu.py."""
import numpy as np


def proj_matrix(K, E):
    """[K E[:3]; 0 0 0 1] in fp64"""
    P = np.eye(4)
    P[:3] = np.asarray(K, np.float64) @ np.asarray(E, np.float64)[:3]
    return P


def project(depth, proj_ref, proj_src, eps=0.0):
    """xs, ys, p2 (H*W,) fp64 of every source pixel in raster order: p = M (x d, y d, d, 1), summed left to right"""
    H, W = depth.shape
    M = (np.asarray(proj_src, np.float64) @ np.linalg.inv(np.asarray(proj_ref, np.float64)))[:3]
    y, x = np.divmod(np.arange(H * W), W)
    d = np.asarray(depth, np.float32).reshape(-1).astype(np.float64)
    xd, yd = x * d, y * d
    with np.errstate(all="ignore"):
        p = [((M[r, 0] * xd + M[r, 1] * yd) + M[r, 2] * d) + M[r, 3] for r in range(3)]
        return p[0] / (p[2] + eps), p[1] / (p[2] + eps), p[2]


def targets(xs, ys, H, W):
    """target raster index per source pixel, -1 where a NaN coordinate drops it"""
    ok = ~(np.isnan(xs) | np.isnan(ys))
    tx = np.clip(np.floor(np.where(ok, xs, 0.0)), 0, W - 1).astype(np.int64)
    ty = np.clip(np.floor(np.where(ok, ys, 0.0)), 0, H - 1).astype(np.int64)
    return np.where(ok, ty * W + tx, -1)


def winners(t, p2, n, mode):
    """winner (n,) int64: per target the source raster index that wins, -1 where nothing landed.
    mode 0: the last source pixel in raster order; mode 1: the smallest fp32 depth, ties to the lowest index"""
    src = np.flatnonzero(t >= 0)
    win = np.full(n, -1, np.int64)
    if mode == 0:
        np.maximum.at(win, t[src], src)
        return win
    with np.errstate(all="ignore"):
        d32 = p2[src].astype(np.float32) + np.float32(0.0)
    order = np.lexsort((src, d32, t[src]))                     # by target, then depth, then index
    ts = t[src][order]
    first = np.r_[True, ts[1:] != ts[:-1]]
    win[ts[first]] = src[order][first]
    return win


def forward_warp(data, depth, proj_ref, proj_src, eps=0.0, mode=0):
    """-> dict(new (H*W, C) | None, new_depth (H*W,) fp32, mask (H*W,) bool, winner (H*W,) int64, xs, ys, p2, t)"""
    H, W = depth.shape
    xs, ys, p2 = project(depth, proj_ref, proj_src, eps)
    t = targets(xs, ys, H, W)
    win = winners(t, p2, H * W, mode)
    landed = win >= 0
    with np.errstate(all="ignore"):
        new_depth = np.where(landed, p2[np.maximum(win, 0)], 0.0).astype(np.float32)
    new = None
    if data is not None:
        rows = np.ascontiguousarray(data, np.float32).reshape(H * W, -1)
        new = np.where(landed[:, None], rows[np.maximum(win, 0)].view(np.uint32), np.uint32(0)).view(np.float32)
    return dict(new=new, new_depth=new_depth, mask=landed, winner=win, xs=xs, ys=ys, p2=p2, t=t)


def window_index(H, W, window):
    """raster indices of the window's pixels, row-major over (iy, ix)"""
    x0, y0, sx, sy, ow, oh = window
    return ((y0 + np.arange(oh) * sy)[:, None] * W + (x0 + np.arange(ow) * sx)[None, :]).reshape(-1)


def select_landed(mask, u):
    """idx (m,) int32: the min(floor((double)u N), N - 1)-th set element of mask in raster order, -1 when N = 0; and N"""
    set_ = np.flatnonzero(np.asarray(mask).reshape(-1))
    N = len(set_)
    u = np.asarray(u, np.float32)
    if N == 0:
        return np.full(u.shape, -1, np.int32), 0
    k = np.minimum(np.floor(u.astype(np.float64) * N), N - 1).astype(np.int64)
    return set_[k].astype(np.int32), N


def fragile_targets(res, H, W, tau, mode, depth_gap):
    """(n,) bool: the targets the tolerance rule sets aside.  A source pixel is fragile if its fp64 xs or ys lies within tau of an
    integer: every target it could reach under a shift of tau is set aside.  In mode 1 a target is also fragile if the fp64 depths of
    its two nearest candidates differ by less than depth_gap."""
    xs, ys, p2, t = res["xs"], res["ys"], res["p2"], res["t"]
    out = np.zeros(H * W, bool)
    ok = t >= 0
    with np.errstate(all="ignore"):
        frag = ok & ((np.abs(xs - np.rint(xs)) < tau) | (np.abs(ys - np.rint(ys)) < tau))
    for i in np.flatnonzero(frag):
        reach = {int(np.clip(np.floor(ys[i] + dy), 0, H - 1)) * W + int(np.clip(np.floor(xs[i] + dx), 0, W - 1))
                 for dx in (-tau, tau) for dy in (-tau, tau)}
        if len(reach) > 1:                       # a coordinate clamped far outside the frame reaches one target whatever its rounding
            out[list(reach)] = True
    if mode == 1:
        src = np.flatnonzero(ok)
        order = np.lexsort((p2[src], t[src]))
        ts, ds = t[src][order], p2[src][order]
        same = ts[1:] == ts[:-1]
        first = np.r_[True, ~same]
        second = np.r_[False, same] & np.r_[False, first[:-1]]          # the runner-up of each target
        close = second & (np.r_[0.0, ds[1:] - ds[:-1]] < depth_gap)
        out[ts[close]] = True
    return out, frag
