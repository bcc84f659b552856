"""The reprojection loss without a GPU: the oracle's analytic gradients (tests/reproject_oracle.py: the chain of include/sinnerf_hip.h written
out) against torch fp64 autograd of the plain expression and against a central difference, the exact families of the definition on the
lattice camera by hand-computable values, the input recipe's margins, the refusals of the Python surface, the neutral defaults of the
system and the two declarations of the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from tests import reproject_oracle as RO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.7, 0.3)]


def torch_total(inp, depth, rgb, w_photo, w_free, masks):
    """the plain expression in torch fp64: projection, bilinear sampling by gathers, the two means; the masks are constants"""
    T = lambda a: torch.from_numpy(np.asarray(a)).double()
    rays, img, dep, P = T(inp["rays"]), T(inp["ref_image"]), T(inp["ref_depth"]), T(inp["ref_proj"])
    tol, eps = float(np.float32(RO.OCC_TOL)), float(np.float32(RO.CHARB_EPS))
    H, W = dep.shape
    X = rays[:, 0:3] + depth[:, None] * rays[:, 3:6]
    q = X @ P[:3, :3].T + P[:3, 3]
    z = q[:, 2]
    u, v = q[:, 0] / z, q[:, 1] / z
    x0 = torch.clamp(torch.floor(u.detach()), 0, W - 2).long()
    y0 = torch.clamp(torch.floor(v.detach()), 0, H - 2).long()
    fx, fy = u - x0, v - y0

    def sample(a):
        s00, s10, s01, s11 = a[y0, x0], a[y0, x0 + 1], a[y0 + 1, x0], a[y0 + 1, x0 + 1]
        bx, by = (fx[:, None], fy[:, None]) if a.dim() == 3 else (fx, fy)
        return (1 - by) * ((1 - bx) * s00 + bx * s10) + by * ((1 - bx) * s01 + bx * s11)

    D, c = sample(dep), sample(img)
    r = (z - D) / D
    V, G = torch.from_numpy(masks["V"]), torch.from_numpy(masks["G"])
    photo_i = torch.sqrt((rgb - c) ** 2 + eps * eps).mean(-1)
    free_i = torch.clamp(-r - tol, min=0)
    zero = torch.zeros((), dtype=torch.float64)
    photo = torch.where(V, photo_i, zero).sum() / V.sum() if V.any() else zero
    free = torch.where(G, free_i, zero).sum() / G.sum() if G.any() else zero
    return float(np.float32(w_photo)) * photo + float(np.float32(w_free)) * free


@pytest.mark.parametrize("n,H,W,C", RO.SHAPES)
def test_oracle_gradients_equal_fp64_autograd(n, H, W, C):
    inp = RO.recipe(n, H, W, C)
    for w_photo, w_free in WEIGHTS:
        ref = RO.evaluate(*RO.call_args(inp), w_photo, w_free)
        RO.assert_margins(ref)
        depth = torch.from_numpy(inp["depth"]).double().requires_grad_(True)
        rgb = torch.from_numpy(inp["rgb"]).double().requires_grad_(True)
        total = torch_total(inp, depth, rgb, w_photo, w_free, ref)
        assert abs(total.item() - ref["out"][2]) <= 1e-12 * max(1.0, abs(total.item()))
        if not total.requires_grad:                                          # a single pixel outside the weighted term's mask
            assert not ref["g_depth"].any() and not ref["g_rgb"].any()
            continue
        g_d, g_c = torch.autograd.grad(total, (depth, rgb), allow_unused=True)
        for name, got, want in (("g_depth", ref["g_depth"], g_d), ("g_rgb", ref["g_rgb"], g_c)):
            want = np.zeros_like(got) if want is None else want.numpy()
            err = float(np.linalg.norm(got - want))
            print(f"({n}, {H}, {W}, {C}) w=({w_photo}, {w_free}) {name}: |oracle - autograd| {err:.3e} of {np.linalg.norm(want):.3e}")
            assert err <= 1e-10 * float(np.linalg.norm(want)), (name, err)


def test_recipe_families_and_fp32_evaluation():
    for n, H, W, C in RO.SHAPES:
        inp = RO.recipe(n, H, W, C)
        r64 = RO.evaluate(*RO.call_args(inp), 0.7, 0.3)
        r32 = RO.evaluate(*RO.call_args(inp), 0.7, 0.3, dtype=np.float32)
        RO.assert_margins(r64)
        m = r64["margins"]
        assert m["occlusion"].min() >= 0.025 - 1e-6 and m["lattice"].min() >= 0.1 - 1e-6 and m["opacity"].min() >= 0.1 - 1e-6
        assert r64["G"].all()                                                # every pixel lands on the foreground
        fam = inp["family"]
        assert (r64["V"] == (fam == 0)).all() and (r64["front"] == (fam == 1)).all()
        assert (r32["flags"] == r64["flags"]).all() and r32["g_depth"].dtype == np.float32
        for k in ("out", "per_pixel", "g_depth", "g_rgb"):
            e32 = RO.rel(r32[k], r64[k])
            print(f"({n}, {H}, {W}, {C}) {k}: oracle fp32 vs fp64 {e32:.3e}")
            assert e32 < 1e-4, k
    assert abs(r64["V"].mean() - 1 / 3) < 0.01 and abs(r64["front"].mean() - 1 / 3) < 0.01


def test_central_difference_on_one_depth():
    inp = RO.recipe(65, 5, 7, 3)
    args = list(RO.call_args(inp))
    ref = RO.evaluate(*args, 0.7, 0.3)
    RO.assert_margins(ref)
    total = lambda depth: RO.evaluate(args[0], depth, *args[2:], 0.7, 0.3)["out"][2]
    for i in (0, 1):                                                         # a visible pixel and one in front
        assert ref["V"][i] if i == 0 else ref["front"][i]
        h = 1e-5
        up, dn = inp["depth"].astype(np.float64), inp["depth"].astype(np.float64)
        up[i] += h
        dn[i] -= h
        fd = (total(up) - total(dn)) / (2 * h)
        print(f"pixel {i}: analytic {ref['g_depth'][i]:.12e}, central difference {fd:.12e}")
        assert abs(fd - ref["g_depth"][i]) <= 1e-8 * max(abs(fd), np.abs(ref["g_depth"]).max())


# ---- the exact families on the lattice camera -------------------------------------------------------------------------------------------
H, W, C = 5, 7, 3


def lattice_eval(change=None, **kw):
    inp = RO.lattice(H, W, C)
    if change is not None:
        change(inp)
    return inp, RO.evaluate(*RO.call_args(inp), 1.0, 1.0, **kw)


def test_lattice_everything_visible_and_photo_is_charb_eps():
    inp, res = lattice_eval()
    n = H * W
    assert (res["u"] == inp["rays"][:, 3]).all() and (res["v"] == inp["rays"][:, 4]).all() and (res["r"] == 0).all()
    assert (res["flags"] == 3).all()                                         # u = W - 1 and v = H - 1 are inside
    eps = np.float64(np.float32(RO.CHARB_EPS))
    assert np.allclose(res["photo_i"], eps, rtol=1e-15, atol=0) and not res["free_i"].any()
    assert abs(res["out"][0] - eps) < 1e-17 and res["out"][1] == 0 and list(res["out"][3:]) == [n, n, 0]
    assert not res["g_rgb"].any()                                            # rgb == the image: s = 0


def test_lattice_invalid_families():
    col, row = RO.lattice(H, W, C)["rays"][:, 3], RO.lattice(H, W, C)["rays"][:, 4]

    def outside(inp):
        inp["rays"][0, 3], inp["rays"][1, 3], inp["rays"][2, 4], inp["rays"][3, 4] = -0.5, W - 0.5, -0.5, H - 0.5
    _, res = lattice_eval(outside)
    assert (res["flags"][:4] == 0).all() and (res["flags"][4:] == 3).all()
    assert not res["g_depth"][:4].any() and not res["g_rgb"][:4].any() and not res["per_pixel"][:4].any()

    def bad_depth(inp):
        inp["depth"][:4] = [np.nan, 0.0, -1.0, np.inf]
    _, res = lattice_eval(bad_depth)
    assert (res["flags"][:4] == 0).all() and (res["flags"][4:] == 3).all() and np.isfinite(res["out"]).all()
    assert np.isfinite(res["g_depth"]).all() and not res["g_depth"][:4].any() and not res["g_rgb"][:4].any()

    _, res = lattice_eval(z_min=1.5)                                         # z = 1 everywhere
    assert not res["flags"].any() and not res["out"].any() and not res["g_depth"].any() and not res["g_rgb"].any()

    def low_opacity(inp):
        inp["opacity"][::2] = 0.5                                            # not ABOVE the threshold
    _, res = lattice_eval(low_opacity)
    assert (res["flags"][::2] == 0).all() and (res["flags"][1::2] == 3).all()

    def hole(inp):
        inp["ref_depth"][2, 3] = 0.0
    _, res = lattice_eval(hole)
    near = (np.abs(col - 3) <= 1) & (np.abs(row - 2) <= 1)
    # the pixels ON the lattice read the corners (x0, y0) .. (x0 + 1, y0 + 1) with x0 = min(x, W - 2): those that touch (3, 2)
    x0, y0 = np.minimum(col, W - 2), np.minimum(row, H - 2)
    touched = ((x0 == 3) | (x0 + 1 == 3)) & ((y0 == 2) | (y0 + 1 == 2))
    assert (res["flags"][touched] == 0).all() and (res["flags"][~touched] == 3).all() and touched.sum() == 4 and near[touched].all()


def test_lattice_front_and_behind_by_hand():
    def move(inp):
        inp["depth"][0], inp["depth"][1] = 0.5, 2.0                          # z = 0.5: r = -0.5; z = 2: r = 1
    _, res = lattice_eval(move)
    tol = np.float64(np.float32(RO.OCC_TOL))
    assert res["flags"][0] == 5 and res["flags"][1] == 1 and (res["flags"][2:] == 3).all()
    assert res["free_i"][0] == 0.5 - tol and res["free_i"][1] == 0
    n = H * W
    assert list(res["out"][3:]) == [n - 2, n, 1] and res["out"][1] == (0.5 - tol) / n
    # r = z / D - 1 with D = 1 constant and z = t: r_t = 1, so d total / d t_0 = -1 / n_geo; the occluded pixel gets nothing
    assert abs(res["g_depth"][0] + 1.0 / n) < 1e-16 and res["g_depth"][1] == 0 and not res["g_rgb"][:2].any()


def test_nothing_valid_gives_exact_zeros():
    def nothing(inp):
        inp["ref_depth"][:] = 0.0
    _, res = lattice_eval(nothing)
    for k in ("out", "per_pixel", "g_depth", "g_rgb", "flags"):
        assert np.isfinite(res[k]).all() and not res[k].any(), k


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_refuses_cpu_tensors():
    import sinnerf_amd
    from sinnerf_amd import reprojection as RP
    assert sinnerf_amd.reprojection_loss is RP.reprojection_loss and "reprojection_loss" in sinnerf_amd.__all__
    inp = RO.recipe(65, 5, 7, 3)
    rays, depth, rgb, opacity, img, dep, P = (torch.from_numpy(a) for a in RO.call_args(inp))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RP.reprojection_loss(rays, depth, rgb, img, dep, P, opacity=opacity)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        RP.reprojection_loss(rays.numpy(), depth, rgb, img, dep, P)


def test_system_defaults_are_neutral():
    from sinnerf_amd.system import DEFAULT_HPARAMS
    want = dict(reproj_weight=0.0, freespace_weight=0.0, reproj_occlusion_tol=0.05, reproj_opacity_threshold=0.5)
    assert {k: DEFAULT_HPARAMS[k] for k in want} == want


def test_header_and_binding_declare_the_entries_alike():
    from sinnerf_amd import _lib
    hdr = open(os.path.join(REPO, "include", "sinnerf_hip.h")).read()
    for name in ("sn_reproject_loss_workspace_bytes", "sn_reproject_loss"):
        m = re.search(r"\b(?:long|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name + " is not declared in include/sinnerf_hip.h"
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params), name
        assert hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["sn_reproject_loss"][1]) == 24 and len(_lib.SIGNATURES["sn_reproject_loss_workspace_bytes"][1]) == 1
