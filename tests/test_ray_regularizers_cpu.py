"""The ray regularisers without a GPU: the closed O(S) form the kernel evaluates (prefix / suffix sums, include/sinnerf_hip.h and
csrc/sn_ray_reg.hip) against the O(S^2) oracle, the oracle's analytic gradients against torch fp64 autograd of the O(S^2) expression,
the refusals of the Python surface, the neutral defaults of the system and the two declarations of the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ray_reg_oracle as RO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 5, 64, 130)
N_RAYS = 16                  # two of every kind of RO.KINDS


def closed_form(weights, z_vals, rays, w_dist, w_ent, threshold):
    """the kernel's formulation in numpy fp64: one pass of running sums per ray, no (S, S) array
        A_k = m_k (W_<k - W_>k) - (M_<k - M_>k),  W / M the exclusive prefix and the suffix sums of w / w m"""
    w, z = weights.astype(np.float64), z_vals.astype(np.float64)
    near, far = rays[:, 6].astype(np.float64), rays[:, 7].astype(np.float64)
    n, S = w.shape
    dist, ent, g = np.zeros(n), np.zeros(n), np.zeros((n, S))
    for r in range(n):
        inv = 1.0 / (far[r] - near[r]) if far[r] > near[r] else 0.0
        s = (z[r] - near[r]) * inv
        m = np.append((s[:-1] + s[1:]) / 2, s[-1])
        d = np.append(s[1:] - s[:-1], 0.0)
        wm = w[r] * m
        W_lt, M_lt = np.cumsum(w[r]) - w[r], np.cumsum(wm) - wm
        W_gt, M_gt = w[r].sum() - W_lt - w[r], wm.sum() - M_lt - wm
        A = m * (W_lt - W_gt) - (M_lt - M_gt)
        dist[r] = (w[r] * A).sum() + (w[r] ** 2 * d).sum() / 3
        g_dist = 2 * A + 2 / 3 * w[r] * d
        o = w[r].sum()
        q = o + 1e-10
        p = w[r] / q
        H = -(p * np.log(p + 1e-10)).sum()
        h = -(np.log(p + 1e-10) + p / (p + 1e-10))
        mask = o > threshold
        ent[r] = H if mask else 0.0
        g[r] = (w_dist * g_dist + (w_ent * (h - (h * p).sum()) / q if mask else 0.0)) / n
    return dist, ent, g


@pytest.mark.parametrize("S", SIZES)
def test_closed_form_equals_the_double_sum(S):
    w, z, rays = RO.cases(N_RAYS, S, seed=1)
    ref = RO.evaluate(w, z, rays, 0.7, 0.3)
    assert (np.abs(ref["o"] - RO.THRESHOLD) > RO.MARGIN).all()
    assert ref["mask"].any() and not ref["mask"].all()                   # rays on both sides of the threshold
    dist, ent, g = closed_form(w, z, rays, 0.7, 0.3, RO.THRESHOLD)
    for name, got, want in (("dist", dist, ref["dist"]), ("ent", ent, ref["ent"]), ("g_weights", g, ref["g_weights"])):
        err = RO.rel(got, want)
        print(f"S={S} {name}: closed form vs O(S^2) {err:.3e}")
        assert err <= 1e-12, (S, name, err)
    # per ray too: a one-hot ray has dist = d_j / 3 exactly (A = 0), an all-zero ray and a far == near ray have dist = 0
    assert np.abs(dist - ref["dist"]).max() <= 1e-12 * max(1.0, np.abs(ref["dist"]).max())
    for r in range(N_RAYS):
        if RO.KINDS[r % len(RO.KINDS)] in ("zero", "flat"):
            assert dist[r] == 0.0 and ref["dist"][r] == 0.0
        if RO.KINDS[r % len(RO.KINDS)] == "zero":
            assert ent[r] == 0.0 and not g[r].any()                      # below the threshold: no entropy term, no gradient


def _torch_total(w, z, rays, w_dist, w_ent, threshold):
    """the O(S^2) expression in torch fp64, mask a constant"""
    near, far = rays[:, 6:7], rays[:, 7:8]
    inv = torch.where(far > near, 1.0 / torch.where(far > near, far - near, torch.ones_like(far)), torch.zeros_like(far))
    s = (z - near) * inv
    m = torch.cat([(s[:, :-1] + s[:, 1:]) / 2, s[:, -1:]], 1)
    d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, -1:])], 1)
    dist = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2)) + (w * w * d).sum(1) / 3
    o = w.sum(1)
    p = w / (o + 1e-10)[:, None]
    H = -(p * torch.log(p + 1e-10)).sum(1)
    mask = (o > threshold).detach()
    ent = torch.where(mask, H, torch.zeros_like(H))
    return w_dist * dist.mean() + w_ent * ent.mean(), dist, ent


@pytest.mark.parametrize("S", SIZES)
def test_oracle_gradients_equal_fp64_autograd(S):
    w, z, rays = RO.cases(N_RAYS, S, seed=2)
    for w_dist, w_ent in ((1.0, 0.0), (0.0, 1.0), (0.7, 0.3)):
        ref = RO.evaluate(w, z, rays, w_dist, w_ent)
        wt = torch.from_numpy(w).double().requires_grad_(True)
        total, dist, ent = _torch_total(wt, torch.from_numpy(z).double(), torch.from_numpy(rays).double(), w_dist, w_ent, RO.THRESHOLD)
        total.backward()
        errs = (RO.rel(ref["out"][2], total.item()), RO.rel(ref["dist"], dist.detach().numpy()), RO.rel(ref["ent"], ent.detach().numpy()))
        # The gradient: 1e-10 of its norm, plus 16 fp64 roundings of the operands of the entropy gradient's subtraction (g_cancel).  The
        # second term matters where one sample holds all of a ray's weight -- every ray at S = 1: there dH/dw = h (1 - p) / q with
        # 1 - p ~ 1e-10 / w, a difference of two numbers near 1, so two correct fp64 evaluations (this one and autograd's chain through
        # p) agree to ~1e-16 absolutely and to no more than ~1e-7 of a gradient that is itself ~1e-9.  Elsewhere it is ~1e-15 of the norm.
        want = wt.grad.numpy()
        g_abs = float(np.linalg.norm(ref["g_weights"] - want))
        g_tol = 1e-10 * float(np.linalg.norm(want)) + 16 * 2.0 ** -53 * float(np.linalg.norm(ref["g_cancel"]))
        print(f"S={S} weights ({w_dist}, {w_ent}): gradient |diff| {g_abs:.3e} (relative {RO.rel(ref['g_weights'], want):.3e}, allowed "
              f"{g_tol:.3e}), total {errs[0]:.3e}, dist {errs[1]:.3e}, ent {errs[2]:.3e}")
        assert max(errs) <= 1e-10, (S, w_dist, w_ent, errs)
        assert g_abs <= g_tol, (S, w_dist, w_ent, g_abs, g_tol)


def test_the_oracles_fp32_evaluation_is_an_fp32_evaluation():
    w, z, rays = RO.cases(N_RAYS, 64, seed=3)
    r64, r32 = RO.evaluate(w, z, rays, 0.7, 0.3), RO.evaluate(w, z, rays, 0.7, 0.3, dtype=np.float32)
    assert all(v.dtype == np.float32 for k, v in r32.items() if k != "mask")
    assert (r64["mask"] == r32["mask"]).all()
    for k in ("out", "per_ray", "g_weights"):
        assert 0 < RO.rel(r32[k], r64[k]) < 1e-4, k
        assert RO.bar(r64[k], r32[k]) >= 1e-6


def test_refuses_cpu_tensors_and_bad_shapes():
    from sinnerf_amd import regularizers as RR
    import sinnerf_amd
    assert sinnerf_amd.ray_regularizers is RR.ray_regularizers and sinnerf_amd.distortion_loss is RR.distortion_loss
    assert sinnerf_amd.ray_entropy_loss is RR.ray_entropy_loss
    w, z, rays = (torch.from_numpy(a) for a in RO.cases(3, 5))
    want = re.escape("weights (N, S), z_vals (N, S), rays (N, 8)")
    for fn in (RR.ray_regularizers, RR.distortion_loss, RR.ray_entropy_loss):
        with pytest.raises(RuntimeError, match="no CPU fallback.*expected " + want):
            fn(w, z, rays)
    # the shapes are checked first, so the refusals show without a device
    for bad in ((w, z[:, :4], rays), (w, z, rays[:2]), (w, z, rays[:, :6]), (w[0], z[0], rays), (w[:, :0], z[:, :0], rays),
                (torch.zeros(2, 1025), torch.zeros(2, 1025), torch.zeros(2, 8))):
        with pytest.raises(RuntimeError, match="expected " + want + ".*got weights"):
            RR.ray_regularizers(*bad)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        RR.ray_regularizers(w.numpy(), z, rays)


def test_system_defaults_are_neutral():
    from sinnerf_amd.system import DEFAULT_HPARAMS
    want = dict(distortion_weight=0.0, entropy_weight=0.0, entropy_threshold=0.1)
    assert {k: DEFAULT_HPARAMS[k] for k in want} == want


def test_header_and_binding_declare_the_entries_alike():
    from sinnerf_amd import _lib
    hdr = open(os.path.join(REPO, "include", "sinnerf_hip.h")).read()
    for name in ("sn_ray_regularizers_workspace_bytes", "sn_ray_regularizers"):
        m = re.search(r"\b(?:long|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name + " is not declared in include/sinnerf_hip.h"
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params), name
        assert hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["sn_ray_regularizers"][1]) == 13
