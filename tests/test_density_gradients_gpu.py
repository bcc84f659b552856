"""GPU, end to end: ``sinnerf_amd.density_gradients`` / ``ray_density_gradients`` / ``render_normals`` against the density gradients
of the reference's own autograd (tools/gen_point_grad_golden.py -> tests/golden/grad_points_*.npz).

Rounding (the reference's own fp32 sits at e_p ~ 4e-7 of its float64 run on these points) is far from a wiring mistake (wrong slot,
sign, band scale or axis: O(1)), so the bar is the project's fp32 gradient floor of 1e-3 (tests/test_ray_grads_gpu.py), per point
and norm-wise; a ReLU mask that flips on a last-bit difference puts a point far outside, and at most 2 % of the 300 points may sit
there (6 flips; the fixture's own fp32 run has at most 0.5 %, asserted by its generator).  The errors are printed (run with -s)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                                        # noqa: E402
from tests import point_grad_oracle as PG                                                # noqa: E402
from tests.test_parity_gpu import dev, embeddings, make_model                            # noqa: E402
from tests.test_point_grads_cpu import POINT_CASES, load_point_case, point_case_params   # noqa: E402
from tests.test_point_grads_gpu import check_wsum                                        # noqa: E402


def case_model(name, dtype):
    z = load_point_case(name)
    if str(z["meta_weights"]) == "trained_student":
        from tests.test_trained_weights_gpu import trained_models
        return trained_models(dtype)[1]
    return make_model(int(z["meta_seed"]), True, dtype)[0]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Untouched:
    """no parameter .grad appears and no requires_grad flag moves while the block runs"""

    def __init__(self, *models):
        self.models = models

    def __enter__(self):
        self.flags = [[p.requires_grad for p in m.parameters()] for m in self.models]
        assert all(p.grad is None for m in self.models for p in m.parameters())

    def __exit__(self, *exc):
        if exc[0] is None:
            assert all(p.grad is None for m in self.models for p in m.parameters())
            assert self.flags == [[p.requires_grad for p in m.parameters()] for m in self.models]


def check_against_fixture(tag, sigma, g, z, ref=None, sigma_ref=None):
    """the bars of this file's docstring for gradients g (300, 3) and raw sigma (300, 1) at the fixture's points"""
    ref = z["g64"] if ref is None else ref
    sigma_ref = z["sigma"] if sigma_ref is None else sigma_ref
    assert g.shape == (300, 3) and np.isfinite(g).all() and sigma.shape == (300, 1)
    e = PG.point_err(g, ref)
    bar = max(3 * float(z["spread_median"]), 1e-3)
    out = e > bar
    keep = ~out
    norm = float(np.linalg.norm(g[keep] - ref[keep]) / np.linalg.norm(ref[keep]))
    ds = float((np.abs(sigma - sigma_ref) / np.maximum(1.0, np.abs(sigma_ref))).max())
    print(f"{tag}: e_p median {np.median(e):.3e} max {e.max():.3e} (reference fp32: median {float(z['spread_median']):.3e} max "
          f"{float(z['spread_max']):.3e}) | outside {int(out.sum())}/300 | norm-wise over the rest {norm:.3e} | sigma {ds:.3e}")
    assert out.mean() <= 0.02, (tag, int(out.sum()))
    assert norm <= 1e-3, (tag, norm)
    assert ds <= 2e-4, (tag, ds)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", POINT_CASES)
def test_density_gradients_golden(name, dtype):
    import sinnerf_amd
    z = load_point_case(name)
    model = case_model(name, dtype)
    pts = t(z["points"])
    with Untouched(model):
        sigma, g = sinnerf_amd.density_gradients(pts, model)
        assert not sigma.requires_grad and not g.requires_grad and tuple(sigma.shape) == (300, 1) and tuple(g.shape) == (300, 3)
        again = sinnerf_amd.density_gradients(pts, model)
    assert torch.equal(g, again[1]) and torch.equal(sigma, again[0])
    check_against_fixture(f"density_gradients {name} {dtype}", sigma.cpu().numpy(), g.cpu().numpy().astype(np.float64), z)
    if dtype == "fp32":                                       # the raw sigma eval_points returns, from the training forward
        with torch.no_grad():
            s_eval = sinnerf_amd.eval_points(pts, [model], embeddings())
        assert (s_eval - sigma).abs().max().item() <= 2e-4 * max(1.0, s_eval.abs().max().item())


@pytest.mark.parametrize("name", POINT_CASES)
def test_bf16_density_gradients_finite(name):
    """mixed precision: bf16 activations under a 2^9 derivative factor have no derivable bar -- the error is printed, not asserted
    (the bf16 state layout is covered exactly by tests/test_point_grads_gpu.py)"""
    import sinnerf_amd
    z = load_point_case(name)
    model = case_model(name, "bf16")
    with Untouched(model):
        sigma, g = sinnerf_amd.density_gradients(t(z["points"]), model)
    assert tuple(g.shape) == (300, 3) and torch.isfinite(g).all() and torch.isfinite(sigma).all()
    e = PG.point_err(g.cpu().numpy(), z["g64"])
    print(f"density_gradients {name} bf16: e_p median {np.median(e):.3e} max {e.max():.3e} | sigma "
          f"{float(np.abs(sigma.cpu().numpy() - z['sigma']).max()):.3e}")


@functools.lru_cache(maxsize=None)
def second_sample_reference(name):
    """float64 helper values (pinned to the reference by tests/test_point_grads_cpu.py) at the second sample of every ray below"""
    z = load_point_case(name)
    rays, zz = fixture_rays(name)
    pts = O._points(rays, zz)[:, 1]
    sigma, g = PG.sigma_grads(point_case_params(z), pts, wide=True)
    return pts, sigma, g


def fixture_rays(name):
    """300 rays with d = (0, 0, 1) and two samples: sample 0 lands on the fixture's point bit for bit (o_z = p_z - z0 is exact for z0 =
    p_z rounded to 1/256, and so is o_z + z0), sample 1 half a unit further along the ray"""
    p = load_point_case(name)["points"]
    z0 = (np.round(p[:, 2].astype(np.float64) * 256) / 256).astype(np.float32)
    rays = np.zeros((300, 8), np.float32)
    rays[:, 0:2], rays[:, 2], rays[:, 5] = p[:, 0:2], p[:, 2] - z0, 1.0
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    zz = np.stack([z0, z0 + np.float32(0.5)], 1).astype(np.float32)
    assert np.array_equal(O._points(rays, zz)[:, 0], p)
    return rays, zz


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", POINT_CASES)
def test_ray_density_gradients_golden(name, dtype):
    import sinnerf_amd
    z = load_point_case(name)
    model = case_model(name, dtype)
    rays, zz = fixture_rays(name)
    w = np.random.RandomState(5).uniform(0, 1, zz.shape).astype(np.float32)
    with Untouched(model):
        g, g_sum = sinnerf_amd.ray_density_gradients(model, t(rays), t(zz), t(w))
        alone = sinnerf_amd.ray_density_gradients(model, t(rays), t(zz))
    assert tuple(g.shape) == (300, 2, 3) and tuple(g_sum.shape) == (300, 3) and not g.requires_grad and not g_sum.requires_grad
    assert torch.equal(alone, g)
    gn = g.cpu().numpy()
    sigma = sinnerf_amd.density_gradients(t(z["points"]), model)[0].cpu().numpy()
    check_against_fixture(f"ray_density_gradients {name} {dtype} sample 0", sigma, gn[:, 0].astype(np.float64), z)
    pts1, sigma1, g1 = second_sample_reference(name)
    s1 = sinnerf_amd.density_gradients(t(pts1), model)[0].cpu().numpy()
    check_against_fixture(f"ray_density_gradients {name} {dtype} sample 1", s1, gn[:, 1].astype(np.float64), z, ref=g1, sigma_ref=sigma1)
    g4 = np.concatenate([gn, np.zeros((300, 2, 1), np.float32)], -1).reshape(-1, 4)
    check_wsum(np.concatenate([g_sum.cpu().numpy(), np.zeros((300, 1), np.float32)], 1), g4, w, f"grad_sum {name} {dtype}")


@functools.lru_cache(maxsize=None)
def normals_run(n_importance, max_points=None):
    import sinnerf_amd
    from tests.test_trained_weights_gpu import trained_models
    models = trained_models("fp32")
    rays = t(O.lego_rays(400, 400, seed=0)[::4001][:37])
    assert rays.shape[0] == 37
    keep = {}
    kw = {} if max_points is None else {"max_points": max_points}
    with Untouched(*models):
        res = sinnerf_amd.render_normals(models, embeddings(), rays, 64, False, n_importance, True, keep=keep, **kw)
    return models, rays, res, keep


@pytest.mark.parametrize("n_importance", [64, 0])
def test_render_normals(n_importance):
    import sinnerf_amd
    models, rays, res, keep = normals_run(n_importance)
    S = 64 + n_importance
    with torch.no_grad():
        plain = sinnerf_amd.render_rays(models, embeddings(), rays, 64, False, 0, 0, n_importance, 32768, True)
    assert set(res) == set(plain) | {"grad_fine", "normal_fine"}
    for k, v in plain.items():
        assert torch.equal(res[k], v), k
    assert not any(v.requires_grad for v in res.values())
    gf, nf = res["grad_fine"], res["normal_fine"]
    assert tuple(gf.shape) == (37, 3) and tuple(nf.shape) == (37, 3) and tuple(keep["grad_samples"].shape) == (37, S, 3)
    assert torch.isfinite(gf).all() and torch.isfinite(nf).all()
    # grad_fine = sum_i w_i grad sigma_i over the pass that produced opacity_fine, from the function's own per-sample gradients
    gs = keep["grad_samples"].cpu().numpy()
    g4 = np.concatenate([gs, np.zeros((37, S, 1), np.float32)], -1).reshape(-1, 4)
    w = res["opacity_fine"].cpu().numpy()
    assert np.abs(w).max() > 0 and np.abs(gs).max() > 0
    check_wsum(np.concatenate([gf.cpu().numpy(), np.zeros((37, 1), np.float32)], 1), g4, w, f"grad_fine S={S}")
    # ... which are the gradients of that pass's model at that pass's depths
    direct = sinnerf_amd.ray_density_gradients(models[1 if n_importance else 0], rays, keep["z_vals"], res["opacity_fine"])
    assert torch.equal(direct[0], keep["grad_samples"]) and torch.equal(direct[1], gf)
    # normal_fine = -grad_fine / max(||grad_fine||, 1e-12), to 4 ulp
    g = gf.cpu().numpy().astype(np.float64)
    want = -g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(nf.cpu().numpy().astype(np.float64) - want) <= 4 * ulp).all()
    assert np.abs(np.linalg.norm(nf.cpu().numpy().astype(np.float64), axis=1) - 1).max() <= 1e-6
    # rays are independent: chunks of 7 rays (64 + 64 samples) give the same bits as one chunk
    _, _, small, keep_small = normals_run(n_importance, 7 * 128)
    for k in res:
        assert torch.equal(res[k], small[k]), k
    assert torch.equal(keep["grad_samples"], keep_small["grad_samples"]) and torch.equal(keep["z_vals"], keep_small["z_vals"])


def test_zero_gradient_gives_a_zero_normal():
    """a network whose sigma does not depend on the position: grad_fine = 0 and the 1e-12 floor keeps the normal finite (zero)"""
    import sinnerf_amd
    mc, _ = make_model(0, True)
    with torch.no_grad():
        mc.sigma.weight.zero_()
    rays = t(O.lego_rays(20, 20, seed=0)[:5])
    res = sinnerf_amd.render_normals([mc], embeddings(), rays, 16)
    assert (res["grad_fine"] == 0).all() and (res["normal_fine"] == 0).all()


def test_refusals():
    import sinnerf_amd
    m16, _ = make_model(0, True, "fp16")
    m32, _ = make_model(0, True)
    rays = t(O.lego_rays(20, 20, seed=0)[:8])
    zz = t(np.tile(np.linspace(2, 6, 4, dtype=np.float32), (8, 1)))
    pts = rays[:, :3].contiguous()
    with Untouched(m16, m32):
        with pytest.raises(NotImplementedError, match="INFERENCE arithmetic"):
            sinnerf_amd.density_gradients(pts, m16)
        with pytest.raises(NotImplementedError, match="INFERENCE arithmetic"):
            sinnerf_amd.ray_density_gradients(m16, rays, zz)
        with pytest.raises(NotImplementedError, match="INFERENCE arithmetic"):
            sinnerf_amd.render_normals([m32, m16], embeddings(), rays, 16, False, 16)
        with pytest.raises(RuntimeError):
            sinnerf_amd.density_gradients(pts.cpu(), m32)
        with pytest.raises(RuntimeError):
            sinnerf_amd.ray_density_gradients(m32, rays.cpu(), zz)
        with pytest.raises(RuntimeError):
            sinnerf_amd.ray_density_gradients(m32, rays, zz.cpu())
        with pytest.raises(RuntimeError):
            sinnerf_amd.ray_density_gradients(m32, rays, zz, zz.cpu())
        with pytest.raises(RuntimeError):
            sinnerf_amd.render_normals([m32], embeddings(), rays.cpu(), 16)
        # NeRF.forward still refuses a gradient with respect to its embedded input
        x = embeddings()[0](pts).requires_grad_(True)
        with pytest.raises(NotImplementedError):
            m32(x, sigma_only=True)
        assert tuple(sinnerf_amd.density_gradients(pts[:0], m32)[1].shape) == (0, 3)
        assert tuple(sinnerf_amd.ray_density_gradients(m32, rays[:0], zz[:0]).shape) == (0, 4, 3)
        assert tuple(sinnerf_amd.render_normals([m32], embeddings(), rays[:0], 16)["normal_fine"].shape) == (0, 3)
