"""GPU: ``sn_ray_regularizers`` (csrc/sn_ray_reg.hip) against the O(S^2) numpy oracle of tests/ray_reg_oracle.py, its NULL outputs,
determinism and refusals, the autograd surface of ``sinnerf_amd.regularizers``, ``render_rays(keep=...)`` and the terms in
``SinNeRFSystem``.

Bars: ``RO.bar(x64, x32) = max(4 e32, 1e-6)``, e32 = the error of the oracle's own fp32 evaluation on the same inputs; a loss value by
relative error, a gradient (and the per-ray vector) by relative L2 norm.  The kernel works in fp64 and rounds once, so it lands at fp32
rounding level (~3e-8), orders of magnitude inside.

End to end (test_parameter_gradients_end_to_end), fp32, 64 rays at 8 + 8: relative L2 over the flat parameter gradient between the
kernel's upstream gradient and the fp64 oracle's cast to fp32.  The bar is 4 x the same figure with the oracle's gradient moved by
one fp32 ulp per element in a random direction -- the sensitivity of the backward to the last bit of its input, which no
implementation of the loss can beat.  The figures are printed; DESIGN.md 3.11 records them."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                                            # noqa: E402
from tests import probe_nets as PN                                                           # noqa: E402
from tests import ray_reg_oracle as RO                                                       # noqa: E402
from tests.test_parity_gpu import dev, embeddings, make_model                                # noqa: E402

# n rays = ceil(n / 4) partial records for the finisher: one, 65, exactly one pass of its 256 threads (1024 rays), a second pass (1027)
SHAPES = [(1, 1), (3, 2), (5, 63), (5, 64), (5, 65), (7, 128), (4, 192), (257, 130), (3, 1023), (2, 1024), (1024, 2), (1027, 65)]
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.7, 0.3)]
BADARG, BADSHAPE = -1, -5
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def inputs(n, S):
    return RO.cases(n, S)


@functools.lru_cache(maxsize=None)
def reference(n, S, w_dist, w_ent):
    """(fp64 evaluation, fp32 evaluation) of the oracle on inputs(n, S): computed once, shared, never modified"""
    w, z, rays = inputs(n, S)
    return RO.evaluate(w, z, rays, w_dist, w_ent), RO.evaluate(w, z, rays, w_dist, w_ent, dtype=np.float32)


def call(w, z, rays, w_dist, w_ent, thr=RO.THRESHOLD, want_g=True, want_per_ray=True, n=None, S=None, null_weights=False):
    """the raw entry on device tensors; every output pre-filled with NaN -> (code, out, per_ray, g_weights)"""
    from sinnerf_amd import _lib
    n = w.shape[0] if n is None else n
    S = w.shape[1] if S is None else S
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev())
    out, per_ray, g = nan(4), (nan(max(n, 1), 2) if want_per_ray else None), (nan(*w.shape) if want_g else None)
    nbytes = _lib.lib.sn_ray_regularizers_workspace_bytes(n)
    assert nbytes >= 24
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    code = _lib.lib.sn_ray_regularizers(None if null_weights else _lib.ptr(w), _lib.ptr(z), _lib.ptr(rays), n, S, w_dist, w_ent, thr,
                                        _lib.ptr(g), _lib.ptr(per_ray), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return code, out, per_ray, g


@pytest.mark.parametrize("w_dist,w_ent", WEIGHTS)
@pytest.mark.parametrize("n,S", SHAPES)
def test_raw_entry_against_the_oracle(n, S, w_dist, w_ent):
    w, z, rays = inputs(n, S)
    r64, r32 = reference(n, S, w_dist, w_ent)
    assert (np.abs(r64["o"] - RO.THRESHOLD) > RO.MARGIN).all()               # every ray: no ray is excluded from a comparison below
    code, out, per_ray, g = call(t(w), t(z), t(rays), w_dist, w_ent)
    assert code == 0
    out, per_ray, g = out.cpu().numpy(), per_ray.cpu().numpy(), g.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(per_ray).all() and np.isfinite(g).all()      # nothing left unwritten
    assert out[3] == r64["mask"].sum()
    rows = [("mean dist", out[0], r64["out"][0], r32["out"][0]), ("mean ent", out[1], r64["out"][1], r32["out"][1]),
            ("total", out[2], r64["out"][2], r32["out"][2]), ("per_ray dist", per_ray[:, 0], r64["dist"], r32["dist"]),
            ("per_ray ent", per_ray[:, 1], r64["ent"], r32["ent"]), ("g_weights", g, r64["g_weights"], r32["g_weights"])]
    figures = [(name, RO.rel(got, x64), RO.rel(x32, x64), RO.bar(x64, x32)) for name, got, x64, x32 in rows]
    for name, err, e32, b in figures:
        print(f"({n}, {S}) w=({w_dist}, {w_ent}) {name}: kernel {err:.3e}, oracle fp32 {e32:.3e}, bar {b:.3e}")
    for name, err, e32, b in figures:
        assert err <= b, (n, S, w_dist, w_ent, name, err, b)


@pytest.mark.parametrize("n,S", [(3, 2), (5, 65), (257, 130), (2, 1024)])
def test_null_outputs_leave_the_others_bit_identical_and_two_calls_agree(n, S):
    w, z, rays = (t(a) for a in inputs(n, S))
    code, out, per_ray, g = call(w, z, rays, 0.7, 0.3)
    assert code == 0
    code2, out2, per_ray2, g2 = call(w, z, rays, 0.7, 0.3)
    assert code2 == 0 and torch.equal(out, out2) and torch.equal(per_ray, per_ray2) and torch.equal(g, g2)
    code3, out3, per_ray3, g3 = call(w, z, rays, 0.7, 0.3, want_g=False)
    assert code3 == 0 and g3 is None and torch.equal(out, out3) and torch.equal(per_ray, per_ray3)
    code4, out4, per_ray4, g4 = call(w, z, rays, 0.7, 0.3, want_per_ray=False)
    assert code4 == 0 and per_ray4 is None and torch.equal(out, out4) and torch.equal(g, g4)
    code5, out5, _, _ = call(w, z, rays, 0.7, 0.3, want_g=False, want_per_ray=False)
    assert code5 == 0 and torch.equal(out, out5)


def test_error_codes():
    w, z, rays = (t(a) for a in inputs(3, 2))
    assert call(w, z, rays, 1.0, 0.0, S=0)[0] == BADSHAPE
    assert call(w, z, rays, 1.0, 0.0, S=1025)[0] == BADSHAPE
    code, out, per_ray, g = call(w, z, rays, 1.0, 0.0, null_weights=True)
    assert code == BADARG
    assert torch.isnan(out).all() and torch.isnan(per_ray).all() and torch.isnan(g).all()      # refused before any launch
    code, out, per_ray, g = call(w, z, rays, 1.0, 1.0, n=0)
    assert code == 0 and not out.any().item() and torch.isnan(g).all()


def test_autograd_hands_out_the_kernels_gradient_bit_for_bit():
    import sinnerf_amd
    w, z, rays = (t(a) for a in inputs(257, 130))
    _, out, per_ray, g = call(w, z, rays, 0.7, 0.3)
    for factor in (1.0, 3.0):
        opacity = w.clone().requires_grad_(True)
        total, stats = sinnerf_amd.ray_regularizers(opacity, z, rays, w_dist=0.7, w_ent=0.3)
        assert not stats["distortion"].requires_grad and not stats["per_ray"].requires_grad
        (factor * total if factor != 1.0 else total).backward()
        assert torch.equal(opacity.grad, factor * g if factor != 1.0 else g)
        assert torch.equal(total.detach(), out[2]) and torch.equal(stats["distortion"], out[0]) and torch.equal(stats["entropy"], out[1])
        assert torch.equal(stats["n_masked"], out[3]) and torch.equal(stats["per_ray"], per_ray)
    # the one-line wrappers, and a call that asks for no gradient
    assert torch.equal(sinnerf_amd.distortion_loss(w, z, rays), call(w, z, rays, 1.0, 0.0)[1][2])
    assert torch.equal(sinnerf_amd.ray_entropy_loss(w, z, rays, 0.1), call(w, z, rays, 0.0, 1.0)[1][2])
    total, stats = sinnerf_amd.ray_regularizers(w[:0], z[:0], rays[:0])
    assert total.item() == 0 and stats["per_ray"].shape == (0, 2)


# ---- render_rays(keep=...) --------------------------------------------------------------------------------------------------------
def probe_models(train=False):
    import sinnerf_amd
    models = []
    for name in ("wide", "low"):
        m = sinnerf_amd.NeRF(use_new_activation=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in PN.head_params(name).items()})
        m = m.to(dev())
        models.append(m.train() if train else m.eval())
    return models


def same_dict(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("perturb", [0.0, 1.0])
def test_render_rays_keep_hands_out_the_depths_the_passes_used(perturb):
    import sinnerf_amd
    from sinnerf_amd import rendering
    models = probe_models()
    rays = t(PN.head_rays()[0][:33])
    args = (models, embeddings(), rays, 8, False, perturb, 0.0, 8, 32768, True)
    render = lambda **kw: sinnerf_amd.render_rays(*args, **kw)
    with torch.no_grad():
        torch.manual_seed(5)
        plain = render()
        torch.manual_seed(5)
        keep = {}
        kept = render(keep=keep)
        after_keep = torch.rand(1, device=dev())
        torch.manual_seed(5)
        render()
        after_plain = torch.rand(1, device=dev())
    same_dict(plain, kept)                                                   # the same keys, the same bits
    assert torch.equal(after_keep, after_plain)                              # the same RNG consumption
    assert sorted(keep) == ["z_vals_coarse", "z_vals_fine"]
    zc, zf = keep["z_vals_coarse"], keep["z_vals_fine"]
    assert zc.shape == (33, 8) and zf.shape == (33, 16) and not zc.requires_grad and not zf.requires_grad
    assert (zf[:, 1:] >= zf[:, :-1]).all() and (zc[:, 1:] >= zc[:, :-1]).all()
    with torch.no_grad():                                                    # re-compositing the handed-out depths: the same weights
        for model, z, key in ((models[1], zf, "opacity_fine"), (models[0], zc, "opacity_coarse")):
            raw = rendering._mlp(model, rays, z, False)                      # sn_mlp_forward
            _, _, weights = rendering._composite(raw, True, z, rays, None, 0.0, True)          # sn_composite_forward, noise_std = 0
            assert torch.equal(weights, plain[key]), key
    # the autograd path against the no-grad path
    torch.manual_seed(5)
    keep_g = {}
    with_grad = sinnerf_amd.render_rays(*args, keep=keep_g)
    assert with_grad["opacity_fine"].requires_grad and with_grad["opacity_coarse"].requires_grad
    same_dict(plain, {k: v.detach() for k, v in with_grad.items()})
    same_dict(keep, keep_g)
    assert not keep_g["z_vals_fine"].requires_grad
    torch.manual_seed(5)
    same_dict(plain, {k: v.detach() for k, v in sinnerf_amd.render_rays(*args).items()})       # keep=None on the autograd path too
    # no fine pass: the coarse depths alone; an empty batch: empty tensors of the right widths
    with torch.no_grad():
        only = {}
        sinnerf_amd.render_rays(models[:1], embeddings(), rays, 8, False, 0.0, 0.0, 0, 32768, True, keep=only)
        assert list(only) == ["z_vals_coarse"] and only["z_vals_coarse"].shape == (33, 8)
        empty = {}
        sinnerf_amd.render_rays(models, embeddings(), rays[:0], 8, False, 0.0, 0.0, 8, 32768, True, keep=empty)
        assert empty["z_vals_coarse"].shape == (0, 8) and empty["z_vals_fine"].shape == (0, 16)


def test_parameter_gradients_end_to_end():
    """figures on the MI355X: see DESIGN.md 3.11"""
    import sinnerf_amd
    mc, _ = make_model(0, True)
    mf, _ = make_model(1, True)
    rays = t(O.lego_rays(400, 400, seed=0)[::2477][:64])
    keep = {}
    res = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 8, False, 0.0, 0.0, 8, 32768, True, keep=keep)
    opacity, z = res["opacity_fine"], keep["z_vals_fine"]
    params = [p for p in mf.parameters()]
    flat = lambda grads: torch.cat([torch.zeros_like(p).reshape(-1) if g is None else g.reshape(-1) for g, p in zip(grads, params)]).double()
    total, _ = sinnerf_amd.ray_regularizers(opacity, z, rays, 0.7, 0.3)
    got = flat(torch.autograd.grad(total, params, retain_graph=True, allow_unused=True))
    r64 = RO.evaluate(opacity.detach().cpu().numpy(), z.cpu().numpy(), rays.cpu().numpy(), 0.7, 0.3)
    assert (np.abs(r64["o"] - RO.THRESHOLD) > RO.MARGIN).all()
    g_oracle = r64["g_weights"].astype(np.float32)
    up = np.random.RandomState(0).randint(0, 2, g_oracle.shape).astype(bool)
    g_moved = np.where(up, np.nextafter(g_oracle, np.float32(np.inf)), np.nextafter(g_oracle, np.float32(-np.inf))).astype(np.float32)
    through = lambda g: flat(torch.autograd.grad(opacity, params, grad_outputs=t(g), retain_graph=True, allow_unused=True))
    want, moved = through(g_oracle), through(g_moved)
    assert want.norm().item() > 0
    err = ((got - want).norm() / want.norm()).item()
    sens = ((moved - want).norm() / want.norm()).item()
    print(f"end to end: kernel vs oracle gradient {err:.3e}; oracle gradient moved by one fp32 ulp per element {sens:.3e}; bar {4 * sens:.3e}")
    assert sens > 0
    assert err <= 4 * sens, (err, sens)


# ---- SinNeRFSystem ----------------------------------------------------------------------------------------------------------------
PATCH = 8


def patch_batch():
    g = torch.Generator().manual_seed(4)
    u = lambda *s: torch.rand(*s, generator=g).to(dev())
    n = PATCH * PATCH
    full, side = O.llff_patch_rays(1, pw=PATCH, ph=PATCH), O.llff_patch_rays(2, pw=PATCH, ph=PATCH)
    return {"rays": t(O.llff_like_rays(n, 0)), "rgbs": u(n, 3), "depth": 1.2 + 6.8 * u(n), "rays_full": t(full), "rgbs_full": u(n, 3),
            "rays_side": t(side), "side_rgb": u(n, 3), "rays_proj": t(O.llff_like_rays(n, 3)), "depth_proj": 1.2 + 6.8 * u(n),
            "real_patch": u(1, 3, PATCH, PATCH)}


def system(seed=3, **hp):
    from sinnerf_amd.system import SinNeRFSystem
    torch.manual_seed(seed)
    sysm = SinNeRFSystem(N_samples=8, N_importance=8, white_back=False, depth_weight=0.5, **hp).to(dev())
    sysm.configure_optimizers()
    return sysm


def step(sysm, batch, seed=100):
    sysm.optimizer.zero_grad()
    torch.manual_seed(seed)
    out = sysm.training_step(batch)
    out["loss"].backward()
    return out, sysm._flat.flat.clone()


def test_system_with_zero_weights_is_the_system_without_the_keys():
    batch = patch_batch()
    out0, g0 = step(system(), batch)
    out1, g1 = step(system(distortion_weight=0.0, entropy_weight=0.0, entropy_threshold=0.1), batch)
    assert torch.equal(out0["loss"], out1["loss"]) and torch.equal(g0, g1) and g0.abs().max().item() > 0
    assert list(out0["log"]) == list(out1["log"])
    assert "train/loss_distortion" not in out0["log"] and "train/loss_ray_entropy" not in out0["log"]


def test_system_adds_the_two_terms_on_the_unseen_view_render():
    import sinnerf_amd
    batch = patch_batch()
    hp = dict(perturb=0.0, noise_std=0.0)                                    # no random draws: the side render can be repeated below
    off, _ = step(system(**hp), batch)
    sysm = system(distortion_weight=0.01, entropy_weight=0.001, **hp)
    on, g_on = step(sysm, batch)
    assert "train/loss_distortion" in on["log"] and "train/loss_ray_entropy" in on["log"]
    keep = {}
    side = sysm(batch["rays_side"], keep=keep)
    assert side["opacity_coarse"].requires_grad                              # so the coarse pass is regularised too
    terms, dist, ent = [], 0.0, 0.0
    for k_w, k_z in (("opacity_fine", "z_vals_fine"), ("opacity_coarse", "z_vals_coarse")):
        term, st = sinnerf_amd.ray_regularizers(side[k_w], keep[k_z], batch["rays_side"], 0.01, 0.001, 0.1)
        terms.append(term.item())
        dist, ent = dist + st["distortion"], ent + st["entropy"]
    assert torch.equal(on["log"]["train/loss_distortion"], dist) and torch.equal(on["log"]["train/loss_ray_entropy"], ent)
    assert dist.item() > 0 and ent.item() > 0
    want = off["loss"].item() + sum(terms)
    # the step adds the same fp32 numbers in another order: at most four roundings of half an ulp of the running sum on either side
    tol = 8 * 2.0 ** -24 * max(abs(want), 1.0)
    print(f"loss with the terms {on['loss'].item():.9g}, zero-weight loss + terms {want:.9g}, terms {terms}, tolerance {tol:.3g}")
    assert abs(on["loss"].item() - want) <= tol
    assert torch.isfinite(g_on).all()


def test_train_step_graph_replays_the_eager_step_with_the_terms_on():
    batch = patch_batch()
    finals = {}
    for graph in (False, True):
        sysm = system(seed=0, perturb=0.0, noise_std=0.0, distortion_weight=0.01, entropy_weight=0.001, lr=5e-4)
        losses = []
        for _ in range(3):                                                   # with graph=True: the capture, then two replays
            out = sysm.train_step(batch, graph=graph)
            losses.append(out["loss"].item())
            assert "train/loss_distortion" in out["log"]
        finals[graph] = (sysm.optimizer.flat.clone(), losses)
        if graph:
            assert len(sysm._step_graphs) == 1
    assert finals[True][1] == finals[False][1], (finals[True][1], finals[False][1])
    assert torch.equal(finals[True][0], finals[False][0])
    assert len(set(finals[True][1])) == 3                                    # the parameters moved between the replays


def test_train_step_sampled_graph_with_the_terms_on():
    from tests.test_sampler_gpu import make_sampler
    sysm = system(seed=19, proj_weight=0.6, distortion_weight=0.01, entropy_weight=0.001)
    s = make_sampler(num=256)
    before = sysm.optimizer.flat.clone()
    for _ in range(3):
        out = sysm.train_step_sampled(s, graph=True)
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]) and torch.isfinite(out["log"]["train/loss_distortion"])
        assert torch.isfinite(out["log"]["train/loss_ray_entropy"])
    assert len(sysm._step_graphs) == 1
    assert not torch.equal(before, sysm.optimizer.flat) and torch.isfinite(sysm.optimizer.flat).all()
