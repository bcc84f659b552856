"""GPU: pose gradients -- ``sn_ray_grads``, ``sn_composite_backward_rays``, ``sn_generate_rays_backward`` against float64
restatements (tests/ray_grad_oracle.py, pinned to the reference by tests/test_ray_grads_cpu.py), and ``render_rays`` /
``get_rays`` under autograd against ray gradients of the reference's own autograd (tools/gen_ray_grad_golden.py).

The end-to-end tests print their measured errors (run with -s); DESIGN.md §3.5 records them."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                                        # noqa: E402
from tests import ray_grad_oracle as R                                                   # noqa: E402
from tests.helpers import x3_state_decode, x3_state_encode                               # noqa: E402
from tests.test_parity_gpu import dev, embeddings, injected_rng, make_model, rng_order   # noqa: E402
from tests.test_ray_grads_cpu import load_ray_case                                       # noqa: E402

CASES = ["grad_rays_lego_train", "grad_rays_lego_det", "grad_rays_trained_det"]
# |got - ref| <= BOUND * A, A = the same computation with every factor replaced by its absolute value: gamma_n A with
# n ~ 512 + 20 + S fp32 accumulation steps (k, embedding terms, samples) -> 800 * 2^-24 = 4.8e-5, valid for ANY summation order
BOUND = 5e-5


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return x if dtype is None else x.to(dtype)


def call_ray_grads(w1, w5, wdir, G, code, rays, z):
    """sn_ray_grads through ctypes: numpy weights / rays / z, G = device tensor in the layout `code` names -> (n, 8) numpy"""
    from sinnerf_amd import _lib as L
    n, S = z.shape
    ws = torch.empty(int(L.lib.sn_ray_grads_workspace_bytes(n, S)), dtype=torch.uint8, device=dev())
    out = torch.full((n, 8), float("nan"), dtype=torch.float32, device=dev())
    w1t, w5t, wdt, rt, zt = t(w1, torch.float32), t(w5, torch.float32), t(wdir, torch.float32), t(rays), t(z)
    L.check(L.lib.sn_ray_grads(L.ptr(w1t), L.ptr(w5t), L.ptr(wdt), code, L.ptr(G), G.shape[1], L.ptr(rt), L.ptr(zt), n, S,
                               L.ptr(ws), L.ptr(out), L.stream_ptr()), "sn_ray_grads")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def make_inputs(n, S, seed):
    r = np.random.RandomState(seed)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = r.uniform(-3, 3, (n, 3))
    rays[:, 3:6] = r.uniform(-1, 1, (n, 3)) * r.uniform(0.5, 1.6, (n, 1))                # non-unit directions
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    z = np.sort(r.uniform(2, 6, (n, S)).astype(np.float32), -1)
    P = n * S
    rows = -(-P // 128) * 128
    G = np.full((10, rows, 256), np.nan, np.float32)                                      # pad rows NaN: they must never be read
    G[:, :P] = r.standard_normal((10, P, 256)).astype(np.float32)
    return rays, z, G, P


def check_bound(got, ref, A, tag):
    assert np.isfinite(got).all(), tag
    err = np.abs(got[:, :6] - ref[:, :6])
    worst = float((err / (BOUND * A[:, :6] + 1e-300)).max())
    print(tag, "max err / (5e-5 A) =", worst)
    assert worst <= 1.0, (tag, worst)
    assert (got[:, 6:] == 0).all(), tag


@functools.lru_cache(maxsize=None)
def weights3():
    _, p = make_model(3, True)
    return p["xyz_encoding_1.0.weight"], p["xyz_encoding_5.0.weight"], p["dir_encoding.0.weight"]


@pytest.mark.parametrize("n,S", [(5, 37), (3, 192), (1, 1), (7, 64), (2, 1024)])
def test_ray_grads_dense_vs_float64(n, S):
    from sinnerf_amd import _lib as L
    w1, w5, wd = weights3()
    rays, z, G, P = make_inputs(n, S, 100 + S)
    Gt = t(G)
    got = call_ray_grads(w1, w5, wd, Gt, L.SN_DTYPE_F32, rays, z)
    ref = R.ray_grads_mlp(G[0, :P], G[4, :P], G[9, :P], w1, w5, wd, rays, z)
    A = R.ray_grads_mlp(G[0, :P], G[4, :P], G[9, :P], w1, w5, wd, rays, z, abs_bound=True)
    check_bound(got, ref, A, f"dense ({n},{S})")
    again = call_ray_grads(w1, w5, wd, Gt, L.SN_DTYPE_F32, rays, z)
    assert got.tobytes() == again.tobytes()                                               # fixed summation order, no atomics
    assert np.array_equal(got, call_ray_grads(w1, w5, wd, Gt, L.SN_DTYPE_BF16, rays, z))  # fp32 state, bf16-operand chain


def test_ray_grads_one_embedding_column_at_a_time():
    """A / |ref| of the dense test is large (the 2^9 band dominates): a wrong identity or low-band column would hide there.
    One-hot weights isolate column order, band scale and the sin / cos sign of every column."""
    from sinnerf_amd import _lib as L
    n, S = 5, 37
    rays, z, G, P = make_inputs(n, S, 7)
    xyz_cols, dir_cols = [0, 1, 2, 3, 5, 6, 8, 57, 59, 60, 62], [0, 2, 3, 8, 21, 26]
    for which, cols in (("w1", xyz_cols), ("w5", xyz_cols), ("wdir", dir_cols)):
        slot = {"w1": 0, "w5": 4, "wdir": 9}[which]
        Gs = np.zeros_like(G)
        Gs[:, P:] = np.nan
        Gs[slot, :P, 0] = G[slot, :P, 0]
        Gt = t(Gs)
        for c in cols:
            w1, w5, wd = np.zeros((256, 63), np.float32), np.zeros((256, 319), np.float32), np.zeros((128, 283), np.float32)
            {"w1": w1, "w5": w5, "wdir": wd}[which][0, c + (256 if which == "wdir" else 0)] = 1.0
            got = call_ray_grads(w1, w5, wd, Gt, L.SN_DTYPE_F32, rays, z)
            ref = R.ray_grads_mlp(Gs[0, :P], Gs[4, :P], Gs[9, :P], w1, w5, wd, rays, z)
            A = R.ray_grads_mlp(Gs[0, :P], Gs[4, :P], Gs[9, :P], w1, w5, wd, rays, z, abs_bound=True)
            assert np.abs(ref).max() > 0
            assert np.isfinite(got).all()
            err = np.abs(got - ref)
            assert (err <= BOUND * A).all(), (which, c, float((err / (BOUND * A + 1e-300)).max()))


def test_ray_grads_state_layouts():
    """the same values stored as bf16 rows / as the (hi, lo) pairs of the bf16x3 state; reference from the DECODED values"""
    from sinnerf_amd import _lib as L
    w1, w5, wd = weights3()
    n, S = 5, 37
    rays, z, G, P = make_inputs(n, S, 11)
    # bf16 rows
    G16 = t(G).to(torch.bfloat16)
    dec = G16.float().cpu().numpy()
    got = call_ray_grads(w1, w5, wd, G16, L.SN_DTYPE_BF16_STATE, rays, z)
    args = (dec[0, :P], dec[4, :P], dec[9, :P], w1, w5, wd, rays, z)
    check_bound(got, R.ray_grads_mlp(*args), R.ray_grads_mlp(*args, abs_bound=True), "bf16 rows")
    # bf16x3 state: slots 0..8 as (hi, lo) pairs, slot 9 fp32
    fin = np.where(np.isfinite(G), G, 0.0).astype(np.float32)
    Gx = np.array(G, copy=True)
    Gx[:9] = x3_state_encode(fin[:9])
    dec = np.array(fin, copy=True)
    dec[:9] = x3_state_decode(Gx[:9])
    Gx[:, P:] = np.nan
    Gx[:9, P:] = np.full(1, 0x7FC07FC0, np.uint32).view(np.float32)[0]                    # two bf16 NaNs per word in the pad rows
    got = call_ray_grads(w1, w5, wd, t(Gx), L.SN_DTYPE_BF16X3, rays, z)
    args = (dec[0, :P], dec[4, :P], dec[9, :P], w1, w5, wd, rays, z)
    check_bound(got, R.ray_grads_mlp(*args), R.ray_grads_mlp(*args, abs_bound=True), "bf16x3 state")
    # anything else, flag bits included, is refused
    for code in (L.SN_DTYPE_F16, L.SN_DTYPE_F32 | L.SN_DTYPE_CLASSIC_HEADS, L.SN_DTYPE_BF16_STATE | L.SN_DTYPE_EMB_BF16, 7):
        with pytest.raises(L.SinnerfHipError):
            call_ray_grads(w1, w5, wd, t(G), code, rays, z)


@pytest.mark.parametrize("S,white_back,noise_std,with_gw", [(64, True, 1.0, False), (128, False, 0.0, True),
                                                            (192, True, 0.5, True), (24, False, 1.0, False)])
def test_composite_backward_rays(S, white_back, noise_std, with_gw):
    from sinnerf_amd import _lib as L
    r = np.random.RandomState(S)
    rays = O.lego_rays(30, 30, seed=2)[::9]
    n = rays.shape[0]
    z = np.sort(r.uniform(2, 6, (n, S)).astype(np.float32), -1)
    raw = r.uniform(0, 1, (n, S, 4)).astype(np.float32)
    raw[..., 3] = (r.standard_normal((n, S)) * 2).astype(np.float32)
    noise = r.standard_normal((n, S)).astype(np.float32)
    g_rgb, g_depth = r.standard_normal((n, 3)).astype(np.float32), r.standard_normal(n).astype(np.float32)
    g_w = r.standard_normal((n, S)).astype(np.float32) if with_gw else None
    ref = R.composite_dir_grad(raw, z, rays[:, 3:6], noise if noise_std else None, noise_std, white_back, g_rgb, g_depth, g_w)
    args = [t(raw), t(z), t(rays), t(noise) if noise_std else None]
    ups = [t(g_rgb), t(g_depth), t(g_w) if with_gw else None]
    g_raw0 = torch.empty((n, S, 4), dtype=torch.float32, device=dev())
    g_raw1 = torch.empty_like(g_raw0)
    g_rays = torch.full((n, 8), float("nan"), dtype=torch.float32, device=dev())
    p = [L.ptr(a) for a in args]
    u = [L.ptr(a) for a in ups]
    L.check(L.lib.sn_composite_backward(p[0], p[1], p[2], p[3], noise_std, n, S, int(white_back), u[0], u[1], u[2], L.ptr(g_raw0),
                                        L.stream_ptr()), "sn_composite_backward")
    L.check(L.lib.sn_composite_backward_rays(p[0], p[1], p[2], p[3], noise_std, n, S, int(white_back), u[0], u[1], u[2],
                                             L.ptr(g_raw1), L.ptr(g_rays), L.stream_ptr()), "sn_composite_backward_rays")
    assert torch.equal(g_raw0, g_raw1)
    got = g_rays.cpu().numpy()
    assert (got[:, :3] == 0).all() and (got[:, 6:] == 0).all()
    scale = np.abs(ref).max()
    assert scale > 0
    assert np.abs(got[:, 3:6] - ref).max() <= 2e-5 * scale, (np.abs(got[:, 3:6] - ref).max(), scale)


def test_composite_backward_rays_zero_direction():
    from sinnerf_amd import _lib as L
    n, S = 2, 8
    rays = np.zeros((n, 8), np.float32)
    rays[1, 3:6] = (0.3, -0.2, 0.9)
    z = np.tile(np.linspace(2, 6, S, dtype=np.float32), (n, 1))
    raw = np.full((n, S, 4), 0.5, np.float32)
    g_raw = torch.empty((n, S, 4), dtype=torch.float32, device=dev())
    g_rays = torch.full((n, 8), float("nan"), dtype=torch.float32, device=dev())
    L.check(L.lib.sn_composite_backward_rays(L.ptr(t(raw)), L.ptr(t(z)), L.ptr(t(rays)), None, 0.0, n, S, 0, L.ptr(t(np.ones((n, 3), np.float32))),
                                             None, None, L.ptr(g_raw), L.ptr(g_rays), L.stream_ptr()), "sn_composite_backward_rays")
    got = g_rays.cpu().numpy()
    assert (got[0] == 0).all() and np.isfinite(got).all() and np.abs(got[1, 3:6]).max() > 0


# ---- end to end --------------------------------------------------------------------------------------------------
def case_models(name, meta, dtype):
    if meta["weights"] == "trained_student":
        from tests.test_trained_weights_gpu import trained_models
        return trained_models(dtype, train=True)
    mc, _ = make_model(meta["seed_coarse"], True, dtype)
    mf, _ = make_model(meta["seed_fine"], True, dtype)
    return [mc.train(), mf.train()]


@functools.lru_cache(maxsize=None)
def end_to_end(name, dtype, rays_grad, frozen=False):
    """one forward + backward of the fixture's linear loss through sinnerf_amd.render_rays; computed once per configuration"""
    import sinnerf_amd
    z, meta, rng, coef = load_ray_case(name)
    models = case_models(name, meta, dtype)
    if frozen:
        for m in models:
            for p in m.parameters():
                p.requires_grad_(False)
    rays = torch.from_numpy(z["rays"]).to(dev())
    if rays_grad:
        rays.requires_grad_()
    with injected_rng(rng_order(dict(meta, use_disp=0), rng, rays.shape[0])) as left:
        res = sinnerf_amd.render_rays(models, embeddings(), rays, meta["N_samples"], False, meta["perturb"], meta["noise_std"],
                                      meta["N_importance"], 32768, bool(meta["white_back"]))
        assert not left
    loss = sum((res[k] * torch.from_numpy(v).to(dev())).sum() for k, v in coef.items())
    loss.backward()
    return dict(loss=loss.item(), rays_grad=None if rays.grad is None else rays.grad.clone(),
                param_grads=[None if p.grad is None else p.grad.clone() for m in models for p in m.parameters()])


def ray_errors(z, g):
    g = g.cpu().numpy()
    return (R.norm_err(g[:, 0:3], z["g_o64"]), R.norm_err(g[:, 3:6], z["g_d64"]),
            R.median_ray_err(g[:, 0:3], z["g_o64"]), R.median_ray_err(g[:, 3:6], z["g_d64"]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", CASES)
def test_render_rays_ray_gradients_golden(name, dtype):
    """The yardstick is the reference's own fp32-vs-fp64 disagreement on these very inputs (the fixture's spreads): the GPU
    differs from the reference by the same kind of last-bit perturbation (ReLU masks, sample bins); 3x because one extra mask
    flip among ~100 rays moves the norm by about that much."""
    z = load_ray_case(name)[0]
    run = end_to_end(name, dtype, True)
    assert abs(run["loss"] - float(z["loss"])) <= 2e-4 * max(1.0, abs(float(z["loss"])))
    g = run["rays_grad"]
    assert g is not None and tuple(g.shape) == (z["rays"].shape[0], 8) and torch.isfinite(g).all()
    assert (g[:, 6:] == 0).all()
    e_o, e_d, m_o, m_d = ray_errors(z, g)
    print(f"{name} {dtype}: norm-wise g_o {e_o:.3e} (spread {float(z['spread_o']):.3e}) g_d {e_d:.3e} (spread {float(z['spread_d']):.3e}) "
          f"| per-ray median g_o {m_o:.3e} ({float(z['spread_med_o']):.3e}) g_d {m_d:.3e} ({float(z['spread_med_d']):.3e})")
    assert e_o <= max(3 * float(z["spread_o"]), 1e-3), e_o
    assert e_d <= max(3 * float(z["spread_d"]), 1e-3), e_d
    assert m_o <= 3 * float(z["spread_med_o"]), m_o
    assert m_d <= 3 * float(z["spread_med_d"]), m_d
    # asking for the ray gradient does not move a bit of the parameter gradients
    plain = end_to_end(name, dtype, False)
    assert plain["rays_grad"] is None
    assert all(torch.equal(a, b) for a, b in zip(run["param_grads"], plain["param_grads"]))


@pytest.mark.parametrize("name", CASES)
def test_bf16_ray_gradients_finite(name):
    """mixed precision: bf16 activations under a 2^9 derivative factor have no derivable bar -- the error is printed, not
    asserted (its state layout is covered exactly by test_ray_grads_state_layouts)"""
    z = load_ray_case(name)[0]
    g = end_to_end(name, "bf16", True)["rays_grad"]
    assert g is not None and tuple(g.shape) == (z["rays"].shape[0], 8) and torch.isfinite(g).all()
    assert (g[:, 6:] == 0).all()
    e_o, e_d, m_o, m_d = ray_errors(z, g)
    print(f"{name} bf16: norm-wise g_o {e_o:.3e} g_d {e_d:.3e} | per-ray median g_o {m_o:.3e} g_d {m_d:.3e}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_frozen_network_ray_gradients(dtype):
    import sinnerf_amd
    name = "grad_rays_lego_train"
    run = end_to_end(name, dtype, True, True)
    assert torch.equal(run["rays_grad"], end_to_end(name, dtype, True)["rays_grad"])
    assert all(g is None for g in run["param_grads"])
    z, meta, rng, coef = load_ray_case(name)
    models = case_models(name, meta, dtype)
    rays = torch.from_numpy(z["rays"]).to(dev()).requires_grad_()
    with torch.no_grad():
        res = sinnerf_amd.render_rays(models, embeddings(), rays, 64, False, 0, 0, 64, 32768, True)
    assert not any(v.requires_grad for v in res.values())


def test_fp16_still_refuses_to_train():
    import sinnerf_amd
    mc, _ = make_model(0, True, "fp16")
    rays = torch.from_numpy(O.lego_rays(20, 20, seed=0)[:8]).to(dev()).requires_grad_()
    with pytest.raises(NotImplementedError):
        sinnerf_amd.render_rays([mc, mc], embeddings(), rays, 64, False, 0, 0, 64, 32768, True)


# ---- get_rays ----------------------------------------------------------------------------------------------------
def lego_pose(seed=0):
    r = np.random.RandomState(1000 + seed)
    th, ph = r.uniform(0, 2 * np.pi), r.uniform(0.15, 0.45) * np.pi
    return O._look_at_c2w(4.0 * np.array([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)])).astype(np.float32)


@pytest.mark.parametrize("window", [None, (3, 2, 4, 3, 9, 7)])
def test_get_rays_backward(window):
    from sinnerf_amd import _lib as L
    from sinnerf_amd.ray_utils import get_rays
    H, W, focal = 30, 40, 37.5
    x0, y0, sx, sy, pw, ph = window if window is not None else (0, 0, 1, 1, W, H)
    n = pw * ph
    c2w_np = lego_pose(3)
    U = np.random.RandomState(5).standard_normal((n, 6)).astype(np.float32)
    grads = []
    for _ in range(2):
        c2w = t(c2w_np).requires_grad_()
        rays = get_rays(H, W, focal, c2w, 2.0, 6.0, window)
        assert rays.requires_grad
        (rays[:, :6] * t(U)).sum().backward()
        grads.append(c2w.grad.clone())
    assert torch.equal(grads[0], grads[1])
    # without requires_grad: today's code path, the same rays bit for bit
    plain = get_rays(H, W, focal, t(c2w_np), 2.0, 6.0, window)
    assert not plain.requires_grad and torch.equal(plain, rays.detach())
    direct = torch.empty((n, 8), dtype=torch.float32, device=dev())
    L.check(L.lib.sn_generate_rays(L.ptr(t(c2w_np)), H, W, focal, 2.0, 6.0, x0, y0, sx, sy, pw, ph, L.ptr(direct), L.stream_ptr()),
            "sn_generate_rays")
    assert torch.equal(plain, direct)
    with torch.no_grad():
        assert not get_rays(H, W, focal, t(c2w_np).requires_grad_(), 2.0, 6.0, window).requires_grad
    # float64 restatement (ray_utils.py:89-91, :109, :112)
    iy, ix = np.divmod(np.arange(n), pw)
    xs, ys = (x0 + ix * sx).astype(np.float64), (y0 + iy * sy).astype(np.float64)
    dirs = np.stack([(xs - W / 2) / focal, -(ys - H / 2) / focal, -np.ones(n)], -1)
    U8 = U.astype(np.float64)
    ref, mag = np.zeros((3, 4)), np.zeros((3, 4))
    ref[:, :3], mag[:, :3] = U8[:, 3:6].T @ dirs, np.abs(U8[:, 3:6]).T @ np.abs(dirs)
    ref[:, 3], mag[:, 3] = U8[:, 0:3].sum(0), np.abs(U8[:, 0:3]).sum(0)
    got = grads[0].cpu().numpy().astype(np.float64)
    assert (np.abs(got - ref) <= 1e-5 * mag).all(), float((np.abs(got - ref) / mag).max())


def test_pose_optimisation_reduces_loss():
    """get_rays -> render_rays -> MSE with the trained student frozen: 30 Adam steps on c2w from a pose translated by 0.05"""
    import sinnerf_amd
    from sinnerf_amd.ray_utils import get_rays
    from tests.test_trained_weights_gpu import trained_models
    models = trained_models("fp32")
    for m in models:
        for p in m.parameters():
            p.requires_grad_(False)
    H = W = 96
    focal = 0.5 * 800 / np.tan(0.5 * 0.6911112) * (W / 800.0)
    window = (2, 2, 4, 4, 24, 24)
    pose = lego_pose(0)
    render = lambda rays: sinnerf_amd.render_rays(models, embeddings(), rays, 64, False, 0, 0, 64, 32768, True)["rgb_fine"]
    with torch.no_grad():
        target = render(get_rays(H, W, focal, t(pose), 2.0, 6.0, window))
    start = pose.copy()
    start[:, 3] += np.array([0.03, -0.03, 0.02828], np.float32)                          # |offset| = 0.05
    c2w = t(start).requires_grad_()
    opt = torch.optim.Adam([c2w], lr=2e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = ((render(get_rays(H, W, focal, c2w, 2.0, 6.0, window)) - target) ** 2).mean()
        loss.backward()
        assert c2w.grad is not None and torch.isfinite(c2w.grad).all()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        final = ((render(get_rays(H, W, focal, c2w, 2.0, 6.0, window)) - target) ** 2).mean().item()
    print("pose optimisation: loss", losses[0], "->", final)
    assert final < losses[0]
