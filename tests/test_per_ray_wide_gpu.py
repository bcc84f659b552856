"""GPU: the per-ray kernels of csrc/sn_render.hip above 64 samples per ray, where each lane owns C = ceil(S / 64) consecutive
elements (C up to 16), through the C ABI.  Inputs and acceptance: tests/per_ray_wide.py, whose sensitivity to a wrong
element-to-lane map tests/test_per_ray_wide_cpu.py proves on numpy restatements of the kernels.  Every bar is the one the same
kernel already has at C = 1.  Each test prints its worst err / bar (pytest -s)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                              # noqa: E402
from tests import per_ray_wide as W                                            # noqa: E402
from tests import ray_grad_oracle as R                                         # noqa: E402
from tests.helpers import GOLDEN, max_abs, max_rel, sample_pdf_tol, well_conditioned   # noqa: E402
from tests.test_parity_gpu import dev, embeddings, injected_rng, make_model    # noqa: E402


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ------------------------------------------------------------------------------------------- sn_sample_coarse
def run_sample_coarse(rays, S, use_disp, perturb, pr):
    from sinnerf_amd import _lib
    n = rays.shape[0]
    r_d, pr_d = t(rays), t(pr)
    z = torch.full((n, S), float("nan"), device=dev())
    _lib.check(_lib.lib.sn_sample_coarse(_lib.ptr(r_d), n, S, int(use_disp), perturb, _lib.ptr(pr_d) if perturb > 0 else None,
                                         _lib.ptr(z), _lib.stream_ptr()), "sn_sample_coarse")
    torch.cuda.synchronize()
    return z.cpu().numpy()


@pytest.mark.parametrize("S", [1, 2, 3, 65, 257, 513, 1024])
@pytest.mark.parametrize("use_disp,perturb", [(False, 0.0), (False, 1.0), (True, 0.5), (True, 1.0)])
def test_sample_coarse_bit_exact_wide(S, use_disp, perturb):
    rays = O.lego_rays(40, 40, seed=1)[::3]
    pr = np.random.RandomState(S).uniform(0, 1, (rays.shape[0], S)).astype(np.float32)
    assert np.array_equal(run_sample_coarse(rays, S, use_disp, perturb, pr), O.coarse_z_vals(rays, S, use_disp, perturb, pr))


def test_sample_coarse_above_the_grid_cap():
    """1100 x 1000 points > 256 * 16 blocks of 256: the grid-stride loop takes a second trip for the last 51 424 points"""
    n, S = 1100, 1000
    assert n * S > 256 * 16 * 256
    rays = O.lego_rays(40, 40, seed=1)[:n]
    pr = np.random.RandomState(7).uniform(0, 1, (n, S)).astype(np.float32)
    assert np.array_equal(run_sample_coarse(rays, S, False, 1.0, pr), O.coarse_z_vals(rays, S, False, 1.0, pr))


# ------------------------------------------------------------------------------------------- sn_sample_pdf
def run_sample_pdf(zc, w, u, NI):
    from sinnerf_amd import _lib
    n, S = zc.shape
    zc_d, w_d, u_d = t(zc), t(w), t(u)                       # referenced until the launch has been enqueued
    zf = torch.full((n, NI), float("nan"), device=dev())
    zm = torch.full((n, S + NI), float("nan"), device=dev())
    rc = _lib.lib.sn_sample_pdf(_lib.ptr(zc_d), _lib.ptr(w_d), _lib.ptr(u_d), n, S, NI, _lib.ptr(zf), _lib.ptr(zm),
                                _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, zf.cpu().numpy(), zm.cpu().numpy()


@pytest.mark.parametrize("S,NI,family,rand_u", W.SAMPLER_CASES)
def test_sample_pdf_wide(S, NI, family, rand_u):
    zc, w, u = W.sampler_inputs(S, NI, family, rand_u)
    rc, zf, zm = run_sample_pdf(zc, w, u, NI)
    assert rc == 0
    tag = f"S{S}_NI{NI}_{family}_{'rand' if rand_u else 'det'}"
    worst, share = W.check_sampler(zc, w, u, NI, zf, zm, tag=tag)
    print(f"sn_sample_pdf {tag}: err/tol {worst:.3f}, well-conditioned share {share:.4f}")


@pytest.mark.parametrize("rand_u", [False, True])
def test_sample_pdf_largest_shape_merge_and_range(rand_u):
    """(1023, 1): the largest sample count whose LDS request fits (65 472 B) -- merge exactness and range only"""
    S, NI = 1023, 1
    zc, w, u = W.sampler_inputs(S, NI, "cube", rand_u, n=9)
    rc, zf, zm = run_sample_pdf(zc, w, u, NI)
    assert rc == 0
    assert np.array_equal(zm, np.sort(np.concatenate([zc, zf], -1), -1))
    mid = np.float32(0.5) * (zc[:, :-1] + zc[:, 1:])
    assert (zf >= mid[:, :1] - 1e-6).all() and (zf <= mid[:, -1:] + 1e-6).all()


def test_sample_pdf_refuses_what_does_not_fit_lds():
    """(1024, 8) asks for 4 * (2 * 1023 + 2 * 1032) * 4 = 65 760 B > 64 KB: a non-zero code and no launch (outputs untouched)"""
    from sinnerf_amd import _lib
    S, NI = 1024, 8
    zc, w, u = W.sampler_inputs(S, NI, "cube", True, n=5)
    rc, zf, zm = run_sample_pdf(zc, w, u, NI)
    assert rc != 0
    assert np.isnan(zf).all() and np.isnan(zm).all()
    with pytest.raises(_lib.SinnerfHipError):
        _lib.check(rc, "sn_sample_pdf")


# ------------------------------------------------------------------------------------------- sn_sample_pdf_bins
@pytest.mark.parametrize("m,k", [(300, 257), (1000, 64)])
def test_sample_pdf_bins_wide_fixture(m, k):
    import sinnerf_amd
    z = np.load(f"{GOLDEN}/sample_pdf_wide.npz")
    bins, w, u = z[f"m{m}_bins"], z[f"m{m}_weights"], z[f"m{m}_u"]
    det = sinnerf_amd.sample_pdf(t(bins), t(w), k, det=True).cpu().numpy()
    with injected_rng([("rand", u)]):
        rnd = sinnerf_amd.sample_pdf(t(bins), t(w), k, det=False).cpu().numpy()
    lin = O.linspace01(k)[None].repeat(bins.shape[0], 0)
    for kind, got, ref, uu in (("det", det, z[f"m{m}_out_det"], lin), ("rand", rnd, z[f"m{m}_out_rand"], u)):
        ok = well_conditioned(bins, w, uu)
        ratio = np.abs(got.astype(np.float64) - ref) / sample_pdf_tol(bins, w, uu)
        print(f"sample_pdf {m} bins {kind}: err/tol {ratio[ok].max():.3f}, well-conditioned share {ok.mean():.4f}")
        assert ok.mean() > 0.97
        assert (ratio <= 1.0)[ok].all()
        assert (got >= bins[:, :1] - 1e-6).all() and (got <= bins[:, -1:] + 1e-6).all()


@pytest.mark.parametrize("eps", [1e-5, 1e-3, 1e-7])
def test_sample_pdf_bins_wide_eps_argument(eps):
    """test_sample_pdf_eps_argument at 300 bins (5 per lane)"""
    import sinnerf_amd
    r = np.random.RandomState(3)
    n, m, NI = 64, 300, 257
    bins = np.sort(r.uniform(2, 6, (n, m + 1)).astype(np.float32), -1)
    w = (r.uniform(0, 1, (n, m)) ** 6).astype(np.float32)                 # many tiny weights: eps matters
    got = sinnerf_amd.sample_pdf(t(bins), t(w), NI, det=True, eps=eps).cpu().numpy()
    ref = O.sample_pdf(bins, w, NI, det=True, eps=eps)
    uu = O.linspace01(NI)[None].repeat(n, 0)
    ok = well_conditioned(bins, w, uu, eps=eps)
    ratio = np.abs(got.astype(np.float64) - ref) / sample_pdf_tol(bins, w, uu, eps=eps)
    print(f"sample_pdf 300 bins eps={eps:g}: err/tol {ratio[ok].max():.3f}, well-conditioned share {ok.mean():.4f}")
    assert ok.mean() >= 0.9
    assert (ratio <= 1.0)[ok].all()
    assert ((got >= bins[:, :1]) & (got <= bins[:, -1:])).all()


# ------------------------------------------------------------------------------------------- sn_composite_forward
@pytest.mark.parametrize("S,white_back,noise_std,has_rgb", [(65, True, 0.0, True), (257, False, 1.0, True), (513, True, 0.5, True),
                                                            (960, False, 1.0, True), (1024, True, 0.5, True),
                                                            (257, True, 1.0, False), (1024, False, 0.5, False)])
def test_composite_forward_wide(S, white_back, noise_std, has_rgb):
    from sinnerf_amd import rendering
    rays, z, raw, noise, _ = W.composite_inputs(S, 7, 3)
    inp = raw if has_rgb else np.ascontiguousarray(raw[..., 3])
    ref = O.composite(inp, z, rays[:, 3:6], noise if noise_std else None, noise_std, white_back, weights_only=not has_rgb)
    rgb, depth, w = rendering._composite(t(inp), has_rgb, t(z), t(rays), t(noise) if noise_std else None, noise_std, white_back)
    torch.cuda.synchronize()
    if has_rgb:
        figs = (max_abs(w.cpu().numpy(), ref[2]) / 2e-7, max_abs(rgb.cpu().numpy(), ref[0]) / 1e-6,
                max_rel(depth.cpu().numpy(), ref[1]) / 2e-6)
    else:
        figs = (max_abs(w.cpu().numpy(), ref) / 2e-7,)
    print(f"sn_composite_forward S{S} has_rgb={int(has_rgb)}: err/bar (weights, rgb, depth) " + " ".join("%.3f" % f for f in figs))
    assert max(figs) <= 1.0, figs


# ------------------------------------------------------------------------------------------- sn_composite_backward(_rays)
def run_backward(rays, z, raw, noise, noise_std, white_back, g_rgb, g_depth, g_w):
    """both entries on the same inputs: (g_raw of sn_composite_backward, g_raw and g_rays of sn_composite_backward_rays)"""
    from sinnerf_amd import _lib as L
    n, S = z.shape
    args = [t(raw), t(z), t(rays), t(noise) if noise_std else None]
    ups = [t(g_rgb), t(g_depth), t(g_w)]
    g_raw0 = torch.full((n, S, 4), float("nan"), dtype=torch.float32, device=dev())
    g_raw1 = torch.full((n, S, 4), float("nan"), dtype=torch.float32, device=dev())
    g_rays = torch.full((n, 8), float("nan"), dtype=torch.float32, device=dev())
    p, u = [L.ptr(a) for a in args], [L.ptr(a) for a in ups]
    L.check(L.lib.sn_composite_backward(p[0], p[1], p[2], p[3], noise_std, n, S, int(white_back), u[0], u[1], u[2], L.ptr(g_raw0),
                                        L.stream_ptr()), "sn_composite_backward")
    L.check(L.lib.sn_composite_backward_rays(p[0], p[1], p[2], p[3], noise_std, n, S, int(white_back), u[0], u[1], u[2],
                                             L.ptr(g_raw1), L.ptr(g_rays), L.stream_ptr()), "sn_composite_backward_rays")
    torch.cuda.synchronize()
    return g_raw0.cpu().numpy(), g_raw1.cpu().numpy(), g_rays.cpu().numpy()


@pytest.mark.parametrize("S", W.COMPOSITE_BWD_S)
def test_composite_backward_wide(S):
    rays, z, raw, noise, r = W.composite_inputs(S, 9, 2)
    n = rays.shape[0]
    white_back, noise_std, with_gw = W.backward_settings(S)
    g_rgb, g_depth = r.standard_normal((n, 3)).astype(np.float32), r.standard_normal(n).astype(np.float32)
    g_w = r.standard_normal((n, S)).astype(np.float32) if with_gw else None
    nz = noise if noise_std else None
    g_raw0, g_raw1, g_rays = run_backward(rays, z, raw, noise, noise_std, white_back, g_rgb, g_depth, g_w)
    assert np.array_equal(g_raw0, g_raw1)
    a = W.check_backward(g_raw0, O.composite_backward(raw, z, rays[:, 3:6], nz, noise_std, white_back, g_rgb, g_depth, g_w), f"S{S} g_raw")
    assert (g_rays[:, :3] == 0).all() and (g_rays[:, 6:] == 0).all()
    b = W.check_backward(g_rays[:, 3:6], R.composite_dir_grad(raw, z, rays[:, 3:6], nz, noise_std, white_back, g_rgb, g_depth, g_w),
                         f"S{S} g_rays")
    print(f"sn_composite_backward S{S}: err/bar g_raw {a:.3f}, g_rays {b:.3f}")


@pytest.mark.parametrize("S", W.COMPOSITE_BWD_S)
def test_composite_backward_position_probe(S):
    """one ray per lane boundary j of the shape, upstream gradient g_w = e_j alone, against the closed form in float64"""
    rays, z, raw, g_w, j = W.probe_inputs(S)
    n = rays.shape[0]
    zero3, zero1 = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    g_raw0, g_raw1, g_rays = run_backward(rays, z, raw, None, 0.0, False, zero3, zero1, g_w)
    assert np.array_equal(g_raw0, g_raw1)
    a = W.check_backward(g_raw0, W.probe_reference(rays, z, raw, j), f"probe S{S} g_raw")
    assert (g_rays[:, :3] == 0).all() and (g_rays[:, 6:] == 0).all()
    b = W.check_backward(g_rays[:, 3:6], R.composite_dir_grad(raw, z, rays[:, 3:6], None, 0.0, False, zero3, zero1, g_w),
                         f"probe S{S} g_rays")
    print(f"position probe S{S} ({n} boundaries): err/bar g_raw {a:.3f}, g_rays {b:.3f}")


# ------------------------------------------------------------------------------------------- limits
def test_render_rays_accepts_1024_samples_and_refuses_1025():
    import sinnerf_amd
    mc, _ = make_model(0, True)
    mf, _ = make_model(1, True)
    rays = t(O.lego_rays(400, 400, seed=0)[::40000][:3])
    with torch.no_grad():
        res = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 1000, False, 1.0, 0.5, 24, 32768, True)
    torch.cuda.synchronize()
    assert res["opacity_fine"].shape == (3, 1024) and all(torch.isfinite(v).all() for v in res.values())
    for S, NI in ((1000, 25), (1025, 0), (512, 513)):
        with pytest.raises(NotImplementedError):
            with torch.no_grad():
                sinnerf_amd.render_rays([mc, mf], embeddings(), rays, S, False, 1.0, 0.5, NI, 32768, True)
