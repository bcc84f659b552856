"""GPU parity tests: the HIP path (through the C ABI, via sinnerf_amd) against the numpy oracle and the
golden vectors generated from the reference.  Run with `pytest -m gpu` on an MI355X."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                              # noqa: E402
from tests.helpers import (GOLDEN, RENDER_CASES, check_render, load_case, max_abs, max_rel, sample_pdf_tol,  # noqa: E402
                           well_conditioned)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def make_model(seed, teacher, dtype="fp32"):
    import sinnerf_amd
    m = sinnerf_amd.NeRF(use_new_activation=True, compute_dtype=dtype)
    p = O.init_params(seed, teacher)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return m.to(dev()).eval(), p


def embeddings():
    import sinnerf_amd
    return [sinnerf_amd.Embedding(3, 10), sinnerf_amd.Embedding(3, 4)]


@contextlib.contextmanager
def injected_rng(order):
    """Make torch.rand / torch.randn return the recorded draws (in the reference's consumption order)."""
    q = list(order)
    real_rand, real_randn = torch.rand, torch.randn

    def take(kind, shape):
        k, arr = q.pop(0)
        assert k == kind and tuple(arr.shape) == tuple(shape), (k, kind, arr.shape, shape)
        return torch.from_numpy(arr).to(dev())

    torch.rand = lambda *a, **kw: take("rand", a[0] if isinstance(a[0], (tuple, list)) else a)
    torch.randn = lambda *a, **kw: take("randn", a[0] if isinstance(a[0], (tuple, list)) else a)
    try:
        yield q
    finally:
        torch.rand, torch.randn = real_rand, real_randn


def rng_order(meta, rng, n):
    """Draws in consumption order; noise draws are made even when the fixture did not keep them."""
    order = []
    s, ni = meta["N_samples"], meta["N_importance"]
    if meta["perturb"] > 0:
        order.append(("rand", rng["perturb"]))
    order.append(("randn", rng.get("noise_coarse", np.zeros((n, s), np.float32))))
    if ni > 0:
        if meta["perturb"] > 0:
            order.append(("rand", rng["u"]))
        order.append(("randn", rng.get("noise_fine", np.zeros((n, s + ni), np.float32))))
    return order


def to_np(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items()}


# ------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("S,use_disp,perturb", [(64, False, 0.0), (64, False, 1.0), (64, True, 0.5), (24, False, 1.0),
                                                (128, False, 0.0), (192, True, 1.0)])
def test_sample_coarse_bit_exact(S, use_disp, perturb):
    from sinnerf_amd import _lib
    rays = O.lego_rays(40, 40, seed=1)[::3]
    n = rays.shape[0]
    pr = np.random.RandomState(0).uniform(0, 1, (n, S)).astype(np.float32)
    ref = O.coarse_z_vals(rays, S, use_disp, perturb, pr)
    r = torch.from_numpy(rays).to(dev())
    z = torch.empty((n, S), device=dev())
    prt = torch.from_numpy(pr).to(dev())
    _lib.check(_lib.lib.sn_sample_coarse(_lib.ptr(r), n, S, int(use_disp), perturb, _lib.ptr(prt) if perturb > 0 else None,
                                         _lib.ptr(z), None), "sn_sample_coarse")
    torch.cuda.synchronize()
    assert np.array_equal(z.cpu().numpy(), ref)            # integer-like bar: identical bits


@pytest.mark.parametrize("sigma_only", [False, True])
def test_mlp_forward_vs_oracle(sigma_only, flags=0):
    from sinnerf_amd import rendering
    model, p = make_model(0, True)
    rays = O.lego_rays(400, 400, seed=0)[::1601][:100]      # 100 rays -> 6400 points (50 workgroups, ragged tail below)
    n = rays.shape[0]
    z = O.coarse_z_vals(rays, 67, False, 1.0, np.random.RandomState(1).uniform(0, 1, (n, 67)).astype(np.float32))
    ref = O._run_model(p, rays, z, O.embedding(rays[:, 3:6], 4), sigma_only, 1 << 20)
    with torch.no_grad():
        out = rendering._mlp(model, torch.from_numpy(rays).to(dev()), torch.from_numpy(z).to(dev()), sigma_only, flags)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref) / (np.abs(ref) + 1e-3)
    assert err.max() <= 2e-4, err.max()


def test_nerf_forward_embedded_golden():
    z = np.load(f"{GOLDEN}/nerf_mlp.npz")
    model, _ = make_model(int(z["seed"]), bool(z["teacher"]))
    x = torch.from_numpy(np.concatenate([z["emb_xyz"], z["emb_dir"]], 1)).to(dev())
    with torch.no_grad():
        full = model(x).cpu().numpy()
        sig = model(x[:, :63].contiguous(), sigma_only=True).cpu().numpy()
    assert full.shape == (300, 4) and sig.shape == (300, 1)
    assert (np.abs(full - z["out_full"]) / (np.abs(z["out_full"]) + 1e-3)).max() <= 2e-4
    assert (np.abs(sig - z["out_sigma"]) / (np.abs(z["out_sigma"]) + 1e-3)).max() <= 2e-4


@pytest.mark.parametrize("S,white_back,noise_std,has_rgb", [(64, True, 0.0, True), (128, False, 1.0, True),
                                                            (192, True, 0.5, True), (24, False, 1.0, True),
                                                            (64, True, 1.0, False), (100, False, 0.0, True),
                                                            (640, True, 0.5, True), (1000, False, 0.0, True)])
def test_composite_vs_oracle(S, white_back, noise_std, has_rgb):
    from sinnerf_amd import rendering
    r = np.random.RandomState(S)
    rays = O.lego_rays(30, 30, seed=2)[::7]
    n = rays.shape[0]
    z = np.sort(r.uniform(2, 6, (n, S)).astype(np.float32), -1)
    raw = r.uniform(0, 1, (n, S, 4)).astype(np.float32)
    raw[..., 3] = (r.standard_normal((n, S)) * 3).astype(np.float32)
    noise = r.standard_normal((n, S)).astype(np.float32)
    inp = raw if has_rgb else np.ascontiguousarray(raw[..., 3])
    ref = O.composite(inp, z, rays[:, 3:6], noise if noise_std else None, noise_std, white_back, weights_only=not has_rgb)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    rgb, depth, w = rendering._composite(t(inp), has_rgb, t(z), t(rays), t(noise) if noise_std else None, noise_std, white_back)
    torch.cuda.synchronize()
    if has_rgb:
        assert max_abs(w.cpu().numpy(), ref[2]) <= 2e-7
        assert max_abs(rgb.cpu().numpy(), ref[0]) <= 1e-6
        assert max_rel(depth.cpu().numpy(), ref[1]) <= 2e-6
    else:
        assert max_abs(w.cpu().numpy(), ref) <= 2e-7


def test_sample_pdf_golden_and_oracle():
    import sinnerf_amd
    z = np.load(f"{GOLDEN}/sample_pdf.npz")
    bins, w, u = (torch.from_numpy(z[k]).to(dev()) for k in ("bins", "weights", "u"))
    det = sinnerf_amd.sample_pdf(bins, w, 64, det=True).cpu().numpy()
    with injected_rng([("rand", z["u"])]):
        rnd = sinnerf_amd.sample_pdf(bins, w, 64, det=False).cpu().numpy()
    lin = O.linspace01(64)[None].repeat(64, 0)
    for got, ref, uu in ((det, z["out_det"], lin), (rnd, z["out_rand"], z["u"])):
        ok = well_conditioned(z["bins"], z["weights"], uu)
        tol = sample_pdf_tol(z["bins"], z["weights"], uu)
        assert (np.abs(got - ref) <= tol)[ok].all()
        assert (got >= z["bins"][:, :1] - 1e-6).all() and (got <= z["bins"][:, -1:] + 1e-6).all()


def test_sample_pdf_merge_sorted_and_complete():
    from sinnerf_amd import _lib
    r = np.random.RandomState(5)
    for S, NI, rand_u in ((64, 64, False), (64, 128, True), (24, 40, True), (64, 64, True)):
        rays = O.lego_rays(20, 20, seed=3)[::3]
        n = rays.shape[0]
        zc = O.coarse_z_vals(rays, S, False, 1.0, r.uniform(0, 1, (n, S)).astype(np.float32))
        w = (r.uniform(0, 1, (n, S)) ** 3).astype(np.float32)
        u = r.uniform(0, 1, (n, NI)).astype(np.float32) if rand_u else None
        mid = (np.float32(0.5) * (zc[:, :-1] + zc[:, 1:])).astype(np.float32)
        zf_ref = O.sample_pdf(mid, w[:, 1:-1], NI, det=not rand_u, u=u)
        # keep every device tensor referenced until the launch has been enqueued (a temporary passed as
        # `_lib.ptr(t(x))` is freed -- and its block re-used by the next temporary -- before the call)
        zc_d, w_d = torch.from_numpy(zc).to(dev()), torch.from_numpy(w).to(dev())
        u_d = torch.from_numpy(u).to(dev()) if rand_u else None
        zf = torch.empty((n, NI), device=dev()); zm = torch.empty((n, S + NI), device=dev())
        _lib.check(_lib.lib.sn_sample_pdf(_lib.ptr(zc_d), _lib.ptr(w_d), _lib.ptr(u_d), n, S, NI,
                                          _lib.ptr(zf), _lib.ptr(zm), None), "sn_sample_pdf")
        torch.cuda.synchronize()
        zf, zm = zf.cpu().numpy(), zm.cpu().numpy()
        assert (np.diff(zm, axis=-1) >= 0).all()                                   # sortedness
        assert np.array_equal(zm, np.sort(np.concatenate([zc, zf], -1), -1))       # a permutation of the inputs
        uu = u if rand_u else O.linspace01(NI)[None].repeat(n, 0)
        ok = well_conditioned(mid, w[:, 1:-1], uu)
        assert ok.mean() >= 0.97, ok.mean()                                        # the exclusion stays a small minority
        assert (np.abs(zf - zf_ref) <= sample_pdf_tol(mid, w[:, 1:-1], uu))[ok].all()


@pytest.mark.parametrize("eps", [1e-5, 1e-3, 1e-7])
def test_sample_pdf_eps_argument(eps):
    """sample_pdf(bins, weights, N, det, eps) of rendering.py:15 with a non-default eps (pdf floor AND the denom < eps rule)."""
    import sinnerf_amd
    r = np.random.RandomState(3)
    n, m, NI = 300, 40, 50
    bins = np.sort(r.uniform(2, 6, (n, m + 1)).astype(np.float32), -1)
    w = (r.uniform(0, 1, (n, m)) ** 6).astype(np.float32)                 # many tiny weights: eps matters
    got = sinnerf_amd.sample_pdf(torch.from_numpy(bins).to(dev()), torch.from_numpy(w).to(dev()), NI, det=True, eps=eps).cpu().numpy()
    ref = O.sample_pdf(bins, w, NI, det=True, eps=eps)
    uu = O.linspace01(NI)[None].repeat(n, 0)
    ok = well_conditioned(bins, w, uu, eps=eps)
    assert ok.mean() >= 0.9
    assert (np.abs(got - ref) <= sample_pdf_tol(bins, w, uu, eps=eps))[ok].all()
    assert ((got >= bins[:, :1]) & (got <= bins[:, -1:])).all()


def test_sample_pdf_merge_with_ties_and_unsorted_samples():
    """The merge-by-rank path (both lists ascending: one binary search per key) against sort(cat) on inputs full of TIES --
    repeated coarse depths, samples that coincide with coarse depths, a degenerate ray (near == far: every key equal) -- and
    the rank-sort fallback on rays whose samples are not ascending (random u), ray by ray in the same launch."""
    from sinnerf_amd import _lib
    r = np.random.RandomState(11)
    S, NI = 64, 64
    n = 96
    near = r.uniform(1.5, 2.5, n).astype(np.float32); far = (near + r.uniform(0.5, 4, n)).astype(np.float32)
    far[:8] = near[:8]                                                       # degenerate rays: coarse depths equal up to rounding
    t = np.linspace(0, 1, S, dtype=np.float32)
    zc = (near[:, None] * (1 - t) + far[:, None] * t).astype(np.float32)
    zc[8:24, 10:20] = zc[8:24, 10:11]                                        # runs of equal coarse depths
    zc = np.sort(zc, -1)
    w = (r.uniform(0, 1, (n, S)) ** 4).astype(np.float32)
    w[24:40] = 0                                                             # uniform pdf: det samples land on bin mid points
    u = r.uniform(0, 1, (n, NI)).astype(np.float32)
    u[:48] = np.sort(u[:48], -1)                                             # first half: ascending u -> ascending samples (merge path)
    u[40:48, 5:30] = u[40:48, 5:6]                                           # ... with repeated samples
    for use_u in (True, False):
        zc_d, w_d = torch.from_numpy(zc).to(dev()), torch.from_numpy(w).to(dev())
        u_d = torch.from_numpy(u).to(dev()) if use_u else None
        zf = torch.empty((n, NI), device=dev()); zm = torch.empty((n, S + NI), device=dev())
        _lib.check(_lib.lib.sn_sample_pdf(_lib.ptr(zc_d), _lib.ptr(w_d), _lib.ptr(u_d), n, S, NI, _lib.ptr(zf), _lib.ptr(zm), None), "sn_sample_pdf")
        torch.cuda.synchronize()
        zf_h, zm_h = zf.cpu().numpy(), zm.cpu().numpy()
        assert np.isfinite(zm_h).all()
        assert np.array_equal(zm_h, np.sort(np.concatenate([zc, zf_h], -1), -1)), use_u      # exactly the sorted multiset


@pytest.mark.parametrize("name", ["render_lego_eval_teacher", "render_llff_eval_128", "render_lego_train_teacher"])
def test_sample_pdf_on_real_render_cases_exclusion_fraction(name):
    """the knot-exclusion of the sample_pdf comparisons (helpers.well_conditioned) must stay a small,
    ASSERTED fraction on the real render cases too, not only on the synthetic fixture: coarse weights of the golden render
    cases (from the reference), importance samples from the HIP sampler vs the oracle on >= 97 % of the entries, every
    sample inside its ray's bin range."""
    from sinnerf_amd import _lib
    rays, meta, rng, ref = load_case(name)
    n, S, NI = rays.shape[0], meta["N_samples"], meta["N_importance"]
    zc = O.coarse_z_vals(rays, S, bool(meta["use_disp"]), meta["perturb"], rng.get("perturb"))
    w = ref["opacity_coarse"]
    det = meta["perturb"] == 0
    u = None if det else rng["u"]
    mid = (np.float32(0.5) * (zc[:, :-1] + zc[:, 1:])).astype(np.float32)
    zf_ref = O.sample_pdf(mid, w[:, 1:-1], NI, det=det, u=u)
    zc_d, w_d = torch.from_numpy(zc).to(dev()), torch.from_numpy(np.ascontiguousarray(w)).to(dev())
    u_d = None if det else torch.from_numpy(u).to(dev())
    zf = torch.empty((n, NI), device=dev()); zm = torch.empty((n, S + NI), device=dev())
    _lib.check(_lib.lib.sn_sample_pdf(_lib.ptr(zc_d), _lib.ptr(w_d), _lib.ptr(u_d), n, S, NI, _lib.ptr(zf), _lib.ptr(zm), None),
               "sn_sample_pdf")
    torch.cuda.synchronize()
    zf = zf.cpu().numpy()
    uu = O.linspace01(NI)[None].repeat(n, 0) if det else u
    ok = well_conditioned(mid, w[:, 1:-1], uu)
    print(name, "excluded fraction", 1 - ok.mean())
    assert ok.mean() >= 0.97, (name, ok.mean())
    assert (np.abs(zf - zf_ref) <= sample_pdf_tol(mid, w[:, 1:-1], uu))[ok].all()
    assert (zf >= mid[:, :1] - 1e-6).all() and (zf <= mid[:, -1:] + 1e-6).all()      # the rest is bounded by the bin range


# ------------------------------------------------------------------------------------- whole path
@pytest.mark.parametrize("name", RENDER_CASES)
def test_render_rays_golden(name):
    import sinnerf_amd
    rays, meta, rng, ref = load_case(name)
    mc, _ = make_model(meta["seed_coarse"], bool(meta["teacher"]))
    mf, _ = make_model(meta["seed_fine"], bool(meta["teacher"]))
    with torch.no_grad(), injected_rng(rng_order(meta, rng, rays.shape[0])) as left:
        res = sinnerf_amd.render_rays([mc, mf], embeddings(), torch.from_numpy(rays).to(dev()), meta["N_samples"],
                                      bool(meta["use_disp"]), meta["perturb"], meta["noise_std"], meta["N_importance"],
                                      meta["chunk"], bool(meta["white_back"]), test_time=bool(meta["test_time"]))
        assert not left, "render_rays consumed fewer random draws than the reference"
    torch.cuda.synchronize()
    assert set(res.keys()) == set(ref.keys())
    check_render(to_np(res), ref, tag=name)


def test_render_rays_matches_oracle_on_subset_of_full_frame_and_properties():
    """BASELINE config[1] size: lego 400x400 (160 000 rays), 64+64, fp32.  The oracle is too slow for the full
    frame, so: (a) a 256-ray subset of the frame against the oracle, (b) size-independent properties on the
    full frame: ray-chunk invariance (bit-exact), ray-permutation equivariance, weights in
    [0,1] with sum <= 1, finite outputs."""
    import sinnerf_amd
    mc, pc = make_model(0, True)
    mf, pf = make_model(1, True)
    rays_np = O.lego_rays(400, 400, seed=0)
    rays = torch.from_numpy(rays_np).to(dev())
    kw = dict(N_samples=64, use_disp=False, perturb=0, noise_std=0, N_importance=64, chunk=1 << 19, white_back=True)
    with torch.no_grad():
        full = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, **kw)
        sel = torch.from_numpy(np.random.RandomState(3).permutation(160000)).to(dev())
        perm = sinnerf_amd.render_rays([mc, mf], embeddings(), rays[sel].contiguous(), **kw)
        half = sinnerf_amd.render_rays([mc, mf], embeddings(), rays[80000:].contiguous(), **kw)
    torch.cuda.synchronize()
    for k, v in full.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v[sel], perm[k]), f"permutation equivariance broken for {k}"
        assert torch.equal(v[80000:], half[k]), f"chunk invariance broken for {k}"
    for k in ("opacity_coarse", "opacity_fine"):
        assert (full[k] >= 0).all() and (full[k] <= 1).all() and (full[k].sum(1) <= 1 + 1e-5).all()
    idx = np.random.RandomState(4).choice(160000, 256, replace=False)
    ref = O.render_rays([pc, pf], rays_np[idx], 64, False, 0, 0, 64, 1 << 19, True, False)
    check_render({k: v[torch.from_numpy(idx).to(dev())].cpu().numpy() for k, v in full.items()}, ref, tag="frame-subset")


def test_psnr_parity_teacher_scene():
    """SURVEY §8d PSNR protocol: gt = oracle render of the teacher scene + fixed pixel noise; |PSNR(new,gt) -
    PSNR(oracle,gt)| <= 0.05 dB (north_star)."""
    import sinnerf_amd
    mc, pc = make_model(0, True)
    mf, pf = make_model(1, True)
    rays_np = O.lego_rays(48, 48, seed=2)
    ref = O.render_rays([pc, pf], rays_np, 64, False, 0, 0, 64, 1 << 19, True, False)["rgb_fine"]
    gt = ref + np.random.RandomState(0).normal(0, 0.02, ref.shape).astype(np.float32)
    with torch.no_grad():
        got = sinnerf_amd.render_rays([mc, mf], embeddings(), torch.from_numpy(rays_np).to(dev()), 64, False, 0, 0, 64,
                                      1 << 19, True)["rgb_fine"].cpu().numpy()
    assert abs(O.psnr(got, gt) - O.psnr(ref, gt)) <= 0.05
    assert O.psnr(got, ref) > 80.0


def test_errors_are_loud():
    import sinnerf_amd
    mc, _ = make_model(0, True)
    with pytest.raises(RuntimeError):
        sinnerf_amd.render_rays([mc], embeddings(), torch.zeros(4, 8), 64)          # CPU tensor: no fallback
    with pytest.raises(NameError):
        with torch.no_grad():
            sinnerf_amd.render_rays([mc], embeddings(), torch.zeros(4, 8, device=dev()), 64, test_time=True)


# ------------------------------------------------------------------------------------------- bf16 path
def test_bf16_mlp_vs_bf16_emulated_oracle():
    """bf16-operand / fp32-accumulate MFMA path: compare with an oracle whose Linear inputs (activations AND weights)
    are rounded to bf16 (RNE) -- the arithmetic the kernel performs -- and, loosely, with the fp32 oracle."""
    from sinnerf_amd import rendering
    model, p = make_model(0, True, dtype="bf16")
    rays = O.lego_rays(400, 400, seed=0)[::1601][:100]
    n = rays.shape[0]
    z = O.coarse_z_vals(rays, 70, False, 1.0, np.random.RandomState(1).uniform(0, 1, (n, 70)).astype(np.float32))

    with O.bf16_operands():                       # both Linear operands rounded to bf16 (RNE), fp32 heads, as in the kernel
        ref_bf16 = O._run_model(p, rays, z, O.embedding(rays[:, 3:6], 4), False, 1 << 20)
    ref_f32 = O._run_model(p, rays, z, O.embedding(rays[:, 3:6], 4), False, 1 << 20)
    for sigma_only in (False, True):
        with torch.no_grad():
            got = rendering._mlp(model, torch.from_numpy(rays).to(dev()), torch.from_numpy(z).to(dev()), sigma_only).cpu().numpy()
        rb = ref_bf16[..., 3] if sigma_only else ref_bf16
        rf = ref_f32[..., 3] if sigma_only else ref_f32
        assert got.shape == rb.shape and np.isfinite(got).all()
        scale = np.abs(rf).max()
        assert np.abs(got - rb).max() <= 2e-3 * scale, np.abs(got - rb).max() / scale      # same arithmetic, fp32 heads
        assert np.abs(got - rf).max() <= 3e-2 * scale, np.abs(got - rf).max() / scale      # bf16 vs fp32


def test_bf16_render_psnr_parity():
    """north_star bar for reduced precision: PSNR within 0.05 dB of the reference render (SURVEY §8d protocol)."""
    import sinnerf_amd
    mc, pc = make_model(0, True, dtype="bf16")
    mf, pf = make_model(1, True, dtype="bf16")
    rays_np = O.lego_rays(48, 48, seed=2)
    ref = O.render_rays([pc, pf], rays_np, 64, False, 0, 0, 64, 1 << 19, True, False)["rgb_fine"]
    gt = ref + np.random.RandomState(0).normal(0, 0.02, ref.shape).astype(np.float32)
    with torch.no_grad():
        res = sinnerf_amd.render_rays([mc, mf], embeddings(), torch.from_numpy(rays_np).to(dev()), 64, False, 0, 0, 64,
                                      1 << 19, True)
    got = res["rgb_fine"].cpu().numpy()
    assert np.isfinite(got).all()
    assert abs(O.psnr(got, gt) - O.psnr(ref, gt)) <= 0.05, (O.psnr(got, gt), O.psnr(ref, gt))
    assert O.psnr(got, ref) > 55.0, O.psnr(got, ref)


def test_eval_points_vs_oracle():
    """rendering.py:64-123: sigma of the fine model at free points."""
    import sinnerf_amd
    mc, _ = make_model(0, True)
    mf, pf = make_model(1, True)
    pts = np.random.RandomState(4).uniform(-3, 3, (1000, 3)).astype(np.float32)
    got = sinnerf_amd.eval_points(torch.from_numpy(pts).to(dev()), [mc, mf], embeddings()).cpu().numpy()
    ref = O.nerf_forward(pf, O.embedding(pts, 10), sigma_only=True)
    assert got.shape == (1000, 1)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-5
    assert sinnerf_amd.eval_points(torch.empty((0, 3), device=dev()), [mc, mf], embeddings()).shape == (0, 1)


# ------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("n,S,NI", [(1, 64, 64), (3, 64, 128), (5, 3, 1), (2, 512, 0), (129, 17, 33)])
def test_ragged_and_extreme_shapes_vs_oracle(n, S, NI):
    """1 ray, sizes that are no multiple of the 32-point / 64-lane tiles, the smallest legal sample_pdf (S=3 -> one pdf
    bin), the largest samples-per-ray the compositor supports (512 = 8 per lane)."""
    import sinnerf_amd
    mc, pc = make_model(0, True)
    mf, pf = make_model(1, True)
    rays_np = O.lego_rays(400, 400, seed=1)[:: 160000 // n][:n]
    r = np.random.RandomState(n + S)
    rng = {"perturb": r.uniform(0, 1, (n, S)).astype(np.float32), "noise_coarse": r.standard_normal((n, S)).astype(np.float32)}
    if NI:
        rng.update(u=r.uniform(0, 1, (n, NI)).astype(np.float32), noise_fine=r.standard_normal((n, S + NI)).astype(np.float32))
    meta = dict(N_samples=S, N_importance=NI, perturb=1.0, noise_std=0.5)
    ref = O.render_rays([pc, pf], rays_np, S, False, 1.0, 0.5, NI, 32768, True, False, rng=rng)
    with torch.no_grad(), injected_rng(rng_order(meta, rng, n)) as left:
        res = sinnerf_amd.render_rays([mc, mf], embeddings(), torch.from_numpy(rays_np).to(dev()), S, False, 1.0, 0.5, NI, 32768, True)
        assert not left
    # tiny S makes the fine depths extremely sensitive to the cdf's last bit (one wide bin): looser opacity bar there
    check_render(to_np(res), ref, tag=f"n{n}_S{S}_NI{NI}", opa=1e-4 if S >= 17 else 5e-3, rel=1e-3 if S >= 17 else 5e-3)


def test_empty_batch_and_unsupported_sizes():
    import sinnerf_amd
    from sinnerf_amd._lib import SinnerfHipError
    mc, _ = make_model(0, True)
    mf, _ = make_model(1, True)
    with torch.no_grad():
        res = sinnerf_amd.render_rays([mc, mf], embeddings(), torch.zeros((0, 8), device=dev()), 64, False, 0, 0, 64, 32768, True)
    assert res["rgb_fine"].shape == (0, 3) and res["opacity_fine"].shape == (0, 128) and res["depth_coarse"].shape == (0,)
    with torch.no_grad():                            # 600 samples per ray (10 per lane) render fine ...
        r600 = sinnerf_amd.render_rays([mc, mf], embeddings(), torch.rand((4, 8), device=dev()) + 1, 600, False, 0, 0, 0, 32768, True)
    assert r600["opacity_coarse"].shape == (4, 600) and torch.isfinite(r600["rgb_coarse"]).all()
    from sinnerf_amd import _lib                     # ... > 16 samples per lane (1024 per ray): the C-ABI compositor refuses loudly
    z = torch.sort(torch.rand((4, 1100), device=dev()) * 4 + 2, -1)[0].contiguous()
    raw = torch.rand((4, 1100, 4), device=dev())
    o = [torch.empty((4, 3), device=dev()), torch.empty((4,), device=dev()), torch.empty((4, 1100), device=dev())]
    rc = _lib.lib.sn_composite_forward(_lib.ptr(raw), 1, _lib.ptr(z), _lib.ptr(torch.rand((4, 8), device=dev())), None, 0.0, 4, 1100, 1,
                                       _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]), _lib.stream_ptr())
    assert rc != 0
    with pytest.raises(SinnerfHipError):
        _lib.check(rc, "sn_composite_forward")
    # ... and so does render_rays itself for such a call (and for other layer / embedding configurations): there is no general
    # torch-op path, tests/test_training_kernels_system_gpu.py::test_unsupported_configurations_are_refused_loudly


def test_bf16_hand_scheduled_kernel_equals_compiler_scheduled():
    """csrc/sn_mlp_fwd_bf16_v3.hip (generated, hand-scheduled trunk; 7-slot weight ring) against csrc/sn_mlp_fwd_bf16.hip
    (SN_FLAG_BF16_COMPILER_SCHEDULED): same roundings in the same order -> identical bits, on a ragged multi-tile launch
    (more point tiles than one workgroup pass, so the weight stream wraps around between tiles)."""
    from sinnerf_amd import rendering
    model, _ = make_model(1, True, dtype="bf16")
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::7][:20000]).to(dev())       # 20000 x 37 points: 2891 tiles of 256
    z = torch.sort(torch.rand((rays.shape[0], 37), device=dev()) * 4 + 2, -1)[0].contiguous()
    with torch.no_grad():
        a = rendering._mlp(model, rays, z, False, 0)
        b = rendering._mlp(model, rays, z, False, 2)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), (a - b).abs().max().item()
