"""GPU: ``sn_reproject_loss`` (csrc/sn_reproject.hip) against the numpy oracle of tests/reproject_oracle.py, the exact families of its
definition, its NULL outputs, determinism and refusals, the autograd surface of ``sinnerf_amd.reprojection``, the agreement of its
conventions with ``get_rays`` and ``warp.projection_matrix``, and the terms in ``SinNeRFSystem``.

Bars: ``RO.bar(x64, x32) = max(4 e32, 1e-6)``, e32 = the error of the oracle's own fp32 evaluation on the same inputs; a scalar by relative
error, a gradient and a per-pixel vector by relative L2 norm; flags and counts are exact.  Every comparison of values or gradients runs on
inputs where no pixel is within 1e-3 of a decision boundary (``RO.assert_margins``); nothing is filtered out.

End to end (test_parameter_gradients_end_to_end), fp32 probe nets, 64 rays at 8 + 8: relative L2 over the fine network's flat parameter
gradient between the kernel's upstream gradients and the fp64 oracle's cast to fp32.  The bar is 4 x the same figure with the oracle's
gradients moved by one fp32 ulp per element in a random direction -- the sensitivity of the backward to the last bit of its input, which
no implementation of the loss can beat.  The figures are printed; DESIGN.md 3.12 records them."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                                            # noqa: E402
from tests import probe_nets as PN                                                           # noqa: E402
from tests import reproject_oracle as RO                                                     # noqa: E402
from tests.test_parity_gpu import dev, embeddings                                            # noqa: E402

SHAPES = RO.SHAPES + [(63, 5, 7, 3), (64, 5, 7, 3)]                          # (n, H, W, C)
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.7, 0.3)]
BADARG, TOOLARGE = -1, -2
PARAMS = (RO.OCC_TOL, RO.CHARB_EPS, RO.Z_MIN, RO.OPACITY_THRESHOLD)
ALL = ("g_depth", "g_rgb", "per_pixel", "flags")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def inputs(n, H, W, C):
    return RO.recipe(n, H, W, C)


@functools.lru_cache(maxsize=None)
def reference(n, H, W, C, w_photo, w_free):
    """(fp64 evaluation, fp32 evaluation) of the oracle on inputs(n, H, W, C): computed once, shared, never modified"""
    args = RO.call_args(inputs(n, H, W, C))
    return RO.evaluate(*args, w_photo, w_free), RO.evaluate(*args, w_photo, w_free, dtype=np.float32)


def call(inp, w_photo, w_free, want=ALL, use_opacity=True, null=(), params=PARAMS, **override):
    """the raw entry on the arrays of `inp`; every output pre-filled with NaN (flags: 0xFF) -> (code, out, dict of the outputs, None
    where not wanted).  override: n, C, H, W passed instead of the arrays' own; null: names of inputs passed as NULL"""
    from sinnerf_amd import _lib
    n, C = inp["rgb"].shape
    H, W = inp["ref_depth"].shape
    d = {k: t(inp[k]) for k in ("rays", "depth", "rgb", "opacity", "ref_image", "ref_depth", "ref_proj")}
    assert d["ref_proj"].dtype == torch.float64
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev())
    outs = {"g_depth": nan(max(n, 1)), "g_rgb": nan(max(n, 1), C), "per_pixel": nan(max(n, 1), 2),
            "flags": torch.full((max(n, 1),), 255, dtype=torch.uint8, device=dev())}
    outs = {k: (v if k in want else None) for k, v in outs.items()}
    out = nan(6)
    nbytes = _lib.lib.sn_reproject_loss_workspace_bytes(n)
    assert nbytes >= 40
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    p = lambda k: None if k in null else _lib.ptr(d[k])
    code = _lib.lib.sn_reproject_loss(p("rays"), p("depth"), p("rgb"), p("opacity") if use_opacity else None, override.get("n", n),
                                      override.get("C", C), p("ref_image"), p("ref_depth"), override.get("H", H), override.get("W", W),
                                      p("ref_proj"), *params, w_photo, w_free, _lib.ptr(outs["g_depth"]), _lib.ptr(outs["g_rgb"]),
                                      _lib.ptr(outs["per_pixel"]), _lib.ptr(outs["flags"]), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return code, out, outs


def compare(tag, got_out, got, r64, r32):
    """flags and counts exactly, every value and gradient at RO.bar; prints the figures first"""
    RO.assert_margins(r64)
    assert np.array_equal(got["flags"], r64["flags"]), tag
    assert list(got_out[3:]) == list(r64["out"][3:]), (tag, got_out[3:], r64["out"][3:])
    rows = [("photo", got_out[0], r64["out"][0], r32["out"][0]), ("free", got_out[1], r64["out"][1], r32["out"][1]),
            ("total", got_out[2], r64["out"][2], r32["out"][2]),
            ("per_pixel photo", got["per_pixel"][:, 0], r64["photo_i"], r32["photo_i"]),
            ("per_pixel free", got["per_pixel"][:, 1], r64["free_i"], r32["free_i"]),
            ("g_depth", got["g_depth"], r64["g_depth"], r32["g_depth"]), ("g_rgb", got["g_rgb"], r64["g_rgb"], r32["g_rgb"])]
    figures = [(name, RO.rel(g, x64), RO.rel(x32, x64), RO.bar(x64, x32)) for name, g, x64, x32 in rows]
    for name, err, e32, b in figures:
        print(f"{tag} {name}: kernel {err:.3e}, oracle fp32 {e32:.3e}, bar {b:.3e}")
    for name, err, e32, b in figures:
        assert err <= b, (tag, name, err, b)


@pytest.mark.parametrize("w_photo,w_free", WEIGHTS)
@pytest.mark.parametrize("n,H,W,C", SHAPES)
def test_raw_entry_against_the_oracle(n, H, W, C, w_photo, w_free):
    r64, r32 = reference(n, H, W, C, w_photo, w_free)
    code, out, outs = call(inputs(n, H, W, C), w_photo, w_free)
    assert code == 0
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    out = out.cpu().numpy()
    assert np.isfinite(out).all() and all(np.isfinite(got[k]).all() for k in ("g_depth", "g_rgb", "per_pixel"))     # nothing left unwritten
    off = (r64["flags"] & 2) == 0                                            # exactly 0 where a mask is off
    assert not got["g_rgb"][off].any() and not got["per_pixel"][off, 0].any()
    assert not got["g_depth"][(r64["flags"] & 6) == 0].any()
    compare(f"({n}, {H}, {W}, {C}) w=({w_photo}, {w_free})", out, got, r64, r32)


def test_without_opacity_every_pixel_takes_part():
    inp = dict(inputs(65, 5, 7, 3))
    inp["opacity"] = np.zeros_like(inp["opacity"])                           # would exclude every pixel if it were read
    args = list(RO.call_args(inp))
    args[3] = None
    code, out, outs = call(inp, 0.7, 0.3, use_opacity=False)
    assert code == 0
    compare("no opacity", out.cpu().numpy(), {k: v.cpu().numpy() for k, v in outs.items()}, RO.evaluate(*args, 0.7, 0.3),
            RO.evaluate(*args, 0.7, 0.3, dtype=np.float32))
    code, out, outs = call(inp, 0.7, 0.3)
    assert code == 0 and not out.any().item() and not outs["flags"].any().item() and not outs["g_depth"].any().item()


# ---- the exact families, on the lattice camera P = [I | 0], o = 0, d = (x, y, 1): u = x exactly --------------------------------------
LH, LW, LC = 5, 7, 3


def lattice_call(change=None, params=PARAMS):
    inp = RO.lattice(LH, LW, LC)
    if change is not None:
        change(inp)
    code, out, outs = call(inp, 1.0, 1.0, params=params)
    assert code == 0
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    out = out.cpu().numpy()
    assert np.isfinite(out).all() and all(np.isfinite(v).all() for v in got.values())          # no NaN leaks from an invalid pixel
    return inp, out, got


def zero_where(got, off):
    return not got["g_depth"][off].any() and not got["g_rgb"][off].any() and not got["per_pixel"][off].any()


def test_lattice_every_pixel_visible_and_the_last_row_and_column_inside():
    inp, out, got = lattice_call()
    n = LH * LW
    assert (got["flags"] == 3).all() and list(out[3:]) == [n, n, 0]          # u = W - 1 and v = H - 1 are inside
    eps = np.float32(RO.CHARB_EPS)
    assert out[0] == eps and out[1] == 0 and out[2] == eps and (got["per_pixel"][:, 0] == eps).all() and not got["per_pixel"][:, 1].any()
    assert not got["g_rgb"].any()                                            # rgb == the image exactly: s = 0


def test_lattice_invalid_families():
    def outside(inp):
        inp["rays"][0, 3], inp["rays"][1, 3], inp["rays"][2, 4], inp["rays"][3, 4] = -0.5, LW - 0.5, -0.5, LH - 0.5
    _, out, got = lattice_call(outside)
    assert (got["flags"][:4] == 0).all() and (got["flags"][4:] == 3).all() and zero_where(got, slice(0, 4)) and out[4] == LH * LW - 4

    def bad_depth(inp):
        inp["depth"][:4] = [np.nan, 0.0, -1.0, np.inf]
    _, out, got = lattice_call(bad_depth)
    assert (got["flags"][:4] == 0).all() and (got["flags"][4:] == 3).all() and zero_where(got, slice(0, 4))

    def nan_rays(inp):
        inp["rays"][0, 0], inp["rays"][1, 4], inp["rgb"][5, 1] = np.nan, np.inf, 0.25
    _, out, got = lattice_call(nan_rays)
    assert (got["flags"][:2] == 0).all() and (got["flags"][2:] == 3).all() and zero_where(got, slice(0, 2)) and got["g_rgb"][5, 1] > 0

    _, out, got = lattice_call(params=(RO.OCC_TOL, RO.CHARB_EPS, 1.5, RO.OPACITY_THRESHOLD))   # z = 1 everywhere, z_min = 1.5
    assert not got["flags"].any() and not out.any() and zero_where(got, slice(None))

    def low_opacity(inp):
        inp["opacity"][::2] = 0.5                                            # not ABOVE the threshold
    _, out, got = lattice_call(low_opacity)
    assert (got["flags"][::2] == 0).all() and (got["flags"][1::2] == 3).all() and zero_where(got, slice(0, None, 2))

    def hole(inp):
        inp["ref_depth"][2, 3] = 0.0
    inp, out, got = lattice_call(hole)
    col, row = inp["rays"][:, 3], inp["rays"][:, 4]
    x0, y0 = np.minimum(col, LW - 2), np.minimum(row, LH - 2)
    touched = ((x0 == 3) | (x0 + 1 == 3)) & ((y0 == 2) | (y0 + 1 == 2))      # the pixels whose four corners include (3, 2)
    assert touched.sum() == 4 and (got["flags"][touched] == 0).all() and (got["flags"][~touched] == 3).all() and zero_where(got, touched)


def test_lattice_front_and_behind_by_hand():
    def move(inp):
        inp["depth"][0], inp["depth"][1], inp["rgb"][1, 0] = 0.5, 2.0, 0.0   # z = 0.5: r = -0.5; z = 2: r = 1
    _, out, got = lattice_call(move)
    n = LH * LW
    tol = np.float64(np.float32(RO.OCC_TOL))
    assert got["flags"][0] == 5 and got["flags"][1] == 1 and (got["flags"][2:] == 3).all() and list(out[3:]) == [n - 2, n, 1]
    assert got["per_pixel"][0, 1] == np.float32(0.5 - tol) and out[1] == np.float32((0.5 - tol) / n)
    # D = 1 is constant and z = t, so r_t = 1: d total / d t_0 = -1 / n_geo; the occluded pixel gets nothing, whatever its colour
    assert got["g_depth"][0] == np.float32(-1.0 / n) and got["g_depth"][1] == 0 and not got["g_rgb"][:2].any()
    assert not got["g_depth"][2:].any()                                      # visible with rgb == image: s = 0 exactly


def test_nothing_valid_gives_exact_zeros():
    def nothing(inp):
        inp["ref_depth"][:] = 0.0
    _, out, got = lattice_call(nothing)
    assert not out.any() and not got["flags"].any() and zero_where(got, slice(None))


# ---- NULL outputs, determinism, refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,C", [(65, 5, 7, 3), (257, 33, 17, 4)])
def test_null_outputs_leave_the_others_bit_identical_and_two_calls_agree(n, H, W, C):
    inp = inputs(n, H, W, C)
    code, out, full = call(inp, 0.7, 0.3)
    assert code == 0
    code2, out2, again = call(inp, 0.7, 0.3)
    assert code2 == 0 and torch.equal(out, out2) and all(torch.equal(full[k], again[k]) for k in ALL)
    for drop in ALL + (ALL,):
        drop = (drop,) if isinstance(drop, str) else drop
        code3, out3, part = call(inp, 0.7, 0.3, want=tuple(k for k in ALL if k not in drop))
        assert code3 == 0 and torch.equal(out, out3), drop
        assert all(part[k] is None if k in drop else torch.equal(full[k], part[k]) for k in ALL), drop


def test_error_codes():
    from sinnerf_amd import _lib
    inp = inputs(65, 5, 7, 3)
    untouched = lambda out, outs: torch.isnan(out).all() and all(torch.isnan(outs[k]).all() for k in ("g_depth", "g_rgb", "per_pixel"))
    for kw in (dict(null=("rays",)), dict(null=("depth",)), dict(null=("rgb",)), dict(null=("ref_image",)), dict(null=("ref_depth",)),
               dict(null=("ref_proj",)), dict(H=1), dict(W=1), dict(C=0), dict(C=5)):
        code, out, outs = call(inp, 1.0, 1.0, **kw)
        assert code == BADARG and untouched(out, outs), kw                   # refused before any launch
    for kw in (dict(n=1 << 31), dict(H=32768, W=32768, C=2)):
        code, out, outs = call(inp, 1.0, 1.0, **kw)
        assert code == TOOLARGE and untouched(out, outs), kw
    assert _lib.lib.sn_reproject_loss_workspace_bytes(1 << 31) == TOOLARGE
    code, out, outs = call(inp, 1.0, 1.0, n=0)
    assert code == 0 and not out.any().item() and torch.isnan(outs["g_depth"]).all()


def test_autograd_hands_out_the_kernels_gradients_bit_for_bit():
    import sinnerf_amd
    inp = inputs(257, 33, 17, 4)
    _, out, raw = call(inp, 0.7, 0.3)
    rays, depth0, rgb0, opacity, img, dep, P = (t(a) for a in RO.call_args(inp))
    for factor in (1.0, 3.0):
        depth, rgb = depth0.clone().requires_grad_(True), rgb0.clone().requires_grad_(True)
        total, stats = sinnerf_amd.reprojection_loss(rays, depth, rgb, img, dep, P, opacity=opacity, w_photo=0.7, w_free=0.3)
        assert not any(v.requires_grad for v in stats.values())
        (factor * total if factor != 1.0 else total).backward()
        assert torch.equal(depth.grad, factor * raw["g_depth"] if factor != 1.0 else raw["g_depth"])
        assert torch.equal(rgb.grad, factor * raw["g_rgb"] if factor != 1.0 else raw["g_rgb"])
        assert torch.equal(total.detach(), out[2])
        assert all(torch.equal(stats[k], out[i]) and stats[k].dim() == 0 for i, k in enumerate(("photo", "free", "total", "n_vis", "n_geo", "n_front")))
        assert torch.equal(stats["flags"], raw["flags"]) and torch.equal(stats["per_pixel"], raw["per_pixel"])
    # only one input asks for a gradient; none does; an empty batch
    depth = depth0.clone().requires_grad_(True)
    total, _ = sinnerf_amd.reprojection_loss(rays, depth, rgb0, img, dep, P, opacity=opacity, w_photo=0.7, w_free=0.3)
    total.backward()
    assert torch.equal(depth.grad, raw["g_depth"])
    total, _ = sinnerf_amd.reprojection_loss(rays, depth0, rgb0, img, dep, P, opacity=opacity, w_photo=0.7, w_free=0.3)
    assert not total.requires_grad and torch.equal(total, out[2])
    total, stats = sinnerf_amd.reprojection_loss(rays[:0], depth0[:0], rgb0[:0], img, dep, P)
    assert total.item() == 0 and stats["per_pixel"].shape == (0, 2) and stats["flags"].shape == (0,)
    # refusals that need a device: the frame and the matrix
    for bad in ((img.permute(2, 0, 1), dep, P), (img[:, :-1], dep, P), (img, dep, P.float()), (img, dep, P[:3])):
        with pytest.raises(RuntimeError, match="channel-last|float64"):
            sinnerf_amd.reprojection_loss(rays, depth0, rgb0, *bad)


# ---- the conventions: get_rays, warp.projection_matrix and this loss name the same pixel ----------------------------------------------
def test_the_reference_views_own_rays_and_depth_land_on_their_own_pixels():
    import sinnerf_amd
    from sinnerf_amd import warp
    from sinnerf_amd.ray_utils import get_rays
    H, W, focal = 33, 17, 20.5
    image, depth_map = RO.frame(H, W, 3)
    depth_map[4:7, 5:8] = 0.0                                                # background: a 3 x 3 hole, and one pixel
    depth_map[20, 11] = 0.0
    ang = np.deg2rad([20.0, -35.0, 10.0])
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    c2w = t(np.concatenate([R, [[0.3], [-1.1], [2.4]]], 1).astype(np.float32))
    K = t(np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]))     # the centre get_rays defaults to
    rays = get_rays(H, W, focal, c2w, 0.5, 6.0)
    P = warp.projection_matrix(K, warp.extrinsics_from_c2w(c2w, "opengl")).contiguous()
    total, stats = sinnerf_amd.reprojection_loss(rays, t(depth_map).reshape(-1), t(image).reshape(-1, 3), t(image), t(depth_map), P)
    flags = stats["flags"].cpu().numpy().reshape(H, W)
    positive = np.pad(depth_map > 0, 1, constant_values=False)
    around = np.ones((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            around &= positive[dy:dy + H, dx:dx + W]                         # the 3 x 3 block: each of the four cells the pixel may fall into
    assert around.sum() == (H - 2) * (W - 2) - 25 - 9 and (flags[around] == 3).all()
    assert (flags[depth_map == 0] == 0).all() and stats["n_front"].item() == 0
    ref = RO.evaluate(rays.cpu().numpy(), depth_map.reshape(-1), image.reshape(-1, 3), None, image, depth_map, P.cpu().numpy())
    assert np.array_equal(stats["flags"].cpu().numpy(), ref["flags"]) and np.abs(ref["r"]).max() < 1e-5
    err = RO.rel(stats["photo"].item(), ref["out"][0])
    print(f"reference view onto itself: {int(stats['n_vis'].item())} of {H * W} visible, photo {stats['photo'].item():.9g} (charb_eps "
          f"{RO.CHARB_EPS}), against the oracle {err:.3e}, max |r| {np.abs(ref['r']).max():.3e}")
    assert err <= 1e-6 and abs(stats["photo"].item() - RO.CHARB_EPS) < 1e-6


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def probe_models():
    import sinnerf_amd
    models = []
    for name in ("wide", "low"):
        m = sinnerf_amd.NeRF(use_new_activation=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in PN.head_params(name).items()})
        models.append(m.to(dev()).train())
    return models


def test_parameter_gradients_end_to_end():
    """figures on the MI355X: see DESIGN.md 3.12"""
    import sinnerf_amd
    mc, mf = probe_models()
    rays = t(PN.head_rays()[0][:64])
    res = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 8, False, 0.0, 0.0, 8, 32768, True)
    depth, rgb = res["depth_fine"], res["rgb_fine"]
    assert depth.requires_grad and rgb.requires_grad and depth.min().item() > 0.05
    # the rays of the LOSS are aimed by the recipe so that the rendered depths reach its targets: margins by construction
    inp = RO.recipe(64, 33, 17, 3, seed=1, t=depth.detach().cpu().numpy())
    inp["rgb"] = rgb.detach().cpu().numpy()
    r64 = RO.evaluate(*RO.call_args(inp), 0.7, 0.3)
    RO.assert_margins(r64)
    assert r64["V"].sum() > 10 and r64["front"].sum() > 10
    params = [p for p in mf.parameters()]
    flat = lambda grads: torch.cat([torch.zeros_like(p).reshape(-1) if g is None else g.reshape(-1) for g, p in zip(grads, params)]).double()
    total, stats = sinnerf_amd.reprojection_loss(t(inp["rays"]), depth, rgb, t(inp["ref_image"]), t(inp["ref_depth"]), t(inp["ref_proj"]),
                                                 opacity=t(inp["opacity"]), w_photo=0.7, w_free=0.3)
    assert np.array_equal(stats["flags"].cpu().numpy(), r64["flags"])
    got = flat(torch.autograd.grad(total, params, retain_graph=True, allow_unused=True))
    rs = np.random.RandomState(0)

    def moved(g):
        up = rs.randint(0, 2, g.shape).astype(bool)
        return np.where(up, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))).astype(np.float32)

    through = lambda g_d, g_c: flat(torch.autograd.grad([depth, rgb], params, grad_outputs=[t(g_d), t(g_c)], retain_graph=True,
                                                        allow_unused=True))
    g_d, g_c = r64["g_depth"].astype(np.float32), r64["g_rgb"].astype(np.float32)
    want, shifted = through(g_d, g_c), through(moved(g_d), moved(g_c))
    assert want.norm().item() > 0
    err = ((got - want).norm() / want.norm()).item()
    sens = ((shifted - want).norm() / want.norm()).item()
    print(f"end to end: kernel vs oracle gradients {err:.3e}; oracle gradients moved by one fp32 ulp per element {sens:.3e}; bar {4 * sens:.3e}")
    assert sens > 0
    assert err <= 4 * sens, (err, sens)


# ---- SinNeRFSystem ---------------------------------------------------------------------------------------------------------------------
from tests.test_ray_regularizers_gpu import PATCH, patch_batch, step, system                 # noqa: E402

FH = FW = 2 * PATCH + 1                          # a frame with one 2 x 2 cell of its own per pixel of the side patch
HP0 = dict(perturb=0.0, noise_std=0.0)           # no random draws: a render can be repeated bit for bit


CENTRE = (0.2, -0.1, -4.0)                       # the reference camera: at the lego cameras' distance, looking along +z at the origin


def teacher_system(seed=3, **hp):
    """system() with the oracle's teacher parameters in both networks: a randomly initialised pair renders depth 0 along these rays
    (no pixel would take part); the teacher field is opaque around the origin"""
    sysm = system(seed, **hp)
    for m, s in ((sysm.nerf_coarse, 0), (sysm.nerf_fine, 1)):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in O.init_params(s, True).items()})
    return sysm


def side_rays():
    """the side patch's rays from the reference camera's own centre (P = K [I | -c], o = c): pixel i aims at (u*, v*) inside cell i of the
    frame, fractional parts in [0.1, 0.9], whatever depth is rendered; z = t"""
    rs = np.random.RandomState(11)
    n = PATCH * PATCH
    cell = np.arange(n)
    us, vs = 2 * (cell % PATCH) + rs.uniform(0.1, 0.9, n), 2 * (cell // PATCH) + rs.uniform(0.1, 0.9, n)
    K = RO.intrinsics(FH, FW)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = CENTRE
    rays[:, 3:6] = np.stack([us, vs, np.ones(n)], 1) @ np.linalg.inv(K).T
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    E = np.eye(4)
    E[:3, 3] = -np.asarray(CENTRE, dtype=np.float32).astype(np.float64)
    return rays, RO.projection(K, E)


def reprojection_batch(seed=3):
    """patch_batch() with the side rays above and a reference view built AFTER one render of them by teacher_system(seed) (the terms
    off): cell i's four depths are D_i = z_fine / (1 + r*) with r* of family i % 3 (0, -3 tol, +3 tol), moved in steps of tol / 5 until
    the coarse render's residual is 5e-3 away from the boundaries too; the opacity threshold is the middle of the widest gap among the
    lower third of the rendered opacities (below all of them where no gap is 4e-3 wide).  -> (batch, hparams): no pixel of either pass is near a decision boundary, by construction."""
    rays, P = side_rays()
    batch = dict(patch_batch(), rays_side=t(rays))
    with torch.no_grad():
        side = teacher_system(seed, **HP0)(batch["rays_side"])
    z = {k: side["depth_" + k].double().cpu().numpy() for k in ("fine", "coarse")}
    op = np.sort(np.concatenate([side["opacity_" + k].sum(-1).double().cpu().numpy() for k in ("fine", "coarse")]))
    gap = int(np.argmax(np.diff(op[:len(op) // 3])))                         # in the lower third: most pixels stay in
    thr = float(np.float32((op[gap] + op[gap + 1]) / 2)) if op[gap + 1] - op[gap] >= 4e-3 else float(np.float32(op[0] - 0.01))
    image, depth_map = RO.frame(FH, FW, 3)
    depth_map[:] = 1.0
    tol = RO.OCC_TOL
    clear = lambda r: min(abs(abs(r) - tol), 1.0) >= 5e-3
    for i in range(PATCH * PATCH):
        for k in range(20):
            r_star = (0.0, -3 * tol, 3 * tol)[i % 3] + k * tol / 5
            D = np.float32(z["fine"][i] / (1 + r_star))
            if D > 0 and clear(z["fine"][i] / D - 1) and clear(z["coarse"][i] / D - 1):
                break
        x, y = 2 * (i % PATCH), 2 * (i // PATCH)
        depth_map[y:y + 2, x:x + 2] = D
    batch.update(ref_view=t(image), ref_depth=t(depth_map), ref_proj=t(P))
    return batch, dict(HP0, reproj_occlusion_tol=tol, reproj_opacity_threshold=thr)


def test_system_with_zero_weights_is_the_system_without_the_keys():
    batch, _ = reprojection_batch()
    plain = {k: v for k, v in batch.items() if not k.startswith("ref_")}
    out0, g0 = step(teacher_system(), plain)
    out1, g1 = step(teacher_system(reproj_weight=0.0, freespace_weight=0.0, reproj_occlusion_tol=0.05, reproj_opacity_threshold=0.5), batch)
    assert torch.equal(out0["loss"], out1["loss"]) and torch.equal(g0, g1) and g0.abs().max().item() > 0
    assert list(out0["log"]) == list(out1["log"])
    assert "train/loss_reproj" not in out1["log"] and "train/loss_freespace" not in out1["log"]


def test_system_adds_the_two_terms_on_the_unseen_view_render():
    batch, hp = reprojection_batch()
    off, g_off = step(teacher_system(**hp), batch)
    w_r, w_f = 0.3, 0.2
    sysm = teacher_system(reproj_weight=w_r, freespace_weight=w_f, **hp)
    on, g_on = step(sysm, batch)
    assert "train/loss_reproj" in on["log"] and "train/loss_freespace" in on["log"] and "train/loss_reproj" not in off["log"]
    side = sysm(batch["rays_side"])
    assert side["depth_coarse"].requires_grad                                # so the coarse pair takes part too
    np_ = lambda v: v.detach().cpu().numpy()
    terms, photo, free, counts = [], 0.0, 0.0, []
    for k in ("fine", "coarse"):
        ref = RO.evaluate(np_(batch["rays_side"]), np_(side["depth_" + k]), np_(side["rgb_" + k]), np_(side["opacity_" + k].sum(-1)),
                          np_(batch["ref_view"]), np_(batch["ref_depth"]), np_(batch["ref_proj"]), w_r, w_f,
                          occ_tol=hp["reproj_occlusion_tol"], opacity_threshold=hp["reproj_opacity_threshold"])
        RO.assert_margins(ref)
        terms.append(ref["out"][2])
        photo, free = photo + ref["out"][0], free + ref["out"][1]
        counts.append([int(c) for c in ref["out"][3:]])
    print(f"(n_vis, n_geo, n_front) fine {counts[0]}, coarse {counts[1]}; photo {photo:.9g}, free {free:.9g}")
    assert counts[0][0] > 5 and counts[0][2] > 5                             # pixels the reference camera sees, and pixels in front
    assert RO.rel(on["log"]["train/loss_reproj"].item(), photo) <= 1e-6 and RO.rel(on["log"]["train/loss_freespace"].item(), free) <= 1e-6
    want = off["loss"].item() + sum(terms)
    # the terms at 1e-6 (the kernel's bar), and the step adds the same fp32 numbers in another order: at most four roundings of half an
    # ulp of the running sum on either side
    tolerance = 1e-6 * sum(terms) + 8 * 2.0 ** -24 * max(abs(want), 1.0)
    print(f"loss with the terms {on['loss'].item():.9g}, zero-weight loss + oracle terms {want:.9g}, terms {terms}, tolerance {tolerance:.3g}")
    assert abs(on["loss"].item() - want) <= tolerance
    assert torch.isfinite(g_on).all() and not torch.equal(g_on, g_off)


def test_train_step_graph_replays_the_eager_step_with_the_terms_on():
    batch, hp = reprojection_batch(seed=0)
    finals = {}
    for graph in (False, True):
        sysm = teacher_system(seed=0, reproj_weight=0.3, freespace_weight=0.2, lr=5e-4, **hp)
        losses = []
        for _ in range(3):                                                   # with graph=True: the capture, then two replays
            out = sysm.train_step(batch, graph=graph)
            losses.append(out["loss"].item())
            assert "train/loss_reproj" in out["log"]
        finals[graph] = (sysm.optimizer.flat.clone(), losses)
        if graph:
            assert len(sysm._step_graphs) == 1
    assert finals[True][1] == finals[False][1], (finals[True][1], finals[False][1])
    assert torch.equal(finals[True][0], finals[False][0])
    assert len(set(finals[True][1])) == 3                                    # the parameters moved between the replays


def test_train_step_sampled_graph_with_the_terms_on():
    from tests.test_sampler_gpu import make_sampler
    grads = {}
    for name, hp in (("off", {}), ("on", dict(reproj_weight=0.3, freespace_weight=0.2))):
        sysm = teacher_system(seed=19, proj_weight=0.6, **HP0, **hp)
        s = make_sampler(num=256, generator=torch.Generator(device=dev()).manual_seed(5))     # the same draws for both systems
        before = sysm.optimizer.flat.clone()
        out = sysm.train_step_sampled(s, graph=True)                         # the capture and its first replay
        torch.cuda.synchronize()
        grads[name] = sysm._flat.flat.clone()
        for _ in range(2):
            out = sysm.train_step_sampled(s, graph=True)
            torch.cuda.synchronize()
            assert torch.isfinite(out["loss"])
            if name == "on":
                assert torch.isfinite(out["log"]["train/loss_reproj"]) and torch.isfinite(out["log"]["train/loss_freespace"])
                assert out["batch"]["ref_proj"] is s.ref_proj
        assert len(sysm._step_graphs) == 1
        assert not torch.equal(before, sysm.optimizer.flat) and torch.isfinite(sysm.optimizer.flat).all()
    assert torch.isfinite(grads["on"]).all() and not torch.equal(grads["on"], grads["off"])
    assert "ref_proj" not in s.draw()                                        # the sampler's own dict is what it was


def test_a_batch_without_the_reference_keys_raises():
    batch, hp = reprojection_batch()
    for missing in ("ref_view", "ref_depth", "ref_proj"):
        sysm = system(reproj_weight=0.3, **hp)
        with pytest.raises(RuntimeError, match="need the reference view in the batch.*" + missing):
            sysm.training_step({k: v for k, v in batch.items() if k != missing})


def test_an_ndc_camera_raises():
    from tests.test_sampler_gpu import make_sampler
    s = make_sampler(num=256, ndc_near=1.0)
    for graph in (False, True):
        with pytest.raises(RuntimeError, match="NDC"):
            system(freespace_weight=0.2).train_step_sampled(s, graph=graph)
