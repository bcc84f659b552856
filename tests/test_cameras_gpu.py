"""GPU: ray generation for the reference's llff (NDC) and dtu cameras, and their pose gradients -- ``sn_generate_rays_cam``,
``sn_generate_rays_cam_backward``, ``sn_ndc_rays``, ``sn_ndc_rays_backward`` and ``ray_utils.get_rays`` / ``get_ndc_rays`` on top.

Against the existing blender entries bit for bit where the camera is theirs, and against tests/golden/rays_cameras.npz
(tools/gen_golden_cameras.py: the reference's own functions in fp32 and fp64, and its fp64 autograd) everywhere else.  Every bar
is a multiple of the reference's own fp32-vs-fp64 error stored in the fixture.  The tests print what they measure (run with -s)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.helpers import GOLDEN                                                          # noqa: E402
from tests.test_parity_gpu import dev, embeddings, make_model                             # noqa: E402

FULL = None


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(f"{GOLDEN}/rays_cameras.npz"))


@functools.lru_cache(maxsize=None)
def blender_frame():
    z = np.load(f"{GOLDEN}/rays.npz")
    return int(z["H"]), int(z["W"]), float(z["focal"]), z["c2w"].astype(np.float32)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def norm_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def window_of(H, W, window):
    return tuple(window) if window is not None else (0, 0, 1, 1, W, H)


def blender_cam(H, W, focal):
    """(fx, fy, cx, cy, convention, ndc, ndc_focal, ndc_near) of the camera sn_generate_rays has built in"""
    return (focal, focal, W / 2, H / 2, 0, 0, focal, 0.0)


def cam_rays(c2w, H, W, cam, near, far, window=FULL, out=None):
    from sinnerf_amd import _lib as L
    win = window_of(H, W, window)
    rays = torch.full((max(win[4] * win[5], 1), 8), float("nan"), dtype=torch.float32, device=dev()) if out is None else out
    L.check(L.lib.sn_generate_rays_cam(L.ptr(c2w), H, W, *cam, near, far, *win, L.ptr(rays), L.stream_ptr()), "sn_generate_rays_cam")
    return rays[:win[4] * win[5]]


def plain_rays(c2w, H, W, focal, near, far, window=FULL):
    from sinnerf_amd import _lib as L
    win = window_of(H, W, window)
    rays = torch.full((win[4] * win[5], 8), float("nan"), dtype=torch.float32, device=dev())
    L.check(L.lib.sn_generate_rays(L.ptr(c2w), H, W, focal, near, far, *win, L.ptr(rays), L.stream_ptr()), "sn_generate_rays")
    return rays


def workspace():
    from sinnerf_amd import _lib as L
    return torch.empty(int(L.lib.sn_generate_rays_backward_workspace_bytes()), dtype=torch.uint8, device=dev())


def cam_backward(g, c2w, H, W, cam, window=FULL):
    from sinnerf_amd import _lib as L
    ws, out = workspace(), torch.full((3, 4), float("nan"), dtype=torch.float32, device=dev())
    L.check(L.lib.sn_generate_rays_cam_backward(L.ptr(g), L.ptr(c2w), H, W, *cam, *window_of(H, W, window), L.ptr(ws), L.ptr(out),
                                                L.stream_ptr()), "sn_generate_rays_cam_backward")
    return out


def plain_backward(g, H, W, focal, window=FULL):
    from sinnerf_amd import _lib as L
    ws, out = workspace(), torch.full((3, 4), float("nan"), dtype=torch.float32, device=dev())
    L.check(L.lib.sn_generate_rays_backward(L.ptr(g), H, W, focal, *window_of(H, W, window), L.ptr(ws), L.ptr(out), L.stream_ptr()),
            "sn_generate_rays_backward")
    return out


def seeded(n, seed):
    return torch.randn((n, 8), generator=torch.Generator().manual_seed(seed)).to(dev())


# ---- 1. the blender camera through the new entries: the bits of the existing ones -----------------------------------------------
def test_forward_identity_with_sn_generate_rays():
    H, W, focal, c2w_np = blender_frame()
    c2w = t(c2w_np)
    for hh, ww, ff, window in ((H, W, focal, FULL), (H, W, focal, (3, 2, 4, 3, 7, 5)),
                               (960, 1100, 1234.5, FULL)):                       # 1 056 000 rays > 4096 x 256: the grid-stride loop wraps
        got = cam_rays(c2w, hh, ww, blender_cam(hh, ww, ff), 2.0, 6.0, window)
        assert torch.equal(got, plain_rays(c2w, hh, ww, ff, 2.0, 6.0, window)), (hh, ww, window)
    assert got.shape == (1056000, 8)


def test_backward_identity_with_sn_generate_rays_backward():
    c2w = t(blender_frame()[3])
    H, W, focal = 260, 300, 311.25                                               # 78 000 rays > 256 x 256: block cap and stride
    g = seeded(H * W, 1)
    for window in (FULL, (7, 5, 1, 1, 1, 1), (2, 1, 3, 2, 90, 100)):
        win = window_of(H, W, window)
        gw = g[:win[4] * win[5]].contiguous()
        ref = plain_backward(gw, H, W, focal, window)
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        assert torch.equal(cam_backward(gw, c2w, H, W, blender_cam(H, W, focal), window), ref), window
        assert torch.equal(cam_backward(gw, None, H, W, blender_cam(H, W, focal), window), ref)       # c2w is not read without NDC
    for cam in (blender_cam(H, W, focal), (focal, focal, W / 2, H / 2, 0, 1, focal, 1.0)):            # an empty window writes 12 zeros
        for window in ((0, 0, 1, 1, 0, 0), (5, 5, 1, 1, 0, 3)):
            assert torch.equal(cam_backward(g, c2w, H, W, cam, window), torch.zeros((3, 4), device=dev()))
    assert torch.equal(plain_backward(g, H, W, focal, (0, 0, 1, 1, 0, 0)), torch.zeros((3, 4), device=dev()))
    sentinel = torch.full((4, 8), 7.0, device=dev())                                                  # ... and no ray
    cam_rays(c2w, H, W, blender_cam(H, W, focal), 2.0, 6.0, (0, 0, 1, 1, 0, 3), out=sentinel)
    assert (sentinel == 7.0).all()


# ---- 2. forward against the reference ----------------------------------------------------------------------------------------
def llff_rays(c2w, window=None):
    from sinnerf_amd.ray_utils import get_rays
    z = fixture()
    return get_rays(int(z["llff_H"]), int(z["llff_W"]), float(z["llff_focal"]), c2w, float(z["llff_near"]), float(z["llff_far"]), window,
                    ndc_near=float(z["llff_ndc_near"]))


def dtu_rays(c2w, window=None):
    from sinnerf_amd.ray_utils import get_rays
    z = fixture()
    return get_rays(int(z["dtu_H"]), int(z["dtu_W"]), tuple(z["dtu_focal"]), c2w, float(z["dtu_near"]), float(z["dtu_far"]), window,
                    center=tuple(z["dtu_center"]), convention="opencv")


CASES = {"llff": llff_rays, "dtu": dtu_rays}


@pytest.mark.parametrize("case", ["llff", "dtu"])
def test_forward_against_reference(case):
    """|rays - fp64 reference| <= 4 e_ref, e_ref = max |reference fp32 - reference fp64| (the 3-term directions @ R^T sum is where the
    order of operations may differ from the reference's matmul; everything else is the reference's ops one rounding each).
    Achieved on the MI355X: llff 3.5e-7 (e_ref 3.5e-7), dtu 7.3e-8 (e_ref 6.3e-8)."""
    z = fixture()
    H, W = int(z[f"{case}_H"]), int(z[f"{case}_W"])
    c2w = t(z[f"{case}_c2w"])
    rays = CASES[case](c2w)
    got = rays.cpu().numpy()
    ref64, e_ref = z[f"{case}_rays64"], float(z[f"{case}_e_ref"])
    assert got.shape == ref64.shape == (H * W, 8) and got.dtype == np.float32 and not rays.requires_grad
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{case}: max |rays - ref64| = {err:.3e}, e_ref = {e_ref:.3e}, bit-equal to ref32: {np.array_equal(got, z[f'{case}_rays32'])}")
    assert err <= 4 * e_ref, (err, e_ref)
    assert np.array_equal(got[:, 6:], z[f"{case}_rays32"][:, 6:])                               # near, far as the dataset packs them
    # a strided window is those pixels of the frame, bit for bit
    x0, y0, sx, sy, pw, ph = win = (2, 1, 3, 2, 9, 10)
    sub = CASES[case](c2w, win)
    assert torch.equal(sub, rays.view(H, W, 8)[y0:y0 + ph * sy:sy, x0:x0 + pw * sx:sx].reshape(-1, 8))


# ---- 3. get_ndc_rays on rays that exist already ------------------------------------------------------------------------------
def test_standalone_ndc_against_reference():
    """Every op of get_ndc_rays is reproduced with one fp32 rounding, in its order: on the reference's own fp32 world rays the result
    is the reference's fp32 result bit for bit (so 3.5e-7 = e_ref from the fp64 one).  In place is allowed (include/sinnerf_hip.h)."""
    from sinnerf_amd import _lib as L
    from sinnerf_amd.ray_utils import get_ndc_rays
    z = fixture()
    H, W, focal, near = int(z["llff_H"]), int(z["llff_W"]), float(z["llff_focal"]), float(z["llff_ndc_near"])
    world = t(z["llff_world32"])
    o, d = get_ndc_rays(H, W, focal, near, world[:, 0:3], world[:, 3:6])
    assert o.shape == d.shape == (H * W, 3)
    got = torch.cat([o, d], 1).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - z["llff_rays64"][:, :6]).max())
    print(f"get_ndc_rays: max |rays - ref64| = {err:.3e}, e_ref = {float(z['llff_e_ref']):.3e}")
    assert err <= 4 * float(z["llff_e_ref"])
    assert np.array_equal(got, z["llff_rays32"][:, :6])
    # the C entry: columns 6, 7 pass through; in place gives the same bits
    rays = torch.cat([world, t(np.tile(np.float32([2.5, 7.5]), (H * W, 1)))], 1).contiguous()
    out = torch.full_like(rays, float("nan"))
    L.check(L.lib.sn_ndc_rays(L.ptr(rays), H * W, H, W, focal, near, L.ptr(out), L.stream_ptr()), "sn_ndc_rays")
    assert np.array_equal(out.cpu().numpy()[:, :6], got) and (out[:, 6] == 2.5).all() and (out[:, 7] == 7.5).all()
    L.check(L.lib.sn_ndc_rays(L.ptr(rays), H * W, H, W, focal, near, L.ptr(rays), L.stream_ptr()), "sn_ndc_rays")
    assert torch.equal(rays, out)


# ---- 4. its backward -----------------------------------------------------------------------------------------------------------
def test_ndc_backward_against_reference():
    """n = 1073 (ragged last block).  Norm-wise error of dL/d(rays_o, rays_d) against the reference's fp64 autograd <= 8x the error of
    the reference's own fp32 autograd on the same data (7.7e-8, in the fixture): the margin is for recomputed intermediates and the
    order of the sums.  Achieved on the MI355X: 7.8e-8."""
    from sinnerf_amd import _lib as L
    from sinnerf_amd.ray_utils import get_ndc_rays
    z = fixture()
    H, W, focal, near = int(z["llff_H"]), int(z["llff_W"]), float(z["llff_focal"]), float(z["llff_ndc_near"])
    n = H * W
    assert n == 1073
    rays = torch.cat([t(z["llff_world32"]), torch.zeros((n, 2), device=dev())], 1).contiguous()
    g = t(z["llff_g"])                                                                          # columns 6, 7 are not zero: ignored
    g_in = torch.full((n, 8), float("nan"), dtype=torch.float32, device=dev())
    L.check(L.lib.sn_ndc_rays_backward(L.ptr(rays), L.ptr(g), n, H, W, focal, near, L.ptr(g_in), L.stream_ptr()), "sn_ndc_rays_backward")
    got = g_in.cpu().numpy()
    err, bar = norm_err(got[:, :6], z["llff_g_world64"]), 8 * float(z["llff_err32_world"])
    print(f"sn_ndc_rays_backward: norm-wise error {err:.3e}, reference fp32 autograd {float(z['llff_err32_world']):.3e}")
    assert np.isfinite(got).all() and err <= bar, (err, bar)
    assert (got[:, 6:] == 0).all()
    # the same through autograd
    o, d = rays[:, 0:3].clone().requires_grad_(), rays[:, 3:6].clone().requires_grad_()
    no, nd = get_ndc_rays(H, W, focal, near, o, d)
    ((no * g[:, 0:3]).sum() + (nd * g[:, 3:6]).sum()).backward()
    assert torch.equal(o.grad, g_in[:, 0:3]) and torch.equal(d.grad, g_in[:, 3:6])


# ---- 5. pose gradient through the camera -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["llff", "dtu"])
def test_pose_gradient_against_reference(case):
    """get_rays with c2w.requires_grad, L = sum(rays * g): dL/dc2w against the reference's fp64 autograd, norm-wise, <= 8x the error of
    the reference's own fp32 autograd (llff 4.6e-7, dtu 2.7e-7, in the fixture).  Achieved on the MI355X: llff 1.1e-7, dtu 3.2e-8."""
    z = fixture()
    g = t(z[f"{case}_g"])
    grads = []
    for _ in range(2):
        c2w = t(z[f"{case}_c2w"]).requires_grad_()
        rays = CASES[case](c2w)
        assert rays.requires_grad
        (rays * g).sum().backward()
        grads.append(c2w.grad.clone())
    assert torch.equal(grads[0], grads[1])                                                     # fixed summation order, no atomics
    assert torch.equal(rays.detach(), CASES[case](t(z[f"{case}_c2w"])))                        # asking for the gradient moves no bit
    with torch.no_grad():
        assert not CASES[case](t(z[f"{case}_c2w"]).requires_grad_()).requires_grad
    err, ref32 = norm_err(grads[0].cpu().numpy(), z[f"{case}_g_c2w64"]), float(z[f"{case}_err32_c2w"])
    print(f"{case}: dL/dc2w norm-wise error {err:.3e}, reference fp32 autograd {ref32:.3e}")
    assert torch.isfinite(grads[0]).all() and err <= 8 * ref32, (err, ref32)
    # a strided window sums those pixels only: the full-frame call with the other rows of g zeroed (fp64 partials in another order)
    H, W = int(z[f"{case}_H"]), int(z[f"{case}_W"])
    x0, y0, sx, sy, pw, ph = win = (2, 1, 3, 2, 9, 10)
    keep = torch.zeros((H, W, 1), device=dev())
    keep[y0:y0 + ph * sy:sy, x0:x0 + pw * sx:sx] = 1.0
    gw = g.view(H, W, 8)[y0:y0 + ph * sy:sy, x0:x0 + pw * sx:sx].reshape(-1, 8)
    pair = []
    for upstream, window in ((gw, win), (g * keep.view(-1, 1), None)):
        c2w = t(z[f"{case}_c2w"]).requires_grad_()
        (CASES[case](c2w, window) * upstream).sum().backward()
        pair.append(c2w.grad.cpu().numpy())
    assert norm_err(pair[0], pair[1]) <= 2.0 ** -23                                            # one fp32 rounding of each of the 12 sums


# ---- 6. end to end: c2w -> NDC rays -> render_rays -> loss ----------------------------------------------------------------------
def test_end_to_end_llff_pose_gradient():
    """c2w.grad of sum(rgb_fine) through get_rays(ndc_near=1) and render_rays == the chain of its two parts taken separately:
    rays.grad of render_rays on the detached NDC rays (tests/test_ray_grads_gpu.py holds it to fp64), then
    sn_generate_rays_cam_backward.  Both sides run the same fp32 kernels on the same values; 1e-5 pins the wiring."""
    import sinnerf_amd
    from sinnerf_amd.ray_utils import get_rays
    z = fixture()
    H, W, focal = 5, 6, 7.0
    models = [make_model(2, True)[0].train(), make_model(3, True)[0].train()]
    render = lambda rays: sinnerf_amd.render_rays(models, embeddings(), rays, 8, False, 0, 0, 8, 32768, False)["rgb_fine"]
    c2w = t(z["llff_c2w"]).requires_grad_()
    rays = get_rays(H, W, focal, c2w, 0.0, 1.0, ndc_near=1.0)
    assert rays.shape == (30, 8) and rays.requires_grad
    render(rays).sum().backward()
    assert c2w.grad is not None and torch.isfinite(c2w.grad).all()
    parts = rays.detach().clone().requires_grad_()
    render(parts).sum().backward()
    ref = cam_backward(parts.grad.contiguous(), c2w.detach(), H, W, (focal, focal, W / 2, H / 2, 0, 1, focal, 1.0))
    assert ref.abs().max() > 0
    err = norm_err(c2w.grad.cpu().numpy(), ref.cpu().numpy())
    print(f"end to end: ||c2w.grad - chain|| / ||chain|| = {err:.3e}")
    assert err <= 1e-5, err


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from sinnerf_amd._lib import SinnerfHipError
    from sinnerf_amd.ray_utils import get_ndc_rays, get_rays
    z = fixture()
    c2w = t(z["dtu_c2w"])
    H, W = 23, 31
    with pytest.raises(SinnerfHipError):
        cam_rays(c2w, H, W, (38.0, 36.5, 14.2, 12.7, 2, 0, 38.0, 0.0), 0.5, 3.5)                # convention not in {0, 1}
    with pytest.raises(SinnerfHipError):
        cam_backward(seeded(H * W, 3), c2w, H, W, (38.0, 36.5, 14.2, 12.7, -1, 0, 38.0, 0.0))
    with pytest.raises(ValueError):
        get_rays(H, W, (38.0, 36.5), c2w, 0.5, 3.5, convention="colmap")
    with pytest.raises(SinnerfHipError):
        get_rays(H, W, (0.0, 36.5), c2w, 0.5, 3.5, convention="opencv")                         # fx = 0
    with pytest.raises(SinnerfHipError):
        get_rays(H, W, 0.0, c2w, 0.0, 1.0, ndc_near=1.0)
    with pytest.raises(SinnerfHipError):
        get_rays(H, W, 38.0, c2w, 0.0, 1.0, window=(25, 0, 4, 1, 3, 5), ndc_near=1.0)           # window leaves the image
    with pytest.raises(SinnerfHipError):
        get_ndc_rays(H, W, float("nan"), 1.0, torch.zeros((4, 3), device=dev()), torch.ones((4, 3), device=dev()))
    with pytest.raises(ValueError):
        get_rays(H, W, (38.0, 36.5), c2w, 0.0, 1.0, ndc_near=1.0)                               # the NDC map has one focal length
    with pytest.raises(RuntimeError):
        get_rays(H, W, (38.0, 36.5), c2w.cpu(), 0.5, 3.5, convention="opencv")
    with pytest.raises(RuntimeError):
        get_ndc_rays(H, W, 38.0, 1.0, torch.zeros(4, 3), torch.ones(4, 3))
