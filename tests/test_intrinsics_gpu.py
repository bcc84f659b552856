"""GPU: the camera intrinsics on the device -- ``sn_generate_rays_cam_dev``, ``sn_generate_rays_cam_dev_backward``, ``sn_ndc_rays_dev``,
``sn_ndc_rays_dev_backward`` and ``ray_utils.get_rays`` / ``get_ndc_rays`` / ``warp.unseen_view_batch`` with tensor ``focal`` / ``center``.

Bit for bit against the host-float entries wherever both compute the same thing (rays, g_c2w, g_rays_in), and the new gradient
dL/d(fx, fy, cx, cy) against tests/golden/rays_intrinsics.npz (tools/gen_golden_intrinsics.py: the reference's fp64 autograd with
``focal`` / ``center`` as leaves, and the error of its own fp32 autograd as the yardstick).  The tests print what they measure (-s)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import intrinsics_np as N                                                      # noqa: E402
from tests.helpers import GOLDEN                                                          # noqa: E402
from tests.test_cameras_gpu import (FULL, cam_backward, cam_rays, dev, fixture as cam_fixture, norm_err, seeded, t,   # noqa: E402
                                    window_of)
from tests.test_parity_gpu import embeddings, make_model                                  # noqa: E402

K = 8
CASES = ("llff", "blender", "dtu")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(f"{GOLDEN}/rays_intrinsics.npz"))


@functools.lru_cache(maxsize=None)
def upstreams(case):
    """the K upstream gradients of a case, on the device once"""
    z = fixture()
    n = int(z[f"{case}_H"]) * int(z[f"{case}_W"])
    return tuple(t(N.upstream(n, seed)) for seed in z[f"{case}_seeds"])


def host_cam(case, H=None, W=None, focal=None):
    """(fx, fy, cx, cy, convention, ndc, ndc_focal, ndc_near) of a fixture case for the host-float entries, optionally at another size"""
    z = fixture()
    h, w, fx, fy, cx, cy, s, ndc_near = N.case_camera(z, case)
    if H is not None:
        fx, fy, cx, cy = (focal, focal, W / 2, H / 2) if case != "dtu" else (fx * W / w, fy * H / h, cx * W / w, cy * H / h)
    return (fx, fy, cx, cy, int(s > 0), int(ndc_near is not None), fx, ndc_near or 0.0)


def dev_args(cam):
    """host camera tuple -> (intr tensor, convention, ndc, ndc_near) of the device entries: the same fp32 values"""
    fx, fy, cx, cy, convention, ndc, _, ndc_near = cam
    return torch.tensor([fx, fy, cx, cy], dtype=torch.float32).to(dev()), convention, ndc, ndc_near


def dev_rays(c2w, H, W, cam, near, far, window=FULL):
    from sinnerf_amd import _lib as L
    intr, convention, ndc, ndc_near = dev_args(cam)
    win = window_of(H, W, window)
    rays = torch.full((win[4] * win[5], 8), float("nan"), dtype=torch.float32, device=dev())
    L.check(L.lib.sn_generate_rays_cam_dev(L.ptr(c2w), L.ptr(intr), H, W, convention, ndc, ndc_near, near, far, *win, L.ptr(rays),
                                           L.stream_ptr()), "sn_generate_rays_cam_dev")
    return rays


def dev_backward(g, c2w, H, W, cam, window=FULL, want=(True, True)):
    """(g_c2w, g_intr); an output not wanted is passed as NULL and returned as None"""
    from sinnerf_amd import _lib as L
    intr, convention, ndc, ndc_near = dev_args(cam)
    ws = torch.empty(int(L.lib.sn_camera_backward_workspace_bytes()), dtype=torch.uint8, device=dev())
    g_c2w = torch.full((3, 4), float("nan"), dtype=torch.float32, device=dev()) if want[0] else None
    g_intr = torch.full((4,), float("nan"), dtype=torch.float32, device=dev()) if want[1] else None
    L.check(L.lib.sn_generate_rays_cam_dev_backward(L.ptr(g), L.ptr(c2w), L.ptr(intr), H, W, convention, ndc, ndc_near, *window_of(H, W, window),
                                                    L.ptr(ws), L.ptr(g_c2w), L.ptr(g_intr), L.stream_ptr()), "sn_generate_rays_cam_dev_backward")
    return g_c2w, g_intr


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def bar(err32):
    """8 x the reference's own fp32 error (the margin tests/test_cameras_gpu.py gives the pose gradient, for recomputed intermediates and
    the order of the sums), and no less than 8 x 2^-24, the rounding of the fp32 result itself"""
    return 8 * max(float(err32), 2.0 ** -24)


def groups(case):
    """column groups of G64 and their yardsticks"""
    z = fixture()
    if case == "dtu":
        return (("focal", slice(0, 2), z["dtu_err32_focal"]), ("centre", slice(2, 4), z["dtu_err32_center"]))
    return (("focal", slice(0, 1), z[f"{case}_err32_focal"]),)


def fold(case, g_intr):
    """g_intr (.., 4) -> the columns of G64: one focal length is fx = fy, its gradient the fp32 sum autograd forms"""
    return g_intr if case == "dtu" else (g_intr[..., 0] + g_intr[..., 1])[..., None]


# ---- 1. forward: the bits of the host-float entries ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_identity_with_the_host_float_entries(case):
    z = fixture()
    H, W = int(z[f"{case}_H"]), int(z[f"{case}_W"])
    c2w = t(z[f"{case}_c2w"])
    for hh, ww, ff, window in ((H, W, None, FULL), (H, W, None, (3, 2, 4, 3, 7, 5)),
                               (960, 1100, 1234.5, FULL)):                       # 1 056 000 rays > 4096 x 256: the grid-stride loop wraps
        cam = host_cam(case) if ff is None else host_cam(case, hh, ww, ff)
        got, ref = dev_rays(c2w, hh, ww, cam, 0.25, 5.5, window), cam_rays(c2w, hh, ww, cam, 0.25, 5.5, window)
        assert torch.isfinite(ref).all() and same_bits(got, ref), (case, hh, ww, window)
    assert got.shape == (1056000, 8)


def test_ndc_forward_identity_with_sn_ndc_rays():
    from sinnerf_amd import _lib as L
    zc = cam_fixture()
    H, W, focal, near = int(zc["llff_H"]), int(zc["llff_W"]), float(zc["llff_focal"]), float(zc["llff_ndc_near"])
    n = H * W
    rays = torch.cat([t(zc["llff_world32"]), t(np.tile(np.float32([2.5, 7.5]), (n, 1)))], 1).contiguous()
    f = torch.tensor([focal], dtype=torch.float32).to(dev())
    ref, got = torch.full_like(rays, float("nan")), torch.full_like(rays, float("nan"))
    L.check(L.lib.sn_ndc_rays(L.ptr(rays), n, H, W, focal, near, L.ptr(ref), L.stream_ptr()), "sn_ndc_rays")
    L.check(L.lib.sn_ndc_rays_dev(L.ptr(rays), n, H, W, L.ptr(f), near, L.ptr(got), L.stream_ptr()), "sn_ndc_rays_dev")
    assert torch.isfinite(ref).all() and same_bits(got, ref)
    L.check(L.lib.sn_ndc_rays_dev(L.ptr(rays), n, H, W, L.ptr(f), near, L.ptr(rays), L.stream_ptr()), "sn_ndc_rays_dev")      # in place
    assert same_bits(rays, ref)


# ---- 2. backward: g_c2w has the bits of sn_generate_rays_cam_backward --------------------------------------------------------------
@pytest.mark.parametrize("ndc", [0, 1])
def test_backward_identity_with_sn_generate_rays_cam_backward(ndc):
    c2w = t(cam_fixture()["llff_c2w"])                                            # forward facing: d_z < 0 at every pixel, NDC is finite
    H, W, focal = 260, 300, 311.25                                               # 78 000 rays > 256 x 256: block cap and stride
    cam = (focal, focal, W / 2, H / 2, 0, ndc, focal, 1.0 if ndc else 0.0)
    g = seeded(H * W, 1)
    for window in (FULL, (7, 5, 1, 1, 1, 1), (2, 1, 3, 2, 90, 100)):
        win = window_of(H, W, window)
        gw = g[:win[4] * win[5]].contiguous()
        ref = cam_backward(gw, c2w, H, W, cam, window)
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        g_c2w, g_intr = dev_backward(gw, c2w, H, W, cam, window)
        assert same_bits(g_c2w, ref), window
        assert torch.isfinite(g_intr).all() and (g_intr != 0).all(), window
        only_pose, none = dev_backward(gw, c2w, H, W, cam, window, want=(True, False))     # a NULL output moves no bit of the other
        assert none is None and same_bits(only_pose, ref)
        none, only_intr = dev_backward(gw, c2w, H, W, cam, window, want=(False, True))
        assert none is None and same_bits(only_intr, g_intr)
    for window in ((0, 0, 1, 1, 0, 0), (5, 5, 1, 1, 0, 3)):                       # an empty window writes 12 + 4 zeros
        g_c2w, g_intr = dev_backward(g, c2w, H, W, cam, window)
        assert same_bits(g_c2w, torch.zeros((3, 4), device=dev())) and same_bits(g_intr, torch.zeros(4, device=dev()))


# ---- 3. g_intr against the reference's fp64 autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_intrinsics_gradient_against_reference(case):
    """L_k = sum(rays * g_k), K = 8 upstreams: Frobenius-norm relative error of dL/d(focal[, centre]) over the K rows against the
    reference's fp64 autograd <= 8 max(err32, 2^-24), err32 the error of the reference's own fp32 autograd (fixture: llff 2.3e-7,
    blender 2.1e-7, dtu focal 1.1e-7 / centre 9.9e-8).  Achieved on the MI355X: llff 1.3e-7, blender 3.6e-8, dtu focal 4.0e-8 / centre
    2.0e-8; two runs give the same bits."""
    z = fixture()
    H, W = int(z[f"{case}_H"]), int(z[f"{case}_W"])
    c2w, cam = t(z[f"{case}_c2w"]), host_cam(case)
    runs = [torch.stack([dev_backward(g, c2w, H, W, cam, want=(False, True))[1] for g in upstreams(case)]) for _ in range(2)]
    assert same_bits(runs[0], runs[1])                                            # fixed summation order, no atomics
    got = fold(case, runs[0]).cpu().numpy()
    assert got.shape == z[f"{case}_G64"].shape and np.isfinite(got).all()
    for name, cols, err32 in groups(case):
        err = norm_err(got[:, cols], z[f"{case}_G64"][:, cols])
        print(f"{case} {name}: ||g_intr - G64|| / ||G64|| = {err:.3e}, reference fp32 autograd {float(err32):.3e}, bar {bar(err32):.3e}")
        assert err <= bar(err32), (case, name, err, bar(err32))


# ---- 4. windows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_strided_window_sums_its_pixels_only(case):
    """the window's g_intr == the full-frame call with the other rows of g zeroed (fp64 partials in another order: one fp32 rounding)"""
    z = fixture()
    H, W = int(z[f"{case}_H"]), int(z[f"{case}_W"])
    c2w, cam, g = t(z[f"{case}_c2w"]), host_cam(case), upstreams(case)[0]
    x0, y0, sx, sy, pw, ph = win = (2, 1, 3, 2, 9, 10)
    keep = torch.zeros((H, W, 1), device=dev())
    keep[y0:y0 + ph * sy:sy, x0:x0 + pw * sx:sx] = 1.0
    gw = g.view(H, W, 8)[y0:y0 + ph * sy:sy, x0:x0 + pw * sx:sx].reshape(-1, 8).contiguous()
    a = dev_backward(gw, c2w, H, W, cam, win)[1].cpu().numpy()
    b = dev_backward((g * keep.view(-1, 1)).contiguous(), c2w, H, W, cam)[1].cpu().numpy()
    assert np.abs(b).min() > 0 and norm_err(a, b) <= 2.0 ** -23, (a, b)


# ---- 5. autograd through get_rays -------------------------------------------------------------------------------------------------
def rays_of(case, c2w, focal, center=None, window=None):
    """get_rays on a fixture case with whatever focal / center are given (numbers or tensors)"""
    from sinnerf_amd.ray_utils import get_rays
    z = fixture()
    H, W = int(z[f"{case}_H"]), int(z[f"{case}_W"])
    kw = dict(center=center, convention="opencv") if case == "dtu" else (dict(ndc_near=float(z["llff_ndc_near"])) if case == "llff" else {})
    return get_rays(H, W, focal, c2w, float(z[f"{case}_near"]), float(z[f"{case}_far"]), window, **kw)


def numbers(case):
    z = fixture()
    return (tuple(float(v) for v in z["dtu_focal"]), tuple(float(v) for v in z["dtu_center"])) if case == "dtu" else (float(z[f"{case}_focal"]), None)


def leaf(v, grad=True):
    return torch.tensor(v, dtype=torch.float32).to(dev()).requires_grad_(grad)


@pytest.mark.parametrize("case", CASES)
def test_autograd_through_get_rays(case):
    """focal.grad (and center.grad for dtu) of L_k = sum(get_rays(...) * g_k) against the fixture's totals (for llff the NDC terms are in
    them), held to the bar of test 3 (achieved on the MI355X: the figures of test 3, 1.3e-7 / 3.6e-8 / 4.0e-8 and 2.0e-8); what does
    not require grad gets none and moves no bit of what does."""
    z = fixture()
    c2w_np, (focal_n, center_n) = z[f"{case}_c2w"], numbers(case)
    host = rays_of(case, t(c2w_np), focal_n, center_n)                                         # the host-float path
    rows = []
    for g in upstreams(case):
        focal, center = leaf(focal_n), (leaf(center_n) if case == "dtu" else None)
        rays = rays_of(case, t(c2w_np), focal, center)
        assert rays.requires_grad and same_bits(rays.detach(), host)                           # asking for the gradient moves no bit
        (rays * g).sum().backward()
        assert focal.grad.shape == focal.shape
        rows.append(torch.cat([focal.grad.reshape(-1)] + ([center.grad] if case == "dtu" else [])))
    got = torch.stack(rows).cpu().numpy()
    for name, cols, err32 in groups(case):
        err = norm_err(got[:, cols], z[f"{case}_G64"][:, cols])
        print(f"{case} {name}: ||grad - G64|| / ||G64|| = {err:.3e}, bar {bar(err32):.3e}")
        assert err <= bar(err32), (case, name, err)
    g = upstreams(case)[-1]
    # only c2w requires grad: the bits of the host path's pose gradient
    pose = []
    for focal, center in ((leaf(focal_n, False), leaf(center_n, False) if case == "dtu" else None), (focal_n, center_n)):
        c2w = t(c2w_np).requires_grad_()
        (rays_of(case, c2w, focal, center) * g).sum().backward()
        pose.append(c2w.grad)
    assert same_bits(pose[0], pose[1])
    # everything requires grad: the same bits again, each from the one pass
    c2w, focal, center = t(c2w_np).requires_grad_(), leaf(focal_n), (leaf(center_n) if case == "dtu" else None)
    (rays_of(case, c2w, focal, center) * g).sum().backward()
    assert same_bits(c2w.grad, pose[1]) and same_bits(focal.grad.reshape(-1), torch.from_numpy(got[-1, :focal.numel()]).to(dev()))
    with torch.no_grad():
        assert not rays_of(case, t(c2w_np).requires_grad_(), leaf(focal_n), leaf(center_n) if case == "dtu" else None).requires_grad
    assert not rays_of(case, t(c2w_np), leaf(focal_n, False), leaf(center_n, False) if case == "dtu" else None).requires_grad


def test_autograd_only_centre_requires_grad():
    """dtu with only the principal point learnt, the focal lengths a tensor without grad, with grad, or plain numbers: the same
    center.grad bits, held to the bar of test 3"""
    z = fixture()
    focal_n, center_n = numbers("dtu")
    per_focal = []
    for focal in (leaf(focal_n, False), leaf(focal_n, True), focal_n):
        rows = []
        for g in upstreams("dtu"):
            center = leaf(center_n)
            (rays_of("dtu", t(z["dtu_c2w"]), focal, center) * g).sum().backward()
            rows.append(center.grad)
        per_focal.append(torch.stack(rows))
        if torch.is_tensor(focal):
            assert (focal.grad is None) == (not focal.requires_grad)
    assert same_bits(per_focal[0], per_focal[1]) and same_bits(per_focal[0], per_focal[2])
    err = norm_err(per_focal[0].cpu().numpy(), z["dtu_G64"][:, 2:])
    print(f"dtu centre alone: {err:.3e}, bar {bar(z['dtu_err32_center']):.3e}")
    assert err <= bar(z["dtu_err32_center"]), err


# ---- 6. get_ndc_rays with a tensor focal ------------------------------------------------------------------------------------------
def test_get_ndc_rays_with_a_tensor_focal():
    """forward and o.grad / d.grad: the bits of the float path; focal.grad against the fp64 autograd of get_ndc_rays alone at the same
    fp32 world rays, <= 8 max(err32, 2^-24) over the K upstreams (err32 1.3e-7 in the fixture).  Achieved on the MI355X: 5.2e-8."""
    from sinnerf_amd.ray_utils import get_ndc_rays
    z, zc = fixture(), cam_fixture()
    H, W, focal_n, near = int(z["llff_H"]), int(z["llff_W"]), float(z["llff_focal"]), float(z["llff_ndc_near"])
    world = t(zc["llff_world32"])

    def run(focal, g):
        o, d = world[:, 0:3].clone().requires_grad_(), world[:, 3:6].clone().requires_grad_()
        no, nd = get_ndc_rays(H, W, focal, near, o, d)
        ((no * g[:, 0:3]).sum() + (nd * g[:, 3:6]).sum()).backward()
        return no.detach(), nd.detach(), o.grad, d.grad

    rows = []
    for g in upstreams("llff"):
        focal = leaf(focal_n)
        assert all(same_bits(a, b) for a, b in zip(run(focal, g), run(focal_n, g)))
        assert focal.grad.shape == ()
        rows.append(focal.grad)
    got = torch.stack(rows).cpu().numpy()
    err, b = norm_err(got, z["llff_ndc_G64"]), bar(z["llff_ndc_err32"])
    print(f"get_ndc_rays: ||focal.grad - G64|| / ||G64|| = {err:.3e}, reference fp32 autograd {float(z['llff_ndc_err32']):.3e}, bar {b:.3e}")
    assert np.isfinite(got).all() and err <= b, (err, b)
    focal = leaf([focal_n], False)                                                             # (1,), no grad: still the device path
    assert all(same_bits(a, b) for a, b in zip(run(focal, g), run(focal_n, g))) and focal.grad is None


# ---- 7. end to end: focal -> NDC rays -> render_rays -> loss -----------------------------------------------------------------------
def test_end_to_end_llff_focal_gradient():
    """focal.grad of sum(rgb_fine) through get_rays(ndc_near=1) and render_rays == the chain of its two parts taken separately:
    rays.grad of render_rays on the detached NDC rays (tests/test_ray_grads_gpu.py holds it to fp64), then
    sn_generate_rays_cam_dev_backward.  Both sides run the same fp32 kernels on the same values; 1e-5 pins the wiring."""
    import sinnerf_amd
    from sinnerf_amd.ray_utils import get_rays
    H, W, focal_n = 5, 6, 7.0
    models = [make_model(2, True)[0].train(), make_model(3, True)[0].train()]
    render = lambda rays: sinnerf_amd.render_rays(models, embeddings(), rays, 8, False, 0, 0, 8, 32768, False)["rgb_fine"]
    c2w, focal = t(cam_fixture()["llff_c2w"]), leaf(focal_n)
    rays = get_rays(H, W, focal, c2w, 0.0, 1.0, ndc_near=1.0)
    assert rays.shape == (30, 8) and rays.requires_grad
    render(rays).sum().backward()
    assert focal.grad is not None and torch.isfinite(focal.grad).all()
    parts = rays.detach().clone().requires_grad_()
    render(parts).sum().backward()
    g_intr = dev_backward(parts.grad.contiguous(), c2w, H, W, (focal_n, focal_n, W / 2, H / 2, 0, 1, focal_n, 1.0), want=(False, True))[1]
    ref = (g_intr[0] + g_intr[1]).cpu().numpy()
    assert abs(ref) > 0
    err = norm_err(focal.grad.cpu().numpy(), ref)
    print(f"end to end: |focal.grad - chain| / |chain| = {err:.3e}")
    assert err <= 1e-5, err


# ---- 8. no sync: the call and its backward in one captured graph --------------------------------------------------------------------
def test_get_rays_and_its_backward_are_capturable():
    """get_rays with tensor focal and centre plus its backward captured in one torch.cuda.graph on one stream (a host read of the
    intrinsics would fail the capture); after an in-place change of the focal tensor a replay gives the rays and the focal.grad of
    an eager call at the new value, bit for bit."""
    z = fixture()
    (focal_n, center_n), g = numbers("dtu"), upstreams("dtu")[0]
    c2w = t(z["dtu_c2w"])
    focal, center = leaf(focal_n), leaf(center_n)

    def step():
        rays = rays_of("dtu", c2w, focal, center)
        (rays * g).sum().backward()
        return rays

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                              # warm-up off the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    focal.grad = center.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rays = step()
    new_focal = (35.25, 39.5)
    with torch.no_grad():
        focal.copy_(leaf(new_focal, False))
    graph.replay()
    torch.cuda.synchronize()
    e_focal, e_center = leaf(new_focal), leaf(center_n)
    e_rays = rays_of("dtu", c2w, e_focal, e_center)
    (e_rays * g).sum().backward()
    assert same_bits(rays.detach(), e_rays.detach())
    assert same_bits(focal.grad, e_focal.grad) and same_bits(center.grad, e_center.grad)
    assert not same_bits(e_rays.detach(), rays_of("dtu", c2w, focal_n, center_n))             # the new value was seen


# ---- 9. the warp takes device intrinsics --------------------------------------------------------------------------------------------
def test_unseen_view_batch_with_tensor_intrinsics():
    from sinnerf_amd import warp
    from tests.test_warp_gpu import unseen_inputs
    c, a = unseen_inputs()
    H, W = int(c["H"]), int(c["W"])
    want = warp.unseen_view_batch(**dict(a, center=(W / 2, H / 2)))
    got = warp.unseen_view_batch(**dict(a, focal=leaf(a["focal"]), center=leaf((W / 2, H / 2))))
    plain = warp.unseen_view_batch(**a)
    assert set(got) == set(want) == set(plain)
    for key in want:
        for x, y, w in zip(*(v if isinstance(v, tuple) else (v,) for v in (got[key], want[key], plain[key]))):
            assert torch.equal(x, y) and torch.equal(x, w), key
            assert not x.requires_grad, key                                                     # labels carry no gradient
    assert got["rays_full"].abs().max() > 0


# ---- 10. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from sinnerf_amd.ray_utils import get_ndc_rays, get_rays
    z = fixture()
    c2w = t(z["dtu_c2w"])
    H, W = 23, 31
    with pytest.raises(ValueError):
        get_rays(H, W, leaf((38.0, 36.5)), c2w, 0.0, 1.0, ndc_near=1.0)                        # the NDC map has one focal length
    with pytest.raises(ValueError):
        get_rays(H, W, (38.0, 36.5), c2w, 0.0, 1.0, center=leaf((14.2, 12.7)), ndc_near=1.0)
    with pytest.raises(RuntimeError, match="focal"):
        get_rays(H, W, torch.tensor(38.0, requires_grad=True), c2w, 0.5, 3.5)                  # a CPU tensor that requires grad
    with pytest.raises(RuntimeError, match="center"):
        get_rays(H, W, 38.0, c2w, 0.5, 3.5, center=torch.tensor([14.2, 12.7], requires_grad=True))
    with pytest.raises(RuntimeError, match="focal"):
        get_ndc_rays(H, W, torch.tensor(38.0, requires_grad=True), 1.0, torch.zeros((4, 3), device=dev()), -torch.ones((4, 3), device=dev()))
    for bad in (leaf((38.0, 36.5, 1.0)), leaf([[38.0], [36.5]]), torch.zeros(0, device=dev())):
        with pytest.raises(RuntimeError):
            get_rays(H, W, bad, c2w, 0.5, 3.5)                                                  # wrong shape
    for bad in (leaf(14.2), leaf((14.2, 12.7, 1.0)), leaf([[14.2, 12.7]])):
        with pytest.raises(RuntimeError):
            get_rays(H, W, leaf(38.0), c2w, 0.5, 3.5, center=bad)
    with pytest.raises(RuntimeError):
        get_ndc_rays(H, W, leaf((38.0, 36.5)), 1.0, torch.zeros((4, 3), device=dev()), -torch.ones((4, 3), device=dev()))
    with pytest.raises(ValueError):
        get_rays(H, W, leaf(38.0), c2w, 0.5, 3.5, convention="colmap")
    from sinnerf_amd._lib import SinnerfHipError
    with pytest.raises(SinnerfHipError):
        get_rays(H, W, leaf(38.0), c2w, 0.0, 1.0, window=(25, 0, 4, 1, 3, 5), ndc_near=1.0)    # window leaves the image: still a host check
    # a CPU tensor or a number without grad goes the host path exactly as before; a zero device focal is IEEE arithmetic, not an error
    host = get_rays(H, W, 38.0, c2w, 0.5, 3.5)
    assert torch.equal(get_rays(H, W, torch.tensor(38.0), c2w, 0.5, 3.5), host) and torch.equal(get_rays(H, W, leaf(38.0, False), c2w, 0.5, 3.5), host)
    assert not torch.isfinite(get_rays(H, W, leaf(0.0, False), c2w, 0.5, 3.5)).all()
