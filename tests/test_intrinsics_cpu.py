"""CPU: the entries that read the camera intrinsics from device memory (sn_generate_rays_cam_dev, sn_generate_rays_cam_dev_backward,
sn_camera_backward_workspace_bytes, sn_ndc_rays_dev, sn_ndc_rays_dev_backward) exist with the header's prototypes mirrored in the
binding and refuse bad arguments on the host before anything is launched; the formulas of their backward, restated in fp64 numpy
(tests/intrinsics_np.py), reproduce the reference's fp64 autograd stored in tests/golden/rays_intrinsics.npz
(tools/gen_golden_intrinsics.py); and that fixture is consistent with itself."""
import ctypes
import os

import numpy as np
import pytest

from tests import intrinsics_np as N
from tests.helpers import GOLDEN
from tests.test_cameras_cpu import header_prototype

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sn_generate_rays_cam_dev", "sn_camera_backward_workspace_bytes", "sn_generate_rays_cam_dev_backward", "sn_ndc_rays_dev",
               "sn_ndc_rays_dev_backward")
CASES = ("llff", "blender", "dtu")
K = 8


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def test_intrinsics_symbols_exported_with_the_headers_prototypes():
    from sinnerf_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "sinnerf_hip.h")).read()
    assert L.lib.sn_abi_version() == L.ABI_VERSION == 5                                      # additive within ABI 5
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert getattr(L.lib, name) is not None
        if name != "sn_camera_backward_workspace_bytes":                                      # (void): no argument to parse
            assert header_prototype(hdr, name) == (L.SIGNATURES[name][0], list(L.SIGNATURES[name][1])), name
    # the wider partials: the 12 pose sums and six more (g_fx, g_fy, g_cx, g_cy, g_ax, g_ay) per block; the old query keeps its size
    assert L.lib.sn_generate_rays_backward_workspace_bytes() == 256 * 12 * 8
    assert L.lib.sn_camera_backward_workspace_bytes() == 256 * 18 * 8


def test_intrinsics_argument_checks_run_on_the_host():
    """every refusal below returns before a launch: the pointers are never dereferenced"""
    from sinnerf_amd import _lib as L
    p = ctypes.c_void_p(64)
    BADARG, BADSHAPE = -1, -5
    FULL = (0, 0, 1, 1, 30, 20)
    fwd = lambda **kw: L.lib.sn_generate_rays_cam_dev(kw.get("c2w", p), kw.get("intr", p), kw.get("H", 20), 30, kw.get("convention", 0),
                                                      kw.get("ndc", 0), 1.0, 0.0, 1.0, *kw.get("win", FULL), kw.get("rays", p), None)
    bwd = lambda **kw: L.lib.sn_generate_rays_cam_dev_backward(kw.get("g", p), kw.get("c2w", p), kw.get("intr", p), kw.get("H", 20), 30,
                                                               kw.get("convention", 0), kw.get("ndc", 0), 1.0, *kw.get("win", FULL),
                                                               kw.get("ws", p), kw.get("g_c2w", p), kw.get("g_intr", p), None)
    for f in (fwd, bwd):                                                                      # exactly what check_camera refuses
        assert f(convention=2) == BADARG and f(convention=-1) == BADARG
        assert f(ndc=2) == BADARG and f(ndc=-1) == BADARG
        assert f(H=0) == BADARG
        assert f(win=(28, 0, 1, 1, 3, 20)) == BADSHAPE and f(win=(0, 0, 2, 3, 16, 7)) == BADSHAPE and f(win=(-1, 0, 1, 1, 3, 3)) == BADSHAPE
        assert f(win=(0, 0, 0, 1, 3, 3)) == BADARG and f(win=(0, 0, 1, 1, -1, 3)) == BADARG
        assert f(c2w=None) == BADARG and f(intr=None) == BADARG                               # c2w is always read
    assert fwd(rays=None) == BADARG
    assert fwd(win=(0, 0, 1, 1, 0, 5)) == 0                                                   # no rays: nothing launched
    assert bwd(g=None) == BADARG and bwd(ws=None) == BADARG
    assert bwd(g_c2w=None, g_intr=None) == BADARG                                             # one of the two may be NULL, not both
    ndc = lambda **kw: L.lib.sn_ndc_rays_dev(kw.get("rays", p), kw.get("n", 5), kw.get("H", 20), 30, kw.get("focal", p), 1.0,
                                             kw.get("out", p), None)
    assert ndc(rays=None) == BADARG and ndc(out=None) == BADARG and ndc(focal=None) == BADARG
    assert ndc(n=-1) == BADARG and ndc(H=0) == BADARG
    assert ndc(n=0) == 0                                                                      # no rays: nothing launched
    nbw = lambda **kw: L.lib.sn_ndc_rays_dev_backward(kw.get("rays", p), kw.get("g", p), kw.get("n", 5), 20, kw.get("W", 30),
                                                      kw.get("focal", p), 1.0, kw.get("ws", p), kw.get("g_in", p), kw.get("g_focal", p), None)
    for name in ("rays", "g", "focal", "ws", "g_in", "g_focal"):
        assert nbw(**{name: None}) == BADARG, name
    assert nbw(n=-1) == BADARG and nbw(W=0) == BADARG


def test_python_refusals_need_no_device():
    """a CPU tensor that requires grad is refused by name before anything else is looked at"""
    torch = pytest.importorskip("torch")
    from sinnerf_amd.ray_utils import _on_device
    with pytest.raises(RuntimeError, match="focal"):
        _on_device("focal", torch.tensor(25.0, requires_grad=True))
    with pytest.raises(RuntimeError, match="center"):
        _on_device("center", torch.tensor([15.0, 10.0], requires_grad=True))
    assert _on_device("focal", torch.tensor(25.0)) is False and _on_device("focal", 25.0) is False      # the host path, as before


@pytest.mark.parametrize("case", CASES)
def test_formulas_reproduce_the_reference_fp64_autograd(case):
    """the sums of include/sinnerf_hip.h, in fp64 numpy, against the reference's fp64 autograd: 1e-12 relative, every upstream"""
    z = np.load(f"{GOLDEN}/rays_intrinsics.npz")
    H, W, fx, fy, cx, cy, s, ndc_near = N.case_camera(z, case)
    G64 = z[f"{case}_G64"]
    cols = [0, 1, 2, 3] if case == "dtu" else [0]
    rows = []
    for seed in z[f"{case}_seeds"]:
        full = N.intrinsics_grad(H, W, fx, fy, cx, cy, s, z[f"{case}_c2w"], N.upstream(H * W, seed), ndc_near)
        if case != "dtu":
            full[0] += full[1]                                                                # one focal length: fx = fy = focal
        rows.append(full[cols])
    got = np.stack(rows)
    assert got.shape == G64.shape == (K, len(cols))
    err = rel(got, G64)
    worst = float(np.abs(got / G64 - 1).max())
    print(f"{case}: formulas vs fp64 autograd: norm-wise {err:.3e}, worst entry {worst:.3e}")
    assert err <= 1e-12 and worst <= 1e-12, (err, worst)


def test_ndc_alone_formula_reproduces_the_reference_fp64_autograd():
    z, zc = np.load(f"{GOLDEN}/rays_intrinsics.npz"), np.load(f"{GOLDEN}/rays_cameras.npz")
    H, W = int(z["llff_H"]), int(z["llff_W"])
    got = np.array([N.ndc_focal_grad(H, W, zc["llff_world32"], float(z["llff_ndc_near"]), N.upstream(H * W, seed)) for seed in z["llff_seeds"]])
    worst = float(np.abs(got / z["llff_ndc_G64"] - 1).max())
    print(f"get_ndc_rays alone: worst entry {worst:.3e}")
    assert worst <= 1e-12, worst


def test_fixture_is_consistent():
    """inputs are those of rays_cameras.npz; the stored fp32 yardsticks are fp32 rounding errors and no more"""
    z, zc = np.load(f"{GOLDEN}/rays_intrinsics.npz"), np.load(f"{GOLDEN}/rays_cameras.npz")
    for case, src, shape, ncol in (("llff", "llff", (29, 37), 1), ("blender", "llff", (29, 37), 1), ("dtu", "dtu", (23, 31), 4)):
        assert (int(z[f"{case}_H"]), int(z[f"{case}_W"])) == shape
        assert np.array_equal(z[f"{case}_c2w"], zc[f"{src}_c2w"]) and np.array_equal(z[f"{case}_focal"], zc[f"{src}_focal"])
        assert z[f"{case}_seeds"].shape == (K,) and len(set(z[f"{case}_seeds"].tolist())) == K
        G64 = z[f"{case}_G64"]
        assert G64.shape == (K, ncol) and G64.dtype == np.float64 and np.isfinite(G64).all() and (np.abs(G64) > 0).all()
        G32, nf = z[f"{case}_G32"], min(ncol, 2)
        assert G32.shape == G64.shape and G32.dtype == np.float32
        assert 2.0 ** -26 < float(z[f"{case}_err32_focal"]) < 1e-6 and rel(G32[:, :nf], G64[:, :nf]) <= float(z[f"{case}_err32_focal"])
    assert float(z["llff_focal"]) == 41.5 and float(z["llff_ndc_near"]) == 1.0 and "blender_ndc_near" not in z.files
    assert tuple(z["dtu_focal"]) == (38.0, 36.5) and tuple(z["dtu_center"]) == (14.2, 12.7)
    assert np.array_equal(z["dtu_center"], zc["dtu_center"])
    assert 2.0 ** -26 < float(z["dtu_err32_center"]) < 1e-6 and rel(z["dtu_G32"][:, 2:], z["dtu_G64"][:, 2:]) <= float(z["dtu_err32_center"])
    assert z["llff_ndc_G64"].shape == z["llff_ndc_G32"].shape == (K,)
    assert 2.0 ** -26 < float(z["llff_ndc_err32"]) < 1e-6 and rel(z["llff_ndc_G32"], z["llff_ndc_G64"]) <= float(z["llff_ndc_err32"])
