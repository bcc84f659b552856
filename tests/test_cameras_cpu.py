"""CPU: the camera entries (sn_generate_rays_cam, sn_generate_rays_cam_backward, sn_ndc_rays, sn_ndc_rays_backward) exist in the
library with the header's prototypes mirrored in the binding, refuse bad arguments on the host before anything is launched, and the
fixture the GPU tests read (tests/golden/rays_cameras.npz, tools/gen_golden_cameras.py) is consistent with itself."""
import ctypes
import os
import re

import numpy as np

from tests.helpers import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sn_generate_rays_cam", "sn_generate_rays_cam_backward", "sn_ndc_rays", "sn_ndc_rays_backward")
CTYPE = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int,
         "long": ctypes.c_long, "float": ctypes.c_float}


def header_prototype(hdr, name):
    """(restype, [argtypes]) of `name` as include/sinnerf_hip.h declares it"""
    m = re.search(r"^(int|long)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M)
    assert m, f"{name} is not declared in include/sinnerf_hip.h"
    args = []
    for a in m.group(2).split(","):
        typ = re.sub(r"\s*\*\s*", "* ", " ".join(a.split())).rsplit(" ", 1)[0].strip()      # drop the parameter name
        args.append(CTYPE[typ])
    return CTYPE[m.group(1)], args


def test_camera_symbols_exported_with_the_headers_prototypes():
    from sinnerf_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "sinnerf_hip.h")).read()
    assert L.lib.sn_abi_version() == L.ABI_VERSION == 5                                      # additive within ABI 5
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert getattr(L.lib, name) is not None
        assert header_prototype(hdr, name) == (L.SIGNATURES[name][0], list(L.SIGNATURES[name][1])), name
    # the parser is not vacuous: it reads the entry these generalise the same way
    assert header_prototype(hdr, "sn_generate_rays") == (L.SIGNATURES["sn_generate_rays"][0], list(L.SIGNATURES["sn_generate_rays"][1]))


def test_camera_argument_checks_run_on_the_host():
    """every refusal below returns before a launch: the pointers are never dereferenced"""
    from sinnerf_amd import _lib as L
    p = ctypes.c_void_p(64)
    BADARG, BADSHAPE = -1, -5
    cam = lambda **kw: L.lib.sn_generate_rays_cam(p, 20, 30, kw.get("fx", 25.0), kw.get("fy", 25.0), 15.0, 10.0, kw.get("convention", 0),
                                                  kw.get("ndc", 0), kw.get("ndc_focal", 25.0), 1.0, 0.0, 1.0,
                                                  *kw.get("win", (0, 0, 1, 1, 30, 20)), kw.get("rays", p), None)
    bwd = lambda **kw: L.lib.sn_generate_rays_cam_backward(p, kw.get("c2w", p), 20, 30, kw.get("fx", 25.0), 25.0, 15.0, 10.0,
                                                           kw.get("convention", 0), kw.get("ndc", 0), 25.0, 1.0,
                                                           *kw.get("win", (0, 0, 1, 1, 30, 20)), p, p, None)
    for f in (cam, bwd):
        assert f(convention=2) == BADARG and f(convention=-1) == BADARG
        assert f(ndc=2) == BADARG and f(ndc=-1) == BADARG
        assert f(fx=0.0) == BADARG and f(fx=-3.0) == BADARG and f(fx=float("nan")) == BADARG and f(fx=float("inf")) == BADARG
        assert f(win=(28, 0, 1, 1, 3, 20)) == BADSHAPE and f(win=(0, 0, 2, 3, 16, 7)) == BADSHAPE and f(win=(-1, 0, 1, 1, 3, 3)) == BADSHAPE
        assert f(win=(0, 0, 0, 1, 3, 3)) == BADARG and f(win=(0, 0, 1, 1, -1, 3)) == BADARG
    assert cam(fy=0.0) == BADARG and cam(ndc_focal=0.0) == BADARG and cam(ndc_focal=float("nan"), ndc=1) == BADARG
    assert cam(rays=None) == BADARG
    assert bwd(ndc=1, c2w=None) == BADARG                                                     # c2w is an input once NDC is on
    assert L.lib.sn_ndc_rays(p, 5, 20, 30, 0.0, 1.0, p, None) == BADARG
    assert L.lib.sn_ndc_rays(p, -1, 20, 30, 25.0, 1.0, p, None) == BADARG
    assert L.lib.sn_ndc_rays(None, 5, 20, 30, 25.0, 1.0, p, None) == BADARG
    assert L.lib.sn_ndc_rays(p, 0, 20, 30, 25.0, 1.0, p, None) == 0                         # no rays: nothing launched
    assert L.lib.sn_ndc_rays_backward(p, p, 5, 20, 30, float("inf"), 1.0, p, None) == BADARG
    assert L.lib.sn_ndc_rays_backward(p, p, 5, 20, 0, 25.0, 1.0, p, None) == BADARG
    assert L.lib.sn_ndc_rays_backward(p, None, 5, 20, 30, 25.0, 1.0, p, None) == BADARG


def test_no_cpu_fallback():
    import pytest
    import torch
    from sinnerf_amd.ray_utils import get_ndc_rays, get_rays
    c2w = torch.eye(4)[:3]
    with pytest.raises(RuntimeError):
        get_rays(20, 30, (25.0, 24.0), c2w, 0.5, 3.0, center=(14.0, 9.0), convention="opencv")
    with pytest.raises(RuntimeError):
        get_ndc_rays(20, 30, 25.0, 1.0, torch.zeros(4, 3), torch.ones(4, 3))


def test_fixture_is_consistent():
    """the fp32 and fp64 runs of the reference agree to the bound stored with them, which is an fp32 rounding error and no more"""
    z = np.load(f"{GOLDEN}/rays_cameras.npz")
    for case, (H, W) in (("llff", (29, 37)), ("dtu", (23, 31))):
        r32, r64 = z[f"{case}_rays32"], z[f"{case}_rays64"]
        assert (int(z[f"{case}_H"]), int(z[f"{case}_W"])) == (H, W)
        assert r32.shape == r64.shape == z[f"{case}_g"].shape == (H * W, 8) and r32.dtype == np.float32 and r64.dtype == np.float64
        e_ref = float(z[f"{case}_e_ref"])
        assert np.abs(r32.astype(np.float64) - r64).max() <= e_ref
        assert 0 < e_ref <= 8 * 2.0 ** -24 * np.abs(r64[:, :6]).max()                          # a few ulps of the largest value
        assert (r32[:, 6] == float(z[f"{case}_near"])).all() and (r32[:, 7] == float(z[f"{case}_far"])).all()
        assert z[f"{case}_g_c2w64"].shape == (3, 4) and z[f"{case}_g_c2w64"].dtype == np.float64
        assert 0 < float(z[f"{case}_err32_c2w"]) < 1e-5
    assert float(z["llff_ndc_near"]) == 1.0 and float(z["llff_near"]) == 0.0 and float(z["llff_far"]) == 1.0    # what the llff dataset packs
    assert z["llff_world32"].shape == (29 * 37, 6) and z["llff_g_world64"].shape == (29 * 37, 6)
    assert (z["llff_world32"][:, 5] < 0).all()                                                  # d_z != 0: the map is finite everywhere
    assert 0 < float(z["llff_err32_world"]) < 1e-5
    assert tuple(z["dtu_focal"]) == (38.0, 36.5) and tuple(z["dtu_center"]) == (14.2, 12.7)
