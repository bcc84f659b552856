"""CPU: the patch-loss entries (sn_patch_loss, sn_depth_smoothness and their workspace queries) exist in the library with the header's
prototypes mirrored in the binding and refuse bad arguments on the host before anything is launched; the yardstick of the GPU tests
(tests/patch_loss_oracle.py) is itself pinned -- its autograd gradients against central differences in fp64; and the Python surface
raises where it has nothing to run."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")

from tests import patch_loss_oracle as PO                                              # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sn_patch_loss_workspace_bytes", "sn_patch_loss", "sn_depth_smoothness_workspace_bytes", "sn_depth_smoothness")
CTYPE = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int,
         "long": ctypes.c_long, "float": ctypes.c_float}
BADARG, UNSUPPORTED, BADSHAPE = -1, -4, -5


def header_prototype(hdr, name):
    """(restype, [argtypes]) of `name` as include/sinnerf_hip.h declares it"""
    m = re.search(r"^(int|long)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M)
    assert m, f"{name} is not declared in include/sinnerf_hip.h"
    args = []
    for a in m.group(2).split(","):
        if a.strip() == "void":
            continue
        typ = re.sub(r"\s*\*\s*", "* ", " ".join(a.split())).rsplit(" ", 1)[0].strip()      # drop the parameter name
        args.append(CTYPE[typ])
    return CTYPE[m.group(1)], args


def test_patch_loss_symbols_exported_with_the_headers_prototypes():
    from sinnerf_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "sinnerf_hip.h")).read()
    assert L.lib.sn_abi_version() == L.ABI_VERSION == 5                                      # additive within ABI 5
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert getattr(L.lib, name) is not None
        assert header_prototype(hdr, name) == (L.SIGNATURES[name][0], list(L.SIGNATURES[name][1])), name
    # the parser is not vacuous: it reads an older entry the same way
    assert header_prototype(hdr, "sn_render_loss_workspace_bytes") == (ctypes.c_long, [])
    assert header_prototype(hdr, "sn_ndc_rays") == (L.SIGNATURES["sn_ndc_rays"][0], list(L.SIGNATURES["sn_ndc_rays"][1]))


def test_patch_loss_argument_checks_run_on_the_host():
    """every refusal below returns before a launch: the pointers are never dereferenced"""
    from sinnerf_amd import _lib as L
    p = ctypes.c_void_p(64)

    def pl(coarse=p, fine=p, target=p, shape=(1, 13, 17, 3), use_ssim=1, window=11, ws=p, out=p):
        return L.lib.sn_patch_loss(coarse, fine, target, *shape, use_ssim, window, 1.0, 2.8333, p, p, ws, out, None)

    for use_ssim in (0, 1):
        assert pl(target=None, use_ssim=use_ssim) == BADARG and pl(ws=None, use_ssim=use_ssim) == BADARG
        assert pl(out=None, use_ssim=use_ssim) == BADARG and pl(coarse=None, fine=None, use_ssim=use_ssim) == BADARG
        for k in range(4):
            for bad in (0, -2):
                shape = [1, 13, 17, 3]
                shape[k] = bad
                assert pl(shape=tuple(shape), use_ssim=use_ssim) == BADARG, (k, bad)
    assert pl(fine=None) == BADARG                                                           # the SSIM term is taken on fine
    assert pl(window=10) == BADARG and pl(window=0) == BADARG and pl(window=-3) == BADARG
    assert pl(shape=(1, 13, 17, 2)) == BADARG and pl(shape=(1, 13, 17, 4)) == BADARG
    assert pl(shape=(1, 5, 17, 3)) == BADSHAPE and pl(shape=(1, 13, 5, 3)) == BADSHAPE      # H, W <= window / 2
    assert pl(shape=(1, 2, 2, 1), window=5) == BADSHAPE and pl(shape=(1, 1, 9, 1), window=3) == BADSHAPE
    assert pl(shape=(1, 40, 40, 3), window=33) == UNSUPPORTED                               # the cap the header names
    assert pl(shape=(65536, 256, 256, 3), use_ssim=0) == -2                                 # 2^31 elements or more
    assert L.lib.sn_patch_loss_workspace_bytes(0, 4, 4, 3, 1) == BADARG
    assert L.lib.sn_patch_loss_workspace_bytes(1, 64, 64, 3, 0) > 0
    assert L.lib.sn_patch_loss_workspace_bytes(1, 64, 64, 3, 1) >= 3 * 8 * 64 * 64 * 3

    def sm(idepth=p, image=p, shape=(1, 13, 17, 3), ws=p, out=p):
        return L.lib.sn_depth_smoothness(idepth, image, *shape, p, p, ws, out, None)

    assert sm(idepth=None) == BADARG and sm(image=None) == BADARG and sm(ws=None) == BADARG and sm(out=None) == BADARG
    for k in range(4):
        shape = [1, 13, 17, 3]
        shape[k] = 0
        assert sm(shape=tuple(shape)) == BADARG
        shape[k] = -1
        assert sm(shape=tuple(shape)) == BADARG
    assert sm(shape=(1, 1, 17, 3)) == BADSHAPE and sm(shape=(1, 13, 1, 3)) == BADSHAPE
    assert L.lib.sn_depth_smoothness_workspace_bytes() > 0


def _central_differences(fn, inputs, k, h=1e-6):
    x = inputs[k]
    g = torch.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        keep = flat[i].item()
        flat[i] = keep + h
        up = fn(*inputs).item()
        flat[i] = keep - h
        dn = fn(*inputs).item()
        flat[i] = keep
        gf[i] = (up - dn) / (2 * h)
    return g


def test_the_oracles_ssim_gradient_against_central_differences():
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(1, 1, 6, 6, generator=g, dtype=torch.float64), torch.rand(1, 1, 6, 6, generator=g, dtype=torch.float64)
    fn = lambda a, b: PO.ssim_loss(a, b, 11)
    val, (ga,) = PO.evaluate(fn, [a, b], [0], torch.float64)
    assert 0.0 < val.item() < 1.0
    assert PO.rel(_central_differences(fn, [a.clone(), b], 0), ga) < 1e-7
    # hand-checked corners of the definition: identical patches give ssim 1 up to the eps = 1e-12 in the denominator, which leaves
    # eps / (2 D) with D ~ mean^2 * variance ~ 1e-2 here; the window is normalised and symmetric
    assert 0 <= PO.ssim_loss(a, a, 11).item() < 1e-9
    w = PO.gaussian(11, torch.float64, "cpu")
    assert abs(w.sum().item() - 1) < 1e-15 and torch.equal(w, w.flip(0)) and w.argmax().item() == 5
    # reflect padding does not repeat the edge pixel: filtering a ramp 0..5 with window 3 at column 0 reads (1, 0, 1)
    ramp = torch.arange(6, dtype=torch.float64).expand(1, 1, 6, 6).contiguous()
    w3 = PO.gaussian(3, torch.float64, "cpu")
    assert abs(PO.filter2d(ramp, 3)[0, 0, 2, 0].item() - (w3[0] + w3[2]).item()) < 1e-15


def test_the_oracles_smoothness_gradients_against_central_differences():
    g = torch.Generator().manual_seed(1)
    d, im = torch.rand(1, 1, 3, 4, generator=g, dtype=torch.float64), torch.rand(1, 3, 3, 4, generator=g, dtype=torch.float64)
    fn = PO.inverse_depth_smoothness_loss
    val, (gd, gi) = PO.evaluate(fn, [d, im], [0, 1], torch.float64)
    assert val.item() > 0
    assert PO.rel(_central_differences(fn, [d.clone(), im], 0), gd) < 1e-7
    assert PO.rel(_central_differences(fn, [d, im.clone()], 1), gi) < 1e-7
    # a constant depth is perfectly smooth; sign(0) = 0 gives it no gradient either
    val0, (gd0, gi0) = PO.evaluate(fn, [torch.full_like(d, 0.3), im], [0, 1], torch.float64)
    assert val0.item() == 0 and not gd0.any() and not gi0.any()


def test_no_cpu_path_and_no_vgg():
    from sinnerf_amd import losses as SL
    assert set(SL.loss_dict) == {"mse", "l2_ssim"} and SL.loss_dict["mse"] is SL.MSELoss and SL.loss_dict["l2_ssim"] is SL.L2_SSIM_Loss
    with pytest.raises(NotImplementedError, match="VGG"):
        SL.loss_dict["l2_vgg"]
    a, b = torch.rand(1, 3, 13, 17), torch.rand(1, 3, 13, 17)
    with pytest.raises(ValueError):
        SL.ssim_loss(a, b, 11)
    with pytest.raises(ValueError):
        SL.inverse_depth_smoothness_loss(a[:, :1], b)
    with pytest.raises(ValueError):
        SL.L2_SSIM_Loss()({"rgb_coarse": a, "rgb_fine": a}, b)
    with pytest.raises(ValueError):
        SL.MSELoss()({"rgb_coarse": a, "rgb_fine": a}, b)
    with pytest.raises(KeyError, match="rgb_fine"):
        SL.L2_SSIM_Loss()({"rgb_coarse": a}, b)


def test_system_defaults_add_no_term():
    from sinnerf_amd.system import DEFAULT_HPARAMS, SinNeRFSystem
    assert (DEFAULT_HPARAMS["patch_loss"], DEFAULT_HPARAMS["depth_smooth_weight"], DEFAULT_HPARAMS["proj_weight"],
            DEFAULT_HPARAMS["dataset_name"]) == ("mse", 0.0, 1.0, None)
    assert callable(SinNeRFSystem.patch_losses)
