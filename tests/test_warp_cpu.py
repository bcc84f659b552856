"""CPU: the yardstick of the forward-warp GPU tests (tests/warp_oracle.py, fp64) held to the unmodified reference's outputs
(tests/golden/warp.npz, tools/gen_golden_warp.py) under the tolerance rule that comes from the reference's own fp32 error; the 1 %
condition that rule stands on; and the new entries in the header, the binding and the library, refusing bad arguments on the host.

The rule: tau = max(4 e_xy, 1e-9) px.  A source pixel is fragile if its fp64 xs or ys lies within tau of an integer; in mode 1 a target
is also fragile if its two nearest candidates' fp64 depths differ by less than 4 e_d.  Outside the targets a fragile pixel could reach,
the winner equals the reference's exactly, `new` is the gather bit for bit, new_depth is within max(4 e_d, 1e-6) of the fp64 value."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import warp_oracle as WO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("rot3d", "proj", "llff", "dtu")
NEW_SYMBOLS = ("sn_forward_warp_workspace_bytes", "sn_forward_warp", "sn_select_landed_workspace_bytes", "sn_select_landed")
CTYPE = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const double*": ctypes.c_void_p,
         "unsigned char*": ctypes.c_void_p, "const unsigned char*": ctypes.c_void_p, "int*": ctypes.c_void_p, "int": ctypes.c_int,
         "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
BADARG, TOOLARGE = -1, -2


def load_case(name):
    z = np.load(os.path.join(REPO, "tests", "golden", "warp.npz"))
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}


def case_tolerances(c):
    return max(4 * float(c["e_xy"]), 1e-9), 4 * float(c["e_d"])


def check_against_reference(c, winner, new, new_depth, mask=None, tag=""):
    """the tolerance rule, for any implementation's full-frame outputs (flat over H*W) -> the fragile share of source pixels"""
    H, W, mode = int(c["H"]), int(c["W"]), int(c["mode"])
    tau, gap = case_tolerances(c)
    res = WO.forward_warp(c["data"], c["depth"], c["P_ref"], c["P_src"], float(c["eps"]), mode)
    aside, frag = WO.fragile_targets(res, H, W, tau, mode, gap)
    keep = ~aside
    ref_new = c["new"].reshape(H * W, -1)
    ref_winner = ref_new[:, 3].astype(np.int64) - 1                        # the data's last channel is the source index + 1
    winner = np.asarray(winner).reshape(-1).astype(np.int64)
    print(f"{tag}: tau {tau:.3e}, fragile sources {frag.sum()} of {H * W}, targets set aside {aside.sum()}, winners differing "
          f"from the reference {(winner != ref_winner).sum()} (kept targets: {(winner != ref_winner)[keep].sum()})")
    assert np.array_equal(winner[keep], ref_winner[keep])
    landed = winner >= 0
    gather = np.where(landed[:, None], c["data"].reshape(H * W, -1)[np.maximum(winner, 0)].view(np.uint32), np.uint32(0))
    assert np.array_equal(np.asarray(new).reshape(H * W, -1).view(np.uint32)[keep], gather[keep])
    assert np.array_equal(gather[keep], ref_new.view(np.uint32)[keep])
    want = np.where(landed, res["p2"][np.maximum(winner, 0)], 0.0)
    err = np.abs(np.asarray(new_depth).reshape(-1).astype(np.float64) - want)[keep]
    ref_err = np.abs(c["new_depth"].reshape(-1).astype(np.float64) - want)[keep]
    print(f"{tag}: max |new_depth - fp64| {err.max():.3e} (reference {ref_err.max():.3e}), bound {max(gap, 1e-6):.3e}")
    assert err.max() <= max(gap, 1e-6) and ref_err.max() <= max(gap, 1e-6)
    if mask is not None:
        assert np.array_equal(np.asarray(mask).reshape(-1).astype(bool)[keep], landed[keep])
        if "mask" in c:
            assert np.array_equal(c["mask"].reshape(-1)[keep], landed[keep])
    return frag.mean()


@pytest.mark.parametrize("name", CASES)
def test_oracle_against_the_reference_under_the_tolerance_rule(name):
    c = load_case(name)
    res = WO.forward_warp(c["data"], c["depth"], c["P_ref"], c["P_src"], float(c["eps"]), int(c["mode"]))
    share = check_against_reference(c, res["winner"], res["new"], res["new_depth"], res["mask"], tag=name)
    assert share <= 0.01                                                    # the condition the rule stands on
    assert res["mask"].sum() > 100 and (~res["mask"]).sum() > 100           # the case has both landed pixels and holes
    if "K" in c:                                                            # the projection matrices are what K and E imply
        assert np.array_equal(WO.proj_matrix(c["K"], c["E_ref"]), c["P_ref"])
        assert np.array_equal(WO.proj_matrix(c["K"], c["E_src"]), c["P_src"])


def test_oracle_collision_rules_and_selection_by_hand():
    # 7 x 5 all-zero depth: every pixel projects to one point
    H, W = 7, 5
    P = np.eye(4)
    P_src = np.eye(4)
    P_src[:3, 3] = (2.6, 3.2, 1.0)                                          # p = (2.6, 3.2, 1) for d = 0: target (2, 3)
    for mode, want in ((0, H * W - 1), (1, 0)):
        res = WO.forward_warp(None, np.zeros((H, W), np.float32), P, P_src, 0.0, mode)
        assert res["mask"].sum() == 1 and res["winner"][3 * W + 2] == want and res["new_depth"][3 * W + 2] == 1.0
    # NaN depth drops the pixel, +-inf clamps
    d = np.ones((2, 3), np.float32)
    d[0, 1] = np.nan
    res = WO.forward_warp(None, d, P, P, 0.0, 0)
    assert list(res["winner"]) == [0, -1, 2, 3, 4, 5]
    assert list(WO.targets(np.array([-np.inf, np.inf, np.nan, 1.5]), np.array([0.0, np.inf, 0.0, np.nan]), 4, 6)) == [0, 23, -1, -1]
    # the k-th set element
    mask = np.array([0, 1, 1, 0, 0, 1, 0, 1], np.uint8)
    u = np.array([0.0, 0.24, 0.25, 0.5, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    idx, N = WO.select_landed(mask, u)
    assert N == 4 and list(idx) == [1, 1, 2, 5, 7]
    idx, N = WO.select_landed(np.zeros(5, np.uint8), u)
    assert N == 0 and list(idx) == [-1] * 5


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


def test_warp_symbols_exported_with_the_headers_prototypes():
    from sinnerf_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "sinnerf_hip.h")).read()
    assert L.lib.sn_abi_version() == L.ABI_VERSION == 5                                      # additive within ABI 5
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert getattr(L.lib, name) is not None
        assert header_prototype(hdr, name) == (L.SIGNATURES[name][0], list(L.SIGNATURES[name][1])), name
    assert header_prototype(hdr, "sn_ndc_rays") == (L.SIGNATURES["sn_ndc_rays"][0], list(L.SIGNATURES["sn_ndc_rays"][1]))
    for cited in ("rot3d :145", "llff_ray_patch_1image_proj.py:117-166", "dtu_proj.py:236-273", "exactly 0.0", "DROPS"):
        assert cited in hdr, cited


def warp_call(L, **kw):
    p = ctypes.c_void_p(64)
    a = dict(depth=p, data=p, H=13, W=17, C=3, P_ref=p, P_src=p, eps=0.0, mode=0, win=(0, 0, 1, 1, 17, 13), new=p, new_depth=p, mask=p,
             winner=p, ws=p)
    a.update(kw)
    return L.lib.sn_forward_warp(a["depth"], a["data"], a["H"], a["W"], a["C"], a["P_ref"], a["P_src"], a["eps"], a["mode"], *a["win"],
                                 a["new"], a["new_depth"], a["mask"], a["winner"], a["ws"], None)


def test_warp_argument_checks_run_on_the_host():
    """every refusal below returns before a launch: the pointers are never dereferenced"""
    from sinnerf_amd import _lib as L
    for name in ("depth", "P_ref", "P_src", "ws"):
        assert warp_call(L, **{name: None}) == BADARG, name
    for name in ("H", "W"):
        for bad in (0, -3):
            assert warp_call(L, **{name: bad}) == BADARG
    assert warp_call(L, C=0) == BADARG and warp_call(L, C=-1) == BADARG
    assert warp_call(L, mode=2) == BADARG and warp_call(L, mode=-1) == BADARG
    for win in ((0, 0, 0, 1, 17, 13), (0, 0, 1, -1, 17, 13), (0, 0, 1, 1, 0, 13), (0, 0, 1, 1, 17, -2),     # strides, sizes
                (-1, 0, 1, 1, 4, 4), (0, -1, 1, 1, 4, 4), (1, 0, 1, 1, 17, 13), (0, 1, 1, 1, 17, 13),      # outside the frame
                (0, 0, 4, 1, 6, 13), (0, 0, 1, 4, 17, 5), (16, 12, 2 ** 30, 2 ** 30, 2, 2)):
        assert warp_call(L, win=win) == BADARG, win
    assert warp_call(L, H=65536, W=32768, win=(0, 0, 1, 1, 4, 4)) == TOOLARGE
    assert L.lib.sn_forward_warp_workspace_bytes(65536, 32768) == TOOLARGE
    assert L.lib.sn_forward_warp_workspace_bytes(0, 4) == BADARG
    assert L.lib.sn_forward_warp_workspace_bytes(13, 17) >= 8 * 13 * 17 + 12 * 8
    p = ctypes.c_void_p(64)
    sel = lambda mask=p, n=100, u=p, m=7, idx=p, nl=p, ws=p: L.lib.sn_select_landed(mask, n, u, m, idx, nl, ws, None)
    assert sel(mask=None) == BADARG and sel(u=None) == BADARG and sel(idx=None) == BADARG and sel(ws=None) == BADARG
    assert sel(n=0) == BADARG and sel(n=-1) == BADARG and sel(m=-1) == BADARG
    assert sel(n=2 ** 31) == TOOLARGE and sel(m=2 ** 31) == TOOLARGE
    assert L.lib.sn_select_landed_workspace_bytes(0) == BADARG and L.lib.sn_select_landed_workspace_bytes(2 ** 31) == TOOLARGE
    assert L.lib.sn_select_landed_workspace_bytes(160000) > 0


def test_no_cpu_path():
    torch = pytest.importorskip("torch")
    import sinnerf_amd
    from sinnerf_amd import warp
    assert sinnerf_amd.forward_warp is warp.forward_warp and sinnerf_amd.unseen_view_batch is warp.unseen_view_batch
    d, K, E = torch.ones(4, 5), torch.eye(3), torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp.forward_warp(torch.ones(4, 5, 3), d, K, E, K, E)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp.forward_warp_proj(None, d, E, E)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp.select_landed(torch.ones(5, dtype=torch.bool), torch.rand(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp.rotate_3d(E, 1.0, 2.0, 3.0)
    with pytest.raises(ValueError):
        warp.forward_warp(None, d, K, E, K, E, collide="first")
    with pytest.raises(ValueError):
        warp.extrinsics_from_c2w(E, "blender")
