"""GPU: sn_forward_warp and sn_select_landed through the C ABI and through sinnerf_amd.warp -- the four fixture cases of the unmodified
reference under the tolerance rule of tests/test_warp_cpu.py, the same inputs and the degenerate shapes against the fp64 oracle
(tests/warp_oracle.py), windows, workspace independence, determinism, the error codes, and unseen_view_batch into the training step.

Against the oracle both sides are fp64 and differ by roundings of ~1e-13 px (|coordinate| < 1e3, a dozen operations of 2^-53 each, and
the 4x4 inverse): targets within TAU64 = 1e-9 px of an integer coordinate, or whose two nearest depths differ by less than 1e-12, are
set aside; everywhere else winners are equal exactly, `new` is the gather bit for bit, and new_depth -- (float) of an fp64 value that
may differ in its last bits -- is within one fp32 spacing."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import warp_oracle as WO                                      # noqa: E402
from tests.test_warp_cpu import (BADARG, CASES, TOOLARGE, check_against_reference, load_case, warp_call)   # noqa: E402

pytestmark = pytest.mark.gpu
TAU64, GAP64 = 1e-9, 1e-12


def dev():
    return torch.device("cuda:0")


def t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype)


def c_warp(depth, data, P_ref, P_src, eps, mode, window=None, fill=None):
    """sn_forward_warp through ctypes -> dict of numpy arrays (new, new_depth, mask, winner), flat over the window"""
    from sinnerf_amd import _lib as L
    H, W = depth.shape
    win = (0, 0, 1, 1, W, H) if window is None else window
    n = win[4] * win[5]
    C = 0 if data is None else data.shape[-1]
    d_depth, d_data = t(depth, torch.float32), None if data is None else t(data, torch.float32)
    d_pr, d_ps = t(np.asarray(P_ref, np.float64)), t(np.asarray(P_src, np.float64))
    new = torch.full((n, max(C, 1)), 7.0, device=dev())
    new_depth, mask = torch.full((n,), 7.0, device=dev()), torch.full((n,), 7, dtype=torch.uint8, device=dev())
    winner = torch.full((n,), 7, dtype=torch.int32, device=dev())
    nbytes = L.lib.sn_forward_warp_workspace_bytes(H, W)
    assert nbytes >= 8 * H * W
    ws = torch.zeros(nbytes // 4 + 1, dtype=torch.int32, device=dev())
    if fill is not None:
        ws.fill_(fill)
    L.check(L.lib.sn_forward_warp(L.ptr(d_depth), L.ptr(d_data), H, W, C, L.ptr(d_pr), L.ptr(d_ps), eps, mode, *win,
                                  L.ptr(new) if C else None, L.ptr(new_depth), L.ptr(mask), L.ptr(winner), L.ptr(ws), L.stream_ptr()),
            "sn_forward_warp")
    torch.cuda.synchronize()
    return dict(new=new.cpu().numpy() if C else None, new_depth=new_depth.cpu().numpy(), mask=mask.cpu().numpy(),
                winner=winner.cpu().numpy())


def check_against_oracle(got, depth, data, P_ref, P_src, eps, mode, tag, min_keep=0.99):
    H, W = depth.shape
    res = WO.forward_warp(data, depth, P_ref, P_src, eps, mode)
    aside, frag = WO.fragile_targets(res, H, W, TAU64, mode, GAP64)
    keep = ~aside
    print(f"{tag}: {H}x{W} mode {mode}: landed {res['mask'].sum()}, set aside {aside.sum()}, winners differing "
          f"{(got['winner'] != res['winner']).sum()}")
    assert keep.mean() >= min_keep                # exact integer coordinates (an identity warp) are all set aside: min_keep=0
    assert np.array_equal(got["winner"][keep], res["winner"][keep])
    assert np.array_equal(got["mask"][keep].astype(bool), res["mask"][keep])
    assert set(np.unique(got["mask"])) <= {0, 1}
    if data is not None:
        assert np.array_equal(got["new"].view(np.uint32)[keep], res["new"].view(np.uint32)[keep])
    a, b = got["new_depth"][keep], res["new_depth"][keep]
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    assert np.all(same | (np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(b)))), np.abs(a - b)[~same].max()
    return res


# ---- the reference's four variants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_through_the_c_abi(name):
    c = load_case(name)
    got = c_warp(c["depth"], c["data"], c["P_ref"], c["P_src"], float(c["eps"]), int(c["mode"]))
    check_against_reference(c, got["winner"], got["new"], got["new_depth"], got["mask"], tag=name + " (C ABI)")
    check_against_oracle(got, c["depth"], c["data"], c["P_ref"], c["P_src"], float(c["eps"]), int(c["mode"]), name)


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_through_warp_py(name):
    from sinnerf_amd import warp
    c = load_case(name)
    collide = ("last", "nearest")[int(c["mode"])]
    data_nchw = t(c["data"]).permute(2, 0, 1).unsqueeze(0)               # as the reference passes it
    if "K" in c:
        K, E_ref, E_src = t(c["K"]), t(c["E_ref"]), t(c["E_src"])
        out = warp.forward_warp(data_nchw, t(c["depth"]).unsqueeze(0), K, E_ref, K, E_src, collide=collide, eps=float(c["eps"]),
                                return_winner=True)
    else:
        out = warp.forward_warp_proj(t(c["data"]), t(c["depth"]), t(c["P_ref"]), t(c["P_src"]), collide=collide, eps=float(c["eps"]),
                                     return_winner=True)
    new, new_depth, mask, winner = out
    H, W = int(c["H"]), int(c["W"])
    assert new.shape == (H, W, 4) and new_depth.shape == (H, W) and mask.shape == (H, W) and mask.dtype == torch.bool
    assert winner.dtype == torch.int32 and not new.requires_grad and not new_depth.requires_grad
    check_against_reference(c, winner.cpu().numpy(), new.cpu().numpy(), new_depth.cpu().numpy(), mask.cpu().numpy(), tag=name + " (warp.py)")


def test_poses_on_the_device_match_the_reference():
    """extrinsics_from_c2w and rotate_3d against the reference's convert / rotate_3d outputs in the fixture (fp32: 1e-6 of entries <= 4)"""
    from sinnerf_amd import warp
    c = load_case("rot3d")
    c2w = torch.eye(4, device=dev())
    c2w[2, 3] = 4.0
    E_ref = warp.extrinsics_from_c2w(c2w)
    assert E_ref.dtype == torch.float64 and E_ref.is_cuda
    assert np.abs(E_ref.cpu().numpy() - c["E_ref"]).max() < 1e-6
    side = warp.rotate_3d(c2w, 9.0, -14.0, 5.0)
    assert side.shape == (4, 4) and side.dtype == c2w.dtype
    assert np.abs(warp.extrinsics_from_c2w(side[:3]).cpu().numpy() - c["E_src"]).max() < 2e-6
    assert torch.equal(warp.rotate_3d(c2w[:3], torch.tensor(9.0, device=dev()), -14.0, 5.0), side[:3])
    # 'opencv' is the plain inverse, of a general affine pose too
    pose = np.array([[0.9, 0.1, -0.3, 1.0], [0.2, 1.1, 0.05, -2.0], [0.3, -0.2, 0.8, 0.5], [0, 0, 0, 1.0]])
    inv = warp.extrinsics_from_c2w(t(pose), "opencv").cpu().numpy()
    assert np.abs(inv - np.linalg.inv(pose)).max() < 1e-13


# ---- degenerate shapes ---------------------------------------------------------------------------------------------------------------
def shift(dx, dy):
    P = np.eye(4)
    P[:3, 3] = (dx, dy, 0.0)                                             # p = (x d + dx, y d + dy, d): xs = x + dx / d
    return P


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)])
@pytest.mark.parametrize("mode", [0, 1])
def test_one_pixel_rows_and_columns(shape, mode):
    rng = np.random.RandomState(3)
    depth = (1.0 + rng.rand(*shape)).astype(np.float32)
    data = rng.rand(*shape, 2).astype(np.float32)
    for P_src in (np.eye(4), shift(1.3, 1.7), shift(-2.4, 0.3)):
        got = c_warp(depth, data, np.eye(4), P_src, 0.0, mode)
        identity = P_src[0, 3] == 0
        res = check_against_oracle(got, depth, data, np.eye(4), P_src, 0.0, mode, f"{shape}", min_keep=0.0 if identity else 0.99)
        assert res["mask"].any()
        if identity:                                                     # x d / d = x exactly: every pixel lands on itself
            assert np.array_equal(got["winner"], np.arange(depth.size)) and np.array_equal(got["new"], data.reshape(-1, 2))


def test_every_pixel_on_one_target():
    H, W = 7, 5
    depth, data = np.zeros((H, W), np.float32), np.arange(H * W * 3, dtype=np.float32).reshape(H, W, 3)
    P_src = np.eye(4)
    P_src[:3, 3] = (2.6, 3.2, 1.0)
    for mode, want in ((0, H * W - 1), (1, 0)):                          # the last index / the tie rule
        got = c_warp(depth, data, np.eye(4), P_src, 0.0, mode)
        # in mode 1 the one target is set aside (equal depths); every depth_src is exactly 1.0, so the tie rule is asserted directly
        check_against_oracle(got, depth, data, np.eye(4), P_src, 0.0, mode, "one target", min_keep=0.9)
        assert got["mask"].sum() == 1 and got["winner"][3 * W + 2] == want and got["new_depth"][3 * W + 2] == 1.0
        assert np.array_equal(got["new"][3 * W + 2], data.reshape(-1, 3)[want]) and (got["winner"] >= 0).sum() == 1


@pytest.mark.parametrize("mode", [0, 1])
def test_a_pose_that_throws_every_pixel_out_of_frame(mode):
    rng = np.random.RandomState(4)
    H, W = 11, 6
    depth, data = (1.0 + rng.rand(H, W)).astype(np.float32), rng.rand(H, W, 1).astype(np.float32)
    for P_src, borders in ((shift(1e7, 2.0), lambda w: w % W == W - 1), (shift(-1e7, -1e7), lambda w: w == 0),
                           (shift(3.0, 1e300), lambda w: w // W == H - 1)):
        got = c_warp(depth, data, np.eye(4), P_src, 0.0, mode)
        check_against_oracle(got, depth, data, np.eye(4), P_src, 0.0, mode, "out of frame")
        landed = np.flatnonzero(got["mask"])
        assert len(landed) > 0 and all(borders(w) for w in landed)
    # +-inf coordinates clamp too: a zero-depth pixel divides by 0
    depth[2, 3] = 0.0
    got = c_warp(depth, data, np.eye(4), shift(1.0, -1.0), 0.0, mode)
    res = check_against_oracle(got, depth, data, np.eye(4), shift(1.0, -1.0), 0.0, mode, "inf")
    assert np.isinf(res["xs"][2 * W + 3]) and got["winner"][W - 1] == 2 * W + 3        # (+inf, -inf) -> the top right corner


@pytest.mark.parametrize("mode", [0, 1])
def test_nan_depths_are_dropped(mode):
    rng = np.random.RandomState(5)
    H, W = 9, 13
    depth, data = (1.0 + rng.rand(H, W)).astype(np.float32), rng.rand(H, W, 3).astype(np.float32)
    holes = [(0, 0), (4, 6), (4, 7), (8, 12)]
    for y, x in holes:
        depth[y, x] = np.nan
    got = c_warp(depth, data, np.eye(4), np.eye(4), 0.0, mode)           # the identity: every other pixel lands on itself
    check_against_oracle(got, depth, data, np.eye(4), np.eye(4), 0.0, mode, "nan", min_keep=0.0)
    want = np.arange(H * W)
    for y, x in holes:
        want[y * W + x] = -1
    assert np.array_equal(got["winner"], want)
    assert np.array_equal(got["new"][want >= 0], data.reshape(-1, 3)[want >= 0]) and not got["new"][want < 0].any()
    all_nan = c_warp(np.full((H, W), np.nan, np.float32), data, np.eye(4), np.eye(4), 0.0, mode)
    assert not all_nan["mask"].any() and (all_nan["winner"] == -1).all() and not all_nan["new_depth"].any()


def big_case():
    """400 x 400 for multi-block coverage: the rot3d pose at the reference's image size, a sphere over a zero-depth background"""
    c = load_case("rot3d")
    H = W = 400
    K = np.array([[555.5, 0, 199.5], [0, 555.5, 199.5], [0, 0, 1]])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = ((x - 199.5) ** 2 + (y - 199.5) ** 2) / 555.5 ** 2
    depth = np.where(r2 < 0.06, 4.0 - np.sqrt(np.maximum(0.0, 1.0 - 15.0 * r2)), 0.0).astype(np.float32)
    data = np.random.RandomState(6).rand(H, W, 3).astype(np.float32)
    return depth, data, WO.proj_matrix(K, c["E_ref"]), WO.proj_matrix(K, c["E_src"])


_BIG = {}


def big_result():
    if not _BIG:
        depth, data, P_ref, P_src = big_case()
        _BIG.update(depth=depth, data=data, P_ref=P_ref, P_src=P_src, got=c_warp(depth, data, P_ref, P_src, 0.0, 0))
    return _BIG


def test_400x400_last_wins():
    b = big_result()
    res = check_against_oracle(b["got"], b["depth"], b["data"], b["P_ref"], b["P_src"], 0.0, 0, "400x400")
    assert res["mask"].sum() > 10000


# ---- windows, workspace, determinism, errors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rot3d", "llff"])
def test_windows_are_slices_of_the_full_frame(name):
    c = load_case(name)
    H, W = int(c["H"]), int(c["W"])
    args = (c["depth"], c["data"], c["P_ref"], c["P_src"], float(c["eps"]), int(c["mode"]))
    full = c_warp(*args)
    for win in ((0, 0, 1, 1, W, H), (3, 5, 1, 1, 8, 8), (W - 1 - 4 * 7, H - 1 - 4 * 7, 4, 4, 8, 8), (W - 8, H - 5, 1, 1, 8, 5),
                (1, 2, 3, 2, 7, 9), (W - 1, H - 1, 1, 1, 1, 1), (2, 0, 5, H - 1, 5, 2)):
        got = c_warp(*args, window=win)
        at = WO.window_index(H, W, win)
        for k in ("new", "new_depth", "mask", "winner"):
            assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                                  full[k][at].view(np.uint32) if full[k].dtype == np.float32 else full[k][at]), (win, k)
    only_depth = c_warp(c["depth"], None, c["P_ref"], c["P_src"], float(c["eps"]), int(c["mode"]))     # data may be NULL
    assert np.array_equal(only_depth["winner"], full["winner"]) and np.array_equal(only_depth["new_depth"], full["new_depth"])


@pytest.mark.parametrize("name", ["proj", "dtu"])
def test_workspace_contents_do_not_matter_and_calls_repeat(name):
    c = load_case(name)
    args = (c["depth"], c["data"], c["P_ref"], c["P_src"], float(c["eps"]), int(c["mode"]))
    runs = [c_warp(*args), c_warp(*args), c_warp(*args, fill=0x7FC00000), c_warp(*args, fill=-1), c_warp(*args, fill=0x7FF80000)]
    for r in runs[1:]:
        for k in ("new", "new_depth", "mask", "winner"):
            assert r[k].tobytes() == runs[0][k].tobytes(), k


def test_error_codes_with_device_pointers():
    from sinnerf_amd import _lib as L
    bufs = {k: torch.zeros(4096, device=dev()) for k in ("depth", "data", "new", "new_depth", "mask", "winner", "ws")}   # no aliasing
    bufs["P_ref"] = bufs["P_src"] = torch.eye(4, dtype=torch.float64, device=dev())
    base = {k: ctypes.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    p = base["depth"]
    assert warp_call(L, **base) == 0                                      # 13 x 17 x 3 fits every buffer
    for name in ("depth", "P_ref", "P_src", "ws"):
        assert warp_call(L, **{**base, name: None}) == BADARG
    assert warp_call(L, **base, H=0) == BADARG and warp_call(L, **base, mode=2) == BADARG and warp_call(L, **base, C=0) == BADARG
    assert warp_call(L, **base, win=(0, 0, 1, 1, 18, 13)) == BADARG and warp_call(L, **base, win=(0, 0, 1, 0, 17, 13)) == BADARG
    assert warp_call(L, **base, H=65536, W=32768, win=(0, 0, 1, 1, 4, 4)) == TOOLARGE
    assert L.lib.sn_select_landed(p, 0, p, 4, p, p, p, None) == BADARG and L.lib.sn_select_landed(p, 2 ** 31, p, 4, p, p, p, None) == TOOLARGE
    torch.cuda.synchronize()
    assert not bufs["mask"].any()                                        # the all-zero depth map at the identity divides 0 by 0: dropped


# ---- sn_select_landed ----------------------------------------------------------------------------------------------------------------
def select(mask, u):
    from sinnerf_amd import warp
    idx, n = warp.select_landed(t(mask), t(np.asarray(u, np.float32)))
    assert idx.dtype == torch.int32 and n.dtype == torch.int32 and n.is_cuda
    return idx.cpu().numpy(), int(n.item())


EDGE_U = [0.0, np.nextafter(np.float32(1), np.float32(0)), 0.5, 0.25, 0.999]


def test_select_landed_against_flatnonzero():
    rng = np.random.RandomState(7)
    big = big_result()["got"]["mask"]                                     # 160 000 elements: 79 scan blocks of 2048
    masks = {"none": np.zeros(5000, np.uint8), "last only": np.r_[np.zeros(4999, np.uint8), np.uint8(1)], "all": np.ones(5000, np.uint8),
             "one element": np.ones(1, np.uint8), "block edge": (np.arange(2 * 2048 + 1) % 2048 == 0).astype(np.uint8),
             "random": (rng.rand(70001) < 0.3).astype(np.uint8) * 255, "400x400": big}
    for name, mask in masks.items():
        for u in (np.array(EDGE_U[:1]), np.array(EDGE_U), np.r_[EDGE_U, rng.rand(4096 - len(EDGE_U))]):     # m = 1, 5, 4096
            want, N = WO.select_landed(mask, u.astype(np.float32))
            got, n = select(mask, u)
            assert n == N == np.count_nonzero(mask), name
            assert np.array_equal(got, want), name
            if N:
                assert np.array_equal(got, np.flatnonzero(mask)[np.minimum(np.floor(u.astype(np.float32).astype(np.float64) * N), N - 1).astype(int)])
    got, n = select(masks["random"], [np.nan, -3.0, 7.0, np.inf])       # outside [0, 1): clamped, no fault
    set_ = np.flatnonzero(masks["random"])
    assert list(got) == [set_[0], set_[0], set_[-1], set_[-1]]
    assert select(big.reshape(400, 400).astype(bool), EDGE_U)[1] == np.count_nonzero(big)      # a bool (H, W) mask is taken as it is


# ---- unseen_view_batch ---------------------------------------------------------------------------------------------------------------
PS, STRIDE = 8, 4
WINDOW = (12, 10, STRIDE, STRIDE, PS, PS)


def unseen_inputs():
    c = load_case("rot3d")
    from sinnerf_amd import warp
    c2w = torch.eye(4, device=dev())
    c2w[2, 3] = 4.0
    side = warp.rotate_3d(c2w, 9.0, -14.0, 5.0)
    u = t(np.r_[EDGE_U, np.random.RandomState(8).rand(27)].astype(np.float32))
    return c, dict(ref_view=t(c["data"][..., :3]), ref_depth=t(c["depth"]), K=t(c["K"]), ref_c2w=c2w, side_c2w=side, near=2.0, far=6.0,
                   window=WINDOW, u_proj=u, focal=float(c["K"][0, 0]))


def test_unseen_view_batch_is_the_composition_of_its_parts():
    from sinnerf_amd import warp
    from sinnerf_amd.ray_utils import get_rays
    c, a = unseen_inputs()
    H, W = int(c["H"]), int(c["W"])
    b = warp.unseen_view_batch(**a)
    E_ref, E_src = warp.extrinsics_from_c2w(a["ref_c2w"]), warp.extrinsics_from_c2w(a["side_c2w"])
    new, new_depth, _ = warp.forward_warp(a["ref_view"], a["ref_depth"], a["K"], E_ref, a["K"], E_src, window=WINDOW)
    assert b["warp_patch"].shape == (3, PS, PS) and torch.equal(b["warp_patch"], new.permute(2, 0, 1))
    assert b["warp_patch_depth"].shape == (PS, PS) and torch.equal(b["warp_patch_depth"], new_depth)
    assert (b["warp_patch_depth"] > 0).any()                                                 # the window has labels
    pose = a["side_c2w"][:3].contiguous()
    assert torch.equal(b["rays_full"], get_rays(H, W, a["focal"], pose, 2.0, 6.0, WINDOW))
    _, depth_full, mask_full = warp.forward_warp(None, a["ref_depth"], a["K"], E_ref, a["K"], E_src)
    idx, n = warp.select_landed(mask_full, a["u_proj"])
    assert int(b["n_landed"].item()) == int(n.item()) == int(mask_full.sum().item()) > 0
    assert torch.equal(b["rays_proj"], get_rays(H, W, a["focal"], pose, 2.0, 6.0)[idx.long()])
    assert torch.equal(b["depth_proj"], depth_full.reshape(-1)[idx.long()]) and bool(mask_full.reshape(-1)[idx.long()].all())
    # the reference's ll indexes rows, up columns: window = (up, ll, sH, sW, ps, ps)
    assert b["side_coord"].tolist() == [[10 + STRIDE * i for i in range(PS)], [12 + STRIDE * i for i in range(PS)]]
    # the device labels against the oracle's: the reference view warped in fp64
    res = WO.forward_warp(c["data"][..., :3], c["depth"], WO.proj_matrix(c["K"], E_ref.cpu().numpy()),
                          WO.proj_matrix(c["K"], E_src.cpu().numpy()), 0.0, 0)
    aside, _ = WO.fragile_targets(res, H, W, TAU64, 0, GAP64)
    at = WO.window_index(H, W, WINDOW)
    assert not aside[at].any()
    assert np.array_equal(b["warp_patch"].permute(1, 2, 0).reshape(-1, 3).cpu().numpy(), res["new"][at])
    # nothing lands: zero rows, and n_landed says so
    a0 = dict(a, ref_depth=torch.full_like(a["ref_depth"], float("nan")))
    b0 = warp.unseen_view_batch(**a0)
    assert int(b0["n_landed"].item()) == 0 and not b0["rays_proj"].any() and not b0["depth_proj"].any()
    assert b0["rays_proj"].shape == b["rays_proj"].shape and not b0["warp_patch_depth"].any()


def test_training_step_takes_the_batch_and_its_side_depth_loss_is_the_oracles():
    """loss_side_depth from the device labels against the same step on the oracle's labels.  The window holds no fragile target (asserted),
    so a label differs from the oracle's by at most one fp32 spacing at depth < 8 (4.8e-7); SmoothL1 is 1-Lipschitz in its target and
    the term is a sum of two means: |difference| <= 2 * 4.8e-7, plus the fp32 rounding of sums of ~64 terms of size < 10 (~1e-6)."""
    from sinnerf_amd import warp
    from sinnerf_amd.ray_utils import get_rays
    from sinnerf_amd.system import SinNeRFSystem
    c, a = unseen_inputs()
    H, W = int(c["H"]), int(c["W"])
    uv = warp.unseen_view_batch(**a)
    g = torch.Generator().manual_seed(9)
    ref_pose = a["ref_c2w"][:3].contiguous()
    n_rand = 64
    pick = torch.randint(0, H * W, (n_rand,), generator=g).to(dev())
    batch = {"rays": get_rays(H, W, a["focal"], ref_pose, 2.0, 6.0)[pick], "rgbs": a["ref_view"].reshape(-1, 3)[pick],
             "depth": a["ref_depth"].reshape(-1)[pick], "rays_full": get_rays(H, W, a["focal"], ref_pose, 2.0, 6.0, WINDOW),
             "rgbs_full": t(c["data"][..., :3].reshape(-1, 3)[WO.window_index(H, W, WINDOW)]),
             "rays_side": uv["rays_full"], "rays_proj": uv["rays_proj"], "depth_proj": uv["depth_proj"],
             "warp_patch": uv["warp_patch"], "warp_patch_depth": uv["warp_patch_depth"], "side_coord": uv["side_coord"],
             "real_patch": torch.rand(1, 3, PS, PS, generator=g).to(dev())}
    torch.manual_seed(0)
    sysm = SinNeRFSystem(N_samples=8, N_importance=8, perturb=0.0, noise_std=0.0, depth_weight=0.5, proj_weight=0.6).to(dev())
    out = sysm.training_step(batch)
    assert torch.isfinite(out["loss"])
    out["loss"].backward()
    grads = [p.grad for p in sysm.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads) and any(gr.abs().max() > 0 for gr in grads)
    side = out["log"]["train/loss_side_depth"].item()
    assert side > 0
    E_ref, E_src = warp.extrinsics_from_c2w(a["ref_c2w"]), warp.extrinsics_from_c2w(a["side_c2w"])
    res = WO.forward_warp(None, c["depth"], WO.proj_matrix(c["K"], E_ref.cpu().numpy()), WO.proj_matrix(c["K"], E_src.cpu().numpy()), 0.0, 0)
    at = WO.window_index(H, W, WINDOW)
    assert not WO.fragile_targets(res, H, W, TAU64, 0, GAP64)[0][at].any()
    oracle_batch = dict(batch, warp_patch_depth=t(res["new_depth"][at].reshape(PS, PS)))
    side_oracle = sysm.training_step(oracle_batch)["log"]["train/loss_side_depth"].item()     # the same kernels: under grad mode too
    print(f"loss_side_depth {side:.9g} (device labels) / {side_oracle:.9g} (oracle labels)")
    assert abs(side - side_oracle) <= 2 * 4.8e-7 + 1e-6
