"""CPU: the sampler's oracle (tests/sampler_oracle.py) against one training sample of the UNMODIFIED reference (tests/golden/sampler.npz,
tools/gen_golden_sampler.py), its valid map against a brute-force loop, the law that "the floor(u N)-th valid origin" is the rejection
loop's distribution, and the argument checks of the two new entries (they return before any launch)."""
import ctypes
import os

import numpy as np
import pytest

from tests import sampler_oracle as SO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler.npz")
BADARG, TOOLARGE = -1, -2
NEW_SYMBOLS = ("sn_valid_windows_workspace_bytes", "sn_valid_windows", "sn_gather_windows")
# (H, W, sx, sy, pw, ph): the shapes of tests/test_sampler_gpu.py
SHAPES = [(9, 7, 1, 1, 1, 1), (9, 7, 2, 3, 4, 2), (40, 40, 2, 2, 8, 8), (67, 130, 3, 1, 5, 64)]

_FIX = {}


def fixture():
    if not _FIX:
        with np.load(GOLDEN) as z:
            _FIX.update({k: z[k] for k in z.files})
    return _FIX


def fixture_window(f):
    """(sx, sy, pw, ph) = (sH, sW, ps, ps)"""
    ps = int(f["patch_size"])
    return int(f["sH"]), int(f["sW"]), ps, ps


def oracle_sample(f):
    tables = dict(all_rays=f["all_rays"], rgb=f["rgb"], depth=f["depth"])
    full = dict(out=f["warp_out"], depth=f["warp_depth"], rays=f["side_rays"])
    draws = dict(origin_real=(int(f["real_up"]), int(f["real_ll"])), origin_side=(int(f["side_up"]), int(f["side_ll"])),
                 ray_idx=f["ray_idx"], ray_idx2=f["ray_idx2"])
    return SO.sample(tables, full, draws, *fixture_window(f))


def masks_for(shape, rng):
    H, W = shape[:2]
    corners = np.zeros((H, W), np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = (1, 255, 2, 128)                       # any non-zero byte is "set"
    return {"zero": np.zeros((H, W), np.uint8), "corners": corners, "1%": (rng.rand(H, W) < 0.01).astype(np.uint8)}


def counts_for(shape):
    """the full candidate count and the reference's (one fewer per axis; skipped where that leaves none)"""
    H, W, sx, sy, pw, ph = shape
    full = (W - (pw - 1) * sx, H - (ph - 1) * sy)
    return [c for c in (full, (full[0] - 1, full[1] - 1)) if min(c) > 0]


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_describes():
    f = fixture()
    H, W, ps = int(f["H"]), int(f["W"]), int(f["patch_size"])
    assert (H, W, ps, int(f["sW"]), int(f["sH"])) == (40, 40, 8, 2, 2)
    assert f["rgb"].shape == (H, W, 3) and f["depth"].shape == (H, W) and f["all_rays"].shape == (H * W, 8)
    assert f["warp_out"].shape == (H, W, 3) and f["warp_depth"].shape == (H, W) and f["side_rays"].shape == (H * W, 8)
    white = f["rgb"].sum(-1) == 3
    assert 0 < white.sum() < H * W and not f["depth"][white].any() and (f["depth"][~white] > 0).all()
    nx, ny = SO.reference_counts(H, W, *fixture_window(f))
    for ll, up in ((f["real_ll"], f["real_up"]), (f["side_ll"], f["side_up"])):          # np.random.randint(0, 25)
        assert 0 <= int(ll) < ny and 0 <= int(up) < nx
    num = 4096
    assert f["ray_idx"].shape == (num // 10,) and f["ray_idx2"].shape == (num - num // 10,) and f["angles"].shape == (3,)
    assert f["ray_idx"].max() < H * W and f["ray_idx2"].max() < (~white).sum()
    assert (f["warp_depth"] >= 0).all()                                                 # what makes "sum != 0" and "any != 0" agree


@pytest.mark.parametrize("key", ["real_patch", "depth_gt", "depth_ray_rgb", "warp_patch", "warp_patch_depth", "side_coord", "depth_ray",
                                 "rays_full", "rays", "rgbs", "depth"])
def test_oracle_reproduces_the_reference_sample(key):
    f = fixture()
    got, want = oracle_sample(f)[key], f["sample_" + key]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    assert got.dtype.kind == want.dtype.kind


def test_ray_rows_are_the_nonwhite_pixels_first_then_all_pixels():
    f = fixture()
    s = oracle_sample(f)
    num, n_all = 4096, 4096 // 10
    nonwhite = np.flatnonzero(f["rgb"].reshape(-1, 3).sum(-1) != 3)
    assert np.array_equal(s["pick"][:num - n_all], nonwhite[f["ray_idx2"]]) and np.array_equal(s["pick"][num - n_all:], f["ray_idx"])
    assert (f["sample_rgbs"][:num - n_all].sum(-1) != 3).all()
    assert np.array_equal(f["sample_rays"], f["all_rays"][s["pick"]])
    # both loops accepted a window with content (rot3d:459, :493)
    assert f["sample_real_patch"].max() != 0 and f["sample_warp_patch_depth"].sum() != 0


def test_the_accepted_origins_are_valid_origins():
    f = fixture()
    H, W = int(f["H"]), int(f["W"])
    win = fixture_window(f)
    nx, ny = SO.reference_counts(H, W, *win)
    valid_side = SO.valid_windows(f["warp_depth"] != 0, *win, nx, ny)
    valid_real = SO.valid_windows((f["rgb"] != 0).any(-1), *win, nx, ny)
    assert valid_side[int(f["side_ll"]), int(f["side_up"])] == 1 and valid_real[int(f["real_ll"]), int(f["real_up"])] == 1
    assert valid_real.all() and 0 < valid_side.sum()                                    # a white background: every real window has content


def test_mirroring_the_quirk_matters_in_the_fixture():
    """depth_gt / depth_ray / depth_ray_rgb are sliced at the UNSEEN view's origin (rot3d:523-528 after :487-490)"""
    f = fixture()
    tables = dict(all_rays=f["all_rays"], rgb=f["rgb"], depth=f["depth"])
    full = dict(out=f["warp_out"], depth=f["warp_depth"], rays=f["side_rays"])
    draws = dict(origin_real=(int(f["real_up"]), int(f["real_ll"])), origin_side=(int(f["side_up"]), int(f["side_ll"])),
                 ray_idx=f["ray_idx"], ray_idx2=f["ray_idx2"])
    other = SO.sample(tables, full, draws, *fixture_window(f), mirror_quirk=False)
    assert not np.array_equal(other["depth_ray"], f["sample_depth_ray"])
    assert np.array_equal(other["real_patch"], f["sample_real_patch"])


# ---- the valid map ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_valid_map_equals_the_triple_loop(shape):
    H, W, sx, sy, pw, ph = shape
    rng = np.random.RandomState(11)
    for name, mask in masks_for(shape, rng).items():
        for nx, ny in counts_for(shape):
            got = SO.valid_windows(mask, sx, sy, pw, ph, nx, ny)
            assert got.dtype == np.uint8 and got.shape == (ny, nx)
            assert np.array_equal(got, SO.valid_windows_brute(mask, sx, sy, pw, ph, nx, ny)), (shape, name, nx, ny)
            if name == "zero":
                assert not got.any()


def test_exactly_one_x_origin_fits():
    assert counts_for(SHAPES[1]) == [(1, 6)]                                            # W - (pw - 1) sx = 7 - 6


# ---- the law ---------------------------------------------------------------------------------------------------------------------------
def test_kth_valid_is_the_rejection_loops_distribution():
    """u_j = (j + 1/2) / N, j < N, returns every valid origin exactly once and no other: uniform u gives a uniform valid origin, which is
    what a loop that redraws a uniform origin until it is valid returns.  A seeded loop over the same map stays inside the set."""
    f = fixture()
    H, W = int(f["H"]), int(f["W"])
    win = fixture_window(f)
    nx, ny = SO.reference_counts(H, W, *win)
    rng = np.random.RandomState(5)
    sparse = np.zeros((H, W), np.uint8)
    sparse[rng.randint(0, H, 6), rng.randint(0, W, 6)] = 1
    small = (f["warp_depth"] != 0) & (np.add.outer(np.arange(H), np.arange(W)) % 7 == 0) & (np.arange(W) > 22)[None, :]
    for name, mask in (("warped depth", f["warp_depth"] != 0), ("part of it", small), ("six pixels", sparse)):
        valid = SO.valid_windows(mask, *win, nx, ny)
        N = int(valid.sum())
        assert 0 < N <= nx * ny and (N < nx * ny or name == "warped depth")              # the fixture's own map has no invalid origin
        want = {(x0, y0) for y0, x0 in zip(*np.nonzero(valid))}
        got = [SO.kth_valid(valid, (j + 0.5) / N) for j in range(N)]
        assert all(n == N for _, n in got)
        assert len({o for o, _ in got}) == N and {o for o, _ in got} == want
        seen = set()
        for _ in range(300):                                                            # rot3d:486-499 with the window test of :493
            while True:
                ll, up = rng.randint(0, ny), rng.randint(0, nx)
                if SO.window(np.asarray(mask, np.float32), up, ll, *win).sum() != 0:
                    break
            seen.add((up, ll))
        assert seen <= want and len(seen) > 1
    assert SO.kth_valid(np.zeros((ny, nx), np.uint8), 0.5) == ((0, 0), 0)               # nothing valid: the fallback origin


# ---- the entries' argument checks ------------------------------------------------------------------------------------------------------
def lib():
    from sinnerf_amd import _lib as L
    return L


def test_new_symbols_are_exported_and_mirrored():
    L = lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in L.SIGNATURES
    assert L.lib.sn_abi_version() == 5


def valid_call(L, H=9, W=7, sx=2, sy=3, pw=4, ph=2, nx=1, ny=6, mask=1, valid=1, n_valid=1, ws=1):
    p = lambda v: ctypes.c_void_p(0x1000) if v else None                                 # never dereferenced: every case returns first
    return L.lib.sn_valid_windows(p(mask), H, W, sx, sy, pw, ph, nx, ny, p(valid), p(n_valid), p(ws), None)


def gather_call(L, n=2, channels=(3, 1), planar=0, H=9, W=7, sx=2, sy=3, pw=4, ph=2, origin=1, null_entry=None, arrays=(1, 1, 1)):
    ptrs = [0x1000] * max(n, 1)
    src, dst = (ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.c_void_p * len(ptrs))(*ptrs)
    if null_entry == "src":
        src[0] = None
    if null_entry == "dst":
        dst[len(ptrs) - 1] = None
    ch = (ctypes.c_int * len(ptrs))(*(list(channels) + [1] * len(ptrs))[:len(ptrs)])
    return L.lib.sn_gather_windows(src if arrays[0] else None, dst if arrays[1] else None, ch if arrays[2] else None, n, planar, H, W,
                                   ctypes.c_void_p(0x1000) if origin else None, sx, sy, pw, ph, None)


def test_bad_arguments_are_refused_before_any_launch():
    L = lib()
    # a candidate window that leaves the frame: nx > W - (pw - 1) sx = 1, ny > H - (ph - 1) sy = 6
    assert valid_call(L, nx=2) == BADARG and valid_call(L, ny=7) == BADARG
    for name in ("mask", "valid", "ws"):
        assert valid_call(L, **{name: 0}) == BADARG
    for name in ("H", "W", "sx", "sy", "pw", "ph", "nx", "ny"):
        assert valid_call(L, **{name: 0}) == BADARG and valid_call(L, **{name: -3}) == BADARG
    assert valid_call(L, H=65536, W=32768) == TOOLARGE
    assert L.lib.sn_valid_windows_workspace_bytes(0, 4) == BADARG and L.lib.sn_valid_windows_workspace_bytes(4, 0) == BADARG
    assert L.lib.sn_valid_windows_workspace_bytes(65536, 32768) == TOOLARGE
    assert L.lib.sn_valid_windows_workspace_bytes(40, 25) >= 40 * 25
    assert gather_call(L, n=0) == BADARG and gather_call(L, n=9) == BADARG and gather_call(L, origin=0) == BADARG
    assert gather_call(L, arrays=(0, 1, 1)) == BADARG and gather_call(L, arrays=(1, 0, 1)) == BADARG and gather_call(L, arrays=(1, 1, 0)) == BADARG
    assert gather_call(L, null_entry="src") == BADARG and gather_call(L, null_entry="dst") == BADARG
    assert gather_call(L, channels=(3, 0)) == BADARG and gather_call(L, planar=4) == BADARG
    for name in ("H", "W", "sx", "sy", "pw", "ph"):
        assert gather_call(L, **{name: 0}) == BADARG
    assert gather_call(L, pw=5) == BADARG and gather_call(L, ph=4) == BADARG             # fits at no origin: (pw - 1) sx = 8 > W - 1
    assert gather_call(L, H=40000, W=40000, channels=(3, 1)) == TOOLARGE
