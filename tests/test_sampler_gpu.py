"""GPU: sn_valid_windows and sn_gather_windows against tests/sampler_oracle.py bit for bit, OneImageSampler.draw against the oracle applied to
the sampler's own tables and full-frame warp, the draws' invariants, and SinNeRFSystem.train_step_sampled eager and captured.

No tolerance appears: the two kernels copy or OR integers, and draw() is compared with the oracle's slicing of the very tensors the sampler
sliced (the warp and get_rays are pinned to the reference by tests/test_warp_*.py and tests/test_cameras_*.py)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import sampler_oracle as SO                                   # noqa: E402
from tests.test_sampler_cpu import BADARG, SHAPES, counts_for, fixture, fixture_window, masks_for   # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- sn_valid_windows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_valid_windows_against_the_oracle(shape):
    from sinnerf_amd import sampler as S
    H, W, sx, sy, pw, ph = shape
    rng = np.random.RandomState(11)
    for name, mask in masks_for(shape, rng).items():
        for nx, ny in counts_for(shape):
            valid, n_valid = S.valid_windows(t(mask), sx, sy, pw, ph, nx, ny)
            assert valid.dtype == torch.uint8 and tuple(valid.shape) == (ny, nx) and n_valid.dtype == torch.int32 and n_valid.is_cuda
            want = SO.valid_windows(mask, sx, sy, pw, ph, nx, ny)
            got = valid.cpu().numpy()
            assert np.array_equal(got, want), (shape, name, nx, ny)
            assert int(n_valid.item()) == int(want.sum()) == int(got.sum())
            again, n_again = S.valid_windows(t(mask).bool(), sx, sy, pw, ph, nx, ny)            # a bool mask is taken as it is; calls repeat
            assert torch.equal(again, valid) and torch.equal(n_again, n_valid)
    if shape == SHAPES[2]:                                                                     # the default counts are the reference's
        valid, _ = S.valid_windows(t(mask), sx, sy, pw, ph)
        assert tuple(valid.shape) == (25, 25) and S.reference_counts(H, W, sx, sy, pw, ph) == (25, 25)


def test_valid_windows_without_the_count_and_its_error_codes():
    from sinnerf_amd import _lib as L
    H, W, sx, sy, pw, ph = SHAPES[1]
    mask = t(np.ones((H, W), np.uint8))
    valid = torch.full((6, 1), 7, dtype=torch.uint8, device=dev())
    n_valid = torch.full((), 7, dtype=torch.int32, device=dev())
    ws = torch.empty(L.lib.sn_valid_windows_workspace_bytes(H, 1), dtype=torch.uint8, device=dev())
    call = lambda nx=1, ny=6, m=mask, v=valid, n=n_valid, w=ws, **kw: L.lib.sn_valid_windows(
        L.ptr(m), kw.get("H", H), kw.get("W", W), kw.get("sx", sx), kw.get("sy", sy), kw.get("pw", pw), kw.get("ph", ph), nx, ny,
        L.ptr(v), L.ptr(n), L.ptr(w), L.stream_ptr())
    # a candidate window that would leave the frame, a null required pointer, a non-positive size: refused, nothing written
    assert call(nx=2) == BADARG and call(ny=7) == BADARG
    assert call(m=None) == BADARG and call(v=None) == BADARG and call(w=None) == BADARG
    for name in ("H", "W", "sx", "sy", "pw", "ph"):
        assert call(**{name: 0}) == BADARG
    assert call(nx=0) == BADARG and call(ny=-1) == BADARG
    torch.cuda.synchronize()
    assert (valid == 7).all() and int(n_valid.item()) == 7
    assert call(n=None) == 0                                                                   # n_valid is optional
    torch.cuda.synchronize()
    assert (valid == 1).all() and int(n_valid.item()) == 7
    assert call() == 0
    torch.cuda.synchronize()
    assert int(n_valid.item()) == 6


# ---- sn_gather_windows -----------------------------------------------------------------------------------------------------------------
GH, GW, GSX, GSY, GPW, GPH = 23, 37, 3, 2, 5, 7                          # 35 pixels: with C = 8 the window spans two blocks of 256 words
LARGEST = (GW - 1 - (GPW - 1) * GSX, GH - 1 - (GPH - 1) * GSY)


def frame(rng, C, dtype=np.float32):
    """any bit pattern: NaNs, infinities and denormals among them"""
    return rng.randint(0, 2 ** 32, (GH, GW, C), dtype=np.uint64).astype(np.uint32).view(dtype)


@pytest.mark.parametrize("origin", [(0, 0), LARGEST, (-1, -1), (2 ** 30, -2 ** 31), (-5, 2 ** 31 - 1)])
def test_gather_windows_against_numpy_slicing(origin):
    from sinnerf_amd import sampler as S
    rng = np.random.RandomState(12)
    o = t(np.array(origin, np.int32))
    win = (GSX, GSY, GPW, GPH)
    for C in (1, 3, 8):
        src = frame(rng, C)
        for planar in (False, True):                                                           # one source
            got, = S.gather_windows([t(src)], o, *win, planar=[planar])
            want = SO.gather(src, *origin, *win, planar=planar)
            assert same_bits(got.cpu().numpy(), want), (C, planar, origin)
    chans = [1, 3, 8, 8, 3, 1, 2, 5]                                                           # eight sources, layouts mixed
    planar = [False, True, False, True, True, False, True, False]
    srcs = [frame(rng, C, np.int32 if k == 5 else np.float32) for k, C in enumerate(chans)]
    srcs[0] = srcs[0][..., 0]                                                                  # an (H, W) source counts as one channel
    got = S.gather_windows([t(s) for s in srcs], o, *win, planar=planar)
    for k, (s, p) in enumerate(zip(srcs, planar)):
        assert same_bits(got[k].cpu().numpy(), SO.gather(s, *origin, *win, planar=p)), (k, origin)
    x0, y0 = SO.clamp_origin(*origin, GH, GW, *win)
    assert (0 <= x0 <= LARGEST[0]) and (0 <= y0 <= LARGEST[1])
    if origin == (-1, -1):
        assert (x0, y0) == (0, 0)


def test_gather_windows_error_codes_and_python_checks():
    from sinnerf_amd import _lib as L
    from sinnerf_amd import sampler as S
    src = torch.zeros((GH, GW, 3), device=dev())
    dst = torch.full((GPH, GPW, 3), 7.0, device=dev())
    o = torch.zeros(2, dtype=torch.int32, device=dev())
    one = lambda v: (ctypes.c_void_p * 1)(v.data_ptr() if v is not None else None)
    call = lambda s=src, d=dst, C=3, n=1, planar=0, org=o, **kw: L.lib.sn_gather_windows(
        one(s), one(d), (ctypes.c_int * 1)(C), n, planar, kw.get("H", GH), kw.get("W", GW), L.ptr(org), kw.get("sx", GSX), kw.get("sy", GSY),
        kw.get("pw", GPW), kw.get("ph", GPH), L.stream_ptr())
    assert call(s=None) == BADARG and call(d=None) == BADARG and call(org=None) == BADARG
    assert call(C=0) == BADARG and call(n=0) == BADARG and call(n=9) == BADARG and call(planar=2) == BADARG
    for name in ("H", "W", "sx", "sy", "pw", "ph"):
        assert call(**{name: 0}) == BADARG
    assert call(pw=14) == BADARG and call(ph=13) == BADARG                                     # fits at no origin
    torch.cuda.synchronize()
    assert (dst == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not dst.any()
    with pytest.raises(RuntimeError):
        S.gather_windows([src.cpu()], o, GSX, GSY, GPW, GPH)                                   # no CPU fallback
    with pytest.raises(RuntimeError):
        S.gather_windows([src], o.long(), GSX, GSY, GPW, GPH)
    with pytest.raises(RuntimeError):
        S.gather_windows([src.half()], o, GSX, GSY, GPW, GPH)
    with pytest.raises(RuntimeError):
        S.valid_windows(torch.zeros(4, 4, dtype=torch.uint8), 1, 1, 2, 2)


# ---- OneImageSampler -------------------------------------------------------------------------------------------------------------------
def make_sampler(num=4096, depth=None, **kw):
    from sinnerf_amd.sampler import OneImageSampler
    f = fixture()
    ps = int(f["patch_size"])
    depth = f["depth"] if depth is None else depth
    return OneImageSampler(t(f["rgb"]), t(depth), t(f["c2w"]), t(f["K"]), focal=float(f["focal"]), near=float(f["near"]), far=float(f["far"]),
                           patch_size=ps, sW=int(f["sW"]), sH=int(f["sH"]), angle=int(f["angle"]), num=num, collide="last", eps=1e-9, **kw)


def numpy_batch(b):
    return {k: (tuple(x.cpu().numpy() for x in v) if isinstance(v, tuple) else v.cpu().numpy()) for k, v in b.items()}


def numpy_view(s, angles):
    """the sampler's own tables and the full frame of the pose drawn with `angles`, as the oracle takes them"""
    full = {k: v.cpu().numpy() for k, v in s.unseen_view(angles).items()}
    tables = dict(all_rays=s.all_rays.cpu().numpy(), rgb=s.ref_view.cpu().numpy(), depth=s.ref_depth.cpu().numpy())
    return tables, full


def oracle_counts(s, tables, full):
    nx, ny = s.nx, s.ny
    valid_real = SO.valid_windows((tables["rgb"] != 0).any(-1), *s.window, nx, ny)
    valid_side = SO.valid_windows(full["depth"] != 0, *s.window, nx, ny)
    return valid_real, valid_side


def test_draw_with_recorded_choices_is_the_oracle_on_the_samplers_own_tables():
    f = fixture()
    s = make_sampler()
    rng = np.random.RandomState(13)
    u_proj = np.r_[0.0, np.nextafter(np.float32(1), np.float32(0)), rng.rand(4094)].astype(np.float32)
    draws = dict(origin_real=(int(f["real_up"]), int(f["real_ll"])), origin_side=(int(f["side_up"]), int(f["side_ll"])),
                 ray_idx=f["ray_idx"], ray_idx2=f["ray_idx2"])
    choices = dict(origin_real=t(np.array(draws["origin_real"], np.int32)), origin_side=t(np.array(draws["origin_side"], np.int32)),
                   ray_idx=t(f["ray_idx"]), ray_idx2=t(f["ray_idx2"]), angles=t(f["angles"]), u_proj=t(u_proj))
    b = s.draw(choices)
    assert all(not v.requires_grad for v in b.values() if torch.is_tensor(v))
    got = numpy_batch(b)
    tables, full = numpy_view(s, choices["angles"])
    want = SO.to_system(SO.sample(tables, full, draws, *s.window), full, u_proj)
    for k, w in want.items():
        if k == "n_landed":
            assert int(got[k]) == w == int(full["mask"].sum()) > 0
        else:
            assert same_bits(got[k], np.ascontiguousarray(w)), k
    assert set(want) | {"n_valid_real", "n_valid_side", "origin_real", "origin_side", "angles", "c2w_side"} == set(got)
    valid_real, valid_side = oracle_counts(s, tables, full)
    assert int(got["n_valid_real"]) == valid_real.sum() and int(got["n_valid_side"]) == valid_side.sum() > 0
    assert got["origin_side"].tolist() == list(draws["origin_side"]) and np.array_equal(got["angles"], f["angles"])
    # wiring only (the cameras and the warp have their own fixtures): the tables are the reference's up to fp32 rounding of |values| <= 6
    assert np.abs(tables["all_rays"] - f["all_rays"]).max() < 1e-5 and np.abs(full["c2w"] - f["side_c2w"]).max() < 1e-5
    assert np.abs(full["rays"] - f["side_rays"]).max() < 1e-5 and s.rgb_num == int((f["rgb"].sum(-1) != 3).sum())
    # ref_patch_origin="real" moves the reference-view patch to the real window's origin and nothing else
    b2 = numpy_batch(make_sampler(ref_patch_origin="real").draw(choices))
    want2 = SO.to_system(SO.sample(tables, full, draws, *s.window, mirror_quirk=False), full, u_proj)
    for k in want2:
        if k != "n_landed":
            assert same_bits(b2[k], np.ascontiguousarray(want2[k])), k
    assert not same_bits(b2["rays_full"], got["rays_full"]) and same_bits(b2["rays_side"], got["rays_side"])


def check_invariants(s, b, tag=""):
    """what every draw must satisfy, against the oracle on the sampler's own tables and the full frame of the drawn pose"""
    got = numpy_batch(b)
    tables, full = numpy_view(s, b["angles"])
    valid_real, valid_side = oracle_counts(s, tables, full)
    if s.require_content:
        assert int(got["n_valid_real"]) == valid_real.sum() and int(got["n_valid_side"]) == valid_side.sum(), tag
    else:                                                                                      # no valid map: every candidate counts
        assert int(got["n_valid_real"]) == int(got["n_valid_side"]) == s.nx * s.ny, tag
    (xr, yr), (xs, ys) = got["origin_real"].tolist(), got["origin_side"].tolist()
    assert 0 <= xr < s.nx and 0 <= yr < s.ny and 0 <= xs < s.nx and 0 <= ys < s.ny, tag        # np.random.randint(0, w - (ps - 1) sW - 1)
    if s.require_content:
        if valid_real.any():
            assert valid_real[yr, xr] == 1 and got["real_patch"].max() != 0, tag               # rot3d:459
        if valid_side.any():
            assert valid_side[ys, xs] == 1 and got["warp_patch_depth"].sum() != 0, tag         # rot3d:493
        else:
            assert (xs, ys) == (0, 0), tag
    draws = dict(origin_real=(xr, yr), origin_side=(xs, ys), ray_idx=np.zeros(0, np.int64), ray_idx2=np.zeros(0, np.int64))
    want = SO.to_system(SO.sample(tables, full, draws, *s.window, mirror_quirk=s.ref_patch_origin == "side"))
    for k in ("rays_full", "rgbs_full", "depth_gt", "rays_side", "real_patch", "warp_patch", "warp_patch_depth", "side_coord", "side_rgb"):
        assert same_bits(got[k], np.ascontiguousarray(want[k])), (tag, k)
    assert got["side_coord"][0].tolist() == [ys + s.sy * i for i in range(s.ph)], tag          # rows = ll + sW i, columns = up + sH i
    assert got["side_coord"][1].tolist() == [xs + s.sx * i for i in range(s.pw)], tag
    n_nonwhite = s.num - s.num // 10
    assert got["rays"].shape == (s.num, 8) and got["rgbs"].shape == (s.num, 3) and got["depth"].shape == (s.num, 1)
    assert (got["rgbs"][:n_nonwhite].sum(-1) != 3).all(), tag                                  # the non-white rows first
    # every ray row is a row of the tables, with its colour and depth
    flat = {tuple(r): i for i, r in enumerate(bits(tables["all_rays"]).tolist())}
    at = np.array([flat[tuple(r)] for r in bits(got["rays"]).tolist()])
    assert same_bits(got["rgbs"], tables["rgb"].reshape(-1, 3)[at]) and same_bits(got["depth"], tables["depth"].reshape(-1, 1)[at]), tag
    n_landed = int(full["mask"].sum())
    assert int(got["n_landed"]) == n_landed and got["rays_proj"].shape == (s.num, 8) and got["depth_proj"].shape == (s.num, 1)
    if n_landed:                                                                               # drawn among the landed pixels of this pose
        landed = {tuple(r) for r in bits(full["rays"][full["mask"].reshape(-1) != 0]).tolist()}
        assert all(tuple(r) in landed for r in bits(got["rays_proj"]).tolist()), tag
    else:
        assert not got["rays_proj"].any() and not got["depth_proj"].any(), tag
    for k, v in got.items():
        if not isinstance(v, tuple) and v.dtype.kind == "f":
            assert np.isfinite(v).all(), (tag, k)
    return (xs, ys), (xr, yr)


def test_twenty_draws_keep_the_invariants():
    s = make_sampler(num=256)
    torch.manual_seed(14)
    sides, reals, angles = set(), set(), []
    for i in range(20):
        b = s.draw()
        side, real = check_invariants(s, b, f"draw {i}")
        sides.add(side), reals.add(real), angles.append(b["angles"].cpu().numpy())
    assert len(sides) > 10 and len(reals) > 10                                                 # 20 draws among hundreds of valid origins
    assert np.std(np.stack(angles)) > 3.0                                                      # N(0, 15) degrees
    torch.manual_seed(14)
    again = s.draw()                                                                           # the documented order from the seeded generator
    torch.manual_seed(14)
    first = s.draw()
    assert all(torch.equal(again[k], first[k]) for k in ("rays", "origin_real", "origin_side", "angles", "rays_proj"))


def test_draws_from_a_view_with_little_content_stay_on_windows_with_content():
    """the fixture's warped depth leaves no origin without content; a 6 x 6 block of depth does, so the valid map decides here"""
    f = fixture()
    depth = np.zeros_like(f["depth"])
    depth[17:23, 17:23] = f["depth"][17:23, 17:23]
    s = make_sampler(num=64, depth=depth)
    torch.manual_seed(20)
    counts = []
    for i in range(10):
        b = s.draw()
        check_invariants(s, b, f"small content {i}")                                           # origin valid, window sum != 0
        counts.append(int(b["n_valid_side"].item()))
    assert all(0 < c < s.nx * s.ny for c in counts)


def test_without_rejection_loops_the_origin_is_uniform_over_all_candidates():
    s = make_sampler(num=64, require_content=False, candidates="all", generator=torch.Generator(device=dev()).manual_seed(15))
    assert (s.nx, s.ny) == (26, 26)
    seen = set()
    for i in range(12):
        b = s.draw()
        side, _ = check_invariants(s, b, f"llff-style draw {i}")
        seen.add(side)
        assert int(b["n_valid_side"].item()) == int(b["n_valid_real"].item()) == 26 * 26
    assert len(seen) > 6


def test_a_depth_map_without_content():
    """An all-zero depth map: every source pixel projects onto ONE target (sn_forward_warp: "zero-depth source pixels take part as in the
    reference"), whose depth is the unseen camera's distance to the reference camera's centre along its axis -- 4 (1 - cos) here, not 0.
    Whether a candidate window reaches that one pixel depends on the pose, so n_valid_side is held to the oracle's count on every draw,
    and to 0 -- with the fallback origin (0, 0), nothing NaN, no exception -- on the draws where the oracle finds no window with content
    (there must be some among the ten).  A depth map from which NOTHING lands (all NaN: dropped) gives 0 on every draw."""
    f = fixture()
    s = make_sampler(num=256, depth=np.zeros_like(f["depth"]))
    torch.manual_seed(16)
    empty = 0
    for i in range(10):
        b = s.draw()
        check_invariants(s, b, f"zero depth {i}")
        if int(b["n_valid_side"].item()) == 0:
            empty += 1
            assert b["origin_side"].tolist() == [0, 0] and not b["warp_patch_depth"].any()
            assert (b["side_rgb"] == 1).all()                                                  # white where nothing landed
    assert empty > 0
    s = make_sampler(num=256, depth=np.full_like(f["depth"], np.nan))
    for i in range(3):
        b = s.draw()
        assert int(b["n_valid_side"].item()) == 0 and int(b["n_landed"].item()) == 0 and b["origin_side"].tolist() == [0, 0]
        assert not b["rays_proj"].any() and not b["depth_proj"].any() and not b["warp_patch_depth"].any()
        assert all(torch.isfinite(v).all() for k, v in b.items() if torch.is_tensor(v) and v.is_floating_point() and k != "depth"
                   and k != "depth_gt")                                                        # the two that ARE the NaN input


def test_constructor_refusals():
    from sinnerf_amd.sampler import OneImageSampler
    f = fixture()
    args = (t(f["rgb"]), t(f["depth"]), t(f["c2w"]), t(f["K"]))
    kw = dict(focal=float(f["focal"]), near=2.0, far=6.0)
    with pytest.raises(RuntimeError):
        OneImageSampler(args[0].cpu(), *args[1:], patch_size=8, **kw)                          # no CPU fallback
    with pytest.raises(ValueError):
        OneImageSampler(*args, patch_size=8, sW=6, sH=6, **kw)                                 # 1 + 7 * 6 > 40: no candidate origin
    with pytest.raises(ValueError):
        OneImageSampler(torch.ones_like(args[0]), *args[1:], patch_size=8, **kw)               # an all-white image: no ray to draw
    with pytest.raises(KeyError):
        make_sampler(num=64).draw({"origin": torch.zeros(2, dtype=torch.int32, device=dev())})
    with pytest.raises(RuntimeError):
        make_sampler(num=64).draw({"angles": torch.zeros(3)})                                  # choices live on the device


def test_draw_can_be_captured_and_each_replay_draws_afresh():
    """torch.cuda.graph raises on anything that synchronises or reads back during capture"""
    for gen in (None, torch.Generator(device=dev()).manual_seed(17)):
        s = make_sampler(num=256, generator=gen)
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            s.draw()
        cur.wait_stream(side)
        g = torch.cuda.CUDAGraph()
        if gen is not None:
            g.register_generator_state(gen)
        with torch.cuda.graph(g):
            b = s.draw()
        seen = []
        for i in range(3):
            g.replay()
            torch.cuda.synchronize()
            check_invariants(s, b, f"replay {i}")
            seen.append((tuple(b["origin_side"].tolist()), tuple(b["angles"].tolist())))
        assert len(set(seen)) == 3


# ---- SinNeRFSystem.train_step_sampled ----------------------------------------------------------------------------------------------------
def tiny_system(seed):
    from sinnerf_amd.system import SinNeRFSystem
    torch.manual_seed(seed)
    sysm = SinNeRFSystem(N_samples=8, N_importance=8, depth_weight=0.5, proj_weight=0.6).to(dev())
    sysm.configure_optimizers()
    return sysm


def test_train_step_sampled_eager():
    sysm, s = tiny_system(18), make_sampler(num=256)
    before = sysm.optimizer.flat.clone()
    for i in range(2):
        out = sysm.train_step_sampled(s)
        assert torch.isfinite(out["loss"]) and out["batch"]["rays"].shape == (256, 8)
        check_invariants(s, out["batch"], f"eager step {i}")
    assert not torch.equal(before, sysm.optimizer.flat) and torch.isfinite(sysm.optimizer.flat).all()
    assert "train/loss_side_depth" in out["log"] and "train/loss_depth_proj" in out["log"]


def test_train_step_sampled_graph():
    sysm, s = tiny_system(19), make_sampler(num=256)
    origins = []
    before = sysm.optimizer.flat.clone()
    for i in range(3):
        out = sysm.train_step_sampled(s, graph=True)
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"])
        side, _ = check_invariants(s, out["batch"], f"replay {i}")
        origins.append(side)
    assert len(sysm._step_graphs) == 1                                                         # captured once, replayed three times
    assert len(set(origins)) > 1                                                               # hundreds of valid origins: not all three equal
    assert not torch.equal(before, sysm.optimizer.flat) and torch.isfinite(sysm.optimizer.flat).all()
    other = make_sampler(num=256)                                                              # another sampler: its own capture
    sysm.train_step_sampled(other, graph=True)
    assert len(sysm._step_graphs) == 2
    sysm.configure_optimizers()                                                                # new flat buffers: the captures are dropped
    assert "_step_graphs" not in sysm.__dict__
