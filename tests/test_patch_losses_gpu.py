"""GPU: the losses on the rendered patches -- sn_patch_loss (MSE pair + kornia SSIM), sn_depth_smoothness, their Python surface
(sinnerf_amd/losses.py) and SinNeRFSystem.patch_losses -- against the fp64 evaluation of tests/patch_loss_oracle.py.

The bar of every compared quantity (a loss value; a gradient as a relative L2 norm) is max(4 e32, 1e-6), e32 being the error of the
oracle evaluated in fp32 against its fp64 evaluation on the same inputs (patch_loss_oracle.bar).  Each test prints its figures before
it asserts."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import patch_loss_oracle as PO                                              # noqa: E402

SSIM_SHAPES = [(1, 6, 6, 1), (1, 13, 17, 3), (2, 23, 70, 3), (1, 56, 70, 1)]          # (B, H, W, C)
SMOOTH_SHAPES = [(1, 2, 2, 3), (2, 13, 17, 3), (1, 56, 70, 3)]


def dev():
    return torch.device("cuda:0")


def nchw(t):
    return t.permute(0, 3, 1, 2)


def patches(shape, family, seed):
    """(coarse, fine, target), channel-last fp32 on the host"""
    g = torch.Generator().manual_seed(seed)
    coarse, fine = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if family == "uniform":
        target = torch.rand(shape, generator=g)
    else:                                        # near-identical: where the fp32 evaluation's own error is largest
        target = torch.clamp(fine + 0.02 * torch.randn(shape, generator=g), 0, 1)
    return coarse, fine, target


def run_patch_loss(coarse, fine, target, use_ssim, window=11, w_mse=1.0, w_ssim=PO.SSIM_WEIGHT, want=(True, True)):
    """the raw entry on channel-last host tensors -> (out[4], g_coarse, g_fine) on the host"""
    from sinnerf_amd import _lib as L
    B, H, W, C = target.shape
    c, f, t = (None if x is None else x.to(dev()).contiguous() for x in (coarse, fine, target))
    g_c = torch.full_like(c, float("nan")) if (want[0] and c is not None) else None
    g_f = torch.full_like(f, float("nan")) if (want[1] and f is not None) else None
    out = torch.full((4,), float("nan"), device=dev())
    nbytes = L.lib.sn_patch_loss_workspace_bytes(B, H, W, C, use_ssim)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    L.check(L.lib.sn_patch_loss(L.ptr(c), L.ptr(f), L.ptr(t), B, H, W, C, use_ssim, window, w_mse, w_ssim, L.ptr(g_c), L.ptr(g_f),
                                L.ptr(ws), L.ptr(out), L.stream_ptr()), "sn_patch_loss")
    torch.cuda.synchronize()
    return out.cpu(), None if g_c is None else g_c.cpu(), None if g_f is None else g_f.cpu()


def run_smoothness(idepth, image, want=(True, True)):
    from sinnerf_amd import _lib as L
    B, H, W, C = image.shape
    d, im = idepth.to(dev()).contiguous(), image.to(dev()).contiguous()
    g_d = torch.full_like(d, float("nan")) if want[0] else None
    g_i = torch.full_like(im, float("nan")) if want[1] else None
    out = torch.full((1,), float("nan"), device=dev())
    ws = torch.empty(L.lib.sn_depth_smoothness_workspace_bytes(), dtype=torch.uint8, device=dev())
    L.check(L.lib.sn_depth_smoothness(L.ptr(d), L.ptr(im), B, H, W, C, L.ptr(g_d), L.ptr(g_i), L.ptr(ws), L.ptr(out), L.stream_ptr()),
            "sn_depth_smoothness")
    torch.cuda.synchronize()
    return out.cpu(), None if g_d is None else g_d.cpu(), None if g_i is None else g_i.cpu()


def compare(tag, pairs):
    """pairs: (name, got, want64, e32).  Prints every figure, then asserts every bar."""
    rows = [(name, PO.rel(got, want), e32, PO.bar(e32)) for name, got, want, e32 in pairs]
    print(tag + ": " + "; ".join("%s err %.2e (e32 %.2e, bar %.2e)" % r for r in rows))
    for name, err, e32, bar in rows:
        assert np.isfinite(err) and err <= bar, (tag, name, err, e32, bar)


# 2 x 192 x 192: 288 tiles = partial records, more than one pass of the 256 threads that re-reduce them (SSIM_SHAPES: 1 to 20 records)
@pytest.mark.parametrize("family", ["uniform", "near"])
@pytest.mark.parametrize("shape", SSIM_SHAPES + [(2, 192, 192, 3)], ids=lambda s: "x".join(map(str, s)))
def test_l2_ssim_kernel_against_fp64(shape, family):
    coarse, fine, target = patches(shape, family, seed=sum(shape))
    out, g_c, g_f = run_patch_loss(coarse, fine, target, 1)
    ins = [nchw(coarse), nchw(fine), nchw(target)]
    tot, (gc64, gf64), e_tot, (e_gc, e_gf) = PO.reference(lambda c, f, t: PO.l2_ssim(c, f, t)[0], ins, [0, 1])
    mc, _, e_mc, _ = PO.reference(lambda c, f, t: PO.mse(c, t), ins, [])
    mf, _, e_mf, _ = PO.reference(lambda c, f, t: PO.mse(f, t), ins, [])
    ss, _, e_ss, _ = PO.reference(lambda c, f, t: PO.ssim_loss(f, t, 11), ins, [])
    compare("l2_ssim %s %s" % (shape, family),
            [("mse_coarse", out[0], mc, e_mc), ("mse_fine", out[1], mf, e_mf), ("ssim", out[2], ss, e_ss), ("total", out[3], tot, e_tot),
             ("g_coarse", nchw(g_c), gc64, e_gc), ("g_fine", nchw(g_f), gf64, e_gf)])


@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_term_alone_and_other_windows(shape):
    """w_mse = 0 leaves kornia's ssim_loss; window 3 and 5 move the reflections and the halo"""
    _, fine, target = patches(shape, "uniform", seed=7 + sum(shape))
    for window in (3, 5, 11):
        out, _, g_f = run_patch_loss(None, fine, target, 1, window=window, w_mse=0.0, w_ssim=1.0)
        ins = [nchw(fine), nchw(target)]
        ss, (g64,), e_ss, (e_g,) = PO.reference(lambda f, t: PO.ssim_loss(f, t, window), ins, [0])
        assert out[0] == 0 and out[3] == out[2]
        compare("ssim %s window %d" % (shape, window), [("ssim", out[2], ss, e_ss), ("g_fine", nchw(g_f), g64, e_g)])


@pytest.mark.parametrize("shape", SSIM_SHAPES + [(1, 7, 9, 2), (3, 300, 301, 1)], ids=lambda s: "x".join(map(str, s)))
def test_mse_pair_kernel_against_fp64(shape):
    """use_ssim = 0: any channel count, the window ignored; 3 x 300 x 301 elements take more than one grid stride"""
    coarse, fine, target = patches(shape, "uniform", seed=3 + sum(shape))
    out, g_c, g_f = run_patch_loss(coarse, fine, target, 0, window=0)
    ins = [nchw(coarse), nchw(fine), nchw(target)]
    tot, (gc64, gf64), e_tot, (e_gc, e_gf) = PO.reference(lambda c, f, t: PO.mse(c, t) + PO.mse(f, t), ins, [0, 1])
    mc, _, e_mc, _ = PO.reference(lambda c, f, t: PO.mse(c, t), ins, [])
    assert out[2] == 0
    compare("mse pair %s" % (shape,), [("mse_coarse", out[0], mc, e_mc), ("total", out[3], tot, e_tot), ("g_coarse", nchw(g_c), gc64, e_gc),
                                      ("g_fine", nchw(g_f), gf64, e_gf)])
    # fine alone (a coarse-only render has no 'rgb_fine'; here the other way round)
    out1, none_c, g_f1 = run_patch_loss(None, fine, target, 0)
    assert none_c is None and out1[0] == 0 and out1[1] == out[1] and out1[3] == out[1] and torch.equal(g_f1, g_f)


def smooth_inputs(shape, seed, constant_block=False):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    idepth, image = 0.2 + 0.8 * torch.rand((B, H, W), generator=g), torch.rand(shape, generator=g)
    if constant_block:                           # zero differences inside the block: |.|' = sign, sign(0) = 0
        idepth[:, 3:8, 4:10] = 0.5
        image[:, 2:9, 6:12, :] = 0.25
    return idepth, image


# 257 x 256 pixels: all 256 partial records of the capped grid, each block more than one stride (SMOOTH_SHAPES: 1 to 16 records)
@pytest.mark.parametrize("shape,block", [(s, False) for s in SMOOTH_SHAPES] + [((2, 13, 17, 3), True), ((1, 257, 256, 3), False)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("const" if v else "rand"))
def test_depth_smoothness_kernel_against_fp64(shape, block):
    idepth, image = smooth_inputs(shape, 11 + sum(shape), block)
    out, g_d, g_i = run_smoothness(idepth, image)
    ins = [idepth[:, None], nchw(image)]
    val, (gd64, gi64), e_v, (e_gd, e_gi) = PO.reference(PO.inverse_depth_smoothness_loss, ins, [0, 1])
    if block:
        assert not gd64[:, 0, 4:7, 5:9].any() and (g_d[:, 4:7, 5:9] == 0).all()                 # depth: no edge with a difference
        assert not gi64[:, :, 3:8, 7:11].any() and (g_i[:, 3:8, 7:11, :] == 0).all()             # image: likewise
    compare("smoothness %s%s" % (shape, " constant block" if block else ""),
            [("loss", out[0], val, e_v), ("g_idepth", g_d[:, None], gd64, e_gd), ("g_image", nchw(g_i), gi64, e_gi)])


def test_runs_are_bitwise_equal_and_gradient_pointers_are_optional():
    coarse, fine, target = patches((2, 23, 70, 3), "uniform", seed=5)
    for use_ssim in (1, 0):
        ref = run_patch_loss(coarse, fine, target, use_ssim)
        again = run_patch_loss(coarse, fine, target, use_ssim)
        assert all(torch.equal(a, b) for a, b in zip(ref, again))
        for want in ((True, False), (False, True), (False, False)):
            out, g_c, g_f = run_patch_loss(coarse, fine, target, use_ssim, want=want)
            assert torch.equal(out, ref[0]) and torch.isfinite(out).all()
            assert (g_c is None) == (not want[0]) and (g_f is None) == (not want[1])
            assert (g_c is None or torch.equal(g_c, ref[1])) and (g_f is None or torch.equal(g_f, ref[2]))
    idepth, image = smooth_inputs((2, 13, 17, 3), 6)
    ref = run_smoothness(idepth, image)
    assert all(torch.equal(a, b) for a, b in zip(ref, run_smoothness(idepth, image)))
    for want in ((True, False), (False, True), (False, False)):
        out, g_d, g_i = run_smoothness(idepth, image, want=want)
        assert torch.equal(out, ref[0]) and (g_d is None) == (not want[0]) and (g_i is None) == (not want[1])
        assert (g_d is None or torch.equal(g_d, ref[1])) and (g_i is None or torch.equal(g_i, ref[2]))


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channel_last_view", "nchw_contiguous"])
def test_python_losses_in_both_layouts(layout):
    from sinnerf_amd import losses as SL
    coarse, fine, target = patches((1, 13, 17, 3), "uniform", seed=21)
    idepth, _ = smooth_inputs((1, 13, 17, 3), 22)

    def leaf(t):
        """-> (the leaf that receives .grad, its NCHW form handed to the loss)"""
        if layout == "channel_last_view":
            l = t.to(dev()).requires_grad_(True)
            return l, nchw(l)
        l = nchw(t).contiguous().to(dev()).requires_grad_(True)
        return l, l

    def grad_nchw(l):
        assert l.grad is not None and l.grad.shape == l.shape and l.grad.stride() == l.stride()      # the caller's layout
        return (nchw(l.grad) if layout == "channel_last_view" else l.grad).cpu()

    if layout == "channel_last_view":            # used in place: no copy of a permuted render result
        v, in_place = SL._channel_last(nchw(fine.to(dev())), "fine")
        assert in_place and v.is_contiguous()
    ins = [nchw(coarse), nchw(fine), nchw(target)]
    tgt = nchw(target).to(dev()) if layout == "channel_last_view" else nchw(target).contiguous().to(dev())
    # L2_SSIM_Loss
    (lc, c), (lf, f) = leaf(coarse), leaf(fine)
    res = SL.L2_SSIM_Loss()({"rgb_coarse": c, "rgb_fine": f}, tgt)
    assert set(res) == {"tot", "l2", "ssim"}
    res["tot"].backward()
    tot, (gc64, gf64), e_tot, (e_gc, e_gf) = PO.reference(lambda c, f, t: PO.l2_ssim(c, f, t)[0], ins, [0, 1])
    l2, _, e_l2, _ = PO.reference(lambda c, f, t: PO.l2_ssim(c, f, t)[1], ins, [])
    ss, _, e_ss, _ = PO.reference(lambda c, f, t: PO.l2_ssim(c, f, t)[2], ins, [])
    compare("L2_SSIM_Loss " + layout, [("tot", res["tot"], tot, e_tot), ("l2", res["l2"], l2, e_l2), ("ssim", res["ssim"], ss, e_ss),
                                       ("g_coarse", grad_nchw(lc), gc64, e_gc), ("g_fine", grad_nchw(lf), gf64, e_gf)])
    # ssim_loss: the gradient goes to img1 only
    lf, f = leaf(fine)
    val = SL.ssim_loss(f, tgt, 11)
    (3.0 * val).backward()
    v64, (g64,), e_v, (e_g,) = PO.reference(lambda f, t: 3.0 * PO.ssim_loss(f, t, 11), ins[1:], [0])
    compare("ssim_loss " + layout, [("value", 3.0 * val, v64, e_v), ("g_img1", grad_nchw(lf), g64, e_g)])
    # inverse_depth_smoothness_loss: gradients to both
    (ld, d), (li, im) = leaf(idepth[..., None]), leaf(fine)
    val = SL.inverse_depth_smoothness_loss(d, im)
    val.backward()
    v64, (gd64, gi64), e_v, (e_gd, e_gi) = PO.reference(PO.inverse_depth_smoothness_loss, [idepth[:, None], nchw(fine)], [0, 1])
    compare("inverse_depth_smoothness_loss " + layout, [("value", val, v64, e_v), ("g_idepth", grad_nchw(ld), gd64, e_gd),
                                                        ("g_image", grad_nchw(li), gi64, e_gi)])
    # MSELoss on 4-D patches (what the reference's patch_loss receives), one channel
    (lc, c), (lf, f) = leaf(coarse[..., :1]), leaf(fine[..., :1])
    res = SL.MSELoss()({"rgb_coarse": c, "rgb_fine": f}, tgt[:, :1])
    res["tot"].backward()
    ins1 = [x[:, :1] for x in ins]
    v64, (gc64, gf64), e_v, (e_gc, e_gf) = PO.reference(lambda c, f, t: PO.mse(c, t) + PO.mse(f, t), ins1, [0, 1])
    compare("MSELoss 4-D " + layout, [("tot", res["tot"], v64, e_v), ("g_coarse", grad_nchw(lc), gc64, e_gc),
                                      ("g_fine", grad_nchw(lf), gf64, e_gf)])


# ---- SinNeRFSystem.patch_losses -------------------------------------------------------------------------------------------------------
PSX, PSY, N_RAND = 13, 17, 64
RESULT_KEYS = ("rgb_coarse", "rgb_fine", "depth_coarse", "depth_fine")


def synthetic(seed=0):
    """four `results` dicts of random tensors and a patch batch with every key of the new terms, on the host"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    n = PSX * PSY
    res = [{"rgb_coarse": u(m, 3), "rgb_fine": u(m, 3), "depth_coarse": 2 + 4 * u(m), "depth_fine": 2 + 4 * u(m)}
           for m in (N_RAND, n, n, N_RAND)]
    depth_gt, warp = 2 + 4 * u(n), 2 + 4 * u(n)
    depth_gt[u(n) < 0.3] = 0                     # background pixels
    warp[u(n) < 0.5] = 0                         # pixels the warp did not reach
    batch = {"rgbs": u(N_RAND, 3), "depth": 2 + 4 * u(N_RAND), "rgbs_full": u(n, 3), "depth_proj": 2 + 4 * u(N_RAND), "depth_gt": depth_gt,
             "warp_patch_depth": warp, "real_patch": u(1, 3, PSX, PSY)}
    return res, batch


def reference_total(R, RF, RS, RP, batch, hp):
    """models/sinnerf.py:309-405, 492-509 with vit_weight = dis_weight = 0, in the dtype of its arguments"""
    P = lambda t, c: t.reshape(1, PSX, PSY, c).permute(0, 3, 1, 2)
    patch_loss = (lambda i, t: PO.mse(i["rgb_coarse"], t) + PO.mse(i["rgb_fine"], t)) if hp["patch_loss"] == "mse" else \
        (lambda i, t: PO.l2_ssim(i["rgb_coarse"], i["rgb_fine"], t)[0])
    loss_depth = PO.sl1(RP["depth_fine"], batch["depth_proj"]) + PO.sl1(RP["depth_coarse"], batch["depth_proj"])              # :310-311
    loss_g = PO.mse(R["rgb_coarse"], batch["rgbs"]) + PO.mse(R["rgb_fine"], batch["rgbs"])                                    # :317
    loss_depth = loss_depth + PO.sl1(R["depth_fine"], batch["depth"]) + PO.sl1(R["depth_coarse"], batch["depth"])             # :318-319
    loss_g = loss_g + patch_loss({k: P(RF[k], 3) for k in ("rgb_coarse", "rgb_fine")}, P(batch["rgbs_full"], 3))              # :348
    gt = batch["depth_gt"]
    if hp["dataset_name"] == "dtu_proj":                                                                                      # :360-365
        loss_depth = loss_depth + PO.sl1(RF["depth_fine"], gt, gt > 0) + PO.sl1(RF["depth_coarse"], gt, gt > 0)
    else:                                                                                                                     # :367-369
        loss_depth = loss_depth + patch_loss({"rgb_fine": P(RF["depth_fine"], 1), "rgb_coarse": P(RF["depth_coarse"], 1)}, P(gt, 1))
    smooth = PO.inverse_depth_smoothness_loss(P(RF["depth_fine"], 1), P(RF["rgb_fine"], 3)) \
        + PO.inverse_depth_smoothness_loss(P(RF["depth_coarse"], 1), P(RF["rgb_fine"], 3))                                    # :370-373
    if "blender" in hp["dataset_name"]:                                                                                       # :382-387
        loss_depth = loss_depth + 2 * PO.sl1(RF["depth_coarse"], gt, gt == 0) + 2 * PO.sl1(RF["depth_fine"], gt, gt == 0)
    smooth = smooth + PO.inverse_depth_smoothness_loss(P(RS["depth_coarse"], 1), P(RS["rgb_fine"], 3)) \
        + PO.inverse_depth_smoothness_loss(P(RS["depth_fine"], 1), P(RS["rgb_fine"], 3))                                      # :395-398
    warp = batch["warp_patch_depth"]
    side = PO.sl1(RS["depth_coarse"], warp, warp > 0) + PO.sl1(RS["depth_fine"], warp, warp > 0) if (warp > 0).any() else 0.0 # :399-406
    loss = loss_g + loss_depth * hp["depth_weight"]                                                                           # :499-500
    loss = loss + hp["proj_weight"] * (hp["depth_weight"] * side)                                                             # :504-505
    return loss + smooth * hp["depth_smooth_weight"]                                                                          # :509


def on_device(res, batch, requires_grad=True):
    res = [{k: v.to(dev()).requires_grad_(requires_grad) for k, v in r.items()} for r in res]
    return res, {k: v.to(dev()) for k, v in batch.items()}


CONFIGS = [("blender", "mse", 0.0), ("blender", "l2_ssim", 0.1), ("llff", "l2_ssim", 0.1), ("dtu_proj", "mse", 0.1)]


@pytest.mark.parametrize("dataset_name,patch_loss,dsw", CONFIGS, ids=["-".join(map(str, c)) for c in CONFIGS])
def test_patch_losses_against_the_reference_step_in_fp64(dataset_name, patch_loss, dsw):
    from sinnerf_amd.system import SinNeRFSystem
    hp = dict(dataset_name=dataset_name, patch_loss=patch_loss, depth_smooth_weight=dsw, depth_weight=0.7, proj_weight=0.6)
    sysm = SinNeRFSystem(N_samples=16, N_importance=16, **hp)
    res, batch = synthetic(1)
    dres, dbatch = on_device(res, batch)
    loss, log = sysm.patch_losses(*dres, dbatch)
    loss.backward()
    assert "train/loss_side_depth" in log and ("train/loss_depth_smooth" in log) == (dsw > 0)
    flat = [r[k] for r in res for k in RESULT_KEYS]
    n_t = len(flat)
    keys = list(batch)

    def fn(*xs):
        rs = [dict(zip(RESULT_KEYS, xs[4 * i:4 * i + 4])) for i in range(4)]
        return reference_total(*rs, dict(zip(keys, xs[n_t:])), hp)

    # the masks are taken on exact zeros: the same in either dtype
    tot, g64, e_tot, e_g = PO.reference(fn, flat + [batch[k] for k in keys], list(range(n_t)))
    got = [r[k].grad for r in dres for k in RESULT_KEYS]
    names = ["%s[%d]" % (k, i) for i in range(4) for k in RESULT_KEYS]
    used = [g is not None for g in got]
    # a results tensor no term reads (rgb of the side and the projected render at these weights) has no gradient on either side
    for name, g, w in zip(names, got, g64):
        assert (g is not None) or not w.any(), name
    compare("patch_losses %s %s dsw %g" % (dataset_name, patch_loss, dsw),
            [("total", loss, tot, e_tot)] + [(nm, g, w, e) for nm, g, w, e, u in zip(names, got, g64, e_g, used) if u])


def test_patch_losses_without_warped_pixels_and_without_the_new_keys():
    from sinnerf_amd.losses import render_loss
    from sinnerf_amd.system import SinNeRFSystem
    res, batch = synthetic(2)
    # all-zero warp_patch_depth: finite, and the same total as without the key (hparams that use every other term)
    sysm = SinNeRFSystem(N_samples=16, N_importance=16, dataset_name="blender", patch_loss="l2_ssim", depth_smooth_weight=0.1,
                         depth_weight=0.7)
    dres, dbatch = on_device(res, batch)
    dbatch["warp_patch_depth"] = torch.zeros_like(dbatch["warp_patch_depth"])
    with_zero, log = sysm.patch_losses(*dres, dbatch)
    with_zero.backward()
    grads = [r[k].grad for r in dres for k in RESULT_KEYS if r[k].grad is not None]
    assert torch.isfinite(with_zero).item() and all(torch.isfinite(g).all().item() for g in grads)
    assert log["train/loss_side_depth"].item() == 0
    del dbatch["warp_patch_depth"]
    dres2, _ = on_device(res, batch)
    without, _ = sysm.patch_losses(*dres2, dbatch)
    assert with_zero.item() == without.item()
    # none of the new keys, default hparams: the composition _training_step_patches has always made, bit for bit
    base = SinNeRFSystem(N_samples=16, N_importance=16, depth_weight=0.7)
    old_batch = {k: v for k, v in batch.items() if k in ("rgbs", "depth", "rgbs_full", "depth_proj")}
    dres, dbatch = on_device(res, old_batch)
    new, log = base.patch_losses(*dres, dbatch)
    new.backward()
    assert "train/loss_side_depth" not in log and "train/loss_depth_smooth" not in log
    ores, _ = on_device(res, old_batch)
    old, _ = render_loss(ores[0], dbatch["rgbs"], dbatch["depth"], w_depth=0.7)
    old = old + render_loss(ores[1], dbatch["rgbs_full"])[0]
    old = old + render_loss(ores[3], None, dbatch["depth_proj"], w_depth=0.7)[0]
    old.backward()
    assert torch.equal(new, old)
    for r_new, r_old in zip(dres, ores):
        for k in RESULT_KEYS:
            assert (r_new[k].grad is None) == (r_old[k].grad is None), k
            assert r_new[k].grad is None or torch.equal(r_new[k].grad, r_old[k].grad), k


def test_training_step_with_ssim_and_smoothness_end_to_end():
    """one patch step through the renders: 16 x 12 patch (192 rays per patch render), 256 random rays, 16 + 16 samples"""
    from oracle import oracle_np as O
    from sinnerf_amd.system import SinNeRFSystem
    ph, pw = 16, 12
    torch.manual_seed(0)
    sysm = SinNeRFSystem(N_samples=16, N_importance=16, white_back=False, depth_weight=0.5, patch_loss="l2_ssim", depth_smooth_weight=0.1,
                         dataset_name="llff").to(dev())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    g = torch.Generator().manual_seed(4)
    u = lambda *s: torch.rand(*s, generator=g).to(dev())
    full, side = O.llff_patch_rays(1, pw=pw, ph=ph), O.llff_patch_rays(2, pw=pw, ph=ph)
    n = ph * pw
    assert full.shape == (n, 8) and n == 192
    warp = 1.2 + 6.8 * u(n)
    warp[::3] = 0
    batch = {"rays": t(O.llff_like_rays(256, 0)), "rgbs": u(256, 3), "depth": 1.2 + 6.8 * u(256), "rays_full": t(full), "rgbs_full": u(n, 3),
             "rays_side": t(side), "rays_proj": t(O.llff_like_rays(256, 3)), "depth_proj": 1.2 + 6.8 * u(256),
             "depth_gt": 1.2 + 6.8 * u(n), "warp_patch_depth": warp, "real_patch": u(1, 3, ph, pw)}
    torch.manual_seed(9)
    out = sysm.training_step(batch)
    out["loss"].backward()
    assert torch.isfinite(out["loss"]).item()
    for key in ("train/loss_depth_smooth", "train/loss_side_depth"):
        assert torch.isfinite(out["log"][key]).item() and out["log"][key].item() > 0, key
    for m in sysm.models:
        for name, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all().item() and p.grad.abs().sum().item() > 0, name
    # the same kernels on the same inputs: patch_losses on the four renders under the same seed
    torch.manual_seed(9)
    renders = [sysm(batch[k].reshape(-1, 8)) for k in ("rays", "rays_full", "rays_side", "rays_proj")]
    again, _ = sysm.patch_losses(*renders, batch)
    rel = abs(again.item() - out["loss"].item()) / abs(out["loss"].item())
    print("training_step loss %.6f, patch_losses on the same renders %.6f (rel %.1e)" % (out["loss"].item(), again.item(), rel))
    assert rel <= 1e-5
