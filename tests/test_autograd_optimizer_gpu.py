"""GPU: the host side of the training path -- NeRF.forward under autograd, the flat optimiser against stale-view / stale-pack failure modes,
the weight-gradient entry against fp64 contractions, the gradient sink, launch-graph capturability (HIP graph == eager).  (Filed by subject in
round 6; these were tests/test_round2_gpu.py.)"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                              # noqa: E402
from tests.test_parity_gpu import dev, embeddings, make_model                  # noqa: E402


def _embedded_inputs(n, seed):
    r = np.random.RandomState(seed)
    pts = r.uniform(-3, 3, (n, 3)).astype(np.float32)
    dirs = r.standard_normal((n, 3)).astype(np.float32)
    return np.concatenate([O.embedding(pts, 10), O.embedding(dirs, 4)], 1)


@pytest.mark.parametrize("sigma_only", [False, True])
def test_nerf_forward_under_autograd_vs_oracle(sigma_only):
    """models/nerf.py:105-148 is an ordinary differentiable module: model(x).backward() must produce the parameter
    gradients torch autograd derives -- checked against oracle_np.nerf_backward (5e-5 per tensor, masks from the stored
    activations as in test_mlp_backward_vs_oracle)."""
    model, p = make_model(2, True)
    model.train()
    n = 700                                                     # ragged 128-point tail
    x_np = _embedded_inputs(n, 0)
    x = torch.from_numpy(x_np[:, :63] if sigma_only else x_np).to(dev())
    out = model(x, sigma_only=sigma_only)                       # grad mode on, parameters require grad
    assert out.requires_grad and out.shape == (n, 1 if sigma_only else 4)
    with torch.no_grad():
        assert torch.equal(out.detach(), model(x, sigma_only=sigma_only))      # training forward == inference forward
    g = np.random.RandomState(1).standard_normal(out.shape).astype(np.float32)
    (out * torch.from_numpy(g).to(dev())).sum().backward()
    got = {k: q.grad.detach().cpu().numpy().astype(np.float64) for k, q in model.named_parameters()}
    cache = {}
    xin = x_np.copy()
    if sigma_only:
        xin[:, 63:] = 0
    ref_out = O.nerf_forward(p, xin, cache=cache)
    assert np.abs(out.detach().cpu().numpy() - (ref_out[:, 3:4] if sigma_only else ref_out)).max() <= 2e-4 * np.abs(ref_out).max()
    g4 = np.concatenate([np.zeros((n, 3), np.float32), g], 1) if sigma_only else g
    ref = O.nerf_backward(p, cache, g4)
    errs = {k: np.linalg.norm(got[k] - v) / max(np.linalg.norm(v), 1e-12) for k, v in ref.items()
            if np.linalg.norm(v) > 0}
    # ReLU masks flip on ~1e-7 activations (1 point in ~2000, see test_mlp_backward_vs_oracle): norm-wise bar
    bad = {k: e for k, e in errs.items() if e > 2e-3}
    assert not bad, bad
    assert np.median(list(errs.values())) <= 5e-5, errs
    if sigma_only:                                              # dir branch / rgb head: exact zeros
        for k in ("rgb.0.weight", "dir_encoding.0.weight", "xyz_encoding_final.weight"):
            assert not got[k].any(), k
    with pytest.raises(NotImplementedError):
        model(x.clone().requires_grad_(True), sigma_only=sigma_only)


def test_nerf_forward_under_autograd_bf16_runs():
    model, _ = make_model(2, True, dtype="bf16")
    model.train()
    x = torch.from_numpy(_embedded_inputs(300, 3)).to(dev())
    out = model(x)
    out.square().mean().backward()
    m32, _ = make_model(2, True)
    m32.train()
    m32(x).square().mean().backward()
    for (k, a), (_, b) in zip(model.named_parameters(), m32.named_parameters()):
        ga, gb = a.grad.flatten().double(), b.grad.flatten().double()
        assert torch.isfinite(ga).all(), k
        if ga.numel() >= 256:
            cos = float(ga @ gb / (ga.norm() * gb.norm()))
            assert cos > 0.995, (k, cos)


def test_flat_adam_survives_zero_grad_set_to_none_and_schedulers():
    """model.zero_grad() with PyTorch's default set_to_none=True detaches the gradient views; the
    step must not run on a stale flat buffer.  Also: FlatAdam is a torch Optimizer (MultiStepLR drives it) and its state
    survives state_dict() / load_state_dict()."""
    from sinnerf_amd import NeRF
    from sinnerf_amd.optim import FlatAdam
    d = dev()
    torch.manual_seed(0)
    a = [NeRF(use_new_activation=True).to(d), NeRF(use_new_activation=True).to(d)]
    b = [NeRF(use_new_activation=True).to(d), NeRF(use_new_activation=True).to(d)]
    for x, y in zip(a, b):
        y.load_state_dict(x.state_dict())
    opt_a = FlatAdam(a, lr=5e-4, eps=1e-8)
    opt_b = torch.optim.Adam([p for m in b for p in m.parameters()], lr=5e-4, eps=1e-8)
    sch_a = torch.optim.lr_scheduler.MultiStepLR(opt_a, milestones=[2], gamma=0.1)
    sch_b = torch.optim.lr_scheduler.MultiStepLR(opt_b, milestones=[2], gamma=0.1)
    rays = torch.from_numpy(O.lego_rays(400, 400, 0)[::640]).to(d)
    import sinnerf_amd
    for step in range(4):
        for m in a + b:
            m.zero_grad(set_to_none=True)                      # the idiom that used to break the flat buffer
        for models in (a, b):
            r = sinnerf_amd.render_rays(models, embeddings(), rays, 64, False, 0, 0, 64, 32768, True)
            (r["rgb_fine"].square().mean() + r["rgb_coarse"].square().mean()).backward()
        if step == 0:
            assert opt_a.grads.sync_views() > 0                 # strays were found and copied back ...
            assert opt_a.grads.sync_views() == 0                # ... and the views are attached again
        opt_a.step(); opt_b.step()
        sch_a.step(); sch_b.step()
        if step == 1:                                           # checkpoint / resume in the middle of the run
            sd = opt_a.state_dict()
            opt_a.exp_avg.zero_(); opt_a.step_count = 0
            opt_a.load_state_dict(sd)
    assert abs(opt_a.param_groups[0]["lr"] - 5e-5) < 1e-12 and abs(opt_b.param_groups[0]["lr"] - 5e-5) < 1e-12
    for x, y in zip(a, b):
        for (k, va), (_, vb) in zip(x.state_dict().items(), y.state_dict().items()):
            assert torch.allclose(va, vb, rtol=1e-4, atol=2e-6), (k, (va - vb).abs().max().item())
    assert sum(float(p.grad.abs().sum()) for m in a for p in m.parameters()) > 0


def test_packed_weights_follow_writes_through_data():
    """a write through .data bumps neither data_ptr nor Parameter._version; invalidate_packed() (called by
    broadcast_parameters / FlatAdam) makes render_rays pick it up."""
    import sinnerf_amd
    mc, _ = make_model(0, True)
    mf, _ = make_model(1, True)
    rays = torch.from_numpy(O.lego_rays(400, 400, 0)[::4000]).to(dev())
    with torch.no_grad():
        r0 = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 64, False, 0, 0, 64, 32768, True)["rgb_fine"].clone()
        mf.rgb[0].bias.data.add_(0.5)                          # behind autograd's back
        r_stale = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 64, False, 0, 0, 64, 32768, True)["rgb_fine"]
        assert torch.equal(r0, r_stale)                        # documented: such a write needs an invalidation
        blob_before = mf.packed().data_ptr()
        mf.invalidate_packed()
        r1 = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 64, False, 0, 0, 64, 32768, True)["rgb_fine"]
        assert mf.packed().data_ptr() == blob_before           # blob re-filled in place, not re-allocated
    assert (r1 - r0).abs().max() > 1e-2
    with torch.no_grad():
        mf.rgb[0].bias.sub_(0.5)                               # a proper in-place update bumps _version: picked up by itself
        r2 = sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 64, False, 0, 0, 64, 32768, True)["rgb_fine"]
    assert torch.allclose(r2, r0, atol=1e-6)


def test_losses_empty_batch_and_device_guard():
    from sinnerf_amd.losses import render_loss, psnr
    e3 = torch.empty((0, 3), device=dev())
    total, stats = render_loss({"rgb_fine": e3, "rgb_coarse": e3}, e3)
    assert torch.isnan(total)                                  # the reference's mean over an empty batch: NaN, no raise
    a, b = torch.rand((100, 3), device=dev()), torch.rand((100, 3), device=dev())
    assert abs(float(psnr(a, b)) - O.psnr(a.cpu().numpy(), b.cpu().numpy())) < 1e-3


# ------------------------------------------------------------------------------------------- fused weight-gradient entry
from tests.helpers import RAW_SHAPES as _RAW_SHAPES, weight_grads_reference as _weight_grads_reference      # noqa: E402


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_state"])
def test_weight_grads_entry_vs_fp64_contractions(mode):
    """sn_weight_grads (plan by value + K-split MFMA launch + one finish launch) against fp64 matmuls of the operands the
    kernel consumes (bf16 modes: rounded to bf16 first), every parameter of a network in its own shape; accumulate=1 adds."""
    import ctypes
    from sinnerf_amd import _lib
    d = dev()
    rows = 4096 + 48                                                          # not a multiple of the K-split size
    torch.manual_seed(3)
    acts = torch.randn((10, rows, 256), device=d); G = torch.randn((10, rows, 256), device=d) * 0.1
    emb = torch.randn((rows, 128), device=d)
    acts[9, :, 128:] = 0
    G[9, :, 132:160] = 0                                                      # the head block carries 4 live columns (sn_mlp_bwd.hip)
    code = {"fp32": 0, "bf16": 1, "bf16_state": 2}[mode]
    if mode == "bf16_state":
        acts, G = acts.bfloat16(), G.bfloat16()
    rnd = (lambda t: t) if mode == "fp32" else (lambda t: t.bfloat16().float())
    ref = _weight_grads_reference(rnd(acts.float()), rnd(emb), rnd(G.float()))
    # bias gradients are fp32 column sums of the STORED values in every mode
    refb = _weight_grads_reference(acts.float(), emb, G.float())
    nbytes = _lib.lib.sn_weight_grads_workspace_bytes(rows, code)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    outs = [torch.full(s, float("nan"), device=d) for s in _RAW_SHAPES]
    arr = (ctypes.c_void_p * 24)(*[o.data_ptr() for o in outs])
    _lib.check(_lib.lib.sn_weight_grads(_lib.ptr(acts), _lib.ptr(emb), _lib.ptr(G), rows, code, _lib.ptr(ws), arr, 0, None), "wg")
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    for i, (o, r, rb) in enumerate(zip(outs, ref, refb)):
        want = (rb if i % 2 else r).reshape(o.shape)
        assert torch.isfinite(o).all(), i
        err = ((o.double() - want).norm() / want.norm()).item()
        # fp32 sums over 4144 points split into up to ~100 K-ranges: 1e-5 covers the association order; bf16 operands 2e-5
        assert err < (1e-5 if mode == "fp32" or i % 2 else 2e-5), (mode, i, err)
    _lib.check(_lib.lib.sn_weight_grads(_lib.ptr(acts), _lib.ptr(emb), _lib.ptr(G), rows, code, _lib.ptr(ws), arr, 1, None), "wg")
    torch.cuda.synchronize()
    for i, (o, f) in enumerate(zip(outs, first)):
        assert torch.equal(o, f + f), i                                       # deterministic partial sums, accumulated once
    # NULL entries are skipped
    arr2 = (ctypes.c_void_p * 24)(*[None if i % 3 else o.data_ptr() for i, o in enumerate(outs)])
    _lib.check(_lib.lib.sn_weight_grads(_lib.ptr(acts), _lib.ptr(emb), _lib.ptr(G), rows, code, _lib.ptr(ws), arr2, 0, None), "wg")
    torch.cuda.synchronize()
    for i, (o, f) in enumerate(zip(outs, first)):
        assert torch.equal(o, f + f if i % 3 else f), i
    assert _lib.lib.sn_weight_grads_workspace_bytes(100, code) == -5          # SN_E_BADSHAPE


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gradient_sink_equals_autograd_accumulation(dtype):
    """FlatGradBuffer's sink (finish kernel accumulates into the flat buffer, backward returns no parameter gradients)
    against the plain autograd route (24 tensors per network returned, AccumulateGrad adds them): same gradients, also when
    two backward passes accumulate."""
    from sinnerf_amd.system import SinNeRFSystem
    d = dev()
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::311][:384]).to(d)
    rgbs = torch.rand((rays.shape[0], 3), device=d)
    flats = {}
    for sink in (True, False):
        torch.manual_seed(0)
        sysm = SinNeRFSystem(N_importance=64, perturb=1.0, noise_std=1.0, compute_dtype=dtype).to(d)
        sysm.configure_optimizers()
        if not sink:
            for m in sysm.models:
                del m._grad_sink
        sysm.optimizer.zero_grad()
        for rep in range(2):
            torch.manual_seed(10 + rep)
            sysm.training_step({"rays": rays, "rgbs": rgbs})["loss"].backward()
        assert sysm._flat.sync_views() == 0                                   # the views stayed attached in both modes
        flats[sink] = sysm._flat.flat.clone()
    assert torch.isfinite(flats[True]).all() and flats[True].abs().max() > 0
    err = (flats[True] - flats[False]).norm() / flats[False].norm()
    assert err < 1e-6, err


def test_train_step_replayed_from_hip_graph_equals_eager():
    """SinNeRFSystem.train_step(graph=True): zero / forward / loss / backward captured once into a HIP graph (nothing on
    that path is built on the host or synchronises) and replayed with new batches, the exchange step eager.  With the
    stochastic parts off (perturb = noise_std = 0) the parameter trajectory must be IDENTICAL to eager steps; with them on
    the loss must still go down (the captured torch.rand / randn draws advance with every replay)."""
    from sinnerf_amd.system import SinNeRFSystem
    d = dev()
    allr = O.lego_rays(400, 400, seed=0)
    batches = [{"rays": torch.from_numpy(allr[k::311][:512].copy()).to(d), "rgbs": torch.rand((512, 3), device=d)} for k in range(3)]
    finals = {}
    for graph in (False, True):
        torch.manual_seed(0)
        sysm = SinNeRFSystem(N_importance=64, perturb=0.0, noise_std=0.0, compute_dtype="bf16", lr=5e-4).to(d)
        sysm.configure_optimizers()
        losses = []
        for it in range(6):
            losses.append(float(sysm.train_step(batches[it % 3], graph=graph)["loss"]))
        finals[graph] = (sysm.optimizer.flat.clone(), losses)
        if graph:
            assert len(sysm._step_graphs) == 1                                # one capture serves every batch of that shape
            with torch.no_grad():                                             # eager use afterwards sees the UPDATED weights
                r1 = sysm(batches[0]["rays"])["rgb_fine"].clone()
            for m in sysm.models:
                m.invalidate_packed()
            with torch.no_grad():
                r2 = sysm(batches[0]["rays"])["rgb_fine"]
            assert torch.equal(r1, r2)
    assert finals[True][1] == finals[False][1], (finals[True][1], finals[False][1])
    assert torch.equal(finals[True][0], finals[False][0])
    torch.manual_seed(1)
    sysm = SinNeRFSystem(N_importance=64, perturb=1.0, noise_std=1.0, lr=5e-4).to(d)
    losses = [float(sysm.train_step(batches[0], graph=True)["loss"]) for _ in range(12)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert len(set(losses)) == len(losses)                                    # fresh random draws on every replay


def test_gradient_sink_is_skipped_for_frozen_or_detached_parameters():
    """The sink is only taken while EVERY parameter that needs a gradient still has its flat-buffer view as .grad: a frozen
    parameter simply receives nothing; a parameter whose .grad was replaced makes the backward fall back to returning the
    gradients (autograd accumulates them as usual) -- same numbers either way."""
    from sinnerf_amd.system import SinNeRFSystem
    d = dev()
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::411][:256]).to(d)
    rgbs = torch.rand((rays.shape[0], 3), device=d)
    torch.manual_seed(0)
    ref = SinNeRFSystem(N_importance=64, perturb=0.0, noise_std=0.0).to(d)
    ref.configure_optimizers()
    ref.optimizer.zero_grad()
    ref.training_step({"rays": rays, "rgbs": rgbs})["loss"].backward()
    want = {n: p.grad.clone() for n, p in ref.named_parameters()}
    # (a) frozen parameter
    torch.manual_seed(0)
    a = SinNeRFSystem(N_importance=64, perturb=0.0, noise_std=0.0).to(d)
    a.nerf_fine.xyz_encoding_3[0].weight.requires_grad_(False)
    a.configure_optimizers()
    a.optimizer.zero_grad()
    a.training_step({"rays": rays, "rgbs": rgbs})["loss"].backward()
    for n, p in a.named_parameters():
        if n == "nerf_fine.xyz_encoding_3.0.weight":
            assert p.grad is None
        else:
            assert torch.allclose(p.grad, want[n], rtol=1e-5, atol=1e-9), n
    # (b) one .grad detached from the flat buffer: fallback route, autograd accumulates into the replacement
    torch.manual_seed(0)
    b = SinNeRFSystem(N_importance=64, perturb=0.0, noise_std=0.0).to(d)
    b.configure_optimizers()
    b.optimizer.zero_grad()
    w = b.nerf_coarse.xyz_encoding_1[0].weight
    w.grad = torch.zeros_like(w)
    b.training_step({"rays": rays, "rgbs": rgbs})["loss"].backward()
    for n, p in b.named_parameters():
        assert torch.allclose(p.grad, want[n], rtol=1e-5, atol=1e-9), n
    assert b._flat.sync_views() == 1                                          # ... and the step repairs the stray view
    assert torch.allclose(b._flat.flat, ref._flat.flat, rtol=1e-5, atol=1e-9)
