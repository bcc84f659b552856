"""GPU: the hand-scheduled bf16-state training kernels (bit identity with the compiler-scheduled ones, fuzz, determinism, the bf16 form of
`emb`), training on the BASELINE config shapes (llff 5292-ray patch, the four-render step), the system surface (optimiser upgrade, FlatAdam state
dict, refusals) and bench.py as its own launcher with two gloo ranks on one GPU.  (Filed by subject in round 6; these were
tests/test_round3_gpu.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                                            # noqa: E402
from tests.test_parity_gpu import dev, embeddings, injected_rng, make_model                  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grads(m):
    return {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}


def test_bf16_training_render_gradients_on_llff_patch_shape():
    """Gradients of a bf16 TRAINING render on the BASELINE configs[2] patch (llff 63x84 stride 4: N = 5292 rays,
    white_back=False, perturb=1, noise_std=1, 64+64) against ``oracle_np.render_rays_backward`` with every contraction's
    operands rounded to bf16 (forward under ``bf16_operands()``, backward with ``operand_round=bf16_round``).  The whole patch
    goes through the GPU path; the loss weights every third ray (rays are independent: the others contribute exact zeros),
    so the numpy oracle only has to differentiate 1764 rays.  Same random draws on both sides (injected in the reference's
    consumption order)."""
    import sinnerf_amd
    rays = O.llff_patch_rays(0)
    n, S, NI = rays.shape[0], 64, 64
    assert n == 5292
    sub = np.arange(0, n, 3)
    r = np.random.RandomState(11)
    rng = {"perturb": r.uniform(0, 1, (n, S)).astype(np.float32), "noise_coarse": r.standard_normal((n, S)).astype(np.float32),
           "u": r.uniform(0, 1, (n, NI)).astype(np.float32), "noise_fine": r.standard_normal((n, S + NI)).astype(np.float32)}
    coef = {k: np.zeros(sh, np.float32) for k, sh in (("rgb_coarse", (n, 3)), ("rgb_fine", (n, 3)), ("depth_coarse", (n,)),
                                                      ("depth_fine", (n,)))}
    for k in coef:
        coef[k][sub] = r.standard_normal(coef[k][sub].shape).astype(np.float32) / len(sub)
    mc, pc = make_model(0, True, dtype="bf16")
    mf, pf = make_model(1, True, dtype="bf16")
    mc.train(); mf.train()
    order = [("rand", rng["perturb"]), ("randn", rng["noise_coarse"]), ("rand", rng["u"]), ("randn", rng["noise_fine"])]
    with injected_rng(order) as left:
        res = sinnerf_amd.render_rays([mc, mf], embeddings(), torch.from_numpy(rays).to(dev()), S, False, 1.0, 1.0, NI, 32768, False)
        assert not left
    assert res["rgb_fine"].shape == (n, 3) and all(torch.isfinite(v).all() for v in res.values())
    sum((res[k] * torch.from_numpy(v).to(dev())).sum() for k, v in coef.items()).backward()
    got = [_grads(mc), _grads(mf)]
    rs = {k: v[sub] for k, v in rng.items()}
    up = {k: v[sub].astype(np.float64) for k, v in coef.items()}
    with O.bf16_operands():
        ref16 = O.render_rays_backward([pc, pf], rays[sub], up, S, False, 1.0, 1.0, NI, False, rs, operand_round=O.bf16_round)
    ref32 = O.render_rays_backward([pc, pf], rays[sub], up, S, False, 1.0, 1.0, NI, False, rs)
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
    cos = lambda a, b: float((a * b).sum() / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
    for tag, g, r16, r32 in (("coarse", got[0], ref16[0], ref32[0]), ("fine", got[1], ref16[1], ref32[1])):
        e16 = {k: rel(g[k], r16[k]) for k in r16}
        e32 = {k: rel(g[k], r32[k]) for k in r32}
        print(tag, "vs bf16-emulated oracle", {k: "%.1e" % e for k, e in e16.items()})
        print(tag, "vs fp32 oracle         ", {k: "%.1e" % e for k, e in e32.items()})
        # same roundings, different accumulation order; ReLU masks / the fine samples' positions (sample_pdf of the coarse
        # weights) flip for a few points whose pre-activation is within a bf16 ulp of zero: a norm-wise bar, plus direction
        big = [k for k in r16 if r16[k].size >= 256]
        assert max(e16[k] for k in big) <= 3e-2, (tag, e16)
        assert min(cos(g[k], r16[k]) for k in big) >= 0.9995, tag
        # mixed precision stays close to the fp32 gradient as well (cosine per parameter tensor)
        assert min(cos(g[k], r32[k]) for k in big) >= 0.99, tag        # measured 0.9971 coarse / 0.9945 fine (xyz_encoding_1: 0.08-0.11 rel vs fp32)


def _patch_batch(cfg):
    sys.path.insert(0, REPO)
    import bench
    return bench.train_cfg_batch(O, dev(), cfg)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_four_render_training_step_equals_the_sum_of_its_renders(dtype):
    """SinNeRFSystem.training_step on a patch batch = the four renders of sinnerf.py:304-307 with MSE + SmoothL1-depth
    terms: its loss and its gradients equal what four separate single-render steps accumulate (same seeds)."""
    from sinnerf_amd.system import SinNeRFSystem
    from sinnerf_amd.losses import render_loss
    import sinnerf_amd
    batch = _patch_batch("train_cfg3")                                   # 4096 + 5292 + 5292 + 4096, white_back=False
    torch.manual_seed(3)
    sysm = SinNeRFSystem(N_importance=64, compute_dtype=dtype, perturb=1.0, noise_std=1.0, white_back=False, depth_weight=0.5).to(dev())
    sysm.configure_optimizers()
    sysm.optimizer.zero_grad()
    torch.manual_seed(100)
    out = sysm.training_step(batch)
    out["loss"].backward()
    g_step = sysm._flat.flat.clone()
    # the same four renders one by one
    sysm.optimizer.zero_grad()
    torch.manual_seed(100)
    total = 0.0
    rr = lambda rays: sinnerf_amd.render_rays(sysm.models, sysm.embeddings, rays, 64, False, 1.0, 1.0, 64, 32768, False)
    r1, r2, r3, r4 = rr(batch["rays"]), rr(batch["rays_full"]), rr(batch["rays_side"]), rr(batch["rays_proj"])
    for res, rgbs, depths in ((r1, batch["rgbs"], batch["depth"]), (r2, batch["rgbs_full"], None), (r4, None, batch["depth_proj"]),
                              (r3, batch["side_rgb"], None)):
        l, _ = render_loss(res, rgbs, depths, w_depth=0.5)
        l.backward()
        total += float(l)
    g_sep = sysm._flat.flat.clone()
    assert abs(float(out["loss"]) - total) <= 1e-5 * max(1.0, abs(total)), (float(out["loss"]), total)
    assert float(g_step.abs().max()) > 0
    err = float((g_step - g_sep).norm() / g_sep.norm())
    assert err <= (1e-5 if dtype == "fp32" else 1e-5), err              # same kernels, same inputs: accumulation order only
    # and a few optimisation steps on this batch reduce the loss
    losses = [float(sysm.train_step(batch)["loss"]) for _ in range(6)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_optimizer_configured_on_host_is_upgraded_on_device():
    """configure_optimizers() before .to(device) builds a stock Adam with no flat buffers; train_step /
    setup_distributed must not run a step without the flat exchange -- the optimiser is rebuilt as FlatAdam (keeping lr and
    the scheduler), replica_checksum works, and a stale captured graph is dropped."""
    from sinnerf_amd.optim import FlatAdam
    from sinnerf_amd.system import SinNeRFSystem
    torch.manual_seed(0)
    sysm = SinNeRFSystem(N_importance=64, lr=3e-4, perturb=1.0, noise_std=0.0)
    opts, scheds = sysm.configure_optimizers()                           # on the host: torch.optim.Adam
    assert not isinstance(opts[0], FlatAdam)
    sysm = sysm.to(dev())
    flat = sysm.setup_distributed()
    assert isinstance(sysm.optimizer, FlatAdam) and flat is sysm.optimizer.grads
    assert abs(sysm.optimizer.param_groups[0]["lr"] - 3e-4) < 1e-12 and scheds[0].optimizer is sysm.optimizer
    # the scheduler is rebuilt on the new optimiser (its step-order bookkeeping wraps FlatAdam.step, not the discarded Adam's)
    assert sysm._schedulers[0] is not scheds[0] and sysm._schedulers[0].optimizer is sysm.optimizer
    assert list(sysm._schedulers[0].milestones.elements()) == list(scheds[0].milestones.elements())
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::313][:512]).to(dev())
    batch = {"rays": rays, "rgbs": torch.rand((512, 3), device=dev())}
    before = sysm.replica_checksum().clone()
    sysm.train_step(batch)
    assert not torch.equal(before, sysm.replica_checksum())              # the step really updated the flat parameters
    # graph cache: a second configure_optimizers() moves the flat buffers; the captured step must not be replayed
    sysm.train_step(batch, graph=True)
    assert len(sysm._step_graphs) == 1
    old_ptr = sysm.optimizer.flat.data_ptr()
    sysm.configure_optimizers()
    assert "_step_graphs" not in sysm.__dict__
    c0 = sysm.replica_checksum().clone()
    sysm.train_step(batch, graph=True)
    assert not torch.equal(c0, sysm.replica_checksum())                  # the NEW buffers were updated
    sysm.hparams.noise_std = 1.0                                          # a hyper-parameter the launches bake in -> new capture
    sysm.train_step(batch, graph=True)
    assert len(sysm._step_graphs) == 2
    del old_ptr


def test_flat_adam_state_dict_is_torch_adam_layout_both_ways():
    """FlatAdam.state_dict() / load_state_dict() speak torch.optim.Adam's layout, so a reference / Lightning
    checkpoint's optimizer state resumes here and the other way round; state of a re-ordered parameter set is refused."""
    from sinnerf_amd import NeRF
    from sinnerf_amd.optim import FlatAdam
    import sinnerf_amd
    d = dev()
    torch.manual_seed(1)
    a = [NeRF(use_new_activation=True).to(d), NeRF(use_new_activation=True).to(d)]
    b = [NeRF(use_new_activation=True).to(d), NeRF(use_new_activation=True).to(d)]
    for x, y in zip(a, b):
        y.load_state_dict(x.state_dict())
    opt_t = torch.optim.Adam([p for m in a for p in m.parameters()], lr=5e-4, eps=1e-8)
    rays = torch.from_numpy(O.lego_rays(400, 400, 0)[::640]).to(d)

    def backward(models):
        for m in models:
            m.zero_grad(set_to_none=False)
        r = sinnerf_amd.render_rays(models, embeddings(), rays, 64, False, 0, 0, 64, 32768, True)
        (r["rgb_fine"].square().mean() + r["rgb_coarse"].square().mean()).backward()
    for _ in range(2):
        backward(a); opt_t.step()
    # torch Adam state -> FlatAdam on an identical copy of the CURRENT parameters
    for x, y in zip(a, b):
        y.load_state_dict(x.state_dict())
    opt_f = FlatAdam(b, lr=1.0, eps=1e-8)
    opt_f.load_state_dict(opt_t.state_dict())
    assert opt_f.step_count == 2 and abs(opt_f.param_groups[0]["lr"] - 5e-4) < 1e-12
    backward(a); opt_t.step()
    opt_f.zero_grad(); backward(b); opt_f.step()
    for x, y in zip(a, b):
        for (k, va), (_, vb) in zip(x.state_dict().items(), y.state_dict().items()):
            assert torch.allclose(va, vb, rtol=1e-4, atol=2e-6), (k, (va - vb).abs().max().item())
    # FlatAdam state -> torch Adam
    opt_t2 = torch.optim.Adam([p for m in a for p in m.parameters()], lr=1.0, eps=1e-8)
    opt_t2.load_state_dict(opt_f.state_dict())
    st = opt_t2.state_dict()["state"]
    assert len(st) == len(opt_f.grads.params) and int(st[0]["step"]) == 3
    off = 0
    for i, p in enumerate(opt_f.grads.params):
        assert torch.equal(st[i]["exp_avg"].reshape(-1), opt_f.exp_avg[off:off + p.numel()])
        off += p.numel()
    # a parameter set in another order is refused (shape check per parameter, not a numel check)
    sd = opt_f.state_dict()
    sd["state"][0], sd["state"][2] = sd["state"][2], sd["state"][0]
    with pytest.raises(ValueError):
        opt_f.load_state_dict(sd)


def test_bench_self_launch_two_gloo_ranks_one_gpu():
    """`python bench.py --gpus 2 --dist-backend gloo` with NO external launcher on a 1-GPU box: both ranks render, the
    data-parallel training leg runs its all-reduce across the two ranks and the replicas stay identical."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full", "--gpus", "2", "--dist-backend", "gloo", "--steps", "1",
                          "--warmup", "1", "--hw", "120", "120", "--no-cpu-baseline"], env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["value"] > 0
    leg = rec["train_dp"]
    assert leg["n_ranks_seen"] == 2 and leg["all_reduce_backend"] == "gloo" and leg["all_reduce_us"] > 0
    # the full (un-shortened) record is written beside the one JSON line; the line itself stays under the driver's 8 KB tail
    assert len(lines[0]) < 8000
    full = json.load(open(os.path.join(REPO, "gpurun_out", "bench_full_fp32_n2.json")))
    assert full["train_dp"]["replicas_identical_after"] >= 3
    # BASELINE configs[4] / configs[3] as the sharded workloads they name: one frame split over the ranks with the
    # rgb tiles gathered on rank 0, and the dtu four-render step per rank with the flat all-reduce
    c5, c4 = rec["records"]["config5_sharded"], rec["records"]["train_cfg4_dp"]
    assert c5["n_ranks"] == 2 and c5["value"] > 0 and c5["gathered_rows_on_rank0"] == 2 * c5["rays_per_rank"] == 240 * 240
    assert c4["n_ranks"] == 2 and c4["all_reduce_backend"] == "gloo" and c4["all_reduce_us"] > 0 and c4["ms_per_step"] > 0
    assert full["records"]["train_cfg4_dp"]["replicas_identical_after"] >= 3
    # ... and the STRONG-scaling form of the headline workload (round 6): ONE frame of the headline shape partitioned over the ranks
    hs = rec["records"]["headline_frame_sharded"]
    assert hs["scaling"] == "strong" and hs["n_ranks"] == 2 and hs["gathered_rows_on_rank0"] == 2 * hs["rays_per_rank"] == 120 * 120
    assert hs["value"] > 0 and hs["dtype"] == "fp32"


def _train_forward(model, rays_t, z_t, flag):
    """sn_mlp_forward_train (SN_DTYPE_BF16_STATE) through the C ABI; flag = 0 (hand-scheduled) or SN_DTYPE_COMPILER_SCHEDULED"""
    from sinnerf_amd import _lib
    n, s = z_t.shape
    P = n * s
    rows = -(-P // 256) * 256
    d = rays_t.device
    out = torch.zeros((n, s, 4), dtype=torch.float32, device=d)
    acts = torch.full((10, rows, 256), float("nan"), dtype=torch.bfloat16, device=d)
    emb = torch.full((rows, 128), float("nan"), dtype=torch.float32, device=d)
    _lib.check(_lib.lib.sn_mlp_forward_train(_lib.ptr(model.packed()), model.kernel_dtype(_lib.SN_DTYPE_BF16_STATE) | flag, _lib.ptr(rays_t),
                                             _lib.ptr(z_t), n, s, _lib.ptr(out), _lib.ptr(acts), _lib.ptr(emb), rows, _lib.stream_ptr()),
               "sn_mlp_forward_train")
    torch.cuda.synchronize()
    return out, acts, emb


@pytest.mark.parametrize("n_rays,S", [(60, 37), (700, 64), (4096, 128)])
def test_hand_scheduled_training_forward_equals_compiler_scheduled_bit_for_bit(n_rays, S):
    """csrc/sn_mlp_fwd_bf16_t.hip (generated trunk, conflict-free staging planes, 4-slot ring) against the compiler-scheduled
    mlp_fwd_bf16_kernel<false, 0, 2>: output, every stored activation row, the ReLU sign words and the embedded inputs are the
    SAME BITS (same operands, same fp32 accumulation order).  2220 points = a ragged last tile; 4096 x 128 = the fine pass of a
    training step (every workgroup walks several tiles: the weight ring wraps)."""
    from sinnerf_amd import _lib
    model, p = make_model(3, True, dtype="bf16")
    rays = O.lego_rays(400, 400, seed=0)[:: max(1, 160000 // n_rays)][:n_rays]
    z = O.coarse_z_vals(rays, S, False, 1.0, np.random.RandomState(1).uniform(0, 1, (rays.shape[0], S)).astype(np.float32))
    rays_t, z_t = torch.from_numpy(rays).to(dev()), torch.from_numpy(z).to(dev())
    new = _train_forward(model, rays_t, z_t, 0)
    old = _train_forward(model, rays_t, z_t, _lib.SN_DTYPE_COMPILER_SCHEDULED)
    P = rays.shape[0] * S
    assert torch.equal(new[0], old[0])
    a_new, a_old = new[1].view(torch.int16), old[1].view(torch.int16)
    rows = a_new.shape[1]
    # rows of whole tiles are written by both kernels (pad rows: copies of the last point); compare everything both define
    for l in range(10):
        if not torch.equal(a_new[l], a_old[l]):
            bad = (a_new[l] != a_old[l]).nonzero()
            raise AssertionError(("acts slot", l, "first mismatches", bad[:5].tolist(), "count", int(bad.shape[0]), "rows", rows, "P", P))
    e_new, e_old = new[2].view(torch.int32), old[2].view(torch.int32)
    cols = torch.cat([torch.arange(0, 63), torch.arange(64, 91)]).to(dev())         # pad columns are never written
    assert torch.equal(e_new[:, cols], e_old[:, cols])
    # and against the oracle: the forward output at the 1e-3-class bf16 bar of the other bf16 tests
    xin = np.concatenate([O.embedding(O._points(rays, z).reshape(-1, 3), 10), np.repeat(O.embedding(rays[:, 3:6], 4), S, 0)], 1)
    if P <= 50000:
        with O.bf16_operands():
            ref = O.nerf_forward(p, xin)
        got = new[0].cpu().numpy().reshape(-1, 4)
        assert np.abs(got - ref).max() <= 6e-3 * np.abs(ref).max()


@pytest.mark.parametrize("n_rays,S", [(60, 37), (4096, 128)])
def test_hand_scheduled_backward_chain_equals_compiler_scheduled_bit_for_bit(n_rays, S):
    """csrc/sn_mlp_bwd_bf16_t.hip (generated slab loop: sign words a layer ahead, staging planes) against
    mlp_bwd_chain_bf16_kernel<true>: G (all ten slots incl. the rgb / sigma pad block) and g_out are the SAME BITS."""
    from sinnerf_amd import _lib
    model, p = make_model(3, True, dtype="bf16")
    rays = O.lego_rays(400, 400, seed=0)[:: max(1, 160000 // n_rays)][:n_rays]
    z = O.coarse_z_vals(rays, S, False, 1.0, np.random.RandomState(1).uniform(0, 1, (rays.shape[0], S)).astype(np.float32))
    rays_t, z_t = torch.from_numpy(rays).to(dev()), torch.from_numpy(z).to(dev())
    out, acts, emb = _train_forward(model, rays_t, z_t, 0)
    P = rays.shape[0] * S
    rows = acts.shape[1]
    g = torch.from_numpy(np.random.RandomState(2).standard_normal((rays.shape[0], S, 4)).astype(np.float32)).to(dev())
    res = []
    for flag in (0, _lib.SN_DTYPE_COMPILER_SCHEDULED):
        G = torch.zeros((10, rows, 256), dtype=torch.bfloat16, device=dev())
        g_o = torch.zeros((P, 4), dtype=torch.float32, device=dev())
        _lib.check(_lib.lib.sn_mlp_backward_chain(_lib.ptr(model.packed_bwd("bf16")), model.kernel_dtype(_lib.SN_DTYPE_BF16_STATE) | flag,
                                                  _lib.ptr(acts), _lib.ptr(out), _lib.ptr(g), P, rows, _lib.ptr(G), _lib.ptr(g_o),
                                                  _lib.stream_ptr()), "sn_mlp_backward_chain")
        torch.cuda.synchronize()
        res.append((G.view(torch.int16), g_o))
    assert torch.equal(res[0][1], res[1][1])
    for l in range(10):
        if not torch.equal(res[0][0][l], res[1][0][l]):
            bad = (res[0][0][l] != res[1][0][l]).nonzero()
            raise AssertionError(("G slot", l, "first mismatches", bad[:5].tolist(), "count", int(bad.shape[0]), "rows", rows, "P", P))
    assert float(res[0][0].float().abs().max()) > 0


def test_hand_scheduled_training_kernels_fuzz_and_determinism():
    """Random shapes (ragged last tiles, one to ~40 tiles per CU-less grid, S from 5 to 192) through both hand-scheduled kernels and
    their compiler-scheduled counterparts: same bits; and ten repetitions of the largest shape give the same bits every time
    (the statements' counted vmcnt / lgkmcnt waits and barrier hand-offs have no slack to hide a race behind)."""
    from sinnerf_amd import _lib
    model, p = make_model(5, True, dtype="bf16")
    r = np.random.RandomState(7)
    shapes = [(int(r.randint(1, 3000)), int(r.choice([5, 17, 37, 64, 96, 128, 192]))) for _ in range(8)] + [(4096, 192)]
    all_rays = O.lego_rays(400, 400, seed=3)

    def both(n_rays, S, seed):
        rays = all_rays[r.permutation(160000)[:n_rays]]
        z = np.sort(np.random.RandomState(seed).uniform(2, 6, (n_rays, S)).astype(np.float32), -1)
        rays_t, z_t = torch.from_numpy(rays).to(dev()), torch.from_numpy(z).to(dev())
        g = torch.from_numpy(np.random.RandomState(seed + 1).standard_normal((n_rays, S, 4)).astype(np.float32)).to(dev())
        res = []
        for flag in (0, _lib.SN_DTYPE_COMPILER_SCHEDULED):
            out, acts, emb = _train_forward(model, rays_t, z_t, flag)
            P, rows = n_rays * S, acts.shape[1]
            G = torch.zeros((10, rows, 256), dtype=torch.bfloat16, device=dev())
            g_o = torch.zeros((P, 4), dtype=torch.float32, device=dev())
            _lib.check(_lib.lib.sn_mlp_backward_chain(_lib.ptr(model.packed_bwd("bf16")), model.kernel_dtype(_lib.SN_DTYPE_BF16_STATE) | flag,
                                                      _lib.ptr(acts), _lib.ptr(out), _lib.ptr(g), P, rows, _lib.ptr(G), _lib.ptr(g_o),
                                                      _lib.stream_ptr()), "chain")
            torch.cuda.synchronize()
            res.append((out, acts.view(torch.int16), G.view(torch.int16), g_o))
        return res

    for i, (n_rays, S) in enumerate(shapes):
        new, old = both(n_rays, S, 100 + i)
        assert torch.equal(new[0], old[0]), (n_rays, S, "out")
        assert torch.equal(new[1], old[1]), (n_rays, S, "acts", int((new[1] != old[1]).sum()))
        assert torch.equal(new[2], old[2]), (n_rays, S, "G", int((new[2] != old[2]).sum()))
        assert torch.equal(new[3], old[3]), (n_rays, S, "g_out")
    first = None
    for rep in range(10):
        r = np.random.RandomState(7)                                         # same permutation every repetition
        for _ in range(8):
            r.randint(1, 3000); r.choice([5, 17, 37, 64, 96, 128, 192])
        new, _ = both(4096, 192, 999)
        sig = (new[1].long().sum().item(), new[2].long().sum().item(), new[1][3, 1234567 % new[1].shape[1]].long().sum().item())
        if first is None:
            first, ref = sig, (new[1].clone(), new[2].clone())
        assert sig == first and torch.equal(new[1], ref[0]) and torch.equal(new[2], ref[1]), rep


def test_unsupported_configurations_are_refused_loudly():
    """One configuration exists in HIP -- NeRF(8, 256, 63, 27, [4]) with Embedding(3, 10) / Embedding(3, 4), <= 1024 samples per ray
    (models/sinnerf.py:133-141, eval.py:134-137).  Everything else the reference's constructors accept (models/nerf.py:47-50, :8-22)
    raises NotImplementedError naming that configuration; nothing falls back to torch ops."""
    import sinnerf_amd
    d = dev()
    mc, _ = make_model(0, True)
    mf, _ = make_model(1, True)
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=0)[::2503][:8]).to(d)
    with pytest.raises(NotImplementedError, match="D=8, W=256"):
        sinnerf_amd.NeRF(D=4, W=128, skips=[2])
    for emb in ([sinnerf_amd.Embedding(3, 6), sinnerf_amd.Embedding(3, 4)],
                [sinnerf_amd.Embedding(3, 10), sinnerf_amd.Embedding(3, 2)],
                [sinnerf_amd.Embedding(3, 10, logscale=False), sinnerf_amd.Embedding(3, 4)]):
        with pytest.raises(NotImplementedError, match="Embedding"):
            sinnerf_amd.render_rays([mc, mf], emb, rays, 16, False, 0, 0, 8, 4096, True)
    with pytest.raises(NotImplementedError, match="samples per ray"):
        sinnerf_amd.render_rays([mc, mf], embeddings(), rays, 1100, False, 0, 0, 0, 32768, True)
    with torch.no_grad():                                  # ... and the boundary case still renders
        big = sinnerf_amd.render_rays([mc, mf], embeddings(), rays[:4], 1024, False, 0, 0, 0, 32768, True)
    assert big["opacity_coarse"].shape == (4, 1024) and torch.isfinite(big["rgb_coarse"]).all()
    # the embedding verdict is cached per object (no per-call host conversions), and follows the bands when they change
    e = embeddings()
    from sinnerf_amd import rendering
    assert rendering._fused_embeddings(e) and e[0]._sn_pow2_verdict[1] is True
    e[0].freq_bands = e[0].freq_bands * 1.5
    assert not rendering._fused_embeddings(e)


# ---- SN_DTYPE_EMB_BF16: the embedded inputs stored as the bf16 operands, in the kernel's K-slot order ---------------------------------
def _emb_xyz_pos(c):
    """column c of Embedding(3, 10) -> position in the stored row (csrc/sn_dw.hip emb_xyz_pos; sn_mlp_common.h xyz_col_slot)"""
    if c < 3:
        return (30, 31, 62)[c]
    k, h = (c - 3) % 30, (c - 3) // 30
    return 32 * h + 2 * (3 * (k // 6) + k % 3) + (k % 6) // 3


def _emb_dir_pos(c):
    if c < 3:
        return (12, 13, 28)[c]
    k, h = (c - 3) % 12, (c - 3) // 12
    return 16 * h + 2 * (3 * (k // 6) + k % 3) + (k % 6) // 3


def test_emb_positions_are_a_permutation():
    assert sorted(_emb_xyz_pos(c) for c in range(63)) == [q for q in range(64) if q != 63]
    assert sorted(_emb_dir_pos(c) for c in range(27)) == [q for q in range(32) if q not in (14, 15, 29, 30, 31)]


@pytest.mark.parametrize("n_rays,S", [(60, 37), (1024, 128)])
def test_bf16_emb_is_the_rounded_fp32_emb_and_gives_the_same_weight_gradients(n_rays, S):
    """sn_mlp_forward_train | SN_DTYPE_EMB_BF16 stores RNE-bf16(emb) at the K-slot positions (everything else it writes is unchanged),
    and sn_weight_grads | SN_DTYPE_EMB_BF16 returns the gradients of the fp32-emb form (same bits while the K-split is the same),
    accumulate or not."""
    import ctypes
    from sinnerf_amd import _lib
    model, p = make_model(3, True, dtype="bf16")
    rays = O.lego_rays(400, 400, seed=0)[:: max(1, 160000 // n_rays)][:n_rays]
    z = O.coarse_z_vals(rays, S, False, 1.0, np.random.RandomState(1).uniform(0, 1, (rays.shape[0], S)).astype(np.float32))
    rays_t, z_t = torch.from_numpy(rays).to(dev()), torch.from_numpy(z).to(dev())
    out, acts, emb = _train_forward(model, rays_t, z_t, 0)
    n, s = z_t.shape
    P, rows = n * s, acts.shape[1]
    out16 = torch.zeros_like(out)
    acts16 = torch.full_like(acts, float("nan"))
    emb16 = torch.full((rows, 128), float("nan"), dtype=torch.bfloat16, device=dev())
    code16 = model.kernel_dtype(_lib.SN_DTYPE_BF16_STATE) | _lib.SN_DTYPE_EMB_BF16
    _lib.check(_lib.lib.sn_mlp_forward_train(_lib.ptr(model.packed()), code16, _lib.ptr(rays_t), _lib.ptr(z_t), n, s, _lib.ptr(out16),
                                             _lib.ptr(acts16), _lib.ptr(emb16), rows, _lib.stream_ptr()), "sn_mlp_forward_train emb16")
    torch.cuda.synchronize()
    assert torch.equal(out16, out) and torch.equal(acts16.view(torch.int16), acts.view(torch.int16))
    xp = torch.tensor([_emb_xyz_pos(c) for c in range(63)], device=dev())
    dp = torch.tensor([64 + _emb_dir_pos(c) for c in range(27)], device=dev())
    assert torch.equal(emb16[:, xp].view(torch.int16), emb[:, :63].bfloat16().view(torch.int16))
    assert torch.equal(emb16[:, dp].view(torch.int16), emb[:, 64:91].bfloat16().view(torch.int16))
    assert bool(torch.isnan(emb16[:, 96:].float()).all())                     # [96, 128) is never written
    # the weight gradients from both forms of emb
    G = (torch.randn((10, rows, 256), device=dev()) * (torch.rand((10, rows, 256), device=dev()) > 0.5)).bfloat16()
    G[:, P:] = 0
    shapes = [tuple(t.shape) for t in model.raw_tensors()]
    res = []
    for e, code in ((emb, _lib.SN_DTYPE_BF16_STATE), (emb16, _lib.SN_DTYPE_BF16_STATE | _lib.SN_DTYPE_EMB_BF16)):
        nbytes = _lib.lib.sn_weight_grads_workspace_bytes(rows, code)
        assert nbytes > 0
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev())
        outs = [torch.full(sh, 0.25, dtype=torch.float32, device=dev()) for sh in shapes]
        arr = (ctypes.c_void_p * _lib.N_RAW_TENSORS)(*[o.data_ptr() for o in outs])
        for accumulate in (0, 1):
            _lib.check(_lib.lib.sn_weight_grads(_lib.ptr(acts), _lib.ptr(e), _lib.ptr(G), rows, code, _lib.ptr(ws), arr, accumulate, None), "wg")
        torch.cuda.synchronize()
        res.append(outs)
    # same bf16 operands, same chunk order inside a K-range; the K-SPLIT may differ (the two forms have their own cost entries), so
    # beyond the one-range-per-problem sizes the fp32 partial sums associate differently: 1e-6-class differences
    for i, (a, b) in enumerate(zip(*res)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        if P <= 4096:
            assert torch.equal(a, b), ("gradient", i, float((a - b).abs().max()))
        else:
            assert float((a - b).abs().max()) <= 2e-6 * float(a.abs().max()), ("gradient", i, float((a - b).abs().max()), float(a.abs().max()))
    # the flag belongs to the hand-scheduled bf16-state kernels only
    assert _lib.lib.sn_weight_grads_workspace_bytes(rows, _lib.SN_DTYPE_BF16 | _lib.SN_DTYPE_EMB_BF16) == -4
    rc = _lib.lib.sn_mlp_forward_train(_lib.ptr(model.packed()), code16 | _lib.SN_DTYPE_COMPILER_SCHEDULED, _lib.ptr(rays_t), _lib.ptr(z_t), n, s,
                                       _lib.ptr(out16), _lib.ptr(acts16), _lib.ptr(emb16), rows, _lib.stream_ptr())
    assert rc == -4


def test_training_render_gradients_do_not_depend_on_the_emb_form():
    """a bf16 training render + backward through the Python surface with the bf16 emb (default) and with the fp32 one: same loss bit for
    bit, same gradients up to the association of the K-split partial sums"""
    import sinnerf_amd
    from sinnerf_amd import autograd as A
    rays = torch.from_numpy(O.lego_rays(400, 400, seed=5)[::131][:1000]).to(dev())
    tgt = torch.rand((rays.shape[0], 3), device=dev())
    grads = []
    for emb_bf16 in (True, False):
        coarse, _ = make_model(1, True, dtype="bf16")
        fine, _ = make_model(2, True, dtype="bf16")
        old = A.EMB_BF16
        A.EMB_BF16 = emb_bf16
        try:
            torch.manual_seed(7)
            res = sinnerf_amd.render_rays([coarse, fine], embeddings(), rays, 64, False, 1.0, 1.0, 64, 32768, True)
            loss = ((res["rgb_coarse"] - tgt) ** 2).mean() + ((res["rgb_fine"] - tgt) ** 2).mean()
            loss.backward()
        finally:
            A.EMB_BF16 = old
        grads.append([loss.detach()] + [q.grad.clone() for m_ in (coarse, fine) for q in m_.parameters()])
    assert torch.equal(grads[0][0], grads[1][0])
    for i, (a, b) in enumerate(zip(*grads)):
        assert float((a - b).abs().max()) <= 2e-6 * float(a.abs().max()) + 1e-12, ("tensor", i, float((a - b).abs().max()), float(a.abs().max()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_pack_is_the_two_separate_packs_in_one_launch(dtype):
    """NeRF.packed() / packed_bwd() under autograd re-pack both blobs with ONE gather launch (concatenated tables, one allocation):
    the bytes are those of the two separate launches the no-grad path uses."""
    model, _ = make_model(4, True, dtype=dtype)
    for q in model.parameters():               # frozen parameters: the two blobs are packed by separate launches
        q.requires_grad_(False)
    fwd = model.packed().clone()
    bwd = model.packed_bwd(dtype).clone()
    assert not any(isinstance(k, tuple) and k[0] == "both" for k in model._packed)
    for q in model.parameters():
        q.requires_grad_(True)
    model.invalidate_packed()
    with torch.no_grad():                      # (autograd.Function.forward runs with grad mode off: must not matter)
        fwd2 = model.packed()                  # trainable parameters: the combined launch
    bwd2 = model.packed_bwd(dtype)
    torch.cuda.synchronize()
    assert fwd2.data_ptr() % 256 == 0 and bwd2.data_ptr() % 256 == 0
    assert bwd2.data_ptr() - fwd2.data_ptr() >= fwd2.numel()          # one allocation, the second blob behind the first
    assert torch.equal(fwd, fwd2) and torch.equal(bwd, bwd2)
    # an optimizer-style in-place update is noticed by both views
    with torch.no_grad():
        model.sigma.weight.mul_(1.5)
    fwd3, bwd3 = model.packed().clone(), model.packed_bwd(dtype).clone()      # (combined launch again)
    for q in model.parameters():
        q.requires_grad_(False)
    model.invalidate_packed()
    ref_f, ref_b = model.packed().clone(), model.packed_bwd(dtype).clone()
    torch.cuda.synchronize()
    assert not torch.equal(fwd, fwd3)
    assert torch.equal(fwd3, ref_f) and torch.equal(bwd3, ref_b)
