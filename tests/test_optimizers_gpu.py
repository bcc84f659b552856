"""GPU: sn_sgd_step / sn_radam_step / sn_ranger_step through the C ABI and through FlatSGD / FlatRAdam / FlatRanger, the state dicts both
ways, and the optimiser / schedule hooks of SinNeRFSystem.

Acceptance of the kernels: the parameters after EVERY step within 4 x e_ref of the fp64 oracle (tests/optim_oracle.py), e_ref = the
deviation of the reference's own fp32 run from that oracle, recorded per configuration in tests/golden/optim.npz -- kernel and reference
are fp32 evaluations of the same formulae in different rounding orders.  tests/test_optimizers_cpu.py shows that five plausible mistakes
miss this bar by more than ten times.  On the two-NeRF buffer the bar is that of the existing Adam test, 1e-7 + 1e-5 |p|."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests import optim_oracle as OO
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

SN_E_BADARG = -1
STATE_KEYS = {"sgd": ("momentum_buffer",), "radam": ("exp_avg", "exp_avg_sq"), "ranger": ("exp_avg", "exp_avg_sq", "slow_buffer")}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(f"{GOLDEN}/optim.npz"))


class AbiRun:
    """Device buffers of `total` floats; the entries are called on the n elements from `first` on, the rest hold sentinels"""

    def __init__(self, kind, p0, n, first=0, tail=8):
        from sinnerf_amd import _lib
        self.L, self.kind, self.n, self.first = _lib, kind, n, first
        total = first + n + tail
        host = np.full(total, 777.0, np.float32)
        host[first:first + n] = p0[:n]
        self.p = torch.from_numpy(host).to(dev())
        self.g = torch.full((total,), 555.0, device=dev())
        self.state = {k: torch.full((total,), -333.0, device=dev()) for k in STATE_KEYS[kind]}
        for k, t in self.state.items():
            t[first:first + n] = self.p[first:first + n] if k == "slow_buffer" else 0.0
        self.step_no = 0

    def ptr(self, t):
        return ctypes.c_void_p(t.data_ptr() + 4 * self.first)

    def step(self, grad, wd):
        L, n, s = self.L, self.n, self.state
        self.step_no += 1
        self.g[self.first:self.first + n] = torch.from_numpy(np.ascontiguousarray(grad[:n])).to(dev())
        if self.kind == "sgd":
            return L.lib.sn_sgd_step(self.ptr(self.p), self.ptr(self.g), self.ptr(s["momentum_buffer"]), n, OO.LR, OO.MOMENTUM, wd,
                                     L.stream_ptr())
        b1, b2 = OO.BETAS[self.kind]
        _, _, rect, coeff, decay = OO.step_scalars(self.kind, self.step_no, OO.LR, (b1, b2), wd)
        if self.kind == "radam":
            return L.lib.sn_radam_step(self.ptr(self.p), self.ptr(self.g), self.ptr(s["exp_avg"]), self.ptr(s["exp_avg_sq"]), n, b1, b2,
                                       OO.EPS, decay, coeff, int(rect), L.stream_ptr())
        return L.lib.sn_ranger_step(self.ptr(self.p), self.ptr(self.g), self.ptr(s["exp_avg"]), self.ptr(s["exp_avg_sq"]), n, b1, b2,
                                    OO.EPS, decay, coeff, int(rect), self.ptr(s["slow_buffer"]), OO.ALPHA, int(self.step_no % OO.K == 0),
                                    L.stream_ptr())

    def live(self, t):
        return t[self.first:self.first + self.n].cpu().numpy().astype(np.float64)

    def sentinels_untouched(self):
        lo, hi = self.first, self.first + self.n
        for t, val in [(self.p, 777.0), (self.g, 555.0)] + [(t, -333.0) for t in self.state.values()]:
            h = t.cpu().numpy()
            if not ((h[:lo] == val).all() and (h[hi:] == val).all()):
                return False
        return True


@pytest.mark.parametrize("kind", OO.KINDS)
def test_kernels_through_the_c_abi_follow_the_oracle_at_every_step(fx, kind):
    for wi, wd in enumerate(OO.WEIGHT_DECAYS):
        for gi in range(len(OO.GRAD_SCALES)):
            t = OO.tag(kind, wi, gi)
            grads = fx["grads_gs%d" % gi]
            want, want_state = OO.run_config(kind, fx["p0"], grads, wd)
            run = AbiRun(kind, fx["p0"], OO.N_ELEMS)
            bar = 4 * float(fx[t + "_e_ref"])
            for s in range(OO.N_STEPS):
                assert run.step(grads[s], wd) == 0
                d = np.abs(run.live(run.p) - want[s]).max()
                print("%s step %2d: |p - oracle| %.3g  (bar %.3g)" % (t, s + 1, d, bar))
                assert d <= bar, (t, s + 1, d, bar)
                for key in STATE_KEYS[kind]:
                    ds, sbar = np.abs(run.live(run.state[key]) - want_state[key][s]).max(), 4 * float(fx[t + "_e_" + key])
                    assert ds <= sbar, (t, s + 1, key, ds, sbar)
            assert run.sentinels_untouched(), t


@pytest.mark.parametrize("kind", OO.KINDS)
def test_kernel_edges_short_buffers_tails_and_bad_arguments(fx, kind):
    """n = 0 is a no-op; n = 1, 3, 5 (below one vector, and one vector + a tail) and an unaligned start give the prefix of the same
    trajectory with the sentinels around the live range untouched; null pointers and n < 0 are refused before anything is launched."""
    wi, gi = 1, 0
    t, wd, grads = OO.tag(kind, wi, gi), OO.WEIGHT_DECAYS[wi], fx["grads_gs0"]
    want, _ = OO.run_config(kind, fx["p0"], grads, wd)
    bar = 4 * float(fx[t + "_e_ref"])
    for n, first in ((0, 0), (1, 0), (3, 0), (5, 0), (5, 1), (1031, 3)):
        run = AbiRun(kind, fx["p0"], n, first=first)
        for s in range(OO.N_STEPS):
            assert run.step(grads[s], wd) == 0, (n, first, s)
        torch.cuda.synchronize()
        assert run.sentinels_untouched(), (kind, n, first)
        if n:
            d = np.abs(run.live(run.p) - want[-1][:n]).max()
            assert d <= bar, (kind, n, first, d, bar)
    # refusals: nothing below launches
    run = AbiRun(kind, fx["p0"], 5)
    L, s, null = run.L, run.state, None
    P, G, sp = run.ptr(run.p), run.ptr(run.g), L.stream_ptr()
    if kind == "sgd":
        B = run.ptr(s["momentum_buffer"])
        calls = [lambda: L.lib.sn_sgd_step(null, G, B, 5, OO.LR, 0.9, 0.0, sp), lambda: L.lib.sn_sgd_step(P, null, B, 5, OO.LR, 0.9, 0.0, sp),
                 lambda: L.lib.sn_sgd_step(P, G, null, 5, OO.LR, 0.9, 0.0, sp), lambda: L.lib.sn_sgd_step(P, G, B, -1, OO.LR, 0.9, 0.0, sp)]
    else:
        M, V = run.ptr(s["exp_avg"]), run.ptr(s["exp_avg_sq"])
        if kind == "radam":
            f = lambda p, g, m, v, n: L.lib.sn_radam_step(p, g, m, v, n, 0.9, 0.999, 1e-8, 0.0, 5e-4, 0, sp)
            calls = []
        else:
            S = run.ptr(s["slow_buffer"])
            f = lambda p, g, m, v, n: L.lib.sn_ranger_step(p, g, m, v, n, 0.95, 0.999, 1e-8, 0.0, 5e-4, 0, S, 0.5, 1, sp)
            calls = [lambda: L.lib.sn_ranger_step(P, G, M, V, 5, 0.95, 0.999, 1e-8, 0.0, 5e-4, 0, null, 0.5, 1, sp),
                     lambda: L.lib.sn_ranger_step(P, G, M, V, 5, 0.95, 0.999, 1e-8, 0.0, -1.0, 0, S, 0.5, 1, sp)]
        calls += [lambda: f(null, G, M, V, 5), lambda: f(P, null, M, V, 5), lambda: f(P, G, null, V, 5), lambda: f(P, G, M, null, 5),
                  lambda: f(P, G, M, V, -1)]
    for i, call in enumerate(calls):
        assert call() == SN_E_BADARG, (kind, i)
    torch.cuda.synchronize()
    assert np.array_equal(run.p.cpu().numpy()[:5], fx["p0"][:5]) and run.sentinels_untouched()


def test_sgd_without_momentum_and_radam_without_degeneration(fx):
    """momentum == 0 takes a NULL buffer (p -= lr (g + wd p)); a negative step_coeff moves the moments and nothing else"""
    from sinnerf_amd import _lib as L
    n, wd = 37, 1e-2
    p0, g = fx["p0"][:n], fx["grads_gs0"][0][:n]
    p = torch.from_numpy(p0.copy()).to(dev())
    gd = torch.from_numpy(g.copy()).to(dev())
    assert L.lib.sn_sgd_step(L.ptr(p), L.ptr(gd), None, n, OO.LR, 0.0, wd, L.stream_ptr()) == 0
    want, _, _ = OO.sgd_run(p0, g[None], OO.LR, 0.0, wd)
    assert np.abs(p.cpu().numpy() - want[0]).max() <= 3e-8                       # three roundings at |p| < 0.25 (ulp 1.5e-8)
    p = torch.from_numpy(p0.copy()).to(dev())
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    _, step_size, rect, coeff, decay = OO.step_scalars("radam", 1, OO.LR, OO.BETAS["radam"], wd, degenerated_to_sgd=False)
    assert step_size == -1 and coeff < 0 and not rect
    assert L.lib.sn_radam_step(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), n, 0.9, 0.999, OO.EPS, decay, coeff, 0, L.stream_ptr()) == 0
    assert np.array_equal(p.cpu().numpy(), p0)                                   # no update and no decay (utils/optimizers.py:99)
    _, st = OO.radam_run("radam", p0, g[None], OO.LR, OO.BETAS["radam"], OO.EPS, wd, degenerated_to_sgd=False)
    assert np.abs(m.cpu().numpy() - st["exp_avg"][0]).max() <= 1e-9 and np.abs(v.cpu().numpy() - st["exp_avg_sq"][0]).max() <= 1e-12
    assert m.abs().sum().item() > 0


# ---- the classes on the two-NeRF buffer ------------------------------------------------------------------------------------------------
def _two_nerfs(seed=0):
    from sinnerf_amd import NeRF
    torch.manual_seed(seed)
    return [NeRF(use_new_activation=True).to(dev()), NeRF(use_new_activation=True).to(dev())]


def _copy_of(models):
    from sinnerf_amd import NeRF
    out = [NeRF(use_new_activation=True).to(dev()) for _ in models]
    for x, y in zip(models, out):
        y.load_state_dict(x.state_dict())
    return out


def _make(kind, models, wd=1e-3, **kw):
    from sinnerf_amd.optim import FlatRAdam, FlatRanger, FlatSGD
    if kind == "sgd":
        return FlatSGD(models, lr=OO.LR, momentum=OO.MOMENTUM, weight_decay=wd, **kw)
    if kind == "radam":
        return FlatRAdam(models, lr=OO.LR, eps=OO.EPS, weight_decay=wd, **kw)
    return FlatRanger(models, lr=OO.LR, eps=OO.EPS, weight_decay=wd, **kw)


@pytest.fixture(scope="module")
def big_grads():
    """13 seeded gradients of scale 1e-2 for the 1 191 688 floats, made once and only read"""
    g = torch.Generator(device=dev()).manual_seed(1)
    return [torch.randn(1191688, device=dev(), generator=g) * 0.01 for _ in range(OO.N_STEPS)]


@pytest.mark.parametrize("kind", OO.KINDS)
def test_flat_classes_on_the_two_nerf_buffer(kind, big_grads):
    import sinnerf_amd
    wd = 1e-3
    a = _two_nerfs()
    opt = _make(kind, a, wd)
    assert opt.flat.numel() == 1191688 and isinstance(opt, torch.optim.Optimizer) and isinstance(opt, sinnerf_amd.optim.FlatOptimizer)
    p0 = opt.flat.cpu().numpy()
    if kind == "sgd":
        b = _copy_of(a)
        b_params = [p for m in b for p in m.parameters()]
        opt_b = torch.optim.SGD(b_params, lr=OO.LR, momentum=OO.MOMENTUM, weight_decay=wd)
    for g in big_grads:
        opt.zero_grad()
        opt.grads.flat.copy_(g)
        opt.step()
        if kind == "sgd":
            off = 0
            for p in b_params:
                p.grad = g[off:off + p.numel()].view_as(p).clone()
                off += p.numel()
            opt_b.step()
    assert opt.step_count == OO.N_STEPS
    grads = np.stack([g.cpu().numpy() for g in big_grads])
    if kind == "sgd":
        want = OO.sgd_run(p0, grads, OO.LR, OO.MOMENTUM, wd, history=False)[0][-1]
    else:
        want = OO.radam_run(kind, p0, grads, OO.LR, OO.BETAS[kind], OO.EPS, wd, history=False)[0][-1]
    got = opt.flat.cpu().numpy().astype(np.float64)
    excess = np.abs(got - want) - (1e-7 + 1e-5 * np.abs(want))
    assert excess.max() <= 0, (kind, excess.max(), int(excess.argmax()))
    assert np.abs(got - p0).max() > 1e-4                                         # it moved
    if kind == "sgd":
        for x, y in zip(a, b):
            for (k, va), (_, vb) in zip(x.state_dict().items(), y.state_dict().items()):
                assert torch.allclose(va, vb, rtol=1e-5, atol=1e-7), k
    # the models still render through the packed-weight cache after the in-place updates
    c = _copy_of(a)
    rays = torch.from_numpy(O.lego_rays(400, 400, 0)[::4000]).to(dev())
    emb = [sinnerf_amd.Embedding(3, 10), sinnerf_amd.Embedding(3, 4)]
    with torch.no_grad():
        ra = sinnerf_amd.render_rays(a, emb, rays, 64, False, 0, 0, 64, 32768, True)["rgb_fine"]
        rc = sinnerf_amd.render_rays(c, emb, rays, 64, False, 0, 0, 64, 32768, True)["rgb_fine"]
    assert torch.allclose(ra, rc, atol=1e-5)


# ---- state dicts -------------------------------------------------------------------------------------------------------------------------
class Tiny(torch.nn.Module):
    """the fixture's 1031 elements as two parameter tensors"""

    def __init__(self, flat):
        super().__init__()
        off, ps = 0, []
        for shape in OO.SHAPES:
            n = int(np.prod(shape))
            ps.append(torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(flat[off:off + n])).reshape(shape).clone()))
            off += n
        self.a, self.b = ps


def _split(flat):
    out, off = [], 0
    for shape in OO.SHAPES:
        n = int(np.prod(shape))
        out.append(torch.from_numpy(np.ascontiguousarray(flat[off:off + n])).reshape(shape).clone())
        off += n
    return out


def _drive(opt, grads):
    for g in grads:
        opt.zero_grad()
        opt.grads.flat.copy_(torch.from_numpy(np.ascontiguousarray(g)).to(dev()))
        opt.step()


@pytest.mark.parametrize("kind", OO.KINDS)
def test_state_dict_round_trip_is_bit_identical(fx, kind):
    grads = fx["grads_gs0"]
    m1 = Tiny(fx["p0"]).to(dev())
    o1 = _make(kind, [m1], 1e-2)
    assert o1.state_dict()["state"] == {}
    _drive(o1, grads[:OO.STATE_STEP])
    sd = o1.state_dict()
    assert sorted(sd["state"]) == [0, 1] and sorted(sd["state"][0]) == sorted(STATE_KEYS[kind] + (("step",) if kind != "sgd" else ()))
    assert "buffer" not in sd["param_groups"][0] and "radam_buffer" not in sd["param_groups"][0]
    if kind != "sgd":
        assert sd["state"][1]["step"] == OO.STATE_STEP
    for key in STATE_KEYS[kind]:
        assert [tuple(sd["state"][i][key].shape) for i in (0, 1)] == list(OO.SHAPES)
    m2 = Tiny(o1.flat.cpu().numpy()).to(dev())
    o2 = _make(kind, [m2], 0.0)                                                  # the group's hyper-parameters come with the state
    o2.load_state_dict(copy.deepcopy(sd))
    assert o2.param_groups[0]["weight_decay"] == 1e-2
    _drive(o1, grads[OO.STATE_STEP:])
    _drive(o2, grads[OO.STATE_STEP:])
    assert torch.equal(o1.flat, o2.flat) and (kind == "sgd" or o2.step_count == OO.N_STEPS)
    assert torch.equal(m2.a.data.reshape(-1), o2.flat[:1000])
    # state of a different parameter set is refused, and nothing is written
    before = {k: getattr(o2, k).clone() for k in STATE_KEYS[kind]}
    bad = copy.deepcopy(sd)
    for key in STATE_KEYS[kind]:
        bad["state"][0][key] = bad["state"][0][key].reshape(50, 20)
    with pytest.raises(ValueError, match="different or re-ordered parameter set"):
        o2.load_state_dict(bad)
    short = copy.deepcopy(sd)
    short["param_groups"][0]["params"] = [0]
    with pytest.raises(ValueError, match="has 1 parameters, this model has 2"):
        o2.load_state_dict(short)
    if kind != "sgd":
        skew = copy.deepcopy(sd)
        skew["state"][1]["step"] = 3
        with pytest.raises(ValueError, match="step counts differ"):
            o2.load_state_dict(skew)
    assert all(torch.equal(before[k], getattr(o2, k)) for k in before)


@pytest.mark.parametrize("kind", ("radam", "ranger"))
def test_recorded_reference_state_resumes_to_the_recorded_parameters(fx, kind):
    """the reference's own state after step 7, in the layout its state_dict() has (memoisation fields included), loaded over the recorded
    step-7 parameters: steps 8-13 land on the recorded step-13 parameters"""
    for wi, wd in enumerate(OO.WEIGHT_DECAYS):
        for gi in range(len(OO.GRAD_SCALES)):
            t = OO.tag(kind, wi, gi)
            traj, grads = fx[t + "_params"], fx["grads_gs%d" % gi]
            per = {key: _split(fx[t + "_state_" + key]) for key in STATE_KEYS[kind]}
            state = {i: dict({"step": OO.STATE_STEP}, **{key: per[key][i] for key in per}) for i in (0, 1)}
            group = dict(lr=OO.LR, betas=OO.BETAS[kind], eps=OO.EPS, weight_decay=wd, params=[0, 1])
            if kind == "radam":
                group["buffer"] = [[None, None, None] for _ in range(10)]
            else:
                group.update(alpha=OO.ALPHA, k=OO.K, step_counter=0, N_sma_threshhold=5)
            m = Tiny(traj[OO.STATE_STEP - 1]).to(dev())
            opt = _make(kind, [m], 0.5)
            opt.load_state_dict({"state": state, "param_groups": [group]})
            assert opt.step_count == OO.STATE_STEP and opt.param_groups[0]["weight_decay"] == wd and "buffer" not in opt.param_groups[0]
            _drive(opt, grads[OO.STATE_STEP:])
            d, bar = np.abs(opt.flat.cpu().numpy().astype(np.float64) - traj[-1]).max(), 4 * float(fx[t + "_e_ref"])
            assert d <= bar, (t, d, bar)


# ---- the system hooks --------------------------------------------------------------------------------------------------------------------
def _batch(n=256, seed=0):
    allr = O.lego_rays(400, 400, seed=0)
    g = torch.Generator().manual_seed(seed)
    return {"rays": torch.from_numpy(allr[seed::577][:n].copy()).to(dev()), "rgbs": torch.rand((n, 3), generator=g).to(dev())}


def test_configure_optimizers_builds_every_kind_and_schedule():
    from sinnerf_amd import optim
    from sinnerf_amd.system import SinNeRFSystem
    S = torch.optim.lr_scheduler
    sysm = SinNeRFSystem(N_importance=0).to(dev())
    opts, schs = sysm.configure_optimizers()
    assert type(opts[0]) is optim.FlatAdam and type(schs[0]) is S.MultiStepLR and len(opts) == 1
    assert opts[0].param_groups[0]["eps"] == 1e-8 and opts[0].all_reduce and sysm._flat is opts[0].grads
    kinds = {"sgd": optim.FlatSGD, "adam": optim.FlatAdam, "radam": optim.FlatRAdam, "ranger": optim.FlatRanger}
    scheds = {"steplr": S.MultiStepLR, "cosine": S.CosineAnnealingLR, "poly": S.LambdaLR}
    for oname, ocls in kinds.items():
        for sname, scls in scheds.items():
            sysm = SinNeRFSystem(N_importance=0, optimizer=oname, lr_scheduler=sname, weight_decay=1e-4, momentum=0.8, num_epochs=7).to(dev())
            opts, schs = sysm.configure_optimizers()
            g = opts[0].param_groups[0]
            assert type(opts[0]) is ocls and type(schs[0]) is scls and g["lr"] == 5e-4 and g["weight_decay"] == 1e-4, (oname, sname)
            assert opts[0] is sysm.optimizer and schs[0].optimizer is opts[0]
            if oname == "sgd":
                assert g["momentum"] == 0.8
            if oname == "ranger":
                assert (g["alpha"], g["k"], g["betas"], g["eps"], g["N_sma_threshhold"]) == (0.5, 6, (0.95, 0.999), 1e-8, 5)
            if sname == "cosine":
                assert schs[0].T_max == 7 and schs[0].eta_min == 1e-8
    sysm = SinNeRFSystem(N_importance=0, optimizer="sgd", warmup_epochs=2, warmup_multiplier=2.0).to(dev())
    _, schs = sysm.configure_optimizers()
    assert type(schs[0]) is optim.GradualWarmupScheduler and type(schs[0].after_scheduler) is S.MultiStepLR
    sysm = SinNeRFSystem(N_importance=0, optimizer="ranger", warmup_epochs=2, warmup_multiplier=2.0).to(dev())
    assert type(sysm.configure_optimizers()[1][0]) is S.MultiStepLR


def test_ranger_with_cosine_lowers_the_loss_and_follows_the_schedule():
    from sinnerf_amd.optim import FlatRanger
    from sinnerf_amd.system import SinNeRFSystem
    torch.manual_seed(0)
    sysm = SinNeRFSystem(N_importance=64, perturb=0.0, noise_std=0.0, optimizer="ranger", lr_scheduler="cosine", num_epochs=10).to(dev())
    opts, schs = sysm.configure_optimizers()
    assert type(opts[0]) is FlatRanger
    want = OO.lr_sequence("cosine", 5, 5e-4, 10, [20], 0.1, 0.9)
    batch, losses = _batch(), []
    for it in range(5):
        assert abs(sysm.optimizer.lr - want[it]) <= 1e-12 * want[it], (it, sysm.optimizer.lr, want[it])
        losses.append(float(sysm.train_step(batch)["loss"]))
        schs[0].step()
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert sysm.optimizer.step_count == 5 and sysm.optimizer.slow_buffer is not None


def test_graphed_train_step_with_flat_radam_equals_eager():
    from sinnerf_amd.optim import FlatRAdam
    from sinnerf_amd.system import SinNeRFSystem
    batch, finals = _batch(), {}
    for graph in (False, True):
        torch.manual_seed(0)
        sysm = SinNeRFSystem(N_importance=64, perturb=0.0, noise_std=0.0, optimizer="radam").to(dev())
        sysm.configure_optimizers()
        assert type(sysm.optimizer) is FlatRAdam
        losses = [float(sysm.train_step(batch, graph=graph)["loss"]) for _ in range(3)]
        finals[graph] = (sysm.optimizer.flat.clone(), losses)
        if graph:
            assert len(sysm._step_graphs) == 1
    assert finals[True][1] == finals[False][1], finals
    assert torch.equal(finals[True][0], finals[False][0])


def test_discriminator_gets_a_flat_radam_without_an_exchange():
    from sinnerf_amd.optim import FlatRAdam
    from sinnerf_amd.system import SinNeRFSystem
    ph, pw = 8, 10
    torch.manual_seed(2)
    D = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.LeakyReLU(0.2), torch.nn.Conv2d(4, 1, 3)).to(dev())
    sysm = SinNeRFSystem(N_importance=64, optimizer="radam", dis_weight=0.01, weight_decay=1e-4).to(dev())
    sysm.attach_discriminator(D, patch_hw=(ph, pw))
    opts, _ = sysm.configure_optimizers()
    assert len(opts) == 2 and type(opts[0]) is FlatRAdam and type(opts[1]) is FlatRAdam and opts[1] is sysm.opt_d
    assert abs(opts[1].param_groups[0]["lr"] - 0.2 * 5e-4) < 1e-12 and not opts[1].all_reduce and opts[0].all_reduce
    assert opts[1].flat.numel() == sum(p.numel() for p in D.parameters())
    allr = O.lego_rays(400, 400, seed=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    g = torch.Generator().manual_seed(0)
    u = lambda *sh: torch.rand(*sh, generator=g).to(dev())
    n = ph * pw
    batch = {"rays": t(allr[5::997][:128]), "rgbs": u(128, 3), "rays_full": t(allr[80000:80000 + n]), "rgbs_full": u(n, 3),
             "rays_side": t(allr[81000:81000 + n]), "rays_proj": t(allr[7::991][:128]), "real_patch": u(1, 3, ph, pw)}
    d0, w0 = opts[1].flat.clone(), opts[0].flat.clone()
    out_g, out_d = sysm.train_step_adversarial(batch)
    assert torch.isfinite(out_g["loss"]).item() and torch.isfinite(out_d["loss"]).item()
    assert opts[1].step_count == 1 and not torch.equal(d0, opts[1].flat) and not torch.equal(w0, opts[0].flat)
    assert all(p.requires_grad for p in D.parameters())
    # adam keeps today's stock optimiser for the discriminator, sgd the stock SGD
    for name, cls in (("adam", torch.optim.Adam), ("sgd", torch.optim.SGD)):
        s2 = SinNeRFSystem(N_importance=0, optimizer=name, dis_weight=0.01).to(dev())
        s2.attach_discriminator(copy.deepcopy(D), patch_hw=(ph, pw))
        assert type(s2.configure_optimizers()[0][1]) is cls


def test_host_built_sgd_is_upgraded_and_its_warmup_drives_the_flat_optimizer(fx):
    from sinnerf_amd.optim import FlatSGD, GradualWarmupScheduler
    from sinnerf_amd.system import SinNeRFSystem
    torch.manual_seed(0)
    hp = dict(lr=5e-4, num_epochs=10, decay_step=[4, 8], decay_gamma=0.1, warmup_epochs=3, warmup_multiplier=2.0)
    sysm = SinNeRFSystem(N_importance=0, perturb=0.0, noise_std=0.0, optimizer="sgd", lr_scheduler="steplr", momentum=0.8, weight_decay=1e-4, **hp)
    opts, schs = sysm.configure_optimizers()                                     # on the host
    assert type(opts[0]) is torch.optim.SGD and type(schs[0]) is GradualWarmupScheduler
    schs[0].step()                                                               # the schedule has already moved once
    sysm.to(dev())
    batch, ref = _batch(64), fx["lr_steplr_warm"]
    for epoch in range(1, 10):
        out = sysm.train_step(batch)
        opt, sch = sysm.optimizer, sysm._schedulers[0]
        if epoch == 1:
            assert type(opt) is FlatSGD and opt.param_groups[0]["momentum"] == 0.8 and opt.param_groups[0]["weight_decay"] == 1e-4
            assert sch.optimizer is opt and sch.after_scheduler.optimizer is opt and sysm._flat is opt.grads
        assert abs(opt.lr - ref[epoch]) <= 1e-12 * ref[epoch], (epoch, opt.lr, ref[epoch])
        assert torch.isfinite(out["loss"]).item()
        sch.step()
    assert sysm.optimizer.step_count == 9 and sysm.optimizer.momentum_buffer is not None
    # state a host optimiser has accumulated is refused, not dropped
    s2 = SinNeRFSystem(N_importance=0, optimizer="sgd")
    s2.configure_optimizers()
    for p in s2.optimizer.param_groups[0]["params"]:
        p.grad = torch.zeros_like(p)
    s2.optimizer.step()
    s2.to(dev())
    with pytest.raises(RuntimeError, match="already holds state"):
        s2.train_step(batch)
