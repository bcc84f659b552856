"""The optimiser and schedule surface without a GPU: the fp64 oracle (tests/optim_oracle.py) against the recorded runs of the reference's own
RAdam / Ranger / GradualWarmupScheduler and torch's SGD (tests/golden/optim.npz, written by tools/gen_optim_golden.py), the sensitivity
of the GPU tests' acceptance bar to five deliberate mistakes, the three new prototypes, and the builders' host-side behaviour."""
import os
import re
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import optim_oracle as OO
from tests.helpers import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sn_sgd_step", "sn_radam_step", "sn_ranger_step")
CTYPE = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double, "float*": ctypes.c_void_p,
         "const float*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const void*": ctypes.c_void_p}
LR_HP = dict(lr=5e-4, num_epochs=10, decay_step=[4, 8], decay_gamma=0.1, poly_exp=0.9)
WARM = dict(warmup_epochs=3, warmup_multiplier=2.0)
SCHEDULES = ("steplr", "cosine", "poly")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(f"{GOLDEN}/optim.npz"))


def test_fixture_holds_what_the_tests_need(fx):
    assert fx["p0"].shape == (OO.N_ELEMS,) and fx["p0"].dtype == np.float32
    for gi, scale in enumerate(OO.GRAD_SCALES):
        g = fx["grads_gs%d" % gi]
        assert g.shape == (OO.N_STEPS, OO.N_ELEMS) and (g[:, :7] == 0).all() and (g[:, 7:] != 0).all()
        assert 0.5 * scale < g[:, 7:].std() < 2 * scale
    for kind, wi, gi in OO.configs():
        t = OO.tag(kind, wi, gi)
        assert fx[t + "_params"].shape == (OO.N_STEPS, OO.N_ELEMS)
        # the condition the generator asserts: the reference's own fp32 error sits well inside the bar of the existing Adam test
        assert 0 < float(fx[t + "_e_ref"]) < 1e-7 + 1e-5 * np.abs(fx[t + "_params"]).max()
        assert float(fx[t + "_e_ref"]) < 2e-7


def test_oracle_reproduces_the_recorded_trajectories_and_host_scalars(fx):
    for kind, wi, gi in OO.configs():
        t = OO.tag(kind, wi, gi)
        ps, states = OO.run_config(kind, fx["p0"], fx["grads_gs%d" % gi], OO.WEIGHT_DECAYS[wi])
        assert np.abs(ps - fx[t + "_params"]).max() <= float(fx[t + "_e_ref"]), t
        for key, hist in states.items():
            assert np.abs(hist[OO.STATE_STEP - 1] - fx[t + "_state_" + key]).max() <= float(fx[t + "_e_" + key]), (t, key)
        if kind == "sgd":
            continue
        rect = []
        for step in range(1, OO.N_STEPS + 1):
            n_sma, step_size, rectified, coeff, decay = OO.step_scalars(kind, step, OO.LR, OO.BETAS[kind], OO.WEIGHT_DECAYS[wi])
            assert n_sma == fx[t + "_n_sma"][step - 1] and step_size == fx[t + "_step_size"][step - 1], (t, step)     # exactly
            assert coeff == step_size * OO.LR and decay == OO.WEIGHT_DECAYS[wi] * OO.LR
            rect.append(rectified)
        assert rect == [False] * 5 + [True] * 8, t                      # steps 1-5 degenerate, 6 the first rectified one -- both rules


def test_package_scalars_equal_the_oracles():
    """sinnerf_amd.optim.radam_step_scalars (what the flat classes hand the kernels) is the same double arithmetic"""
    from sinnerf_amd.optim import radam_step_scalars
    for kind in ("radam", "ranger"):
        for step in (1, 5, 6, 13, 1000):
            for d2s in (True, False):
                got = radam_step_scalars(step, 5e-4, OO.BETAS[kind], 1e-2, strict=kind == "ranger", degenerated_to_sgd=d2s or kind == "ranger")
                assert got == OO.step_scalars(kind, step, 5e-4, OO.BETAS[kind], 1e-2, degenerated_to_sgd=d2s), (kind, step, d2s)
    assert radam_step_scalars(3, 5e-4, (0.9, 0.999), 0.0, degenerated_to_sgd=False)[1:4] == (-1, False, -5e-4)


def test_each_mutant_misses_the_bar_by_more_than_ten_times(fx):
    """the 4 x e_ref bar of the GPU tests can fail: each deliberate mistake leaves the recorded trajectory by > 10 x the bar somewhere"""
    for mutant in OO.MUTANTS:
        worst = 0.0
        for kind, wi, gi in OO.configs():
            if kind == "sgd":
                continue
            t = OO.tag(kind, wi, gi)
            ps, _ = OO.run_config(kind, fx["p0"], fx["grads_gs%d" % gi], OO.WEIGHT_DECAYS[wi], mutant=mutant)
            worst = max(worst, np.abs(ps - fx[t + "_params"]).max() / (4 * float(fx[t + "_e_ref"])))
        assert worst > 10, (mutant, worst)


def _lr_hparams(schedule, warm, optimizer="sgd"):
    return SimpleNamespace(lr_scheduler=schedule, optimizer=optimizer, **LR_HP, **(WARM if warm else dict(warmup_epochs=0, warmup_multiplier=1.0)))


def test_oracle_learning_rates_match_the_recorded_sequences(fx):
    for schedule in SCHEDULES:
        for warm in (False, True):
            hp = _lr_hparams(schedule, warm)
            seq = OO.lr_sequence(schedule, 10, hp.lr, hp.num_epochs, hp.decay_step, hp.decay_gamma, hp.poly_exp, hp.warmup_epochs,
                                 hp.warmup_multiplier)
            ref = fx["lr_" + schedule + ("_warm" if warm else "")]
            assert np.all(np.abs(seq - ref) <= 1e-12 * np.abs(ref)), (schedule, warm, seq, ref)


def test_get_scheduler_reproduces_the_recorded_sequences(fx):
    from sinnerf_amd.optim import GradualWarmupScheduler, get_scheduler
    for schedule in SCHEDULES:
        for warm in (False, True):
            hp = _lr_hparams(schedule, warm)
            opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=hp.lr)
            sch = get_scheduler(hp, opt)
            assert isinstance(sch, GradualWarmupScheduler) == warm
            seq = []
            for _ in range(10):
                seq.append(opt.param_groups[0]["lr"])
                opt.step()
                sch.step()
            ref = fx["lr_" + schedule + ("_warm" if warm else "")]
            assert np.all(np.abs(np.array(seq) - ref) <= 1e-12 * np.abs(ref)), (schedule, warm, seq, ref)
            if warm:                                                            # the quirk: the wrapped schedule's base rate is rescaled
                assert sch.finished and sch.after_scheduler.base_lrs == [hp.lr * hp.warmup_multiplier]
                assert sch.get_last_lr() == [opt.param_groups[0]["lr"]]
    # no warm-up wrapper for the rectified optimisers, whatever warmup_epochs says (utils/__init__.py:48)
    for name in ("radam", "ranger"):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=5e-4)
        assert isinstance(get_scheduler(_lr_hparams("cosine", True, optimizer=name), opt), torch.optim.lr_scheduler.CosineAnnealingLR)


def test_warmup_scheduler_refuses_a_multiplier_below_one_and_resumes():
    from sinnerf_amd.optim import GradualWarmupScheduler, get_scheduler
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=5e-4)
    with pytest.raises(ValueError, match="multiplier should be greater thant or equal to 1."):
        GradualWarmupScheduler(opt, multiplier=0.5, total_epoch=3)
    # without a wrapped schedule the rate stays at the target
    sch = GradualWarmupScheduler(opt, multiplier=2.0, total_epoch=2)
    seq = []
    for _ in range(5):
        seq.append(opt.param_groups[0]["lr"]); opt.step(); sch.step()
    assert np.allclose(seq, [5e-4, 7.5e-4, 1e-3, 1e-3, 1e-3], rtol=1e-12, atol=0)
    # state_dict round trip in the middle of the wrapped schedule: the copy carries on with the same rates
    hp = _lr_hparams("cosine", True)
    a_opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=hp.lr)
    a = get_scheduler(hp, a_opt)
    for _ in range(6):
        a_opt.step(); a.step()
    b_opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=hp.lr)
    b = get_scheduler(hp, b_opt)
    b.load_state_dict(a.state_dict())
    b_opt.param_groups[0]["lr"] = a_opt.param_groups[0]["lr"]                   # (the optimiser's own state_dict carries the rate)
    for _ in range(3):
        a_opt.step(); a.step(); b_opt.step(); b.step()
        assert a_opt.param_groups[0]["lr"] == b_opt.param_groups[0]["lr"]


def test_builders_raise_the_references_errors():
    from sinnerf_amd.optim import get_optimizer, get_scheduler
    net = torch.nn.Linear(3, 2)
    hp = SimpleNamespace(optimizer="lamb", lr=5e-4, momentum=0.9, weight_decay=0.0)
    with pytest.raises(ValueError, match="optimizer not recognized!"):
        get_optimizer(hp, [net])
    opt = torch.optim.SGD(net.parameters(), lr=5e-4)
    with pytest.raises(ValueError, match="scheduler not recognized!"):
        get_scheduler(_lr_hparams("exponential", False), opt)
    # host-side modules: the reference's own Adam / SGD; the device-only kinds say so
    hp.optimizer = "sgd"
    o = get_optimizer(hp, [net], rate=0.2, flat=False)
    assert type(o) is torch.optim.SGD and o.param_groups[0]["lr"] == 5e-4 * 0.2 and o.param_groups[0]["momentum"] == 0.9
    hp.optimizer = "adam"
    o = get_optimizer(hp, [net], flat=False)
    assert type(o) is torch.optim.Adam and o.param_groups[0]["eps"] == 1e-8
    for name in ("radam", "ranger"):
        hp.optimizer = name
        with pytest.raises(RuntimeError, match="to\\(device\\)"):
            get_optimizer(hp, [net], flat=False)


def test_system_on_the_host():
    from sinnerf_amd.optim import GradualWarmupScheduler
    from sinnerf_amd.system import DEFAULT_HPARAMS, SinNeRFSystem
    want = dict(optimizer="adam", momentum=0.9, lr_scheduler="steplr", num_epochs=80, poly_exp=0.9, warmup_multiplier=1.0, warmup_epochs=0)
    assert {k: DEFAULT_HPARAMS[k] for k in want} == want
    opts, schs = SinNeRFSystem().configure_optimizers()
    assert type(opts[0]) is torch.optim.Adam and type(schs[0]) is torch.optim.lr_scheduler.MultiStepLR
    opts, schs = SinNeRFSystem(optimizer="sgd", lr_scheduler="poly", warmup_epochs=2, warmup_multiplier=1.5).configure_optimizers()
    assert type(opts[0]) is torch.optim.SGD and opts[0].param_groups[0]["momentum"] == 0.9
    assert isinstance(schs[0], GradualWarmupScheduler) and isinstance(schs[0].after_scheduler, torch.optim.lr_scheduler.LambdaLR)
    for name in ("radam", "ranger"):
        with pytest.raises(RuntimeError, match="to\\(device\\)"):
            SinNeRFSystem(optimizer=name).configure_optimizers()
    with pytest.raises(ValueError, match="optimizer not recognized!"):
        SinNeRFSystem(optimizer="lamb").configure_optimizers()
    with pytest.raises(ValueError, match="scheduler not recognized!"):
        SinNeRFSystem(lr_scheduler="exponential").configure_optimizers()


def test_rebuild_scheduler_repoints_a_wrapped_schedule():
    """system.rebuild_scheduler on a warm-up wrapper: wrapper and wrapped schedule drive the new optimiser, at the epoch reached"""
    from sinnerf_amd.optim import get_scheduler
    from sinnerf_amd.system import rebuild_scheduler
    for schedule in SCHEDULES:
        hp = _lr_hparams(schedule, True)
        ref_opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=hp.lr)
        ref_sch = get_scheduler(hp, ref_opt)
        old = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=hp.lr)
        sch = get_scheduler(hp, old)
        for _ in range(2):
            ref_opt.step(); ref_sch.step(); old.step(); sch.step()
        g = old.param_groups[0]
        new = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=g["lr"])
        new.param_groups[0]["initial_lr"] = g["initial_lr"]
        sch = rebuild_scheduler(sch, new)
        assert sch.optimizer is new and sch.after_scheduler.optimizer is new
        for _ in range(7):
            ref_opt.step(); ref_sch.step(); new.step(); sch.step()
            assert abs(new.param_groups[0]["lr"] - ref_opt.param_groups[0]["lr"]) <= 1e-12 * ref_opt.param_groups[0]["lr"], schedule


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


def test_optimizer_symbols_exported_with_the_headers_prototypes():
    from sinnerf_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "sinnerf_hip.h")).read()
    assert L.lib.sn_abi_version() == L.ABI_VERSION == 5                                      # additive within ABI 5
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert getattr(L.lib, name) is not None
        assert header_prototype(hdr, name) == (L.SIGNATURES[name][0], list(L.SIGNATURES[name][1])), name
    assert header_prototype(hdr, "sn_adam_step") == (L.SIGNATURES["sn_adam_step"][0], list(L.SIGNATURES["sn_adam_step"][1]))
    # the scalars cross the boundary as doubles (rounded to fp32 once, in the kernel's launcher)
    assert L.SIGNATURES["sn_radam_step"][1].count(ctypes.c_double) == 5 and L.SIGNATURES["sn_ranger_step"][1].count(ctypes.c_double) == 6
    assert L.SIGNATURES["sn_sgd_step"][1].count(ctypes.c_double) == 3
