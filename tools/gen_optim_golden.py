"""Record tests/golden/optim.npz: runs of the reference's own optimiser and warm-up classes that the optimiser tests compare against.

CPU only.  Loads the UNMODIFIED ``utils/optimizers.py`` and ``utils/warmup_scheduler.py`` of the reference by path (the package
``__init__`` pulls in cv2 and is not imported), drives ``RAdam``, ``Ranger`` and ``GradualWarmupScheduler`` from them and
``torch.optim.SGD`` / the torch schedulers, and writes arrays only:

* ``p0``, ``grads_gs{i}``: the inputs -- 1031 elements, 0.06 N(0, 1), 13 gradients per scale whose first 7 elements are exactly 0;
* per configuration ``<kind>_wd{i}_gs{j}`` (tests/optim_oracle.py ``configs``): ``_params`` (13, n) after every step, ``_state_<key>``
  the optimiser state after step 7, ``_e_ref`` the largest deviation of that fp32 run from the fp64 oracle over all steps and
  ``_e_<key>`` the same for each state buffer, ``_n_sma`` / ``_step_size`` the host scalars the reference memoised per step;
* ``lr_<schedule>`` / ``lr_<schedule>_warm``: the rate before each of 10 epochs, without and with warm-up.

usage: python tools/gen_optim_golden.py [reference_root]        (default /root/reference)
"""
import importlib.util
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import optim_oracle as OO      # noqa: E402

LR_HP = dict(lr=5e-4, num_epochs=10, decay_step=[4, 8], decay_gamma=0.1, poly_exp=0.9, warmup_epochs=3, warmup_multiplier=2.0)
LR_EPOCHS = 10


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(seed=20):
    rng = np.random.default_rng(seed)
    p0 = (0.06 * rng.standard_normal(OO.N_ELEMS)).astype(np.float32)
    unit = rng.standard_normal((OO.N_STEPS, OO.N_ELEMS))
    unit[:, :7] = 0.0
    return p0, [(unit * s).astype(np.float32) for s in OO.GRAD_SCALES]


def split(flat):
    out, off = [], 0
    for shape in OO.SHAPES:
        n = int(np.prod(shape))
        out.append(torch.from_numpy(np.ascontiguousarray(flat[off:off + n])).reshape(shape).clone())
        off += n
    return out


def flatten(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).copy()


def drive(ref, kind, p0, grads, wd):
    """-> params (steps, n) fp32, state per step {key: (steps, n)}, scalars (steps, 2) or None"""
    params = [torch.nn.Parameter(t) for t in split(p0)]
    if kind == "sgd":
        opt = torch.optim.SGD(params, lr=OO.LR, momentum=OO.MOMENTUM, weight_decay=wd)
        keys = ("momentum_buffer",)
    elif kind == "radam":
        opt = ref.RAdam(params, lr=OO.LR, eps=OO.EPS, weight_decay=wd)
        keys = ("exp_avg", "exp_avg_sq")
    else:
        opt = ref.Ranger(params, lr=OO.LR, eps=OO.EPS, weight_decay=wd)
        keys = ("exp_avg", "exp_avg_sq", "slow_buffer")
    traj, states, scalars = [], {k: [] for k in keys}, []
    for step in range(1, OO.N_STEPS + 1):
        for p, g in zip(params, split(grads[step - 1])):
            p.grad = g
        opt.step()
        traj.append(flatten(params))
        for k in keys:
            states[k].append(flatten([opt.state[p][k] for p in params]))
        if kind != "sgd":
            memo = (opt.param_groups[0]["buffer"] if kind == "radam" else opt.radam_buffer)[step % 10]
            assert memo[0] == step and all(int(opt.state[p]["step"]) == step for p in params)
            scalars.append((memo[1], memo[2]))
    return np.stack(traj), {k: np.stack(v) for k, v in states.items()}, (np.array(scalars, np.float64) if scalars else None)


def lr_run(warm_cls, schedule, warm):
    hp = SimpleNamespace(**LR_HP)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=hp.lr)
    S = torch.optim.lr_scheduler
    if schedule == "steplr":
        sch = S.MultiStepLR(opt, milestones=hp.decay_step, gamma=hp.decay_gamma)
    elif schedule == "cosine":
        sch = S.CosineAnnealingLR(opt, T_max=hp.num_epochs, eta_min=1e-8)
    else:
        sch = S.LambdaLR(opt, lambda epoch: (1 - epoch / hp.num_epochs) ** hp.poly_exp)
    if warm:
        sch = warm_cls(opt, multiplier=hp.warmup_multiplier, total_epoch=hp.warmup_epochs, after_scheduler=sch)
    seq = []
    for _ in range(LR_EPOCHS):
        seq.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return np.array(seq, np.float64)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    warnings.filterwarnings("ignore", category=UserWarning)        # the reference's deprecated add_(Number, Tensor) overloads
    ref = load_by_path("_reference_optimizers", os.path.join(root, "utils", "optimizers.py"))
    warm = load_by_path("_reference_warmup", os.path.join(root, "utils", "warmup_scheduler.py"))
    torch.set_num_threads(1)
    p0, grads = make_inputs()
    out = {"p0": p0}
    for gi, g in enumerate(grads):
        out["grads_gs%d" % gi] = g
    for kind, wi, gi in OO.configs():
        t = OO.tag(kind, wi, gi)
        wd = OO.WEIGHT_DECAYS[wi]
        traj, states, scalars = drive(ref, kind, p0, grads[gi], wd)
        o_traj, o_states = OO.run_config(kind, p0, grads[gi], wd)
        dev = np.abs(traj.astype(np.float64) - o_traj)
        assert (dev <= 1e-7 + 1e-5 * np.abs(o_traj)).all(), (t, dev.max())        # the bar of the existing Adam test, as a sanity condition
        out[t + "_params"] = traj
        out[t + "_e_ref"] = np.float64(dev.max())
        for k, v in states.items():
            out[t + "_state_" + k] = v[OO.STATE_STEP - 1]
            out[t + "_e_" + k] = np.float64(np.abs(v.astype(np.float64) - o_states[k]).max())
        if scalars is not None:
            out[t + "_n_sma"], out[t + "_step_size"] = scalars[:, 0], scalars[:, 1]
        print("%-18s e_ref %.3g  (%.1f %% of the sanity bar at its element)  state: %s" % (
            t, dev.max(), 100 * (dev / (1e-7 + 1e-5 * np.abs(o_traj))).max(),
            "  ".join("%s %.3g" % (k, out[t + "_e_" + k]) for k in states)))
    for schedule in ("steplr", "cosine", "poly"):
        out["lr_" + schedule] = lr_run(warm.GradualWarmupScheduler, schedule, False)
        out["lr_" + schedule + "_warm"] = lr_run(warm.GradualWarmupScheduler, schedule, True)
        print(schedule, out["lr_" + schedule], out["lr_" + schedule + "_warm"], sep="\n  ")
    path = os.path.join(REPO, "tests", "golden", "optim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
