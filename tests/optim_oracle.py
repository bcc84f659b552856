"""NumPy fp64 restatement of the flat optimiser steps (include/sinnerf_hip.h: sn_sgd_step, sn_radam_step, sn_ranger_step), of the host
scalars that drive them and of the learning-rate sequences of the three schedules with and without warm-up.  Shared by
tests/test_optimizers_cpu.py (which holds it to the recorded runs of the reference's own classes, tests/golden/optim.npz) and the GPU
tests.  `mutant` switches on one deliberate mistake at a time: the CPU test shows that the acceptance bar of the GPU tests rejects each.
"""
import math

import numpy as np

MUTANTS = ("decay_in_gradient", "eps_under_sqrt", "rectify_early", "sync_off_by_one", "no_copy_back")

# the fixture's configurations: kind x weight decay x gradient scale, at lr 5e-4, eps 1e-8
KINDS = ("sgd", "radam", "ranger")
WEIGHT_DECAYS = (0.0, 1e-2)
GRAD_SCALES = (1e-2, 1e-5)
LR, EPS, MOMENTUM, N_STEPS, N_ELEMS, STATE_STEP = 5e-4, 1e-8, 0.9, 13, 1031, 7
BETAS = {"radam": (0.9, 0.999), "ranger": (0.95, 0.999)}
ALPHA, K = 0.5, 6
SHAPES = ((20, 50), (31,))            # the two parameter tensors the 1031 elements are split into


def configs():
    return [(kind, wi, gi) for kind in KINDS for wi in range(len(WEIGHT_DECAYS)) for gi in range(len(GRAD_SCALES))]


def tag(kind, wi, gi):
    return "%s_wd%d_gs%d" % (kind, wi, gi)


def step_scalars(kind, step, lr, betas, weight_decay, threshold=5, degenerated_to_sgd=True, mutant=None):
    """(N_sma, step_size, rectified, step_size * lr, weight_decay * lr) of step `step` (1-based), in Python doubles.  radam rectifies
    from N_sma >= threshold, ranger from N_sma > threshold; step_size -1 = no parameter update (radam, degenerated_to_sgd=False)."""
    beta1, beta2 = betas

    def n_sma_of(t):
        beta2_t = beta2 ** t
        return 2 / (1 - beta2) - 1 - 2 * t * beta2_t / (1 - beta2_t), beta2_t
    n_sma_max = 2 / (1 - beta2) - 1
    n_sma, beta2_t = n_sma_of(step)
    decide = n_sma_of(step + 1)[0] if mutant == "rectify_early" else n_sma
    rectified = decide > threshold if kind == "ranger" else decide >= threshold
    if rectified:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) \
            / (1 - beta1 ** step)
    elif degenerated_to_sgd or kind == "ranger":
        step_size = 1.0 / (1 - beta1 ** step)
    else:
        step_size = -1
    return n_sma, step_size, bool(rectified), step_size * lr, weight_decay * lr


def sgd_run(p0, grads, lr, momentum, weight_decay, buf=None, history=True):
    """torch.optim.SGD (dampening 0, no Nesterov) -> (parameters after every step, final momentum buffer, buffers after every step);
    history=False keeps the last step only (large buffers)"""
    p = np.asarray(p0, np.float64).copy()
    buf = np.zeros_like(p) if buf is None else np.asarray(buf, np.float64).copy()
    out, bufs = [], []
    for g in np.asarray(grads, np.float64):
        if weight_decay != 0:
            g = g + weight_decay * p
        if momentum != 0:
            buf = momentum * buf + g
            g = buf
        p = p - lr * g
        if not history:
            out, bufs = [], []
        out.append(p.copy()); bufs.append(buf.copy())
    return np.stack(out), buf, np.stack(bufs)


def radam_run(kind, p0, grads, lr, betas, eps, weight_decay, alpha=ALPHA, k=K, threshold=5, degenerated_to_sgd=True, state=None,
              first_step=1, mutant=None, history=True):
    """The reference's RAdam (kind 'radam') / Ranger ('ranger') from step `first_step` on, `state` = dict(exp_avg, exp_avg_sq[, slow_buffer])
    when resuming -> (parameters after every step, dict of the state after every step); history=False keeps the last step only."""
    p = np.asarray(p0, np.float64).copy()
    m = np.zeros_like(p) if state is None else np.asarray(state["exp_avg"], np.float64).copy()
    v = np.zeros_like(p) if state is None else np.asarray(state["exp_avg_sq"], np.float64).copy()
    slow = None
    if kind == "ranger":
        slow = p.copy() if state is None else np.asarray(state["slow_buffer"], np.float64).copy()
    beta1, beta2 = betas
    out, hist = [], {"exp_avg": [], "exp_avg_sq": [], "slow_buffer": []}
    for i, g in enumerate(np.asarray(grads, np.float64)):
        step = first_step + i
        if mutant == "decay_in_gradient" and weight_decay != 0:
            g = g + weight_decay * p
        v = v * beta2 + (1 - beta2) * g * g
        m = m * beta1 + (1 - beta1) * g
        _, step_size, rectified, coeff, decay = step_scalars(kind, step, lr, betas, weight_decay, threshold, degenerated_to_sgd, mutant)
        if step_size > 0 or kind == "ranger":
            if decay != 0 and mutant != "decay_in_gradient":
                p = p - decay * p
            if rectified:
                denom = np.sqrt(v + eps) if mutant == "eps_under_sqrt" else np.sqrt(v) + eps
                p = p - coeff * m / denom
            else:
                p = p - coeff * m
        if kind == "ranger" and step % k == (1 if mutant == "sync_off_by_one" else 0):
            slow = slow + alpha * (p - slow)
            if mutant != "no_copy_back":
                p = slow.copy()
        if not history:
            out, hist = [], {"exp_avg": [], "exp_avg_sq": [], "slow_buffer": []}
        out.append(p.copy())
        hist["exp_avg"].append(m.copy()); hist["exp_avg_sq"].append(v.copy())
        if slow is not None:
            hist["slow_buffer"].append(slow.copy())
    return np.stack(out), {key: np.stack(val) for key, val in hist.items() if val}


def run_config(kind, p0, grads, weight_decay, mutant=None, **kw):
    """One fixture configuration -> (parameters after every step, state after every step as a dict of (steps, n) arrays)"""
    if kind == "sgd":
        ps, _, bufs = sgd_run(p0, grads, LR, MOMENTUM, weight_decay)
        return ps, {"momentum_buffer": bufs}
    return radam_run(kind, p0, grads, LR, BETAS[kind], EPS, weight_decay, mutant=mutant, **kw)


# ---- learning rates: the rate in force BEFORE each epoch (optimizer.step(); scheduler.step() once per epoch) ---------------------------
def _advance(kind, t, cur, base, num_epochs, decay_step, decay_gamma, poly_exp, eta_min=1e-8):
    """the wrapped schedule's rate at ITS epoch t, from the optimiser's current rate `cur` and the schedule's base rate"""
    if kind == "steplr":            # MultiStepLR: the current rate, times gamma at a milestone
        return cur * decay_gamma ** list(decay_step).count(t)
    if kind == "cosine":            # CosineAnnealingLR works recursively from the current rate
        return (1 + math.cos(math.pi * t / num_epochs)) / (1 + math.cos(math.pi * (t - 1) / num_epochs)) * (cur - eta_min) + eta_min
    if kind == "poly":              # LambdaLR: closed form from the base rate
        return base * (1 - t / num_epochs) ** poly_exp
    raise ValueError("scheduler not recognized!")


def lr_sequence(kind, n, lr, num_epochs, decay_step, decay_gamma, poly_exp, warmup_epochs=0, warmup_multiplier=1.0):
    """The rates before epochs 0 .. n-1.  With warm-up: epochs 0 .. warmup_epochs ramp linearly from lr to warmup_multiplier x lr; the
    epoch after that the wrapped schedule -- its base rate rescaled by the multiplier -- computes the rate of ITS epoch 0 from the
    optimiser's current rate (for the recursive cosine that is one step of the recursion from t = -1, i.e. slightly ABOVE the target),
    and then advances one epoch per epoch."""
    args = (num_epochs, decay_step, decay_gamma, poly_exp)
    seq, cur = [], lr
    for e in range(n):
        if warmup_epochs > 0:
            if e <= warmup_epochs:
                cur = lr * ((warmup_multiplier - 1.0) * e / warmup_epochs + 1.0)
            else:
                cur = _advance(kind, e - warmup_epochs - 1, cur, lr * warmup_multiplier, *args)
        elif e > 0:
            cur = _advance(kind, e, cur, lr, *args)
        seq.append(cur)
    return np.array(seq, np.float64)
