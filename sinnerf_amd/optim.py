"""Flat-buffer optimisers -- SURVEY.md §8f rank 3 -- and the reference's optimiser / schedule builders.

Reference: ``utils/__init__.py:11-57`` ``get_optimizer`` / ``get_scheduler`` build ``--optimizer {sgd, adam, radam, ranger}`` with
``--lr_scheduler {steplr, cosine, poly}`` (``opt.py:45-71``), stepped by Lightning after ``backward``.  The two NeRFs have 48 small
parameter tensors; a stock optimiser launches several kernels per tensor (the reference's own ``RAdam`` / ``Ranger``,
``utils/optimizers.py``, are Python loops over them).  Here parameters AND gradients of the models live in two flat fp32 buffers
(``param.data`` / ``param.grad`` are views), so one step is: one RCCL all-reduce of the flat gradient buffer
(``parallel.FlatGradBuffer``) + ONE launch (``sn_adam_step`` / ``sn_sgd_step`` / ``sn_radam_step`` / ``sn_ranger_step``).  State-dict
compatible with the reference modules (the views keep their names and shapes).

Every class is a ``torch.optim.Optimizer``: torch LR schedulers drive ``param_groups[0]['lr']``, ``state_dict()`` /
``load_state_dict()`` carry the per-parameter state of the class each one mirrors for checkpoint-resume, ``zero_grad()`` keeps the
gradient views attached.  The per-step scalars of RAdam / Ranger (``N_sma``, the rectified step size, whether the lookahead fires) come
from the HOST step counter in Python doubles, as the reference computes them: nothing is read back from the device.
"""
import math
import warnings

import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, MultiStepLR

from . import _lib
from .parallel import FlatGradBuffer

try:
    from torch.optim.lr_scheduler import LRScheduler as _SchedulerBase
except ImportError:                                    # torch < 2.0
    from torch.optim.lr_scheduler import _LRScheduler as _SchedulerBase


class FlatOptimizer(torch.optim.Optimizer):
    """What the flat optimisers share: the flat parameter buffer, the ``FlatGradBuffer``, the exchange before the step, one param group.

    A subclass names its per-element state in ``STATE`` (state-dict key -> attribute holding a flat tensor, ``None`` until allocated),
    says with ``HAS_STEP`` whether the mirrored class keeps a per-parameter ``step``, and launches its kernel in ``_launch(group)``.
    ``all_reduce=False``: ``step()`` skips the exchange (a module whose gradients the caller averages itself)."""
    STATE = ()
    HAS_STEP = True
    # the reference's memoisation fields (utils/optimizers.py:26-27, 329): a cache of host scalars, neither written nor read
    _IGNORED_GROUP_KEYS = ("params", "buffer", "radam_buffer")

    def __init__(self, modules, defaults, all_reduce=True):
        self._modules = list(modules)
        self.grads = FlatGradBuffer(self._modules)
        params = self.grads.params
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("sinnerf_amd.optim.%s: parameters must live on a ROCm device (no CPU fallback)" % type(self).__name__)
        super().__init__(params, defaults)
        self.all_reduce = bool(all_reduce)
        self.flat = torch.empty(self.grads.numel, dtype=torch.float32, device=dev)
        off = 0
        for p in params:                              # move every parameter into the flat buffer (keeps values)
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view_as(p)
            off += n
        self.step_count = 0
        self._invalidate()

    # (the hyper-parameters live in param_groups[0], where schedulers and utils.get_learning_rate -- utils/__init__.py:55-57 --
    #  read and write them)
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def _invalidate(self):
        # parameters were (re)written behind autograd's back: their MFMA-packed copies are stale (blobs are kept and refilled)
        for m in self._modules:
            if hasattr(m, "invalidate_packed"):
                m.invalidate_packed()

    def zero_grad(self, set_to_none=False):
        """One memset of the flat gradient buffer; the ``param.grad`` views stay attached (``set_to_none`` is ignored on
        purpose: detaching the views is what would make the flat buffer go stale)."""
        self.grads.zero()

    @torch.no_grad()
    def step(self, closure=None):
        """all-reduce (mean over ranks, no-op at world size 1) + one fused launch.  Gradients that are no longer views
        of the flat buffer (someone called ``module.zero_grad(set_to_none=True)``) are copied back first
        (``FlatGradBuffer.sync_views``) -- the step never runs on a stale buffer."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.all_reduce:
            self.grads.all_reduce_mean()
        else:
            self.grads.sync_views()
        self.step_count += 1
        with torch.cuda.device(self.flat.device):
            self._launch(self.param_groups[0])
        self._invalidate()
        return loss

    def _launch(self, g):
        raise NotImplementedError

    def _state_tensor(self, attr):
        t = getattr(self, attr)
        if t is None:
            t = torch.zeros_like(self.flat)
            setattr(self, attr, t)
        return t

    def _has_state(self):
        return self.step_count > 0

    # ---- checkpoint / resume ---------------------------------------------------------------------------------------
    def state_dict(self):
        """The layout of the mirrored class ({'state': {i: {...}}, 'param_groups': [...]}, per parameter in parameter order), so a
        checkpoint written here resumes under the reference's optimiser (``utils/__init__.py:16-27``) and the other way round."""
        g = self.param_groups[0]
        params = self.grads.params
        state, off = {}, 0
        if self._has_state():
            for i, p in enumerate(params):
                n = p.numel()
                e = {"step": self._step_entry()} if self.HAS_STEP else {}
                for key, attr in self.STATE:
                    e[key] = getattr(self, attr)[off:off + n].view_as(p).clone()
                state[i] = e
                off += n
        group = {k: v for k, v in g.items() if k != "params"}
        group["params"] = list(range(len(params)))
        return {"state": state, "param_groups": [group]}

    def _step_entry(self):
        return self.step_count

    def load_state_dict(self, state):
        """Accepts the layout ``state_dict()`` writes (the reference's / Lightning's ``optimizer_states`` entry).  Shapes are checked
        per parameter: state of a different or re-ordered parameter set is refused."""
        name = type(self).__name__
        params = self.grads.params
        st = state["state"]
        groups = state["param_groups"]
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(params):
            raise ValueError("%s.load_state_dict: optimizer state has %d parameters, this model has %d" % (name, len(ids), len(params)))
        if len(st) not in (0, len(params)):
            raise ValueError("%s.load_state_dict: partial per-parameter state (%d of %d)" % (name, len(st), len(params)))
        entries = [(st[i] if i in st else st[str(i)]) for i in ids] if st else []
        for i, e, p in zip(ids, entries, params):      # every check before the first write
            for key, _ in self.STATE:
                if key not in e:
                    raise ValueError("%s.load_state_dict: state %s has no %r -- the state of another optimiser" % (name, i, key))
                if e[key] is not None and tuple(e[key].shape) != tuple(p.shape):
                    raise ValueError("%s.load_state_dict: state %s has shape %s, parameter has %s -- a different or "
                                     "re-ordered parameter set" % (name, i, tuple(e[key].shape), tuple(p.shape)))
        steps = set(int(e["step"]) for e in entries) if self.HAS_STEP else set([1] if entries else [])
        if len(steps) > 1:
            raise ValueError("%s.load_state_dict: per-parameter step counts differ (%s): one fused step has one count" % (name, sorted(steps)))
        off = 0
        for e, p in zip(entries, params):
            n = p.numel()
            for key, attr in self.STATE:
                if e[key] is not None:                 # (torch.optim.SGD without momentum keeps `momentum_buffer: None`)
                    self._state_tensor(attr)[off:off + n].copy_(e[key].to(self.flat.device).reshape(-1))
            off += n
        if not st:
            self._reset_state()
        self.step_count = steps.pop() if steps else 0
        self._load_group(groups[0])

    def _reset_state(self):
        for _, attr in self.STATE:
            t = getattr(self, attr)
            if t is not None:
                t.zero_()

    def _load_group(self, src):
        for k, v in src.items():
            if k not in self._IGNORED_GROUP_KEYS:
                self.param_groups[0][k] = v


class FlatAdam(FlatOptimizer):
    """``torch.optim.Adam`` (``utils/__init__.py:19-21``): the all-reduce + one ``sn_adam_step`` launch."""
    STATE = (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"))

    def __init__(self, modules, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, all_reduce=True):
        super().__init__(modules, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), all_reduce=all_reduce)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)

    def _launch(self, g):
        _lib.check(_lib.lib.sn_adam_step(_lib.ptr(self.flat), _lib.ptr(self.grads.flat), _lib.ptr(self.exp_avg),
                                         _lib.ptr(self.exp_avg_sq), self.flat.numel(), float(g["lr"]),
                                         float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                         float(g["weight_decay"]), self.step_count, _lib.stream_ptr()), "sn_adam_step")

    def _step_entry(self):
        return torch.tensor(float(self.step_count))

    def load_state_dict(self, state):
        """Accepts the ``torch.optim.Adam`` layout (the reference's / Lightning's ``optimizer_states`` entry, or
        ``state_dict()``) and the round-2 private layout (top-level ``step`` / ``exp_avg`` / ``exp_avg_sq``).  Shapes are
        checked per parameter: state of a different or re-ordered parameter set is refused."""
        if "state" in state:
            return super().load_state_dict(state)
        if state["exp_avg"].numel() != self.flat.numel():
            raise ValueError("FlatAdam.load_state_dict: optimizer state belongs to a different parameter set")
        self.step_count = int(state["step"])
        self.exp_avg.copy_(state["exp_avg"].to(self.flat.device).reshape(-1))
        self.exp_avg_sq.copy_(state["exp_avg_sq"].to(self.flat.device).reshape(-1))
        self._load_group(state["param_groups"][0])


class FlatSGD(FlatOptimizer):
    """``torch.optim.SGD`` with dampening 0 and no Nesterov (``utils/__init__.py:16-18``): the all-reduce + one ``sn_sgd_step`` launch.
    The momentum buffer starts at zero, which reproduces torch's first step (``buf = g``); state: ``momentum_buffer``."""
    STATE = (("momentum_buffer", "momentum_buffer"),)
    HAS_STEP = False

    def __init__(self, modules, lr=5e-4, momentum=0, weight_decay=0, all_reduce=True):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("FlatSGD: lr, momentum and weight_decay must not be negative")
        # the keys of torch.optim.SGD's group that change the update are kept (and refused in _launch when set): a state dict
        # written by a torch SGD with dampening or Nesterov momentum must not resume here silently
        super().__init__(modules, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False),
                         all_reduce=all_reduce)
        self.momentum_buffer = None                   # allocated by the first step with momentum (torch: no state without it)

    def _has_state(self):
        return self.step_count > 0 and self.momentum_buffer is not None

    def _launch(self, g):
        if g.get("dampening", 0) != 0 or g.get("nesterov", False) or g.get("maximize", False):
            raise NotImplementedError("FlatSGD: dampening, Nesterov momentum and maximize are not mirrored")
        buf = self._state_tensor("momentum_buffer") if g["momentum"] != 0 else None
        _lib.check(_lib.lib.sn_sgd_step(_lib.ptr(self.flat), _lib.ptr(self.grads.flat), _lib.ptr(buf), self.flat.numel(),
                                        float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), _lib.stream_ptr()),
                   "sn_sgd_step")

    def _reset_state(self):
        self.momentum_buffer = None


def radam_step_scalars(step, lr, betas, weight_decay, threshold=5, strict=False, degenerated_to_sgd=True):
    """The host scalars of one RAdam / Ranger step in Python doubles, as ``utils/optimizers.py:74-88`` / ``:404-414`` compute them:
    -> (N_sma, step_size, rectified, step_size * lr, weight_decay * lr).  RAdam rectifies when ``N_sma >= threshold``, Ranger
    (``strict``) when ``N_sma > threshold``; below it ``step_size`` is the bias correction alone, or -1 ("no update") when RAdam was
    built with ``degenerated_to_sgd=False``."""
    beta1, beta2 = betas
    beta2_t = beta2 ** step
    n_sma_max = 2 / (1 - beta2) - 1
    n_sma = n_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    rectified = n_sma > threshold if strict else n_sma >= threshold
    if rectified:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) \
            / (1 - beta1 ** step)
    elif degenerated_to_sgd:
        step_size = 1.0 / (1 - beta1 ** step)
    else:
        step_size = -1
    return n_sma, step_size, bool(rectified), step_size * lr, weight_decay * lr


class FlatRAdam(FlatOptimizer):
    """The reference's ``RAdam`` (``utils/optimizers.py:7-106``): the all-reduce + one ``sn_radam_step`` launch.  Weight decay is
    decoupled (applied to the parameter, scaled by lr); state: ``step``, ``exp_avg``, ``exp_avg_sq``."""
    STATE = (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"))

    def __init__(self, modules, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True, all_reduce=True):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        for i in (0, 1):
            if not 0.0 <= betas[i] < 1.0:
                raise ValueError("Invalid beta parameter at index {}: {}".format(i, betas[i]))
        self.degenerated_to_sgd = degenerated_to_sgd
        super().__init__(modules, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), all_reduce=all_reduce)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)

    def _launch(self, g):
        _, _, rectified, coeff, decay = radam_step_scalars(self.step_count, g["lr"], g["betas"], g["weight_decay"],
                                                           degenerated_to_sgd=self.degenerated_to_sgd)
        _lib.check(_lib.lib.sn_radam_step(_lib.ptr(self.flat), _lib.ptr(self.grads.flat), _lib.ptr(self.exp_avg),
                                          _lib.ptr(self.exp_avg_sq), self.flat.numel(), float(g["betas"][0]), float(g["betas"][1]),
                                          float(g["eps"]), float(decay), float(coeff), int(rectified), _lib.stream_ptr()),
                   "sn_radam_step")


class FlatRanger(FlatOptimizer):
    """The reference's ``Ranger`` (``utils/optimizers.py:292-439``: RAdam + lookahead every ``k`` steps): the all-reduce + one
    ``sn_ranger_step`` launch.  The slow weights are a copy of the parameters taken at the first step (``:380-381``); state: ``step``,
    ``exp_avg``, ``exp_avg_sq``, ``slow_buffer``."""
    STATE = (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"), ("slow_buffer", "slow_buffer"))

    def __init__(self, modules, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-8, weight_decay=0,
                 all_reduce=True):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        super().__init__(modules, dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=tuple(betas), N_sma_threshhold=N_sma_threshhold,
                                       eps=eps, weight_decay=weight_decay), all_reduce=all_reduce)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.slow_buffer = None

    def _launch(self, g):
        if self.slow_buffer is None:
            self.slow_buffer = self.flat.clone()
        _, _, rectified, coeff, decay = radam_step_scalars(self.step_count, g["lr"], g["betas"], g["weight_decay"],
                                                           threshold=g["N_sma_threshhold"], strict=True)
        _lib.check(_lib.lib.sn_ranger_step(_lib.ptr(self.flat), _lib.ptr(self.grads.flat), _lib.ptr(self.exp_avg),
                                           _lib.ptr(self.exp_avg_sq), self.flat.numel(), float(g["betas"][0]), float(g["betas"][1]),
                                           float(g["eps"]), float(decay), float(coeff), int(rectified), _lib.ptr(self.slow_buffer),
                                           float(g["alpha"]), int(self.step_count % g["k"] == 0), _lib.stream_ptr()),
                   "sn_ranger_step")

    def _reset_state(self):
        self.exp_avg.zero_(); self.exp_avg_sq.zero_()
        self.slow_buffer = None


# ---- utils/__init__.py:11-52 ------------------------------------------------------------------------------------------------------
class GradualWarmupScheduler(_SchedulerBase):
    """Linear warm-up from the base rate to ``multiplier`` x it over ``total_epoch`` epochs, then ``after_scheduler``
    (the learning-rate sequence of the reference's ``utils/warmup_scheduler.py``, its two hand-over quirks included):

    * epochs 0 .. total_epoch: ``base * ((multiplier - 1) * epoch / total_epoch + 1)``;
    * the first epoch past the warm-up hands over: the wrapped schedule's ``base_lrs`` become ``multiplier`` x this one's, and the
      epoch's rates are whatever the wrapped schedule computes in the state it is in -- it took only its constructor's step, so it
      stands at ITS epoch 0, one warm-up epoch is spent at the target rate, and a schedule that works recursively from the optimiser's
      current rate (cosine) carries on from the warm-up's last rate;
    * from then on ``step()`` steps the wrapped schedule and this object's own epoch counter stands still.

    Without a wrapped schedule the rate stays at ``multiplier`` x base.  Wrapping ``ReduceLROnPlateau`` is not supported."""

    def __init__(self, optimizer, multiplier, total_epoch, after_scheduler=None):
        if multiplier < 1.0:
            raise ValueError("multiplier should be greater thant or equal to 1.")
        if isinstance(after_scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            raise NotImplementedError("GradualWarmupScheduler: ReduceLROnPlateau as the wrapped schedule is not supported")
        self.multiplier = multiplier
        self.total_epoch = total_epoch
        self.after_scheduler = after_scheduler
        self.finished = False
        super().__init__(optimizer)

    def _hand_over(self):
        self.after_scheduler.base_lrs = [b * self.multiplier for b in self.base_lrs]
        self.finished = True

    def get_lr(self):
        if self.last_epoch <= self.total_epoch:
            return [b * ((self.multiplier - 1.) * self.last_epoch / self.total_epoch + 1.) for b in self.base_lrs]
        if self.after_scheduler is None:
            return [b * self.multiplier for b in self.base_lrs]
        if not self.finished:
            self._hand_over()
        with warnings.catch_warnings():                # the wrapped schedule's get_lr outside its own step(): intended here
            warnings.simplefilter("ignore", UserWarning)
            return self.after_scheduler.get_lr()

    def step(self, epoch=None):
        if self.finished and self.after_scheduler is not None:
            if epoch is None:
                self.after_scheduler.step()
            else:
                self.after_scheduler.step(epoch - self.total_epoch)
            self._last_lr = [g["lr"] for g in self.optimizer.param_groups]
            return None
        return super().step() if epoch is None else super().step(epoch)

    def state_dict(self):
        """This object's counters, with the wrapped schedule's own ``state_dict`` in place of the object"""
        sd = {k: v for k, v in self.__dict__.items() if k not in ("optimizer", "after_scheduler")}
        sd["after_scheduler"] = None if self.after_scheduler is None else self.after_scheduler.state_dict()
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        after = state_dict.pop("after_scheduler", None)
        self.__dict__.update(state_dict)
        if after is not None and self.after_scheduler is not None:
            self.after_scheduler.load_state_dict(after)


def _on_device(modules):
    p = next((p for m in modules for p in m.parameters()), None)
    if p is None:
        raise ValueError("no trainable parameters")
    return p.is_cuda


def get_optimizer(hparams, models, rate=1, flat=True, all_reduce=True):
    """``utils/__init__.py:11-31``: the optimiser ``hparams.optimizer`` names over the parameters of ``models``, at ``lr * rate``,
    ``eps=1e-8``.  ``flat=True`` (the NeRFs): the flat-buffer class of each kind.  ``flat=False`` (a side module that stays on stock
    PyTorch, or a module still on the host): ``torch.optim.Adam`` / ``SGD`` as the reference builds them; ``radam`` / ``ranger`` have
    one form only, the flat class on the device -- on the host they raise ``RuntimeError``."""
    eps = 1e-8
    models = list(models)
    name = hparams.optimizer
    if name not in ("sgd", "adam", "radam", "ranger"):
        raise ValueError("optimizer not recognized!")
    lr, wd = hparams.lr * rate, hparams.weight_decay
    if not flat and name in ("sgd", "adam"):
        parameters = [p for m in models for p in m.parameters()]
        if name == "sgd":
            return torch.optim.SGD(parameters, lr=lr, momentum=hparams.momentum, weight_decay=wd)
        return torch.optim.Adam(parameters, lr=lr, eps=eps, weight_decay=wd)
    if not _on_device(models):
        raise RuntimeError("optimizer=%r runs on the device only (one fused launch over a flat buffer; there is no host form): "
                           "move the module with .to(device) before configure_optimizers()" % (name,))
    if name == "sgd":
        return FlatSGD(models, lr=lr, momentum=hparams.momentum, weight_decay=wd, all_reduce=all_reduce)
    if name == "adam":
        return FlatAdam(models, lr=lr, eps=eps, weight_decay=wd, all_reduce=all_reduce)
    if name == "radam":
        return FlatRAdam(models, lr=lr, eps=eps, weight_decay=wd, all_reduce=all_reduce)
    return FlatRanger(models, lr=lr, eps=eps, weight_decay=wd, all_reduce=all_reduce)


def get_scheduler(hparams, optimizer):
    """``utils/__init__.py:34-52``: ``steplr`` / ``cosine`` / ``poly``, wrapped in the warm-up when ``warmup_epochs > 0`` -- not for
    ``radam`` / ``ranger``, whose rectification is their warm-up."""
    eps = 1e-8
    if hparams.lr_scheduler == "steplr":
        scheduler = MultiStepLR(optimizer, milestones=hparams.decay_step, gamma=hparams.decay_gamma)
    elif hparams.lr_scheduler == "cosine":
        scheduler = CosineAnnealingLR(optimizer, T_max=hparams.num_epochs, eta_min=eps)
    elif hparams.lr_scheduler == "poly":
        num_epochs, poly_exp = hparams.num_epochs, hparams.poly_exp
        scheduler = LambdaLR(optimizer, lambda epoch: (1 - epoch / num_epochs) ** poly_exp)
    else:
        raise ValueError("scheduler not recognized!")
    if hparams.warmup_epochs > 0 and hparams.optimizer not in ["radam", "ranger"]:
        scheduler = GradualWarmupScheduler(optimizer, multiplier=hparams.warmup_multiplier, total_epoch=hparams.warmup_epochs,
                                           after_scheduler=scheduler)
    return scheduler
