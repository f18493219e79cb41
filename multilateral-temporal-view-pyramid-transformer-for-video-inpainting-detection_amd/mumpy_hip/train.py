"""Training tail of config 5: parameter groups, fused AdamW / SGD / RMSprop on flat buffers, the polynomial LR
schedule and the bucketed gradient all-reduce.  The model backward lives in mumpy_hip/autograd.py (full_model_train and the graphed
step built on it); the pieces here are also exercised on their own: loss + gradient wrt the logits, optimizer update, schedule,
collective.

Reference behaviour reproduced:
  * three optimizers: encoder parameters whose name contains "cva" / the other encoder parameters / the decoder
    (train.py:198-213), each built by `get_optimizer` (utils/utils.py:252-261): `torch.optim.SGD(lr, weight_decay,
    momentum=0.9)`, `torch.optim.AdamW(lr, weight_decay)` or `torch.optim.RMSprop(lr, weight_decay)`, torch defaults
    otherwise; the decoder's from -optim, the encoder's and cva's from -optim_cnn (train.py:209-213);
  * `PolynomialLR` (utils/optimizer/scheduler.py:6-43) with power 0.9, min_lr 1e-5, step_size 1, no warm-up
    (train.py:226-262), stepped once per optimizer step;
  * gradient accumulation: loss / accumulation_steps (train.py:115), update every accumulation_steps iterations (eager,
    or replayed: GraphedTrainStep(accumulation_steps=k));
  * nn.DataParallel's gradient (grad of the mean loss over the global batch) == the mean over ranks of per-rank gradients
    for equal shards: one sum all-reduce of the flat gradient buffer in buckets + the 1/world factor folded into the update;
  * timm's `clip_grad=` knob of the optimizer recipes (train.py:223-273, None there): `GradClip`, torch's clip_grad_norm_ measured on
    the flat gradient buffers and folded into the update's gradient scale on the device (eager, or GraphedTrainStep(clip_grad=...)).
"""
from typing import Dict, Iterable, List, Optional

import os

import torch
import torch.distributed as dist

from . import ops
from .state import bump_weights_epoch


def split_param_groups(encoder: torch.nn.Module, decoder: torch.nn.Module) -> Dict[str, List[torch.nn.Parameter]]:
    """train.py:198-213: {"cva": encoder params with "cva" in the name, "enc": the other encoder params, "dec": decoder}."""
    groups = {"cva": [], "enc": [], "dec": [p for p in decoder.parameters() if p.requires_grad]}
    for name, p in encoder.named_parameters():
        if p.requires_grad:
            groups["cva" if "cva" in name else "enc"].append(p)
    return groups


def polynomial_lr(base_lr: float, current_lr: float, it: int, iter_max: int, power: float = 0.9, min_lr: float = 1e-5,
                  iter_warmup: int = 0, step_size: int = 1) -> float:
    """Learning rate after the `it`-th scheduler step (scheduler.py:24-41, `last_epoch` = it).  Faithful to its guards:
    the rate is left unchanged at it == 0, when it is not a multiple of step_size, and past iter_max."""
    iter_max, iter_warmup = int(iter_max), int(iter_warmup)
    if it == 0 or it % step_size != 0 or it > iter_max:
        return current_lr
    if it < iter_warmup:
        coef = it / iter_warmup * (1 - iter_warmup / iter_max) ** power
    else:
        coef = (1 - it / iter_max) ** power
    return (base_lr - min_lr) * coef + min_lr


class _FlatOptimizer:
    """One parameter group held as flat fp32 buffers: the parameters are re-pointed at views of `self.param`, their `.grad` at
    views of `self.grad`, so a step is ONE kernel over the group and the gradient all-reduce runs over one contiguous buffer.
    Subclasses add their state buffers and the update (`_launch`, `_hyper`, `step_dev`) and torch's state_dict layout."""
    KIND = ""          # the torch.optim class whose semantics and state_dict layout the subclass follows
    HYPER = 8          # floats of step constants staged in device memory for hipGraph replay

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float):
        name = type(self).__name__
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError(f"{name}: empty parameter group")
        dev = self.params[0].device      # buffers can be built anywhere; step() needs the GPU (the HIP kernel has no CPU twin)
        sizes = [(p.numel() + 3) // 4 * 4 for p in self.params]          # 16-B aligned slots
        self.offsets = [0]
        for s in sizes:
            self.offsets.append(self.offsets[-1] + s)
        self.param = self._zeros()
        self.grad = self._zeros()
        for p, o in zip(self.params, self.offsets):
            view = self._slot(self.param, p, o)
            view.copy_(p.data)
            p.data = view
            p.grad = self._slot(self.grad, p, o)
            p._mumpy_flat_grad = p.grad           # marker: the backward kernels may accumulate into this view (autograd._grad_slot)
        self.base_lr = self.lr = lr
        self.steps = 0            # optimizer steps taken (with an UpdateGuard: attempted -- the nominal count)
        self.sched_it = 0         # scheduler steps taken (PolynomialLR.last_epoch)
        self._guard = None        # the UpdateGuard attached last: step_dev then runs behind its gate
        self._skipped_host = 0    # steps - applied steps as read from a checkpoint (the guard's device counter takes over from it)

    def _zeros(self):
        return torch.zeros(self.offsets[-1], device=self.params[0].device, dtype=torch.float32)

    @staticmethod
    def _slot(buf, p, o):
        """The view of flat buffer `buf` that has p's logical shape.  Spatial nn.Conv2d weights (Cout,Cin,kh,kw) are stored in
        channels_last order: the (Cout,kh,kw,Cin) image the implicit-GEMM kernels read is then a VIEW of the parameter (no permuted
        copy per step) and the weight-gradient kernel accumulates straight into the matching view of the gradient.  Logical shapes,
        state_dict keys / shapes / dtypes are unchanged."""
        if p.dim() == 4 and p.shape[1] > 1 and p.shape[2] * p.shape[3] > 1:
            co, ci, kh, kw = p.shape
            return buf[o:o + p.numel()].view(co, kh, kw, ci).permute(0, 3, 1, 2)
        return buf[o:o + p.numel()].view(p.shape)

    def zero_grad(self):
        self.grad.zero_()

    # ---- checkpointing: torch.optim's own state_dict layout, so a file written here reads like the reference's
    # enc_opt_{e}.pt / dec_opt_{e}.pt (utils/utils.py:264-276) and vice versa; the counters torch keeps elsewhere
    # (scheduler position, base rate) ride in an extra "mumpy" entry that torch's loader ignores
    def _state_slot(self, buf, i):
        return self._slot(buf, self.params[i], self.offsets[i]).detach().contiguous().clone()

    def _sd(self, state: dict, group: dict) -> dict:
        group["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [group], "mumpy": {"steps": self.steps, "sched_it": self.sched_it, "base_lr": self.base_lr}}

    def _load_group(self, sd: dict) -> dict:
        name = type(self).__name__
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError(f"{name}.load_state_dict: expected one group of {len(self.params)} parameters")
        g = groups[0]
        kind = "AdamW" if "betas" in g else "RMSprop" if "alpha" in g else "SGD" if "nesterov" in g else "an unknown optimizer"
        if kind != self.KIND:
            raise ValueError(f"{name}.load_state_dict: the state dict is from {kind}, not from {self.KIND}")
        return g

    def _load_counters(self, sd: dict, g: dict, steps: int) -> None:
        extra = sd.get("mumpy", {})
        self.steps = int(extra.get("steps", steps))          # (one step count per group: every parameter steps together here)
        self.sched_it = int(extra.get("sched_it", self.steps))
        self.base_lr = float(extra.get("base_lr", g.get("initial_lr", self.lr)))

    def _seed_applied(self, applied: int) -> None:
        """After load_state_dict: `applied` updates were applied of the `self.steps` attempted; an attached guard's device counter
        is re-seeded with it."""
        self._skipped_host = max(0, self.steps - int(applied))
        if self._guard is not None:
            self._guard.seed(self)

    def applied_steps(self) -> int:
        """Updates actually applied: `steps` minus the ones an UpdateGuard skipped.  With a guard attached this reads its device
        counter (a device-to-host copy: it synchronises, which is fine where a checkpoint is written)."""
        if self._guard is not None:
            return self._guard.applied_steps(self)
        return self.steps - self._skipped_host

    def _load_slots(self, sd: dict, key: str, buf) -> None:
        """Copy state[i][key] into buf's slots; a parameter without that state (torch omits parameters that never received a
        gradient, and SGD keeps no state before its first step) gets zeros."""
        name = type(self).__name__
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is None or key not in st:
                buf[o:o + p.numel()].zero_()
                continue
            if tuple(st[key].shape) != tuple(p.shape):
                raise ValueError(f"{name}.load_state_dict: parameter {i} has shape {tuple(p.shape)}, state {tuple(st[key].shape)}")
            self._slot(buf, p, o).copy_(st[key])

    def all_reduce_grads(self, bucket_bytes: int = 64 << 20):
        """Sum all-reduce of the flat gradient in buckets (RCCL ring over xGMI: per-link bound, so a few tens of MB per
        call keeps the ring busy without delaying the first bucket); returns the factor the update must apply (1/world)."""
        if not (dist.is_available() and dist.is_initialized()) or \
                (dist.get_world_size() == 1 and os.environ.get("MUMPY_FORCE_DIST", "0") != "1"):    # (forced: one-rank RCCL rehearsal)
            return 1.0
        per = max(1, bucket_bytes // 4)
        host = self.grad.is_cuda and dist.get_backend() == "gloo"        # CPU rehearsal backend: stage each bucket on the host
        for o in range(0, self.grad.numel(), per):
            bucket = self.grad[o:o + per]
            if host:
                h = bucket.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM)
                bucket.copy_(h)
            else:
                dist.all_reduce(bucket, op=dist.ReduceOp.SUM)
        return 1.0 / dist.get_world_size()

    def step(self, grad_scale: float = 1.0):
        self.steps += 1
        self._launch(grad_scale)
        bump_weights_epoch()              # weight-derived caches (models.modules.layers.Derived) must be rebuilt

    # ---- hipGraph replay: the launch is frozen at capture, so the step-dependent constants live in device memory ----
    def enable_device_hyper(self):
        self.hyper_dev = torch.zeros(self.HYPER, device=self.param.device, dtype=torch.float32)

    def stage_hyper(self, grad_scale: float = 1.0, advance: bool = True):
        """Host side of a (captured) step: advance the step count and copy this step's constants to the device buffer.
        advance=False stages the constants of the NEXT step without counting it (used while capturing: nothing executes)."""
        if advance:
            self.steps += 1
        step = self.steps if advance else self.steps + 1
        self._hyper_host = self._hyper(step, grad_scale)
        self.hyper_dev.copy_(self._hyper_host, non_blocking=True)
        if self._guard is not None:
            self._guard.stage(self, step)

    def scheduler_step(self, iter_max: int, power: float = 0.9, min_lr: float = 1e-5):
        """One scheduler step.  Host-side: under an UpdateGuard it keeps advancing on skipped updates too (torch's behaviour when
        `scheduler.step()` follows `scaler.step(optimizer)`): the rate follows the updates attempted, not the ones applied."""
        self.sched_it += 1
        self.lr = polynomial_lr(self.base_lr, self.lr, self.sched_it, iter_max, power, min_lr)
        return self.lr


class FlatAdamW(_FlatOptimizer):
    """One parameter group of the reference's AdamW (utils/utils.py:258) on flat buffers.  State layout (exp_avg,
    exp_avg_sq, step) matches torch.optim.AdamW."""
    KIND = "AdamW"

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float, weight_decay: float = 1e-2, betas=(0.9, 0.999),
                 eps: float = 1e-8):
        super().__init__(params, lr)
        self.exp_avg = self._zeros()
        self.exp_avg_sq = self._zeros()
        self.weight_decay, self.betas, self.eps = weight_decay, betas, eps

    def state_dict(self) -> dict:
        applied = float(self.applied_steps())            # what torch holds: the updates applied (== steps unless a guard skipped some)
        state = {i: {"step": torch.tensor(applied), "exp_avg": self._state_slot(self.exp_avg, i),
                     "exp_avg_sq": self._state_slot(self.exp_avg_sq, i)} for i in range(len(self.params))}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None}
        return self._sd(state, group)

    def load_state_dict(self, sd: dict) -> None:
        g = self._load_group(sd)
        self.lr, self.betas, self.eps, self.weight_decay = float(g["lr"]), tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"])
        self._load_slots(sd, "exp_avg", self.exp_avg)
        self._load_slots(sd, "exp_avg_sq", self.exp_avg_sq)
        steps = max([int(float(st["step"])) for st in sd["state"].values()], default=0)
        self._load_counters(sd, g, steps)
        self._seed_applied(steps if sd["state"] else self.steps)

    def _launch(self, grad_scale):
        ops.adamw_step(self.param, self.grad, self.exp_avg, self.exp_avg_sq, self.steps, self.lr, self.betas, self.eps,
                       self.weight_decay, grad_scale)

    def _hyper(self, step, grad_scale):
        return ops.adamw_hyper(step, self.lr, self.betas, self.eps, self.weight_decay, grad_scale)

    def step_dev(self):
        """Device side: the update with constants from `hyper_dev` (what gets captured); behind the gate of an attached UpdateGuard."""
        if self._guard is not None:
            ops.adamw_step_gated_dev(self.param, self.grad, self.exp_avg, self.exp_avg_sq, self.hyper_dev, self._guard.gate)
        else:
            ops.adamw_step_dev(self.param, self.grad, self.exp_avg, self.exp_avg_sq, self.hyper_dev)


class FlatSGD(_FlatOptimizer):
    """One parameter group of the reference's SGD (utils/utils.py:254: momentum 0.9, coupled weight decay, dampening 0)
    on flat buffers.  The momentum buffer exists only when momentum != 0 (4 B per parameter against AdamW's 8).  State
    layout (momentum_buffer; no state before the first step) matches torch.optim.SGD."""
    KIND = "SGD"
    HYPER = 4

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float, weight_decay: float = 0.0, momentum: float = 0.0,
                 nesterov: bool = False):
        if nesterov and momentum <= 0:
            raise ValueError("FlatSGD: Nesterov momentum requires a momentum")
        super().__init__(params, lr)
        self.weight_decay, self.momentum, self.nesterov = weight_decay, momentum, bool(nesterov)
        self.momentum_buffer = self._zeros() if momentum != 0 else None
        self._loaded_state = False      # a torch.optim.SGD file has momentum buffers but no step count

    def state_dict(self) -> dict:
        state = {}
        if self.momentum_buffer is not None and (self.steps > 0 or self._loaded_state):
            state = {i: {"momentum_buffer": self._state_slot(self.momentum_buffer, i)} for i in range(len(self.params))}
        group = {"lr": self.lr, "momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay,
                 "nesterov": self.nesterov, "maximize": False, "foreach": None, "differentiable": False, "fused": None}
        return self._sd(state, group)

    def load_state_dict(self, sd: dict) -> None:
        g = self._load_group(sd)
        if float(g.get("dampening", 0)) != 0:
            raise ValueError("FlatSGD.load_state_dict: dampening != 0 is not supported")
        self.lr, self.momentum, self.weight_decay = float(g["lr"]), float(g["momentum"]), float(g["weight_decay"])
        self.nesterov = bool(g["nesterov"])
        if self.momentum == 0:
            self.momentum_buffer = None
        else:
            if self.momentum_buffer is None:
                self.momentum_buffer = self._zeros()
            self._load_slots(sd, "momentum_buffer", self.momentum_buffer)
        self._loaded_state = self.momentum_buffer is not None and bool(sd["state"])
        self._load_counters(sd, g, 0)
        self._seed_applied(self.steps)                   # (torch's SGD state has no step count to restore)

    def _launch(self, grad_scale):
        ops.sgd_step(self.param, self.grad, self.momentum_buffer, self.lr, self.momentum, self.weight_decay, self.nesterov,
                     grad_scale)

    def _hyper(self, step, grad_scale):
        return ops.sgd_hyper(self.lr, self.momentum, self.weight_decay, self.nesterov, grad_scale)

    def step_dev(self):
        if self._guard is not None:
            ops.sgd_step_gated_dev(self.param, self.grad, self.momentum_buffer, self.hyper_dev, self._guard.gate, self.nesterov)
        else:
            ops.sgd_step_dev(self.param, self.grad, self.momentum_buffer, self.hyper_dev, self.nesterov)


class FlatRMSprop(_FlatOptimizer):
    """One parameter group of the reference's RMSprop (utils/utils.py:260, torch defaults otherwise; not centered) on flat
    buffers.  State layout (step, square_avg, momentum_buffer when momentum > 0) matches torch.optim.RMSprop."""
    KIND = "RMSprop"

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float, weight_decay: float = 0.0, alpha: float = 0.99,
                 eps: float = 1e-8, momentum: float = 0.0):
        super().__init__(params, lr)
        self.weight_decay, self.alpha, self.eps, self.momentum = weight_decay, alpha, eps, momentum
        self.square_avg = self._zeros()
        self.momentum_buffer = self._zeros() if momentum > 0 else None

    def state_dict(self) -> dict:
        state = {}
        if self.steps > 0:
            applied = float(self.applied_steps())        # as FlatAdamW.state_dict
            for i in range(len(self.params)):
                state[i] = {"step": torch.tensor(applied), "square_avg": self._state_slot(self.square_avg, i)}
                if self.momentum_buffer is not None:
                    state[i]["momentum_buffer"] = self._state_slot(self.momentum_buffer, i)
        group = {"lr": self.lr, "momentum": self.momentum, "alpha": self.alpha, "eps": self.eps, "centered": False,
                 "weight_decay": self.weight_decay, "capturable": False, "foreach": None, "maximize": False,
                 "differentiable": False}
        return self._sd(state, group)

    def load_state_dict(self, sd: dict) -> None:
        g = self._load_group(sd)
        if g.get("centered", False):
            raise ValueError("FlatRMSprop.load_state_dict: centered RMSprop is not supported")
        self.lr, self.alpha, self.eps = float(g["lr"]), float(g["alpha"]), float(g["eps"])
        self.weight_decay, self.momentum = float(g["weight_decay"]), float(g["momentum"])
        self._load_slots(sd, "square_avg", self.square_avg)
        if self.momentum > 0:
            if self.momentum_buffer is None:
                self.momentum_buffer = self._zeros()
            self._load_slots(sd, "momentum_buffer", self.momentum_buffer)
        else:
            self.momentum_buffer = None
        steps = max([int(float(st["step"])) for st in sd["state"].values()], default=0)
        self._load_counters(sd, g, steps)
        self._seed_applied(steps if sd["state"] else self.steps)

    def _launch(self, grad_scale):
        ops.rmsprop_step(self.param, self.grad, self.square_avg, self.momentum_buffer, self.lr, self.alpha, self.eps,
                         self.weight_decay, self.momentum, grad_scale)

    def _hyper(self, step, grad_scale):
        return ops.rmsprop_hyper(self.lr, self.alpha, self.eps, self.weight_decay, self.momentum, grad_scale)

    def step_dev(self):
        if self._guard is not None:
            ops.rmsprop_step_gated_dev(self.param, self.grad, self.square_avg, self.momentum_buffer, self.hyper_dev, self._guard.gate)
        else:
            ops.rmsprop_step_dev(self.param, self.grad, self.square_avg, self.momentum_buffer, self.hyper_dev)


def get_optimizer(name: str, lr: float, params: Iterable[torch.nn.Parameter], weight_decay: float = 1e-4,
                  momentum: float = 0.9) -> _FlatOptimizer:
    """utils/utils.py:252-261: 'sgd' -> SGD(lr, weight_decay, momentum=0.9), 'adam' -> AdamW(lr, weight_decay),
    'rmsprop' -> RMSprop(lr, weight_decay); torch defaults otherwise.  (The reference never passes `momentum` in, so
    its SGD always runs at 0.9; an unknown name fails there with UnboundLocalError, here with ValueError.)"""
    if name == "sgd":
        return FlatSGD(params, lr, weight_decay=weight_decay, momentum=momentum)
    if name == "adam":
        return FlatAdamW(params, lr, weight_decay=weight_decay)
    if name == "rmsprop":
        return FlatRMSprop(params, lr, weight_decay=weight_decay)
    raise ValueError(f"get_optimizer: unknown optimizer {name!r} (expected 'sgd', 'adam' or 'rmsprop')")


def build_optimizers(encoder, decoder, lr_cnn: float, lr: float, lr_cva: Optional[float] = None, weight_decay: float = 1e-2,
                     weight_decay_cnn: float = 1e-2, optim: str = "adam", optim_cnn: str = "adam") -> Dict[str, _FlatOptimizer]:
    """train.py:209-213: cva / encoder / decoder optimizers (cva omitted when the encoder has no such parameters); the
    decoder's is built with `optim` (-optim), the encoder's and cva's with `optim_cnn` (-optim_cnn)."""
    g = split_param_groups(encoder, decoder)
    opts = {"enc": get_optimizer(optim_cnn, lr_cnn, g["enc"], weight_decay_cnn),
            "dec": get_optimizer(optim, lr, g["dec"], weight_decay)}
    if g["cva"]:
        opts["cva"] = get_optimizer(optim_cnn, lr_cva if lr_cva is not None else lr_cnn, g["cva"], weight_decay)
    return opts


class GradClip:
    """Gradient-norm clipping (torch.nn.utils.clip_grad_norm_, L2) over the flat gradient buffers of up to 8 optimizers, folded into
    their device-side updates.  `measure()` reads each gradient buffer once (one launch per optimizer) and one finish launch forms
        total_norm = sqrt(sum_g s_g^2 |grad_g|^2),   coef = min(1, max_norm / (total_norm + 1e-6))
    where s_g is the gradient scale `stage_hyper` staged for optimizer g (the 1/world factor of the all-reduce, a loss-scale
    correction), and multiplies every staged scale by coef.  The `.grad` buffers are NOT rewritten: they keep the unclipped sum and
    are zeroed by the update as before; the clipped gradient is what `step_dev` forms from grad * scale.  No host synchronisation,
    no allocation per call: capturable into a hipGraph (GraphedTrainStep(clip_grad=...)).

    One GradClip over several optimizers clips by one global norm, like clip_grad_norm_ over all their parameters; one GradClip
    per optimizer is timm's per-optimizer `clip_grad` (the knob of the reference's recipes, train.py:223-273).
    max_norm=None only measures: coef is exactly 1 and the staged constants are left alone.
    `stats` (device, 4 + G floats) = [total_norm, coef, non-finite element count, 0, norm_0 ... norm_{G-1}].
    skip_nonfinite=True: an update whose gradient holds a NaN or an Inf is skipped on the device, for ALL the optimizers here (what
    torch's GradScaler.step does when it found an inf): `.guard` is the UpdateGuard, `step()` runs stage -> measure -> gate -> gated
    updates.  Without it coef is NaN or 0 exactly as torch's is for such a gradient, and the update runs.
    Not covered: clip_grad_value_, adaptive clipping, norms other than L2, dynamic loss scaling."""
    MAX_GROUPS = ops.GRAD_NORM_MAX_GROUPS

    @staticmethod
    def _validate(opts, max_norm):
        if not opts:
            raise ValueError("GradClip: no optimizers")
        if len(opts) > GradClip.MAX_GROUPS:
            raise ValueError(f"GradClip: {len(opts)} optimizers (at most {GradClip.MAX_GROUPS} share one norm)")
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError(f"GradClip: max_norm must be positive (or None to measure only), got {max_norm}")
        for o in opts:
            if getattr(o, "KIND", None) not in ops._OPT_KINDS:
                raise ValueError(f"GradClip: {type(o).__name__} is not a flat optimizer of this package")

    def __init__(self, optimizers, max_norm: Optional[float] = None, skip_nonfinite: bool = False):
        self.opts = list(optimizers.values()) if isinstance(optimizers, dict) else list(optimizers)
        self._validate(self.opts, max_norm)
        if not isinstance(skip_nonfinite, bool):
            raise ValueError(f"GradClip: skip_nonfinite must be True or False, got {skip_nonfinite!r}")
        self.max_norm = None if max_norm is None else float(max_norm)
        for o in self.opts:
            if not hasattr(o, "hyper_dev"):
                o.enable_device_hyper()
        dev = self.opts[0].grad.device
        self.sizes = [o.grad.numel() for o in self.opts]
        counts = [2 * ops.grad_norm_partials(n) for n in self.sizes]
        self._ws = torch.zeros(sum(counts), device=dev, dtype=torch.float32)
        self.partials = list(self._ws.split(counts))
        self.stats = torch.zeros(4 + len(self.opts), device=dev, dtype=torch.float32)
        self.guard = UpdateGuard(self.opts, [self]) if skip_nonfinite else None

    def measure(self):
        """Enqueue the G partial launches and the finish on the current stream.  Must follow the optimizers' `stage_hyper` in stream
        order (it reads, and with a max_norm rescales, the staged gradient scales) and precede their `step_dev`."""
        for o, part in zip(self.opts, self.partials):
            ops.grad_norm_partial(o.grad, part)
        ops.grad_norm_finish(self.partials, self.sizes, [o.hyper_dev for o in self.opts], [o.KIND for o in self.opts], self.stats,
                             self.max_norm)
        return self.stats

    def step(self, scales=None):
        """The eager update with clipping, in place of `for o in opts: o.step(grad_scale=scale)`: stage every optimizer's constants
        (scales: None = 1.0, one float for all, or one per optimizer -- e.g. what all_reduce_grads returned), measure, update.
        Gradients are not reset (call zero_grad as after step()).  Synchronises nowhere; `read()` does."""
        if scales is None or isinstance(scales, (int, float)):
            scales = [1.0 if scales is None else float(scales)] * len(self.opts)
        scales = list(scales)
        if len(scales) != len(self.opts):
            raise ValueError(f"GradClip.step: {len(scales)} scales for {len(self.opts)} optimizers")
        for o, sc in zip(self.opts, scales):
            o.stage_hyper(sc)
        self.measure()
        if self.guard is not None:
            self.guard.launch()
        for o in self.opts:
            o.step_dev()
        bump_weights_epoch()
        return self.stats

    def read(self) -> dict:
        """The statistics of the last measure() on the host.  This is the one call here that synchronises (a device-to-host copy)."""
        s = self.stats.cpu().tolist()
        return {"total_norm": s[0], "coef": s[1], "nonfinite": int(s[2]), "norms": s[4:]}


class UpdateGuard:
    """Skips, on the device, the update of a step whose gradient is non-finite: ONE decision for all `optimizers` (1 ... 8), taken
    from the statistics of all `clips` (1 ... 8 GradClip, each measuring some of them; optimizers no clip measures are not looked
    at): a non-finite element or a NaN norm anywhere and nobody is updated, so the groups never go out of step with one another.
    A finite gradient whose norm overflows to +Inf is not skipped.  Owns the gate words, the raw AdamW constants and the
    applied-step counters, all on the device; attaches itself to the optimizers, whose `stage_hyper` then calls `stage()` and whose
    `step_dev()` runs behind the gate.  Order within a step: stage_hyper of every optimizer, measure() of every clip, `launch()`,
    step_dev() of every optimizer.  No host synchronisation, no allocation per call: capturable.

    `opt.steps` stays the number of updates ATTEMPTED (what the staged constants and the LR schedule follow); AdamW's bias
    corrections follow the updates APPLIED: the gate launch recomputes them on the device once the two counts differ, and leaves
    the staged constants untouched while they agree (a run that never skips is bitwise the unguarded one).  `state_dict()["state"]
    [i]["step"]` of FlatAdamW / FlatRMSprop is the applied count, `load_state_dict` re-seeds it.  The skip statistics (`read()`) are
    not part of a checkpoint.  The gradient reset stays the caller's zero_grad(): the bad gradient -- the whole accumulated cycle
    under gradient accumulation -- is dropped whether or not the update ran."""
    MAX_GROUPS = ops.UPDATE_GATE_MAX

    @staticmethod
    def _validate(opts, n_clips):
        if not opts:
            raise ValueError("UpdateGuard: no optimizers")
        if len(opts) > UpdateGuard.MAX_GROUPS:
            raise ValueError(f"UpdateGuard: {len(opts)} optimizers (at most {UpdateGuard.MAX_GROUPS} share one decision)")
        if not 1 <= n_clips <= UpdateGuard.MAX_GROUPS:
            raise ValueError(f"UpdateGuard: {n_clips} clips (1 to {UpdateGuard.MAX_GROUPS} statistics buffers feed one decision)")
        for o in opts:
            if getattr(o, "KIND", None) not in ops._OPT_KINDS:
                raise ValueError(f"UpdateGuard: {type(o).__name__} is not a flat optimizer of this package")

    def __init__(self, optimizers, clips):
        self.opts = list(optimizers.values()) if isinstance(optimizers, dict) else list(optimizers)
        self.clips = list(clips)
        self._validate(self.opts, len(self.clips))
        for c in self.clips:
            if not isinstance(c, GradClip) or any(all(o is not mine for mine in self.opts) for o in c.opts):
                raise ValueError("UpdateGuard: every clip must be a GradClip over some of the guard's optimizers")
        dev = self.opts[0].grad.device
        for o in self.opts:
            if not hasattr(o, "hyper_dev"):
                o.enable_device_hyper()
        g = len(self.opts)
        self.gate = torch.zeros(ops.GATE_WORDS, device=dev, dtype=torch.int32)
        self.raw = torch.zeros(4 * g, device=dev, dtype=torch.float64)          # per group: lr, beta1, beta2, nominal step (AdamW)
        self.applied = torch.tensor([o.steps - o._skipped_host for o in self.opts], dtype=torch.int64).to(dev)
        self._raw_host = [None] * g
        for o in self.opts:
            o._guard = self

    def _index(self, opt) -> int:
        for g, o in enumerate(self.opts):
            if o is opt:
                return g
        raise ValueError("UpdateGuard: not one of this guard's optimizers")

    def stage(self, opt, step: int) -> None:
        """Host side, from opt.stage_hyper: the raw constants the gate launch re-derives AdamW's bias corrections from."""
        if opt.KIND != "AdamW":
            return
        g = self._index(opt)
        self._raw_host[g] = ops.adamw_gate_hyper(step, opt.lr, opt.betas)        # (pinned; kept until the next one replaces it)
        self.raw[4 * g:4 * g + 4].copy_(self._raw_host[g], non_blocking=True)

    def seed(self, opt) -> None:
        """Set opt's applied-step counter from the host (after load_state_dict)."""
        self.applied[self._index(opt)] = opt.steps - opt._skipped_host

    def applied_steps(self, opt) -> int:
        return int(self.applied[self._index(opt)].item())

    def launch(self):
        """Enqueue the gate launch on the current stream: after the clips' measure(), before the optimizers' step_dev()."""
        ops.update_gate([c.stats for c in self.clips], self.gate, [o.hyper_dev for o in self.opts], [o.KIND for o in self.opts],
                        self.applied, self.raw)
        return self.gate

    def read(self) -> dict:
        """The skip counters on the host.  The one call here that synchronises (a device-to-host copy), like GradClip.read(): poll it
        where the loss is read back."""
        w = self.gate.cpu().tolist()
        return {"skipped": w[1], "consecutive": w[2], "longest": w[4], "updates": w[3], "last_skipped": bool(w[0])}


class GraphedTrainStep:
    """One training step (taped forward, mask loss, backward, the update of every group, gradient reset) captured into a hipGraph
    and replayed: at config 5's micro-batch the eager step is bound by ~10^4 host-side launches, not by the GPU.
    `forward_fn(x) -> logits` must be built from mumpy_hip.autograd functions (capture-safe: no host synchronisation).
    Train mode works: the stochastic-depth masks are drawn by torch's graph-safe Philox generator inside the capture, so every
    replay draws new ones (test_hip_graphed_train_step_draws_fresh_drop_path_masks).  Learning-rate schedules keep working: the
    optimizers' constants are staged into device memory before each update.  Call `step(x, target)` -> loss3 (device tensor
    [total, iou, focal]).
    clip_grad: gradient-norm clipping inside the replayed update (GradClip).  A float clips all the optimizers by one global norm;
    a dict keyed like the `optimizers` dict clips each named optimizer by its own norm (a missing key leaves that optimizer
    unclipped).  The norm is measured at the head of the update -- after the all-reduce, with the 1/world factor staged, once per
    update under accumulation -- and `.grad_stats` is the device statistics tensor (a dict of them for the dict form; GradClip.stats
    gives the layout).  The `.grad` buffers keep the unclipped sum until the update zeroes them.  None: nothing is launched.
    skip_nonfinite=True: the replayed update is skipped, for every optimizer at once, when a gradient holds a NaN or an Inf
    (UpdateGuard; `.guard`, poll `.guard.read()` next to the loss read-back -- a replay never raises).  It gates on all the step's
    clips together; optimizers that no clip_grad entry covers (all of them when clip_grad is None) get one measure-only GradClip, so
    every gradient is looked at.  The norm is measured after the all-reduce, so every rank takes the same decision; under
    accumulation the whole cycle's gradient is dropped.  The gradient reset runs either way.  False: nothing new is launched."""

    def __init__(self, forward_fn, optimizers, x, target, warmup: int = 3, loss_scale: float = 1.0, all_reduce: bool = False,
                 accumulation_steps: int = 1, clip_grad=None, skip_nonfinite: bool = False):
        """all_reduce=True (data-parallel ranks): TWO graphs -- forward + loss + backward, and update + gradient reset -- with
        the bucketed gradient all-reduce (RCCL) issued eagerly between their replays.
        accumulation_steps=k > 1 (train.py:115-120): every step() is one micro-batch whose loss gradient is scaled by
        loss_scale / k and accumulated in the flat gradient buffers; every k-th micro-batch (counted from the first warm-up
        one) then runs the update graph (two graphs, as with all_reduce).  The warm-up covers at least one whole cycle."""
        if accumulation_steps < 1:
            raise ValueError(f"GraphedTrainStep: accumulation_steps must be >= 1, got {accumulation_steps}")
        if not isinstance(skip_nonfinite, bool):
            raise ValueError(f"GraphedTrainStep: skip_nonfinite must be True or False, got {skip_nonfinite!r}")
        self.opts = list(optimizers.values()) if isinstance(optimizers, dict) else list(optimizers)
        clip_plan = []                    # [(key or None, optimizers, max_norm)], checked before anything touches the GPU
        if isinstance(clip_grad, dict):
            if not isinstance(optimizers, dict):
                raise ValueError("GraphedTrainStep: a clip_grad dict needs the optimizers as a dict with the same keys")
            for key, c in clip_grad.items():
                if key not in optimizers:
                    raise ValueError(f"GraphedTrainStep: clip_grad names {key!r}, which is not one of the optimizers {sorted(optimizers)}")
                clip_plan.append((key, [optimizers[key]], c))
        elif clip_grad is not None:
            clip_plan.append((None, self.opts, clip_grad))
        for _, group, c in clip_plan:
            if c is None or isinstance(c, bool) or not isinstance(c, (int, float)):
                raise ValueError(f"GraphedTrainStep: clip_grad must be a positive number, got {c!r}")
            GradClip._validate(group, c)
        if skip_nonfinite:
            covered = [o for _, group, _ in clip_plan for o in group]
            rest = [o for o in self.opts if all(o is not c for c in covered)]
            if rest:
                GradClip._validate(rest, None)
                clip_plan.append((None, rest, None))         # measure only: the guard must see every gradient
            UpdateGuard._validate(self.opts, len(clip_plan))
        self.x, self.target = x.clone(), target.clone()
        self.all_reduce = all_reduce
        self.accumulation_steps = k = int(accumulation_steps)
        self.iteration = 0                # micro-batches run (warm-up included): the reference's `iteration`
        self._updated = False
        for o in self.opts:
            o.enable_device_hyper()
        self.clips = [GradClip(group, c) for _, group, c in clip_plan]
        self.guard = UpdateGuard(self.opts, self.clips) if skip_nonfinite else None
        self.grad_stats = None
        if isinstance(clip_grad, dict):
            self.grad_stats = {key: clip.stats for (key, _, _), clip in zip(clip_plan, self.clips) if key is not None}
        elif self.clips:
            self.grad_stats = self.clips[0].stats

        def fwd_bwd():
            logits = forward_fn(self.x)
            loss3, dlogits = ops.mask_loss(logits.detach(), self.target, loss_scale=loss_scale / k)
            logits.backward(dlogits)
            return loss3

        def update():
            for clip in self.clips:               # reads the staged gradient scales and folds the clip coefficient into them
                clip.measure()
            if self.guard is not None:            # one decision for all the optimizers, from all the clips' statistics
                self.guard.launch()
            for o in self.opts:
                o.step_dev()
                o.zero_grad()

        from .streams import new_distinct_stream
        side = new_distinct_stream(self.x.device, (torch.cuda.current_stream().cuda_stream,))
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        for _ in range(warmup if k == 1 else max(warmup, k)):    # warm-up micro-batches are real ones (caches, allocator, lazy inits)
            with torch.cuda.stream(side):
                fwd_bwd()
            self._updated = self._due()
            self.iteration += 1
            if not self._updated:
                continue
            scales = [1.0] * len(self.opts)
            if all_reduce:
                # The collectives are issued from the CALLER's stream, never from the stream that captures: ProcessGroupNCCL's
                # watchdog thread polls the end event of every pending collective, and on ROCm 7.2 that query fails with
                # hipErrorCapturedEvent (process abort) when the stream the collective was issued from has meanwhile begun a
                # capture -- reproduced in isolation by tools/rccl_capture_probe.py (issued from the capture stream: abort;
                # from another stream, or with the watchdog drained first: fine).
                main.wait_stream(side)
                scales = [o.all_reduce_grads() for o in self.opts]
                side.wait_stream(main)
            with torch.cuda.stream(side):
                for o, sc in zip(self.opts, scales):
                    o.stage_hyper(sc)
                update()
        main.wait_stream(side)
        from .streams import quiesce_collectives
        quiesce_collectives()
        for o in self.opts:
            o.stage_hyper(advance=False)                 # capture records the launches; it does not run a step
        self.graph = torch.cuda.CUDAGraph()
        self.graph_update = None
        if all_reduce or k > 1:
            with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):   # (same stream as the warm-up and thread-local capture errors: see GraphedForward._capture)
                self.loss3 = fwd_bwd()
            self.graph_update = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_update, pool=self.graph.pool(), stream=side, capture_error_mode="thread_local"):
                update()
        else:
            with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
                self.loss3 = fwd_bwd()
                update()
        bump_weights_epoch()

    def _due(self) -> bool:
        return (self.iteration + 1) % self.accumulation_steps == 0

    @property
    def updated(self) -> bool:
        """Whether the last step() (or the last warm-up micro-batch) ran the optimizer update."""
        return self._updated

    def step(self, x=None, target=None, grad_scale: float = 1.0):
        """One micro-batch: replay forward + loss + backward; on every accumulation_steps-th call also the all-reduce (if
        all_reduce), the staged constants and the update.  -> loss3 = [total * loss_scale / k, iou, focal]."""
        if x is not None:
            self.x.copy_(x)
        if target is not None:
            self.target.copy_(target)
        self._updated = self._due()
        self.iteration += 1
        if self.graph_update is None:
            for o in self.opts:
                o.stage_hyper(grad_scale)
            self.graph.replay()
        else:
            self.graph.replay()
            if self._updated:
                for o in self.opts:
                    o.stage_hyper(grad_scale * (o.all_reduce_grads() if self.all_reduce else 1.0))   # the step's collectives, on the replay's stream
                self.graph_update.replay()
        if self._updated:
            bump_weights_epoch()
        return self.loss3
