"""Gradients with respect to the input clip: saliency and signed-gradient attacks on the three-view detector.

`input_gradient(encoder, decoder, x, target)` is dL/dx of the mask loss of the deployed function, computed on the training tape
(mumpy_hip.autograd.encoder_train(..., input_grad=True): the tokenizer AND the FAF branch) with every parameter frozen for the
duration: no `.grad`, no flat gradient buffer is touched, and the GEMM / convolution weight- and bias-gradient products are not
launched (LinearFn, MlpFn and Conv2dFn follow needs_input_grad; the norm, depthwise, bias-table and final-convolution kernels
produce their small parameter reductions in the same launch as dx, and those are dropped).  `PGDAttack` iterates
x_adv <- project(x_adv + alpha * sgn(dL/dx_adv)) (ops.pgd_step) with one iteration captured into a hipGraph and replayed.

`faf_bwd_reference` and `tokenize_dx_reference` restate the two backward kernels of include/mumpy_hip_ext10.h in torch; they run
without a GPU and are what the tests hold the kernels against."""
import contextlib

import numpy as np
import torch

from . import ops
from .ops import EVAL_MEAN, EVAL_STD


# ---------------------------------------------------------------------------------------------- host restatements
def faf_bwd_reference(dout, size=224, lo_hi=None, mid_lo=None, mid_hi=None):
    """dout (B,9,N,N), channel = band*3 + rgb -> dxf (B,3,N,N) = D^T (sum_band M_band o (D dout[band,rgb] D^T)) D with the band
    masks M_band = [lo <= i + j <= hi] of models.modules.dct.FAF (low [0, N//2.82], mid [N//2.82, N//2], high [N, 2N]).  The DCT matrix
    is built in fp64 and rounded to fp32 as FAF does; the products are evaluated in fp64 and returned in dout's dtype."""
    from models.modules.dct import DCT_mat, generate_filter
    n = int(size)
    lo_hi = int(n // 2.82) if lo_hi is None else int(lo_hi)
    mid_lo = int(n // 2.82) if mid_lo is None else int(mid_lo)
    mid_hi = int(n // 2) if mid_hi is None else int(mid_hi)
    b = dout.shape[0]
    if tuple(dout.shape) != (b, 9, n, n):
        raise RuntimeError(f"faf_bwd_reference: expects dout (B,9,{n},{n}), got {tuple(dout.shape)}")
    d = torch.tensor(DCT_mat(n)).float().double().to(dout.device)
    masks = [torch.tensor(generate_filter(lo, hi, n)).to(dout.device) for lo, hi in ((0, lo_hi), (mid_lo, mid_hi), (n, 2 * n))]
    g = dout.double().reshape(b, 3, 3, n, n)                                  # (B, band, rgb, N, N)
    spec = sum(masks[k] * (d @ g[:, k] @ d.t()) for k in range(3))           # (B, rgb, N, N)
    return (d.t() @ spec @ d).to(dout.dtype)


def tokenize_dx_reference(dcols, tubelets, b, t, h, w, dxf=None, frame=1):
    """dcols[v] (B * tt_v * (H/4) * (W/4), ld_v >= 48 t_v), columns (ch, t, py, px) -> dx (B,T,3,H,W): each view's columns scattered
    back to the frames its tubelets cover (frames past tt_v * t_v get nothing from view v), summed in the order v = 0, 1, 2, and dxf
    (B,3,H,W) added to frame `frame`.  The pad columns are not read."""
    dx = torch.zeros(b, t, 3, h, w, dtype=dcols[0].dtype, device=dcols[0].device)
    for c, tv in zip(dcols, tubelets):
        tt = (t - tv) // tv + 1
        k = 48 * tv
        part = c[:, :k].reshape(b, tt, h // 4, w // 4, 3, tv, 4, 4).permute(0, 1, 5, 4, 2, 6, 3, 7).reshape(b, tt * tv, 3, h, w)
        dx[:, :tt * tv] += part
    if dxf is not None:
        dx[:, frame] += dxf
    return dx


def pgd_bounds(eps, mean=EVAL_MEAN, std=EVAL_STD):
    """Host only.  eps in [0,1] pixel units -> (eps3, lo3, hi3) in the normalised units of the clip, three float32 values each:
    eps3 = eps / std, lo3 = (0 - mean) / std, hi3 = (1 - mean) / std (the image of the valid pixel range)."""
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError(f"pgd_bounds: eps must be >= 0, got {eps}")
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    if mean.shape != (3,) or std.shape != (3,) or not (std > 0).all():
        raise ValueError("pgd_bounds: mean and std must be three values, std positive")
    eps3 = np.float32(eps) / std
    lo3, hi3 = (np.float32(0.0) - mean) / std, (np.float32(1.0) - mean) / std
    return tuple(tuple(float(v) for v in a) for a in (eps3, lo3, hi3))


# ---------------------------------------------------------------------------------------------- the gradient
@contextlib.contextmanager
def frozen_parameters(*modules):
    """Every parameter of the modules with requires_grad = False for the duration; the flags are restored on every exit path."""
    params = [p for m in modules for p in m.parameters()]
    flags = [p.requires_grad for p in params]
    try:
        for p in params:
            p.requires_grad_(False)
        yield
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)


def _loss_and_dx(encoder, decoder, x, target, coupling):
    """Taped forward, mask loss, backward to the clip.  Call with the parameters frozen."""
    from . import autograd as A
    xg = x.detach().requires_grad_()
    logits, _ = A.decoder_train(decoder, *A.encoder_train(encoder, xg, coupling=coupling, input_grad=True))
    loss3, dlogits = ops.mask_loss(logits.detach(), target)
    with A.grad_slots(False):                                  # belt and braces: nothing accumulates into a flat gradient buffer
        (dx,) = torch.autograd.grad(logits, xg, dlogits)
    return loss3, dx


def input_gradient(encoder, decoder, x, target, coupling=None):
    """-> (loss3, dx): the mask loss of ops.mask_loss at x (B,T,3,224,224) against target, and its gradient with respect to x.
    The modules are used as the caller left them (eval mode for saliency and attacks: no stochastic depth).  No parameter's `.grad`
    and no flat gradient buffer is touched; requires_grad flags are restored on every exit path.  coupling: as encoder_train."""
    with frozen_parameters(encoder, decoder):
        return _loss_and_dx(encoder, decoder, x, target, coupling)


class PGDAttack:
    """Projected gradient ascent on the mask loss inside an L-infinity ball of eps (pixel units, [0,1]) around the clip:
        x_adv <- clamp(clamp(x_adv + alpha * sgn(dL/dx_adv), x0 - eps3, x0 + eps3), lo3, hi3)        (ops.pgd_step, pgd_bounds)
    graph=True: one iteration (taped forward, loss, backward to dx, the step on the static x_adv) is captured once into a hipGraph
    and `run` replays it `steps` times; nothing is read back inside the loop.  graph=False: the same iteration eagerly.
    eps and alpha are in pixel units ([0,1]); the step is taken with ONE size in normalised units, alpha / min(std) (see __init__).
    steps = 1 with alpha = eps is FGSM; a negative alpha descends (a targeted attack towards `target`).  There is no random start;
    run(x_start=) seeds x_adv.  x and target given here fix the shapes; run(x=, target=) replaces their contents without a
    re-capture.  `.loss3` is the loss of the last iteration, evaluated BEFORE its step."""

    def __init__(self, encoder, decoder, x, target, eps, alpha, coupling=None, graph=True, mean=EVAL_MEAN, std=EVAL_STD, warmup=2):
        if x.dim() != 5 or x.shape[2] != 3 or x.dtype != torch.float32 or not x.is_cuda:
            raise RuntimeError(f"PGDAttack: x must be a float32 GPU clip (B,T,3,H,W), got {x.dtype} {tuple(x.shape)} on {x.device}")
        self.encoder, self.decoder, self.coupling = encoder, decoder, coupling
        self.eps3, self.lo3, self.hi3 = pgd_bounds(eps, mean, std)
        # the kernel takes ONE step size in normalised units: alpha / min(std), i.e. alpha pixel units in the channel with the smallest
        # std and alpha * std_c / min(std) (at most 12 % more with the evaluation statistics) in the others.  The eps ball is exact per
        # channel, and alpha = eps reaches its surface in every channel (FGSM)
        self.alpha = float(np.float32(alpha) / np.asarray(std, dtype=np.float32).min())
        self.x0 = x.detach().clone()
        self.target = target.detach().clone()
        self.x_adv = self.x0.clone()
        self.loss3 = None
        self.graph = None
        if graph:
            self._capture(int(warmup))

    def _iteration(self):
        loss3, dx = _loss_and_dx(self.encoder, self.decoder, self.x_adv, self.target, self.coupling)
        ops.pgd_step(self.x_adv, dx, self.x0, self.alpha, self.eps3, self.lo3, self.hi3)
        return loss3

    def _capture(self, warmup):
        from .streams import new_distinct_stream
        side = new_distinct_stream(self.x0.device, (torch.cuda.current_stream().cuda_stream,))
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with frozen_parameters(self.encoder, self.decoder):
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):                          # real iterations: caches, allocator, lazy inits
                    self._iteration()
            main.wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
                self.loss3 = self._iteration()
        self.x_adv.copy_(self.x0)

    def run(self, steps, x=None, target=None, x_start=None):
        """-> x_adv (a new tensor) after `steps` iterations from x_start (default: the clean clip)."""
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"PGDAttack.run: steps must be >= 0, got {steps}")
        if x is not None:
            self.x0.copy_(x)
        if target is not None:
            self.target.copy_(target.reshape(self.target.shape))
        self.x_adv.copy_(self.x0 if x_start is None else x_start)
        if self.graph is not None:
            for _ in range(steps):
                self.graph.replay()
        else:
            with frozen_parameters(self.encoder, self.decoder):
                for _ in range(steps):
                    self.loss3 = self._iteration()
        return self.x_adv.clone()
