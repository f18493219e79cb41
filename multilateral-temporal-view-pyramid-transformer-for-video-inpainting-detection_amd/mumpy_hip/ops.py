"""Tensor-level wrappers over the C ABI.  Each takes/returns torch CUDA(HIP) fp32 tensors, allocates outputs with
torch (caching allocator => graph-capturable), and enqueues on torch's current stream.  No fallbacks."""
import math
import os
from typing import Optional

import torch

from .lib import load_library

ACT_NONE, ACT_GELU = 0, 1
MATH_FP32, MATH_BF16, MATH_BF16X3, MATH_BF16X2 = 0, 0x100, 0x200, 0x400
_MATH = MATH_FP32          # OR-ed into the `act` argument of every linear / conv launch
_WS_BYTES = {}


def set_matrix_math(mode: str) -> None:
    """"fp32" (default): exact fp32 products on v_mfma_f32_32x32x2_f32.  "bf16": operands of every GEMM / convolution are
    rounded to bf16 while being staged and multiplied on the bf16 MFMA with fp32 accumulation (config 3's arithmetic);
    tensors in memory, LayerNorm / softmax / GroupNorm statistics and all other kernels stay fp32.
    "bf16x3": fp32 products on the bf16 matrix pipe -- each operand is split into three bf16 pieces while staged and the
    six significant piece products are accumulated in fp32; fp32-level accuracy (see include/mumpy_hip.h).
    "bf16x2": two pieces / three products: 16-bit-mantissa operands (TF32-class and better), a reduced-precision mode."""
    global _MATH
    if mode not in _MODES:
        raise ValueError(f"unknown matrix math mode {mode!r}")
    _MATH = _MODES[mode]


_MODES = {"fp32": MATH_FP32, "bf16": MATH_BF16, "bf16x3": MATH_BF16X3, "bf16x2": MATH_BF16X2}


def matrix_math() -> str:
    return {v: k for k, v in _MODES.items()}[_MATH]


_STORAGE = "fp32"


def set_storage(mode: str) -> None:
    """"fp32" (default) or "bf16": BASELINE config 3 as written -- inside the Swin blocks (and the MLPs of the global
    blocks) LayerNorm writes bf16, the qkv / fc1 GEMMs read bf16 activations and bf16 copies of their weights and write
    bf16, window attention reads and writes bf16, and the proj / fc2 GEMMs read bf16 and add into the fp32 residual stream.
    Accumulation, softmax and LayerNorm statistics stay fp32.  Implies set_matrix_math("bf16") for the remaining GEMMs."""
    global _STORAGE
    if mode not in ("fp32", "bf16"):
        raise ValueError(f"unknown storage mode {mode!r}")
    _STORAGE = mode
    set_matrix_math("bf16" if mode == "bf16" else "fp32")


def storage() -> str:
    return _STORAGE


NEG = -1e30


def _lib():
    return load_library()


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"mumpy_hip: {name} is on {t.device}; the HIP kernels need a GPU tensor (there is no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"mumpy_hip: {name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional per-launch timing (bench.py): when PROFILE is a dict, every C-ABI call is bracketed by events on the
# stream it is launched on and recorded as PROFILE[name] -> [(start_event, end_event, work), ...].
PROFILE = None


def _call(name, *args, work=0.0):
    lib = _lib()
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = getattr(lib, name)(*args)
        e1.record()
        PROFILE.setdefault(name, []).append((e0, e1, work))
    else:
        rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed (rc={rc}): {lib.mumpy_last_error().decode()}")


def _opt(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    """An optional fp32 operand (a bias): checked like any other when given."""
    return None if t is None else _chk(t, name)


def _rd(t: torch.Tensor, name: str, numel: int, who: str, dtype=torch.float32) -> torch.Tensor:
    """A read operand, measured against the launch that will read it: on the GPU, of the dtype the kernel reads, exactly `numel`
    elements.  A non-contiguous one is copied (the copy is read, nothing is lost).  A handful of integer comparisons."""
    if not t.is_cuda or t.dtype != dtype or t.numel() != numel:
        raise RuntimeError(f"mumpy_hip: {who} needs {name} as a {dtype} GPU tensor of {numel} elements, got {t.dtype} {tuple(t.shape)} "
                           f"on {t.device}")
    return t if t.is_contiguous() else t.contiguous()


def _rd_opt(t: Optional[torch.Tensor], name: str, numel: int, who: str) -> Optional[torch.Tensor]:
    return None if t is None else _rd(t, name, numel, who)


def _wr(t: torch.Tensor, name: str, numel: int, who: str, dtype=torch.float32) -> torch.Tensor:
    """A buffer a kernel writes or accumulates into (out=, *_out, optimizer state): taken where it is or refused -- a copy would
    receive the result and be dropped.  Where the wrapper knows the exact shape it uses _chk_exact instead."""
    if not t.is_cuda or t.dtype != dtype or t.numel() != numel or not t.is_contiguous():
        raise RuntimeError(f"mumpy_hip: {who} writes {name} in place and needs a contiguous {dtype} GPU tensor of {numel} elements, got "
                           f"{t.dtype} {tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ' (not contiguous)'}")
    return t


def _drop_ln_stats(t: torch.Tensor) -> None:
    """t is about to be overwritten: the LayerNorm-fold statistics a producer attached to it describe the old contents."""
    if hasattr(t, "_mumpy_ln_stats"):
        del t._mumpy_ln_stats


def _ws_bytes(key, fn_name, *args):
    """Workspace size of a launch (in the library a pure host function of the shape), asked once per shape."""
    wsb = _WS_BYTES.get(key)
    if wsb is None:
        wsb = _WS_BYTES[key] = int(getattr(_lib(), fn_name)(*args))
    return wsb


def _chk16(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.bfloat16:
        raise RuntimeError(f"mumpy_hip: {name} must be a bfloat16 GPU tensor, got {t.dtype} on {t.device}")
    return t if t.is_contiguous() else t.contiguous()


def layernorm_bf16(x, gamma, beta, eps=1e-5):
    """LayerNorm of an fp32 tensor, written as bf16 (statistics in fp32)."""
    x = _chk(x, "x")
    c = x.shape[-1]
    out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    gamma, beta = _rd(gamma, "gamma", c, "layernorm_bf16"), _rd(beta, "beta", c, "layernorm_bf16")
    _call("mumpy_layernorm_bf16_fwd", _p(x), _p(gamma), _p(beta), _p(out), x.numel() // c, c, eps,
          _stream(), work=6.0 * x.numel())
    return out


def linear_bf16s(x16, w16, bias=None, act=ACT_NONE, residual=None, out_bf16=True):
    """y = act(x16 @ w16.T + bias) + residual with bf16 x / W in memory, fp32 accumulate; y bf16 or fp32 (residual fp32)."""
    x16, w16 = _chk16(x16, "x"), _chk16(w16, "weight")
    n, k = w16.shape[0], w16.numel() // w16.shape[0]
    if x16.shape[-1] != k:
        raise RuntimeError(f"linear_bf16s: x has {x16.shape[-1]} features, weight expects {k}")
    m = x16.numel() // k
    out = torch.empty(*x16.shape[:-1], n, device=x16.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    if residual is not None:
        residual = _chk(residual, "residual")
        if residual.numel() != m * n or out_bf16:
            raise RuntimeError("linear_bf16s: the residual is fp32 and needs an fp32 output of the same shape")
    _call("mumpy_linear_bf16s_fwd", _p(x16), _p(w16), _p(_rd_opt(bias, "bias", n, "linear_bf16s")), _p(residual), _p(out),
          m, n, k, act, 1 if out_bf16 else 0, _stream(), work=2.0 * m * n * k)
    return out


def _choice(value, choices, what, var=None):
    """`value` if it is one of `choices`, else a ValueError saying what it was to be (and the environment variable it came from)."""
    if value not in choices:
        raise ValueError(f"{var}: unknown {what} {value!r}" if var else f"unknown {what} {value!r}")
    return value


def _env_choice(var, choices, default, what):
    """Initial value of a process-wide switch: the environment variable `var`; unset or empty means `default`."""
    return _choice(os.environ.get(var, "") or default, choices, what, var)


# the process-wide switches: one tuple of values each, for the environment reader, the setter and the ops' explicit arguments
_ATTN_MATHS, _ATTN_WHAT = ("fp32", "bf16"), "attention math mode"
_CVA_MATHS, _CVA_WHAT = ("fp32", "bf16"), "cross-view attention math mode"
_COUPLINGS, _COUPLING_WHAT = ("batch", "clip"), "clip coupling"
# each read once, at import
_ATTN_MATH = _env_choice("MUMPY_ATTN_MATH", _ATTN_MATHS, "fp32", _ATTN_WHAT)
_CVA_MATH = _env_choice("MUMPY_CVA_MATH", _CVA_MATHS, "fp32", _CVA_WHAT)
_CLIP_COUPLING = _env_choice("MUMPY_CLIP_COUPLING", _COUPLINGS, "batch", _COUPLING_WHAT)
_MLP_FUSED = _env_choice("MUMPY_MLP_FUSED", ("0", "1"), "0", "MLP fusion setting (\"0\" or \"1\")") == "1"


def set_attention_math(mode: str) -> None:
    """Arithmetic of the Swin window attention core in the two places that have a bf16-MFMA form.  "fp32" (default): the fp32 MFMA
    flow everywhere.  "bf16": Q K^T, P V and the backward's products run on the bf16 MFMA with fp32 accumulation and an fp32 softmax
      * when qkv is STORED as bf16 (set_storage("bf16")): mumpy_window_attention_bf16mm_fwd instead of the widening
        mumpy_window_attention_bf16_fwd (inference forward);
      * on the TRAINING TAPE (autograd.WindowAttentionFn, so swin_block_train and the full training step): activations stay fp32 in
        memory, the operands are rounded to bf16 in registers -- window_attention_mm16 in the forward, window_attention_bwd(...,
        math="bf16") in the backward.  The mode is read in the tape's forward and carried to its backward.
    Direct ops.window_attention / ops.window_attention_bwd calls on fp32 qkv never follow the switch (window_attention_bwd takes an
    explicit math=), and set_storage does not touch it.  The initial value is the environment variable MUMPY_ATTN_MATH, read when
    this module is imported.  Like set_storage it is read at launch time: set it BEFORE a GraphedForward or a graphed training step
    is captured -- a captured graph keeps the kernels it was captured with."""
    global _ATTN_MATH
    _ATTN_MATH = _choice(mode, _ATTN_MATHS, _ATTN_WHAT)


def attention_math() -> str:
    return _ATTN_MATH


def set_cva_math(mode: str) -> None:
    """Arithmetic of the cross-view attention module (SwinDAttention).  "fp32" (default): the module's existing routes.  "bf16":
      * in the INFERENCE forward sample -> [k|v], the attention core and (in the cross block) proj_out -> combine run their bf16-MFMA
        kernels (deform_sample_kv / deform_attention / deform_out_combine with math="bf16");
      * on the TRAINING TAPE (autograd.DeformAttentionFn, so swin_dattention_train and the full training step) the attention core runs
        deform_attention(..., math="bf16") in the forward and deform_attention_bwd(..., math="bf16") in the backward.  The mode is read
        in the tape's forward and carried to its backward.  The tape's GEMMs (proj_q, k|v, proj_out) keep following set_matrix_math;
        the offset network and the sampling are untouched.
    All tensors stay fp32 in memory, the matrix operands are rounded to bf16 (nearest even) in registers or while staged, multiplied
    on v_mfma_f32_32x32x16_bf16 and accumulated in fp32; the bilinear sum, softmax, bias adds and residual terms stay fp32.
    Independent of set_matrix_math, set_storage and set_attention_math: none of them touches it and it touches none of them.  The ops
    never follow the switch by themselves (their math= defaults to "fp32").  The initial value is the environment variable
    MUMPY_CVA_MATH, read when this module is imported.  Read at launch time: set it BEFORE a GraphedForward or a graphed training step
    is captured -- a captured graph keeps the kernels it was captured with."""
    global _CVA_MATH
    _CVA_MATH = _choice(mode, _CVA_MATHS, _CVA_WHAT)


def cva_math() -> str:
    return _CVA_MATH


def set_clip_coupling(mode: str) -> None:
    """How the cross-view attention (SwinDAttention) pairs windows across the clips of a batch in the module's forward.
    "batch" (default): the reference's rule -- kv window i attends with q window i mod B1 (`x1.repeat`, deform:330), B1 counting the
    q windows of EVERY clip, so a clip's result depends on the batch it travels in.  "clip": the same rule applied inside each clip
    (groups = batch size on the grouped kernels, include/mumpy_hip_ext8.h): every clip is computed as the reference computes a batch
    of one, whatever the batch size, the order of the clips or the padding of a tail; the launches are the full-batch ones.
    For a batch of one, and wherever r = 1, the two coincide.  The ops never follow the switch by themselves (their groups= defaults
    to 1); the module does.  The training tape does NOT follow this switch: it trains the per-clip function by explicit argument,
    autograd.encoder_train(enc, x, coupling="clip") (the grouped backward entries of include/mumpy_hip_ext9.h), and its default
    call refuses to run while the switch says "clip" rather than differentiate another function than the one the forward computes.
    The initial value is the environment variable MUMPY_CLIP_COUPLING, read when this module is imported.  Read at launch
    time: a GraphedForward keeps the pairing it was captured with (its coupling= argument pins it)."""
    global _CLIP_COUPLING
    _CLIP_COUPLING = _choice(mode, _COUPLINGS, _COUPLING_WHAT)


def clip_coupling() -> str:
    return _CLIP_COUPLING


class clip_coupling_as:
    """`with ops.clip_coupling_as("clip"): ...` -- set_clip_coupling for the body; the previous value is restored on exit, also when
    the body raises.  None leaves the switch alone (the body follows whatever it says)."""

    def __init__(self, mode: Optional[str]):
        self.mode = _choice(mode, (None,) + _COUPLINGS, _COUPLING_WHAT)

    def __enter__(self):
        self.prev = _CLIP_COUPLING
        if self.mode is not None:
            set_clip_coupling(self.mode)
        return self

    def __exit__(self, *exc):
        set_clip_coupling(self.prev)
        return False


def cva_pairing(nkv: int, nq: int, groups: int = 1):
    """Host statement of the pairing rule of the cross-view attention kernels: -> (q_of_kv, out_of_kv), numpy int64 arrays of length
    nkv.  kv window i attends with q window q_of_kv[i] and is summed into output window out_of_kv[i] = i // r, r = nkv // nq.  The
    launch is cut into `groups` equal contiguous groups of nqg = nq // groups q windows and r nqg kv windows, and inside group
    g = i // (r nqg) the reference's rule holds: q = g nqg + (i - g r nqg) mod nqg.  groups = 1: i mod nq (deform:330)."""
    import numpy as np
    nkv, nq, groups = int(nkv), int(nq), int(groups)
    if nq < 1 or nkv < 1 or nkv % nq:
        raise ValueError(f"cva_pairing: {nkv} kv windows are not a positive multiple of {nq} q windows")
    if groups < 1 or nq % groups:
        raise ValueError(f"cva_pairing: groups={groups} must be at least 1 and divide the {nq} q windows")
    r, nqg = nkv // nq, nq // groups
    i = np.arange(nkv, dtype=np.int64)
    g = i // (r * nqg)
    return g * nqg + (i - g * r * nqg) % nqg, i // r


def cva_pairing_members(nkv: int, nq: int, groups: int = 1):
    """The inverse of cva_pairing, as the backward walks it: -> an (nq, r) numpy int64 array, row qw = the kv windows that attend with
    q window qw in the order their contributions to it are summed (ascending).  With nqg = nq // groups, g = qw // nqg and
    j = qw - g nqg, the m-th one is g r nqg + j + m nqg; groups = 1: qw + m nq."""
    import numpy as np
    nkv, nq, groups = int(nkv), int(nq), int(groups)
    if nq < 1 or nkv < 1 or nkv % nq:
        raise ValueError(f"cva_pairing_members: {nkv} kv windows are not a positive multiple of {nq} q windows")
    if groups < 1 or nq % groups:
        raise ValueError(f"cva_pairing_members: groups={groups} must be at least 1 and divide the {nq} q windows")
    r, nqg = nkv // nq, nq // groups
    qw = np.arange(nq, dtype=np.int64)[:, None]
    g = qw // nqg
    return g * (r * nqg) + (qw - g * nqg) + np.arange(r, dtype=np.int64)[None, :] * nqg


def set_mlp_fusion(on: bool) -> None:
    """The MLP of a transformer block ON THE TRAINING TAPE (autograd.MlpFn: the Swin, global and cross-view blocks).  Off (default):
    fc1, GELU, fc2 as three tape nodes -- five launches a step that touch the hidden tensor.  On: fc1 writes z and a = gelu(z) from one
    launch (linear_gelu_dual) and fc2's backward takes gelu'(z) into its dX product (linear_gelu_bwd): two launches fewer per MLP,
    the same arithmetic.  Follows set_matrix_math ("fp32" / "bf16"); under a split-precision mode, and under autograd.LEGACY_LINEAR_BWD,
    the tape keeps its unfused lines.  Independent of set_storage, set_attention_math and set_cva_math; the inference forward is
    untouched.  The initial value is the environment variable MUMPY_MLP_FUSED ("0" / "1"), read when this module is imported.  Read
    at launch time in the tape's forward and carried to its backward: set it BEFORE a graphed training step is captured."""
    global _MLP_FUSED
    if not isinstance(on, (bool, int)) or on not in (0, 1):
        raise ValueError(f"set_mlp_fusion: expected a bool, got {on!r}")
    _MLP_FUSED = bool(on)


def mlp_fusion() -> bool:
    return _MLP_FUSED


def _mm16(entry, math):
    """C-ABI entry of a cross-view attention op for math= "fp32" (the entry itself) or "bf16" (its _mm16 form)."""
    return entry.replace("_fwd", "_mm16_fwd") if _choice(math, _CVA_MATHS, _CVA_WHAT) == "bf16" else entry


def _window_attention(entry, chk, dtype, who, qkv, bias_pad, b, hs, w, c, shift, scale, mask_tab, mask_id, out=None):
    """One body for the window-attention forward entries: C-ABI entry name, input check (_chk / _chk16) and output dtype."""
    qkv = chk(qkv, "qkv")
    if qkv.numel() != b * hs * w * 3 * c:
        raise RuntimeError(f"{who}: qkv shape mismatch")
    out = torch.empty(b, hs * w, c, device=qkv.device, dtype=dtype) if out is None else _chk_exact(out, "out", dtype, (b, hs * w, c), who)
    bias_pad = _rd(bias_pad, "bias", (c // 32) * 64 * 64, who)
    mask_tab, mask_id, n_mask = _chk_mask(mask_tab, mask_id, b * (hs // 7) * (w // 7), who)
    _call(entry, _p(qkv), _p(out), _p(bias_pad), _p(mask_tab), _p(mask_id), n_mask,
          b, hs, w, c, shift, scale, _stream(), work=307328.0 * b * (hs // 7) * (w // 7) * (c // 32))
    return out


def _chk_mask(mask_tab, mask_id, nwin, who):
    """The shifted-window mask operands -> (mask_tab, mask_id, n_mask): mask_id int32 (the kernel reads mask_id[window % n_mask],
    4 bytes each: an int64 tensor would be read as pairs) with n_mask dividing the nwin windows of the launch (the broadcast of
    swin:155), mask_tab whole (64, 64) fp32 patterns.  How many patterns the ids refer to is device data: that the table holds them
    all is the word of compact_attn_mask."""
    if mask_id is None:
        if mask_tab is not None:
            raise RuntimeError(f"mumpy_hip: {who}: mask_tab needs mask_id")
        return None, None, 0
    n_mask = mask_id.numel()
    if n_mask < 1 or nwin % n_mask:
        raise RuntimeError(f"mumpy_hip: {who}: {n_mask} mask ids do not divide the {nwin} windows of the launch")
    mask_id = _rd(mask_id, "mask_id", n_mask, who, torch.int32)
    if mask_tab is None or mask_tab.numel() < 4096 or mask_tab.numel() % 4096:
        raise RuntimeError(f"mumpy_hip: {who} needs mask_tab (nU, 64, 64) with mask_id")
    return _rd(mask_tab, "mask_tab", mask_tab.numel(), who), mask_id, n_mask


def window_attention_bf16(qkv16, bias_pad, b, hs, w, c, shift, scale, mask_tab=None, mask_id=None, math=None):
    """bf16 qkv (B, hs*w, 3C) -> bf16 (B, hs*w, C).  math: None follows attention_math(); "fp32" / "bf16" force the fp32-flow /
    the bf16-MFMA kernel."""
    math = _ATTN_MATH if math is None else _choice(math, _ATTN_MATHS, _ATTN_WHAT)
    return _window_attention("mumpy_window_attention_bf16mm_fwd" if math == "bf16" else "mumpy_window_attention_bf16_fwd", _chk16,
                             torch.bfloat16, "window_attention_bf16", qkv16, bias_pad, b, hs, w, c, shift, scale, mask_tab, mask_id)


# ------------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta, eps=1e-5, out=None):
    x = _chk(x, "x")
    c = x.shape[-1]
    gamma, beta = _rd(gamma, "gamma", c, "layernorm"), _rd(beta, "beta", c, "layernorm")
    if out is None:
        out = torch.empty_like(x)
    else:
        _drop_ln_stats(_wr(out, "out", x.numel(), "layernorm"))
    _call("mumpy_layernorm_fwd", _p(x), _p(gamma), _p(beta), _p(out), x.numel() // c, c,
          eps, _stream(), work=8.0 * x.numel())
    return out


def linear(x, weight, bias=None, act=ACT_NONE, residual=None, out=None, emit_stats=False):
    """y = act(x @ weight.T + bias) + residual; weight (N,K) or a 1x1-conv kernel (N,K,1,1).
    emit_stats: y feeds a LayerNorm whose consumer can fold it (linear_ln): when the shape runs on the persistent kernel the
    epilogue also writes the per-tile row statistics, attached to the result as y._mumpy_ln_stats (else nothing happens)."""
    x = _chk(x, "x")
    weight = _chk(weight, "weight")
    n, k = weight.shape[0], weight.numel() // weight.shape[0]
    if x.shape[-1] != k:
        raise RuntimeError(f"linear: x has {x.shape[-1]} features, weight expects {k}")
    m = x.numel() // k
    if out is None:
        out = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float32)
    else:
        _drop_ln_stats(_wr(out, "out", m * n, "linear"))
    residual, bias = _rd_opt(residual, "residual", m * n, "linear"), _rd_opt(bias, "bias", n, "linear")
    if _in_background():
        _call("mumpy_linear_rd_fwd", _p(x), _p(weight), _p(bias), _p(residual), _p(out), m, n, k,
              act, _stream(), work=2.0 * m * n * k)
        return out
    wsb = _ws_bytes((m, n, k), "mumpy_linear_workspace_bytes", m, n, k)
    if emit_stats:
        # measured (tools/ln_fold_shapes.py, profiles/r03_ln_fold_shapes.txt): the statistics epilogue costs 4-5 us on a producer with
        # >= 16 chunks per tile (K >= 512) -- less than the LayerNorm launch it saves -- but 9-21 us on the short-K producers of
        # stages 0 / 1 (K = 128, 256: their epilogue waves are the bottleneck already), more than the launch
        gn = linear_ln_tiles(m, n, k) if k >= LN_FOLD_MIN_K else 0
        if gn:
            stats = torch.empty(m, gn, 2, device=x.device, dtype=torch.float32)
            ws = _kept_workspace(max(wsb, 4096), x.device)
            _call("mumpy_linear_lnx_fwd", _p(x), _p(weight), _p(bias), _p(residual), _p(out), m, n, k,
                  act, _p(ws), ws.numel() * 4, _p(stats), None, 0, None, 0.0, _stream(), work=2.0 * m * n * k)
            out._mumpy_ln_stats = stats
            return out
    ws = _kept_workspace(wsb, x.device) if wsb else None      # split-K slabs / the persistent kernel's flags + slabs
    _call("mumpy_linear_wsz_fwd", _p(x), _p(weight), _p(bias), _p(residual),
          _p(out), m, n, k, act | _MATH, _p(ws), 0 if ws is None else ws.numel() * 4, _stream(), work=2.0 * m * n * k)
    return out


# ---- "background" kernels (no LDS: resident beside the persistent GEMM, csrc/gemm_rd.hip) ---------------------------------------
_BACKGROUND = [0]
# Measured and NOT adopted (default off; profiles/r03_coresidency_probe.txt): the LDS-free GEMM is resident-compatible with the
# persistent kernel but two MFMA-bound kernels gain nothing from sharing a CU (together = sum on the two-stream probe), and alone
# it is slower than the tiled kernels -- the forward went 21.5 -> 23.3 ms with it.  MUMPY_BACKGROUND=1 turns it on for A/B runs.
BACKGROUND_ON = os.environ.get("MUMPY_BACKGROUND", "0") == "1"


class background:
    """Context manager for work that is forked beside a chain of large GEMMs (views 1 / 2 beside view 3 inside a pyramid stage):
    inside it, fp32 `linear` and `window_attention` launch their LDS-free forms (mumpy_linear_rd_fwd, mumpy_window_attention_bg_fwd),
    which can be resident on a CU whose whole LDS belongs to the persistent GEMM.  Same results; slower when run alone."""

    def __enter__(self):
        _BACKGROUND[0] += 1
        return self

    def __exit__(self, *exc):
        _BACKGROUND[0] -= 1
        return False


def _in_background():
    return _BACKGROUND[0] > 0 and BACKGROUND_ON and _MATH == MATH_FP32 and _STORAGE == "fp32"


# ---- LayerNorm folded into the GEMMs either side of it (mumpy_linear_lnx_fwd; swin:266,305 / blocks:86-88) -----------------
LN_FOLD = os.environ.get("MUMPY_LN_FOLD", "1") != "0"      # A/B switch
LN_FOLD_MIN_K = 512
_LN_TILES = {}


def linear_ln_tiles(m, n, k):
    """Column tiles of a shape whose fp32 launch runs on the persistent 128x128 kernel (the one that can emit / consume the
    per-tile LayerNorm statistics), else 0.  0 as well whenever folding is off or another arithmetic mode is active."""
    if not LN_FOLD or _MATH != MATH_FP32 or _STORAGE != "fp32":
        return 0
    key = (m, n, k)
    t = _LN_TILES.get(key)
    if t is None:
        t = _LN_TILES[key] = int(_lib().mumpy_linear_ln_tiles(m, n, k))
    return t


def ln_stats_of(x):
    """The per-tile row statistics the producing GEMM attached to x (linear(..., emit_stats=True)), or None."""
    return getattr(x, "_mumpy_ln_stats", None)


def linear_ln(x, stats, wg, colsum, bprime, eps, act=ACT_NONE):
    """y = act(LayerNorm(x) W^T + b) with the LayerNorm folded into the GEMM: x RAW, stats from the producer of x, wg = W diag(gamma),
    colsum = row sums of wg, bprime = W beta + b (see fold_ln_weights).  The caller checked linear_ln_tiles(m, n, k) > 0."""
    x, wg = _chk(x, "x"), _chk(wg, "wg")
    n, k = wg.shape
    if x.shape[-1] != k:
        raise RuntimeError(f"linear_ln: x has {x.shape[-1]} features, wg expects {k}")
    m = x.numel() // k
    if stats.dim() != 3 or stats.shape[0] != m or stats.shape[2] != 2 or stats.shape[1] < 1:
        raise RuntimeError(f"linear_ln: stats must be ({m}, tiles, 2), got {tuple(stats.shape)}")
    stats, colsum, bprime = _rd(stats, "stats", stats.numel(), "linear_ln"), _rd(colsum, "colsum", n, "linear_ln"), _rd(bprime, "bprime", n, "linear_ln")
    out = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float32)
    wsb = _ws_bytes((m, n, k), "mumpy_linear_workspace_bytes", m, n, k)
    ws = _kept_workspace(max(wsb, 4096), x.device)
    _call("mumpy_linear_lnx_fwd", _p(x), _p(wg), _p(bprime), None, _p(out), m, n, k, act, _p(ws), ws.numel() * 4, None,
          _p(stats), stats.shape[-2], _p(colsum), eps, _stream(), work=2.0 * m * n * k)
    return out


def fold_ln_weights(weight, bias, gamma, beta):
    """(W diag(gamma), its row sums, W beta + b) in fp32, formed in float64: the operands of linear_ln."""
    w64 = weight.detach().double()
    wg = w64 * gamma.detach().double()[None, :]
    bp = w64 @ beta.detach().double()
    if bias is not None:
        bp = bp + bias.detach().double()
    return wg.float().contiguous(), wg.sum(1).float().contiguous(), bp.float().contiguous()


_KEPT_WS = {}
_RETIRED_WS = []          # superseded workspaces: never freed (a captured hipGraph may have their address baked in)


def _kept_workspace(nbytes, device):
    """One zero-initialised workspace per (device, stream), grown on demand and kept: launches on one stream execute in
    order, so they can share it; the persistent GEMM's arrival flags (its first page) return to zero after every launch
    (mumpy_linear_wsz_fwd), so nothing has to be reset between launches.  Allocated outside any graph capture (the eager
    warm-up pass that precedes a capture creates the buffers the captured launches then point at).
    Lifetime: a workspace that is outgrown is RETIRED, not freed -- GraphedForward / GraphedTrainStep replays keep writing
    flags and slabs through the address they captured, so handing that memory back to the caching allocator would let a
    later tensor alias it.  (Two torch Stream objects with one raw handle are one HIP stream: sharing a workspace between
    them is the in-order case above; mumpy_hip.streams never hands out a side stream whose handle aliases its parent.)"""
    s = torch.cuda.current_stream(device)
    key = (str(device), s.cuda_stream)
    ws = _KEPT_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        if torch.cuda.is_current_stream_capturing():
            return torch.zeros(nbytes // 4, device=device, dtype=torch.float32)     # (captured fill: still correct, just not free)
        if ws is not None:
            _RETIRED_WS.append(ws)
        ws = _KEPT_WS[key] = torch.zeros(max(nbytes // 4, 1024), device=device, dtype=torch.float32)
    return ws


def check_workspaces():
    """Synchronising check of every kept workspace's sticky status word: raises if a split GEMM launch reported a part that
    never arrived (its output would be incomplete), after re-zeroing the workspaces so that the process can go on."""
    import ctypes
    bad = []
    for key, ws in list(_KEPT_WS.items()):
        st = ctypes.c_int(0)
        rc = _lib().mumpy_workspace_status(ws.data_ptr(), ctypes.byref(st))
        if rc:
            raise RuntimeError(f"mumpy_workspace_status failed (rc={rc}): {_lib().mumpy_last_error().decode()}")
        if st.value == -1:
            # LayerNorm-folding precision guard: a row with |mean| > 256 sigma went through the folded form (~1e-4 instead of ~1e-6
            # relative error on that row).  Results are complete; from here on this process takes the two-launch route.
            global LN_FOLD
            LN_FOLD = False
            ws.view(torch.int32)[1022] = 0
            import warnings
            warnings.warn("mumpy_hip: a folded LayerNorm met a row with |mean| > 256 sigma; LayerNorm folding is now off "
                          "(ops.LN_FOLD = False) -- re-capture any hipGraph to apply it")
        elif st.value:
            bad.append((key, st.value))
    if bad:
        reset_workspaces()
        raise RuntimeError(f"mumpy_hip: split GEMM launch(es) timed out waiting for a partial tile {bad}; results since the last "
                           "check are invalid (workspaces re-zeroed)")


def reset_workspaces():
    """Re-zero every kept workspace (arrival-flag pages included).  For use after a launch reported an error or was
    aborted mid-kernel: the persistent GEMM's flags are only guaranteed to be back at zero after a launch that completed."""
    for ws in list(_KEPT_WS.values()) + _RETIRED_WS:
        ws.zero_()


def linear_rows(x_view, weight, bias=None, residual=None, out=None):
    """Linear over a (nblk, rows, K) VIEW whose rows are contiguous but whose blocks are strided (no copy)."""
    if not x_view.is_cuda or x_view.dtype != torch.float32:
        raise RuntimeError("mumpy_hip: linear_rows needs a float32 GPU tensor (there is no CPU path)")
    nblk, rows, k = x_view.shape
    if x_view.stride(2) != 1 or x_view.stride(1) != k:
        raise RuntimeError("linear_rows: rows of a block must be contiguous")
    weight = _chk(weight, "weight")
    n = weight.shape[0]
    if weight.numel() != n * k:
        raise RuntimeError(f"linear_rows: x has {k} features, weight {tuple(weight.shape)}")
    m = nblk * rows
    bias, residual = _rd_opt(bias, "bias", n, "linear_rows"), _rd_opt(residual, "residual", m * n, "linear_rows")
    if out is None:
        out = torch.empty(m, n, device=x_view.device, dtype=torch.float32)
    else:
        _drop_ln_stats(_wr(out, "out", m * n, "linear_rows"))
    wsb = _ws_bytes((m, n, k), "mumpy_linear_workspace_bytes", m, n, k)
    ws = torch.empty(wsb // 4, device=x_view.device, dtype=torch.float32) if wsb else None
    _call("mumpy_linear_rows_fwd", _p(x_view), rows, x_view.stride(0), _p(weight),
          _p(bias), _p(residual), _p(out), m, n, k, ACT_NONE | _MATH, _p(ws), wsb, _stream(),
          work=2.0 * m * n * k)
    return out


def linear_time_slices(x4, weight, bias=None, residual=None):
    """x4 (B, T, n, C) contiguous, weight (N, T*C) with K index (t, c): y[(b, i), :] = sum_t x4[b, t, i, :] @ weight[:, t*C:(t+1)*C].T
    -- a Conv3d(k = s = (T,1,1)) head on channels-last tokens (decoder.py:62-66) in ONE launch (segmented-K rows mode)."""
    x4, weight = _chk(x4, "x"), _chk(weight, "weight")
    b, t, n, c = x4.shape
    nout, k = weight.shape
    if k != t * c or c % 32:
        raise RuntimeError(f"linear_time_slices: weight expects K = T*C = {t * c} (got {k}); C % 32 == 0")
    m = b * n
    out = torch.empty(m, nout, device=x4.device, dtype=torch.float32)
    residual, bias = _rd_opt(residual, "residual", m * nout, "linear_time_slices"), _rd_opt(bias, "bias", nout, "linear_time_slices")
    wsb = _ws_bytes((m, nout, k), "mumpy_linear_workspace_bytes", m, nout, k)
    ws = torch.empty(wsb // 4, device=x4.device, dtype=torch.float32) if wsb else None
    _call("mumpy_linear_rows_kseg_fwd", _p(x4), n, t * n * c, c, n * c, _p(weight), _p(bias),
          _p(residual), _p(out), m, nout, k, ACT_NONE | _MATH, _p(ws), wsb, _stream(), work=2.0 * m * nout * k)
    return out


def conv2d_nhwc(x, w_krsc, bias=None, act=ACT_NONE, residual=None):
    """x logical (B,Cin,H,W) with NHWC memory; w_krsc (Cout,kh,kw,Cin) contiguous; stride 1, same padding.
    Returns logical (B,Cout,H,W) with NHWC memory."""
    x = _nhwc(x, "x")
    b, cin, h, w = x.shape
    w_krsc = _chk(w_krsc, "weight")
    cout, kh, kw, cin2 = w_krsc.shape
    if cin2 != cin:
        raise RuntimeError(f"conv2d: input has {cin} channels, weight expects {cin2}")
    out = empty_nhwc(b, cout, h, w, x.device)
    if residual is not None:
        residual = _nhwc(residual, "residual")
        if tuple(residual.shape) != (b, cout, h, w):
            raise RuntimeError(f"conv2d: residual {tuple(residual.shape)} != output {(b, cout, h, w)}")
    bias = _rd_opt(bias, "bias", cout, "conv2d")
    wsb = _ws_bytes(("conv", b, h, w, cin, cout, kh, kw), "mumpy_conv2d_workspace_bytes", b, h, w, cin, cout, kh, kw)
    ws = torch.empty(wsb // 4, device=x.device, dtype=torch.float32) if wsb else None
    _call("mumpy_conv2d_nhwc_fwd", _p(x), _p(w_krsc), _p(bias), _p(residual), _p(out),
          b, h, w, cin, cout, kh, kw, act | _MATH, _p(ws), wsb, _stream(), work=2.0 * b * h * w * cout * kh * kw * cin)
    return out


def final_conv(x, w_krsc, bias, with_mask=False, thr=0.5):
    """x logical (B,C,H,W) NHWC, C a multiple of 32 -> logits (B,1,H,W) [, uint8 mask (B,1,H,W)]."""
    x = _nhwc(x, "x")
    b, c, h, w = x.shape
    if c % 32 or tuple(w_krsc.shape) != (1, 3, 3, c):
        raise RuntimeError(f"final_conv is built for Conv2d(32k, 1, 3, padding=1); got C={c}, weight {tuple(w_krsc.shape)}")
    logits = torch.empty(b, 1, h, w, device=x.device, dtype=torch.float32)
    mask = torch.empty(b, 1, h, w, device=x.device, dtype=torch.uint8) if with_mask else None
    w_krsc, bias = _chk(w_krsc, "weight"), _rd(bias, "bias", 1, "final_conv")
    _call("mumpy_final_conv_fwd", _p(x), _p(w_krsc), _p(bias), _p(logits), _p(mask), b, h, w, c, thr,
          _stream(), work=4.0 * (x.numel() + logits.numel()))
    return (logits, mask) if with_mask else logits


def _nhwc(t: torch.Tensor, name: str) -> torch.Tensor:
    """Logical (B,C,H,W) tensor whose memory is NHWC (torch.channels_last)."""
    if not t.is_cuda:
        raise RuntimeError(f"mumpy_hip: {name} is on {t.device}; the HIP kernels need a GPU tensor (there is no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"mumpy_hip: {name} must be a 4-D float32 tensor")
    b, c, h, w = t.shape
    if t.stride() != (h * w * c, 1, w * c, c):
        t = t.contiguous(memory_format=torch.channels_last)
        if t.stride() != (h * w * c, 1, w * c, c):           # degenerate sizes: force the exact NHWC strides
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


def empty_nhwc(b, c, h, w, device):
    return torch.empty(b, h, w, c, device=device, dtype=torch.float32).permute(0, 3, 1, 2)


ACT_RELU, ACT_SIGMOID = 1, 2
EP_NONE, EP_ADD_MUL, EP_MUL = 0, 1, 2


def gn_stats(x, groups):
    """x: logical (B,C,H,W), NHWC memory -> (partial, nsplit)."""
    x = _nhwc(x, "x")
    b, c, h, w = x.shape
    # 64 KB of the image per workgroup (16 dependent 16-byte loads per thread): the first rule (256 KB, at most 64 splits) left the
    # decoder's 28x28 .. 112x112 maps on 24-96 workgroups of 256 CUs, each walking 64 loads in sequence (19 us per launch)
    nsplit = max(1, min(256, (h * w * c) // 16384))
    partial = torch.empty(b, nsplit, groups, 2, device=x.device, dtype=torch.float32)
    _call("mumpy_gn_stats_nhwc_fwd", _p(x), _p(partial), b, h * w, c, groups, nsplit, _stream(), work=4.0 * x.numel())
    return x, partial, nsplit


def gn_apply_resample(x, gn=None, act=0, mean4=False, scale=1, align_corners=False, ep_mode=0, ep_a=None, ep_b=None,
                      out=None, out_coff=0):
    """x logical (B,C,H,W) NHWC.  gn = (partial, nsplit, gamma, beta, groups, eps) or None.  Returns logical NCHW / NHWC memory."""
    x = _nhwc(x, "x")
    b, c, h, w = x.shape
    cout = c // 4 if mean4 else c
    ho, wo = h * scale, w * scale
    if out is None:
        out = empty_nhwc(b, cout, ho, wo, x.device)
    else:
        ctot = out.shape[1] if out.dim() == 4 else -1
        if not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (b, ctot, ho, wo) or \
                out.stride() != (ho * wo * ctot, 1, wo * ctot, ctot) or out_coff < 0 or out_coff + cout > ctot:
            raise RuntimeError(f"mumpy_hip: gn_apply_resample writes out in place and needs a dense NHWC float32 GPU map ({b}, >= "
                               f"{out_coff + cout}, {ho}, {wo}), got {out.dtype} {tuple(out.shape)} strides {out.stride()} on {out.device}")
    if ep_a is not None:
        ep_a = _nhwc(ep_a, "ep_a")
        if tuple(ep_a.shape) != (b, cout, ho, wo):
            raise RuntimeError(f"gn_apply_resample: epilogue operand {tuple(ep_a.shape)} != output {(b, cout, ho, wo)}")
    if ep_b is not None:
        ep_b = _nhwc(ep_b, "ep_b")
        if tuple(ep_b.shape) != (b, cout, ho, wo):
            raise RuntimeError(f"gn_apply_resample: epilogue operand {tuple(ep_b.shape)} != output {(b, cout, ho, wo)}")
    partial, nsplit, gamma, beta, groups, eps = gn if gn is not None else (None, 0, None, None, 1, 0.0)
    if gn is not None:
        partial = _rd(partial, "partial", b * nsplit * groups * 2, "gn_apply_resample")
        gamma, beta = _rd(gamma, "gamma", c, "gn_apply_resample"), _rd(beta, "beta", c, "gn_apply_resample")
    _call("mumpy_gn_apply_resample_nhwc_fwd", _p(x), _p(partial), nsplit, _p(gamma), _p(beta), groups, eps, act,
          1 if mean4 else 0, scale, 1 if align_corners else 0, ep_mode, _p(ep_a), _p(ep_b), _p(out), out.shape[1], out_coff,
          b, h, w, c, _stream(), work=4.0 * (x.numel() + b * cout * ho * wo))
    return out


def avgpool2_pad(x, cpad=None, nchw_in=False):
    """2x2 average pooling -> logical (B,Cpad,H/2,W/2) with NHWC memory; channels [C,Cpad) are zero.  x: logical (B,C,H,W) with
    NHWC memory, or (nchw_in) a contiguous NCHW tensor such as the FAF output."""
    if nchw_in:
        x = _chk(x, "x")
    else:
        x = _nhwc(x, "x")
    b, c, h, w = x.shape
    cpad = c if cpad is None else cpad
    out = empty_nhwc(b, cpad, h // 2, w // 2, x.device)
    _call("mumpy_avgpool2_pad_nhwc_fwd", _p(x), _p(out), b, h, w, c, cpad, 1 if nchw_in else 0, _stream(),
          work=4.0 * (x.numel() + out.numel()))
    return out


def copy_rows(src, src_stride, dst, dst_stride, rows, cols):
    """dst[r, :cols] = src[r, :cols] for r < rows, row pitches in floats; src / dst are tensors whose data_ptr() is row 0."""
    if not (src.is_cuda and dst.is_cuda and src.dtype == dst.dtype == torch.float32):
        raise RuntimeError("mumpy_hip: copy_rows needs float32 GPU tensors (there is no CPU path)")
    for name, t, pitch in (("src", src, src_stride), ("dst", dst, dst_stride)):
        if t.numel() > 1 and not any(st == 1 for sz, st in zip(t.shape, t.stride()) if sz > 1):
            raise RuntimeError(f"mumpy_hip: copy_rows: {name} has no dense dimension (strides {t.stride()}): its rows are not contiguous")
        if rows < 1 or cols < 1 or pitch < cols or t.storage_offset() + (rows - 1) * pitch + cols > t.untyped_storage().nbytes() // 4:
            raise RuntimeError(f"mumpy_hip: copy_rows: {rows} rows of {cols} floats at a pitch of {pitch} do not fit into {name}'s storage")
    _drop_ln_stats(dst)
    _call("mumpy_copy_rows_fwd", _p(src), src_stride, _p(dst), dst_stride, rows, cols, _stream(), work=8.0 * rows * cols)
    return dst


def set_channels(dst, coff, src):
    """dst[:, coff:coff+C] = src for logical (B,*,H,W) tensors with NHWC memory (a slice of a channel-concatenated map).
    src may be any per-pixel-contiguous strided view whose pixels are uniformly pitched (e.g. the first 3 of 5 temporal slices)."""
    b, c, h, w = src.shape
    ctot = dst.shape[1]
    if dst.stride() != (h * w * ctot, 1, w * ctot, ctot) or tuple(dst.shape[2:]) != (h, w) or dst.shape[0] != b or coff < 0 or coff + c > ctot:
        raise RuntimeError("set_channels: dst must be a dense NHWC map of the same batch and size that holds channels [coff, coff + C)")
    _drop_ln_stats(dst)
    pitch = src.stride(3)
    if src.stride(1) != 1 or src.stride(2) != w * pitch or (b > 1 and src.stride(0) != h * w * pitch) or pitch < c:
        src = _nhwc(src, "src")
        pitch = c
    return copy_rows(src, pitch, dst[:, coff:], ctot, b * h * w, c)


def merge_views(views, token_t, n=49):
    """[(B, t_v * n, C_v)] x 3 -> ((B n T), sum C_v): the channel merge in front of the global embedding (mTVE:710-718, 739)."""
    v = [_chk(t, "view") for t in views]
    b = v[0].shape[0]
    tmax = max(token_t)
    if len(v) != 3 or any(t.dim() != 3 or t.shape[0] != b or t.shape[1] != tv * n for t, tv in zip(v, token_t)):
        raise RuntimeError(f"merge_views: three views (B, t_v * {n}, C_v) of one batch, got {[tuple(t.shape) for t in v]} for t_v = {list(token_t)}")
    out = torch.empty(b * n * tmax, sum(t.shape[2] for t in v), device=v[0].device, dtype=torch.float32)
    _call("mumpy_merge_views_fwd", _p(v[0]), _p(v[1]), _p(v[2]), _p(out), b, tmax, n, v[0].shape[2], v[1].shape[2], v[2].shape[2],
          token_t[0], token_t[1], token_t[2], _stream(), work=8.0 * out.numel())
    return out


def trunk_head(g, f, gcn, freq):
    """gcn * freq + PixelShuffle(2)(g * f): g, f logical (B,4C,h,w), gcn, freq (B,C,2h,2w), all NHWC memory (decoder.py:198-205)."""
    g, f, gcn, freq = _nhwc(g, "g"), _nhwc(f, "f"), _nhwc(gcn, "gcn"), _nhwc(freq, "freq")
    b, c4, h, w = g.shape
    c = c4 // 4
    if f.shape != g.shape or tuple(gcn.shape) != (b, c, 2 * h, 2 * w) or freq.shape != gcn.shape:
        raise RuntimeError("trunk_head: shape mismatch")
    z = empty_nhwc(b, c, 2 * h, 2 * w, g.device)
    _call("mumpy_trunk_head_fwd", _p(g), _p(f), _p(gcn), _p(freq), _p(z), b, h, w, c, _stream(), work=4.0 * (2 * g.numel() + 3 * z.numel()))
    return z


def add(a, b, out=None):
    a = _chk(a, "a")
    b = _rd(b, "b", a.numel(), "add")
    if out is None:
        out = torch.empty_like(a)
    else:
        _drop_ln_stats(_wr(out, "out", a.numel(), "add"))
    _call("mumpy_add_fwd", _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def rel_index32(index: torch.Tensor) -> torch.Tensor:
    """The (49*49,) int32 image of a `relative_position_index` buffer on its device, kept ON the buffer object (the buffer is a
    constant of the model; the conversion used to be two launches per W-MSA call of a training step).  A module moved with
    `.to(device)` gets new buffer objects, hence a fresh image."""
    t = getattr(index, "_mumpy_i32", None)
    if t is None or t.device != index.device or getattr(index, "_mumpy_i32_version", -1) != index._version:
        t = index.to(torch.int32).reshape(-1).contiguous()
        index._mumpy_i32, index._mumpy_i32_version = t, index._version
    return t


def expand_relpos_bias(table: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """relative_position_bias_table (169,nH) + relative_position_index (49,49) -> (nH,64,64) padded bias
    [head][query][key]: rows >= 49 zero, key columns >= 49 = -1e30 (swin:148-151).  One launch
    (mumpy_relpos_bias_expand_fwd)."""
    table = _chk(table, "table")
    nh = table.shape[1]
    if not index.is_cuda:
        index = index.to(table.device)
    idx = index if index.dtype == torch.int32 and index.dim() == 1 else rel_index32(index)
    idx = _rd(idx, "index", 49 * 49, "expand_relpos_bias", torch.int32)
    if table.dim() != 2 or table.shape[0] != 169:
        raise RuntimeError(f"expand_relpos_bias: table must be (169, nH), got {tuple(table.shape)}")
    out = torch.empty(nh, 64, 64, device=table.device, dtype=torch.float32)
    _call("mumpy_relpos_bias_expand_fwd", _p(table), _p(idx), _p(out), nh, _stream())
    return out


_PAD_MASK = {}


def pad_mask(device=None) -> torch.Tensor:
    """(1,64,64) key-padding mask of the deformable attention (0 / -1e30 on key columns >= 49); cached per device."""
    if device is None:
        m = torch.zeros(1, 64, 64, dtype=torch.float32)
        m[:, :, 49:] = NEG
        return m
    key = str(device)
    if key not in _PAD_MASK:
        _PAD_MASK[key] = pad_mask().to(device)
    return _PAD_MASK[key]


def compact_attn_mask(mask: torch.Tensor):
    """attn_mask (nW,49,49) of 0/-100 (swin:252) -> (mask_tab (nU,64,64), mask_id (nW) int32, -1 = all-zero)."""
    m = mask.detach().float().cpu().reshape(mask.shape[0], -1)
    uniq, inv = torch.unique(m, dim=0, return_inverse=True)
    nz = [i for i in range(uniq.shape[0]) if bool((uniq[i] != 0).any())]
    remap = torch.full((uniq.shape[0],), -1, dtype=torch.int32)
    for j, i in enumerate(nz):
        remap[i] = j
    tab = torch.zeros(max(len(nz), 1), 64, 64)
    for j, i in enumerate(nz):
        tab[j, :49, :49] = uniq[i].reshape(49, 49)
    return tab.to(mask.device), remap[inv].to(torch.int32).to(mask.device)


def window_attention(qkv, bias_pad, b, hs, w, c, shift, scale, mask_tab=None, mask_id=None, out=None):
    """qkv (B, hs*w, 3C) raster -> (B, hs*w, C) raster attention output (before proj)."""
    return _window_attention("mumpy_window_attention_bg_fwd" if _in_background() else "mumpy_window_attention_fwd", _chk, torch.float32,
                             "window_attention", qkv, bias_pad, b, hs, w, c, shift, scale, mask_tab, mask_id, out)


def window_attention_mm16(qkv, bias_pad, b, hs, w, c, shift, scale, mask_tab=None, mask_id=None, out=None):
    """window_attention with bf16 matrix math on fp32 storage: q / k / v are rounded to bf16 in registers, both products run on the
    bf16 MFMA (fp32 accumulation, fp32 softmax), the fp32 output is stored unrounded.  The forward of the training tape under
    set_attention_math("bf16"); its backward is window_attention_bwd(..., math="bf16")."""
    return _window_attention("mumpy_window_attention_mm16_fwd", _chk, torch.float32, "window_attention_mm16", qkv, bias_pad, b, hs, w, c,
                             shift, scale, mask_tab, mask_id, out)


def deform_offsets(q, dw_w, dw_b, ln_g, ln_b, pw_w, b, h, w, c):
    who = "deform_offsets"
    q = _rd(q, "q", b * h * w * c, who)
    nwin = b * (h // 7) * (w // 7)
    cg = c // 3                                                           # the offset network works per group of C / 3 channels
    dw_w, dw_b = _rd(dw_w, "dw_w", cg * 25, who), _rd(dw_b, "dw_b", cg, who)
    ln_g, ln_b, pw_w = _rd(ln_g, "ln_g", cg, who), _rd(ln_b, "ln_b", cg, who), _rd(pw_w, "pw_w", 2 * cg, who)
    pos = torch.empty(nwin, 3, 49, 2, device=q.device, dtype=torch.float32)
    _call("mumpy_deform_offsets_fwd", _p(q), _p(dw_w), _p(dw_b), _p(ln_g),
          _p(ln_b), _p(pw_w), _p(pos), b, h, w, c, _stream())
    return pos


def _grouped(entry, groups, b, nq, who):
    """-> (C-ABI entry, trailing arguments before the stream) of a cross-view attention op for groups = 1 (the frozen entry, called
    exactly as before there was a grouped one) or more (its _grouped form, include/mumpy_hip_ext8.h).  The refusals are the
    library's, restated here so that a bad grouping never reaches a launch."""
    if not isinstance(groups, int) or isinstance(groups, bool) or groups < 1 or nq % groups or b % groups:
        raise ValueError(f"{who}: groups={groups!r} must be a positive int that divides the {nq} q windows and the batch {b}")
    return (entry, ()) if groups == 1 else (entry.replace("_fwd", "_grouped_fwd"), (groups,))


def deform_sample(x2, pos, b, hs2, w, c, nq, groups=1):
    """groups: the pairing rule (cva_pairing): 1 is the reference's `i mod nq`, b is per-clip pairing."""
    entry, extra = _grouped("mumpy_deform_sample_fwd", groups, b, nq, "deform_sample")
    x2, pos = _rd(x2, "x2", b * hs2 * w * c, "deform_sample"), _rd(pos, "pos", nq * 3 * 49 * 2, "deform_sample")
    nw2 = b * (hs2 // 7) * (w // 7)
    out = torch.empty(nw2, 49, c, device=x2.device, dtype=torch.float32)
    _call(entry, _p(x2), _p(pos), _p(out), b, hs2, w, c, nq, *extra, _stream(),
          work=4.0 * (2 * nw2 * 49 * c + nw2 * 3 * 49 * 2))       # bytes: read kv once, write sampled once, read offsets
    return out


def deform_sample_kv(x2, pos, wkv, bkv, b, hs2, w, c, nq, math="fp32", groups=1):
    """[proj_k | proj_v] of the bilinearly sampled kv windows in one launch (the sampled map is never materialised).
    math="bf16": the fp32 sample and wkv are rounded to bf16 while staged and multiplied on the bf16 MFMA (see set_cva_math).
    groups: the pairing rule (cva_pairing): 1 is the reference's `i mod nq`, b is per-clip pairing."""
    who = "deform_sample_kv"
    entry, extra = _grouped(_mm16("mumpy_deform_sample_kv_fwd", math), groups, b, nq, who)
    x2, pos = _rd(x2, "x2", b * hs2 * w * c, who), _rd(pos, "pos", nq * 3 * 49 * 2, who)
    wkv, bkv = _rd(wkv, "wkv", 2 * c * c, who), _rd(bkv, "bkv", 2 * c, who)
    nw2 = b * (hs2 // 7) * (w // 7)
    kv = torch.empty(nw2, 49, 2 * c, device=x2.device, dtype=torch.float32)
    _call(entry, _p(x2), _p(pos), _p(wkv), _p(bkv), _p(kv), b, hs2, w, c, nq, *extra,
          _stream(), work=2.0 * nw2 * 49 * 2 * c * c)
    return kv


def deform_out_combine(o, wout, bout, x1, b, h, w, c, math="fp32"):
    """x1 + x1[window order] + scrambled proj_out(o) in one launch (replaces linear + deform_combine).
    math="bf16": wout and o are rounded to bf16 while staged and multiplied on the bf16 MFMA; the epilogue stays fp32."""
    entry = _mm16("mumpy_deform_out_combine_fwd", math)
    who = "deform_out_combine"
    o, x1 = _rd(o, "o", b * h * w * c, who), _rd(x1, "x1", b * h * w * c, who)
    wout, bout = _rd(wout, "wout", c * c, who), _rd(bout, "bout", c, who)
    out = torch.empty_like(x1)
    _call(entry, _p(o), _p(wout), _p(bout), _p(x1), _p(out), b, h, w, c, _stream(),
          work=2.0 * o.numel() * c)
    return out


def deform_attention(q, kv, padmask, b, h, w, c, r, scale, math="fp32", groups=1):
    """Cross-view attention core + r-tuple sum.  math is explicit and defaults to "fp32" whatever set_cva_math says: the callers that
    follow the switch (the module's inference forward, and the training tape's DeformAttentionFn, which carries the mode to its
    backward) pass it.  math="bf16": q / k / v rounded to bf16 in registers, both products on the bf16 MFMA, fp32 softmax and
    accumulation; its backward is deform_attention_bwd(..., math="bf16").  groups: the pairing rule (cva_pairing): 1 is the
    reference's `i mod B1`, b is per-clip pairing; the backward is deform_attention_bwd(..., groups=groups)."""
    b1w = b * (h // 7) * (w // 7)
    entry, extra = _grouped(_mm16("mumpy_deform_attention_fwd", math), groups, b, b1w, "deform_attention")
    q, kv = _rd(q, "q", b * h * w * c, "deform_attention"), _rd(kv, "kv", b1w * r * 49 * 2 * c, "deform_attention")
    padmask = _rd(padmask, "padmask", 64 * 64, "deform_attention")
    out = torch.empty(b1w, 49, c, device=q.device, dtype=torch.float32)
    _call(entry, _p(q), _p(kv), _p(padmask), _p(out), b, h, w, c, r, scale, *extra,
          _stream(), work=307328.0 * b1w * r * (c // 32))
    return out


def deform_combine(x1, yt, b, h, w, c):
    x1, yt = _rd(x1, "x1", b * h * w * c, "deform_combine"), _rd(yt, "yt", b * h * w * c, "deform_combine")
    out = torch.empty_like(x1)
    _call("mumpy_deform_combine_fwd", _p(x1), _p(yt), _p(out), b, h, w, c, _stream())
    return out


def faf(x, d, dt, frame, lo_hi, mid_lo, mid_hi):
    x = _chk(x, "x")
    b, t = x.shape[0], x.shape[1]
    if tuple(x.shape[2:]) != (3, 224, 224):
        raise RuntimeError(f"faf: expects (B,T,3,224,224) clips (dct.py:57,72), got {tuple(x.shape)}")
    scratch = torch.empty(b, 3, 224, 224, device=x.device, dtype=torch.float32)
    out = torch.empty(b, 9, 224, 224, device=x.device, dtype=torch.float32)
    d, dt = _rd(d, "D", 224 * 224, "faf"), _rd(dt, "Dt", 224 * 224, "faf")
    _call("mumpy_faf_fwd", _p(x), _p(d), _p(dt), _p(scratch), _p(out), b, t, frame, lo_hi, mid_lo,
          mid_hi, _stream())
    return out


# ---------------------------------------------------------------------------------------------- input-clip gradients (mumpy_hip_ext10.h)
def faf_bwd(dout, d, dt, lo_hi, mid_lo, mid_hi, out=None):
    """The gradient of `faf` with respect to the frame it read: dout (B,9,224,224) -> dxf (B,3,224,224)
    = D^T (sum_band M_band o (D dout[band,rgb] D^T)) D.  Two launches, deterministic."""
    if dout.dim() != 4 or tuple(dout.shape[1:]) != (9, 224, 224) or dout.shape[0] < 1:
        raise RuntimeError(f"faf_bwd: expects dout (B,9,224,224), got {tuple(dout.shape)}")
    b = dout.shape[0]
    dout = _rd(dout, "dout", b * 9 * 224 * 224, "faf_bwd")
    d, dt = _rd(d, "D", 224 * 224, "faf_bwd"), _rd(dt, "Dt", 224 * 224, "faf_bwd")
    scratch = torch.empty(b, 3, 224, 224, device=dout.device, dtype=torch.float32)
    out = torch.empty(b, 3, 224, 224, device=dout.device, dtype=torch.float32) if out is None else \
        _wr(out, "out", b * 3 * 224 * 224, "faf_bwd")
    _call("mumpy_faf_bwd", _p(dout), _p(d), _p(dt), _p(scratch), _p(out), b, int(lo_hi), int(mid_lo), int(mid_hi), _stream(),
          work=2.0 * 224 ** 3 * 2 * 4 * 3 * b)
    return out


def tokenize_dx(dcols, tubelets, b, t, h, w, dxf=None, frame=1, out=None):
    """One launch: the three views' column gradients (+ the FAF gradient of frame `frame`) -> dx (B,T,3,H,W).  dcols[v]: a 2-D
    (B * tt_v * (H/4) * (W/4), ld_v) matrix with columns (ch, t, py, px), tt_v = (T - t_v) // t_v + 1, ld_v >= 48 t_v (the padded K; the
    pad columns are not read).  Every element of dx is written; frames a view's tubelets do not reach get nothing from it."""
    if len(dcols) != 3 or len(tubelets) != 3:
        raise RuntimeError("tokenize_dx: needs the column gradients and tubelet lengths of three views")
    b, t, h, w, frame = int(b), int(t), int(h), int(w), int(frame)
    if b < 1 or t < 1 or h < 4 or w < 4 or h % 4 or w % 4:
        raise RuntimeError(f"tokenize_dx: bad sizes B={b} T={t}, {h}x{w} (H and W must be positive multiples of 4)")
    cols, lds = [], []
    for v, (c, tv) in enumerate(zip(dcols, tubelets)):
        tv = int(tv)
        if not 1 <= tv <= t:
            raise RuntimeError(f"tokenize_dx: tubelet {tv} of view {v} outside [1, T={t}]")
        rows = b * ((t - tv) // tv + 1) * (h // 4) * (w // 4)
        if c.dim() != 2 or c.shape[0] != rows or c.shape[1] < 48 * tv or c.shape[1] % 4:
            raise RuntimeError(f"tokenize_dx: view {v} needs dcols of shape ({rows}, ld >= {48 * tv}, ld % 4 == 0), got {tuple(c.shape)}")
        cols.append(_rd(c, f"dcols[{v}]", rows * c.shape[1], "tokenize_dx"))
        lds.append(int(c.shape[1]))
    if dxf is not None:
        if not 0 <= frame < t:
            raise RuntimeError(f"tokenize_dx: frame {frame} outside clip of {t}")
        dxf = _rd(dxf, "dxf", b * 3 * h * w, "tokenize_dx")
    out = torch.empty(b, t, 3, h, w, device=cols[0].device, dtype=torch.float32) if out is None else \
        _wr(out, "out", b * t * 3 * h * w, "tokenize_dx")
    _call("mumpy_tokenize_dx", _p(cols[0]), _p(cols[1]), _p(cols[2]), _p(dxf), _p(out), b, t, h, w, int(tubelets[0]), int(tubelets[1]),
          int(tubelets[2]), lds[0], lds[1], lds[2], frame, _stream(), work=4.0 * out.numel() * 4)
    return out


def pgd_step(x_adv, g, x0, alpha, eps3, lo3, hi3):
    """One projected signed-gradient step IN PLACE on x_adv (..., 3, H, W):
    x_adv <- clamp(clamp(x_adv + alpha * sgn(g), x0 - eps_c, x0 + eps_c), lo_c, hi_c), per channel c, in fp32 in this order.
    sgn(0) = 0, a NaN gradient counts as 0, +-inf as +-1; alpha may be negative.  eps3 / lo3 / hi3: three host floats each
    (mumpy_hip.inputgrad.pgd_bounds).  Returns x_adv."""
    import ctypes
    import math
    if x_adv.dim() < 3 or x_adv.shape[-3] != 3:
        raise RuntimeError(f"pgd_step: expects clips (..., 3, H, W), got {tuple(x_adv.shape)}")
    n, hw = x_adv.numel(), x_adv.shape[-1] * x_adv.shape[-2]
    if hw < 1:
        raise RuntimeError(f"pgd_step: empty planes in {tuple(x_adv.shape)}")
    x_adv = _wr(x_adv, "x_adv", n, "pgd_step")
    g, x0 = _rd(g, "g", n, "pgd_step"), _rd(x0, "x0", n, "pgd_step")
    eps3, lo3, hi3 = [tuple(float(v) for v in a) for a in (eps3, lo3, hi3)]
    if len(eps3) != 3 or len(lo3) != 3 or len(hi3) != 3 or not all(e >= 0.0 for e in eps3) or not all(l <= h for l, h in zip(lo3, hi3)):
        raise RuntimeError(f"pgd_step: needs three eps >= 0 and three lo <= hi, got {eps3}, {lo3}, {hi3}")
    if not math.isfinite(alpha):
        raise RuntimeError(f"pgd_step: alpha must be finite, got {alpha}")
    f3 = ctypes.c_float * 3
    _call("mumpy_pgd_step", _p(x_adv), _p(g), _p(x0), n, hw, float(alpha), f3(*eps3), f3(*lo3), f3(*hi3), _stream(), work=16.0 * n)
    return x_adv


def patch_embed(x, wt, bias, gamma, beta, t, eps=1e-5):
    """x (B,T,3,H,W), wt (48t, C) -> (B, t_out*H/4*W/4, C)."""
    x = _chk(x, "x")
    b, tt, _, h, w = x.shape
    if wt.dim() != 2 or wt.shape[0] != 48 * t or x.shape[2] != 3:
        raise RuntimeError(f"patch_embed: x (B,T,3,H,W) and wt (48 t, C) for t = {t}, got {tuple(x.shape)} and {tuple(wt.shape)}")
    c = wt.shape[1]
    wt, bias = _rd(wt, "wt", 48 * t * c, "patch_embed"), _rd(bias, "bias", c, "patch_embed")
    gamma, beta = _rd(gamma, "gamma", c, "patch_embed"), _rd(beta, "beta", c, "patch_embed")
    t_out = (tt - t) // t + 1
    out = torch.empty(b, t_out * (h // 4) * (w // 4), c, device=x.device, dtype=torch.float32)
    _call("mumpy_patch_embed_fwd", _p(x), _p(wt), _p(bias), _p(gamma),
          _p(beta), _p(out), b, tt, h, w, t, c, eps, _stream())
    return out


def patch_merge_ln(x, gamma, beta, b, hs, w, c, eps=1e-5):
    x = _rd(x, "x", b * hs * w * c, "patch_merge_ln")
    gamma, beta = _rd(gamma, "gamma", 4 * c, "patch_merge_ln"), _rd(beta, "beta", 4 * c, "patch_merge_ln")
    out = torch.empty(b, (hs // 2) * (w // 2), 4 * c, device=x.device, dtype=torch.float32)
    _call("mumpy_patch_merge_ln_fwd", _p(x), _p(gamma), _p(beta), _p(out), b, hs, w, c, eps,
          _stream())
    return out


def temporal_attention(qkv, s, t, c, heads, scale, tq=None):
    """tq: number of leading temporal tokens that are queries (default all): out (s, tq, c)."""
    qkv = _rd(qkv, "qkv", s * t * 3 * c, "temporal_attention")
    tq = t if tq is None else tq
    out = torch.empty(s, tq, c, device=qkv.device, dtype=torch.float32)
    _call("mumpy_temporal_attention_q_fwd", _p(qkv), _p(out), s, t, tq, c, heads, scale, _stream())
    return out


def attention_probs(q, k, outer, heads, nq, nk, d, q_strides, k_strides, scale, q_mod=None):
    """softmax(scale * q k^T) maps (outer, heads, nq, nk) for the `return_attention=True` variants; q_strides / k_strides =
    (outer stride, row stride) in floats, head h adds h * d; q_mod: q outer index = outer % q_mod."""
    for t in (q, k):                      # views into a larger tensor are fine: addressing is by the strides given (no copy)
        if not t.is_cuda or t.dtype != torch.float32 or t.stride(-1) != 1:
            raise RuntimeError("mumpy_hip: attention_probs needs float32 GPU tensors with a dense last dimension (there is no CPU path)")
    q_outer = outer if q_mod is None else q_mod
    for name, t, rows, n_outer, st in (("q", q, nq, q_outer, q_strides), ("k", k, nk, outer, k_strides)):
        last = (n_outer - 1) * st[0] + (rows - 1) * st[1] + heads * d          # one past the last float the launch reads, from data_ptr()
        if min(st) < 0 or t.storage_offset() + last > t.untyped_storage().nbytes() // 4:
            raise RuntimeError(f"mumpy_hip: attention_probs: the strides given reach past the end of {name}'s storage")
    out = torch.empty(outer, heads, nq, nk, device=q.device, dtype=torch.float32)
    _call("mumpy_attention_probs_fwd", _p(q), _p(k), _p(out), outer, heads, nq, nk, d, q_strides[0], q_strides[1], k_strides[0],
          k_strides[1], outer if q_mod is None else q_mod, scale, _stream())
    return out


def sigmoid_threshold(logits, thr=0.5):
    logits = _chk(logits, "logits")
    mask = torch.empty(logits.shape, device=logits.device, dtype=torch.uint8)
    _call("mumpy_sigmoid_threshold_fwd", _p(logits), _p(mask), logits.numel(), thr, _stream())
    return mask


EVAL_MEAN, EVAL_STD = (0.4776, 0.479, 0.4465), (0.230, 0.2085, 0.2324)      # test.py:23-24


_NEAREST_TABLES = {}


def _nearest_table(src: int, dst: int, device) -> torch.Tensor:
    """Pillow's NEAREST source indices for a src -> dst resize (built by the library's host helper, cached on the device)."""
    import ctypes
    key = (src, dst, str(device))
    t = _NEAREST_TABLES.get(key)
    if t is None:
        host = (ctypes.c_int32 * dst)()
        rc = _lib().mumpy_resize_nearest_table(src, dst, host)
        if rc:
            raise RuntimeError(f"mumpy_resize_nearest_table failed ({rc}): {_lib().mumpy_last_error().decode()}")
        t = _NEAREST_TABLES[key] = torch.tensor(list(host), dtype=torch.int32, device=device)
    return t


def normalize_u8(frames, mean=EVAL_MEAN, std=EVAL_STD, size=None):
    """frames (..., H, W, 3) uint8 on the GPU -> (..., 3, H, W) float32, ToTensor + Normalize (test.py:22-25).
    size=(H_out, W_out): the loader's `img.resize(inputRes)` (universaldataset.py:75-79, PIL NEAREST as in the pinned
    pillow==4.0.0) runs in the same kernel, e.g. size=(224, 224) for 432x240 footage."""
    import ctypes
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.shape[-1] != 3:
        raise RuntimeError("mumpy_hip: normalize_u8 needs a uint8 GPU tensor (..., H, W, 3) (there is no CPU path)")
    frames = frames.contiguous()
    lead, (h, w) = frames.shape[:-3], frames.shape[-3:-1]
    n = 1
    for d in lead:
        n *= d
    if size is not None and tuple(size) != (h, w):
        ho, wo = size
        out = torch.empty(*lead, 3, ho, wo, device=frames.device, dtype=torch.float32)
        m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        ytab, xtab = _nearest_table(h, ho, frames.device), _nearest_table(w, wo, frames.device)
        _call("mumpy_resize_normalize_u8_fwd", _p(frames), _p(out), _p(ytab), _p(xtab), n, h, w, ho, wo, m3, s3, _stream(),
              work=float(5 * out.numel()))
        return out
    out = torch.empty(*lead, 3, h, w, device=frames.device, dtype=torch.float32)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _call("mumpy_normalize_u8_fwd", _p(frames), _p(out), n, h, w, m3, s3, _stream(), work=float(frames.numel() + 4 * out.numel()))
    return out


def _chk_exact(t, name, dtype, shape, who="augment_stage_u8"):
    """A buffer the kernel reads or writes where it is: never copied, so anything that would need a copy is an error."""
    if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"mumpy_hip: {who} needs {name} as a contiguous {dtype} GPU tensor of shape {tuple(shape)}, "
                           f"got {t.dtype} {tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ' (not contiguous)'}")
    return t


def augment_stage_u8(frames, tab_a, tab_b, swap, masks=None, out=None, target=None, mean=EVAL_MEAN, std=EVAL_STD):
    """The training input stage in one launch (mumpy_augment_stage_u8_fwd, include/mumpy_hip_ext3.h): frames (nclips, T, Hs, Ws, 3)
    uint8 -> (nclips, T, 3, L, L) float32, gathered through the per-clip tables tab_a / tab_b (nclips, L) int32 and swap (nclips)
    int32 of mumpy_hip.augment.clip_tables (resize + flip / rotation + crop), then ToTensor + Normalize as normalize_u8.
    masks (nmasks, Hs, Ws) uint8: also -> target (nclips, L * L) float32 = (mask c % nmasks, gathered) > 0; returns (out, target).
    out= / target= are written in place and must be contiguous float32 of exactly that shape.  Everything lives on the GPU; the
    tables are read when the kernel runs, so a captured launch follows later uploads into them."""
    import ctypes
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise RuntimeError("mumpy_hip: augment_stage_u8 needs a contiguous uint8 GPU tensor (nclips, T, H, W, 3) (there is no CPU path)")
    nclips, t, hs, ws = frames.shape[:4]
    if tab_a.dim() != 2:
        raise RuntimeError("mumpy_hip: augment_stage_u8 needs tab_a of shape (nclips, L)")
    L = tab_a.shape[1]
    _chk_exact(tab_a, "tab_a", torch.int32, (nclips, L))
    _chk_exact(tab_b, "tab_b", torch.int32, (nclips, L))
    _chk_exact(swap, "swap", torch.int32, (nclips,))
    if target is not None and masks is None:
        raise RuntimeError("mumpy_hip: augment_stage_u8: target= needs masks")
    nmasks = 0
    if masks is not None:
        if masks.dim() != 3:
            raise RuntimeError("mumpy_hip: augment_stage_u8 needs masks of shape (nmasks, H, W)")
        nmasks = masks.shape[0]
        _chk_exact(masks, "masks", torch.uint8, (nmasks, hs, ws))
        target = torch.empty(nclips, L * L, device=frames.device, dtype=torch.float32) if target is None else \
            _chk_exact(target, "target", torch.float32, (nclips, L * L))
    out = torch.empty(nclips, t, 3, L, L, device=frames.device, dtype=torch.float32) if out is None else \
        _chk_exact(out, "out", torch.float32, (nclips, t, 3, L, L))
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _call("mumpy_augment_stage_u8_fwd", _p(frames), _p(masks), _p(out), _p(target), _p(tab_a), _p(tab_b), _p(swap), nclips, t, nmasks,
          hs, ws, L, m3, s3, _stream(), work=float(5 * out.numel() + (5 * target.numel() if masks is not None else 0)))
    return out if masks is None else (out, target)


def augment_warp_u8(frames, tab_a, tab_b, swap, mode, pos_y, pos_x, coef_y, coef_x, affine, masks=None, out=None, target=None,
                    mean=EVAL_MEAN, std=EVAL_STD):
    """augment_stage_u8 with the interpolating augmentations (mumpy_augment_warp_u8_fwd, include/mumpy_hip_ext4.h), one launch for
    clips of mixed modes: mode (nclips) int32 is 0 for the gather of augment_stage_u8, 1 for the separable 4-tap fixed-point resample
    through pos_y / pos_x (nclips, L) and coef_y / coef_x (nclips, L, 4) int32 (RandomScaleCrop), 2 for the bilinear warp under affine
    (nclips, 8) float32 at pos_x / pos_y (RandomRotate); the rows are those of mumpy_hip.augment.clip_warp_params.  Everything else,
    and what is returned, as augment_stage_u8."""
    import ctypes
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise RuntimeError("mumpy_hip: augment_warp_u8 needs a contiguous uint8 GPU tensor (nclips, T, H, W, 3) (there is no CPU path)")
    nclips, t, hs, ws = frames.shape[:4]
    if tab_a.dim() != 2:
        raise RuntimeError("mumpy_hip: augment_warp_u8 needs tab_a of shape (nclips, L)")
    L = tab_a.shape[1]
    for name, buf, dtype, shape in (("tab_a", tab_a, torch.int32, (nclips, L)), ("tab_b", tab_b, torch.int32, (nclips, L)),
                                    ("swap", swap, torch.int32, (nclips,)), ("mode", mode, torch.int32, (nclips,)),
                                    ("pos_y", pos_y, torch.int32, (nclips, L)), ("pos_x", pos_x, torch.int32, (nclips, L)),
                                    ("coef_y", coef_y, torch.int32, (nclips, L, 4)), ("coef_x", coef_x, torch.int32, (nclips, L, 4)),
                                    ("affine", affine, torch.float32, (nclips, 8))):
        _chk_exact(buf, name, dtype, shape, "augment_warp_u8")
    if target is not None and masks is None:
        raise RuntimeError("mumpy_hip: augment_warp_u8: target= needs masks")
    nmasks = 0
    if masks is not None:
        if masks.dim() != 3:
            raise RuntimeError("mumpy_hip: augment_warp_u8 needs masks of shape (nmasks, H, W)")
        nmasks = masks.shape[0]
        _chk_exact(masks, "masks", torch.uint8, (nmasks, hs, ws), "augment_warp_u8")
        target = torch.empty(nclips, L * L, device=frames.device, dtype=torch.float32) if target is None else \
            _chk_exact(target, "target", torch.float32, (nclips, L * L), "augment_warp_u8")
    out = torch.empty(nclips, t, 3, L, L, device=frames.device, dtype=torch.float32) if out is None else \
        _chk_exact(out, "out", torch.float32, (nclips, t, 3, L, L), "augment_warp_u8")
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _call("mumpy_augment_warp_u8_fwd", _p(frames), _p(masks), _p(out), _p(target), _p(tab_a), _p(tab_b), _p(swap), _p(mode), _p(pos_y),
          _p(pos_x), _p(coef_y), _p(coef_x), _p(affine), nclips, t, nmasks, hs, ws, L, m3, s3, _stream(),
          work=float(5 * out.numel() + (5 * target.numel() if masks is not None else 0)))
    return out if masks is None else (out, target)


# ---------------------------------------------------------------------------------------------- whole-video inference
def clip_window_u8(frames, frame_idx, size, out=None, mean=EVAL_MEAN, std=EVAL_STD):
    """Sliding clips out of a video that lives on the GPU (mumpy_clip_window_u8_fwd, include/mumpy_hip_ext5.h): frames
    (nframes, Hs, Ws, 3) uint8 and frame_idx (nclips, T) int32 -> (nclips, T, 3, H, W) float32, size = (H, W): frame (c, t) is
    normalize_u8(frames[clamp(frame_idx[c, t], 0, nframes - 1)], size=size) bit for bit.  out= is written in place and must be
    contiguous float32 of exactly that shape.  frame_idx is read when the kernel runs, so a captured launch follows later uploads."""
    import ctypes
    who = "clip_window_u8"
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise RuntimeError("mumpy_hip: clip_window_u8 needs a contiguous uint8 GPU tensor (nframes, H, W, 3) (there is no CPU path)")
    if frame_idx.dim() != 2:
        raise RuntimeError("mumpy_hip: clip_window_u8 needs frame_idx of shape (nclips, T)")
    nframes, hs, ws = frames.shape[:3]
    nclips, t = frame_idx.shape
    ho, wo = size
    _chk_exact(frame_idx, "frame_idx", torch.int32, (nclips, t), who)
    out = torch.empty(nclips, t, 3, ho, wo, device=frames.device, dtype=torch.float32) if out is None else \
        _chk_exact(out, "out", torch.float32, (nclips, t, 3, ho, wo), who)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    ytab, xtab = _nearest_table(hs, ho, frames.device), _nearest_table(ws, wo, frames.device)
    _call("mumpy_clip_window_u8_fwd", _p(frames), _p(out), _p(frame_idx), _p(ytab), _p(xtab), nclips, t, nframes, hs, ws, ho, wo, m3, s3,
          _stream(), work=float(5 * out.numel()))
    return out


def mask_score_u8(mask, dest, bank, gt=None, counts=None):
    """The masks of a batch of clips into the per-frame bank (mumpy_mask_score_u8_fwd): mask (nclips, ...) uint8 with npix elements per
    clip (what Decoder.predict_mask emits), dest (nclips) int32, bank (nbank, npix) uint8, written in place: bank[dest[c]] =
    mask[c] ? 255 : 0 for every clip with 0 <= dest[c] < nbank; the others (the padding of a batch tail) write nothing.
    gt (nbank, npix) uint8: also counts[dest[c]] = [sum p & g, sum p, sum g, sum p | g] (int32 (nbank, 4), written in place; allocated
    zeroed when not given).  Returns bank, or (bank, counts) with gt.  dest is read when the kernel runs."""
    who = "mask_score_u8"
    if bank.dim() != 2:
        raise RuntimeError("mumpy_hip: mask_score_u8 needs bank of shape (nbank, npix)")
    nbank, npix = bank.shape
    _chk_exact(bank, "bank", torch.uint8, (nbank, npix), who)
    nclips = dest.shape[0] if dest.dim() == 1 else -1
    _chk_exact(dest, "dest", torch.int32, (nclips,), who)
    if not mask.is_cuda or mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.dim() < 1 or mask.shape[0] != nclips or \
            mask.numel() != nclips * npix:
        raise RuntimeError(f"mumpy_hip: mask_score_u8 needs mask as a contiguous uint8 GPU tensor ({nclips}, ...) of {npix} elements per "
                           f"clip, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
    if counts is not None and gt is None:
        raise RuntimeError("mumpy_hip: mask_score_u8: counts= needs gt")
    if gt is not None:
        _chk_exact(gt, "gt", torch.uint8, (nbank, npix), who)
        counts = torch.zeros(nbank, 4, device=bank.device, dtype=torch.int32) if counts is None else \
            _chk_exact(counts, "counts", torch.int32, (nbank, 4), who)
    _call("mumpy_mask_score_u8_fwd", _p(mask), _p(gt), _p(dest), _p(bank), _p(counts), nclips, npix, nbank, _stream(),
          work=float((2 if gt is None else 3) * mask.numel()))
    return bank if gt is None else (bank, counts)


def frame_metrics(counts, nscored, npix, acc=None, accumulate=False):
    """[sum F1, sum IoU, n] float64 over frames 0 .. nscored - 1 of counts (>= nscored, 4) int32 as mask_score_u8 writes them
    (mumpy_frame_metrics_fwd; the per-image formulas of measure.py:57-62, 86-89 as distributed.eval_metric_vector states them).
    acc= (3,) float64 is written in place -- added into with accumulate=True -- and is what evaluate.finalize_metrics takes."""
    who = "frame_metrics"
    if counts.dim() != 2 or counts.shape[0] < nscored:
        raise RuntimeError(f"mumpy_hip: frame_metrics needs counts of shape (>= {nscored}, 4)")
    _chk_exact(counts, "counts", torch.int32, (counts.shape[0], 4), who)
    if acc is None:
        if accumulate:
            raise RuntimeError("mumpy_hip: frame_metrics: accumulate=True needs acc=")
        acc = torch.empty(3, device=counts.device, dtype=torch.float64)
    else:
        _chk_exact(acc, "acc", torch.float64, (3,), who)
    _call("mumpy_frame_metrics_fwd", _p(counts), int(nscored), int(npix), _p(acc), int(bool(accumulate)), _stream())
    return acc


SWEEP_MAX_THRESHOLDS = 1023      # MUMPY_SWEEP_MAX_THRESHOLDS of include/mumpy_hip_ext7.h


def _chk_exceed(exceed, who):
    """-> (rows, K) of an exceed buffer (rows, 2, K + 1) int32, read or written where it is."""
    if exceed.dim() != 3 or exceed.shape[1] != 2 or not 2 <= exceed.shape[2] <= SWEEP_MAX_THRESHOLDS + 1:
        raise RuntimeError(f"mumpy_hip: {who} needs exceed of shape (rows, 2, K + 1) with 1 <= K <= {SWEEP_MAX_THRESHOLDS}, got "
                           f"{tuple(exceed.shape)}")
    _chk_exact(exceed, "exceed", torch.int32, tuple(exceed.shape), who)
    return exceed.shape[0], exceed.shape[2] - 1


def score_exceed(logits, gt, dest, table, exceed):
    """Per frame and class, the pixels whose probability exceeds each threshold of a table (mumpy_score_exceed_fwd,
    include/mumpy_hip_ext7.h): logits (nclips, ...) float32 with npix elements per clip (what final_conv writes), gt (nbank, npix)
    uint8 (> 0 is forged), dest (nclips) int32, table (K) float32 ascending, exceed (nbank, 2, K + 1) int32, written in place: for
    every clip with 0 <= dest[c] < nbank, exceed[dest[c]][g][k] = #{pixels of class g with sigmoid(logit) > table[k]} and
    exceed[dest[c]][g][K] = #{pixels of class g}; the other clips write nothing, the other rows stay.  Row k holds the counts
    mask_score_u8 takes from final_conv's mask at thr = table[k], bit for bit (video.exceed_counts reads them out).  K is taken from
    the table.  dest and table are read when the kernel runs.  Returns exceed."""
    who = "score_exceed"
    if table.dim() != 1 or not 1 <= table.shape[0] <= SWEEP_MAX_THRESHOLDS:
        raise RuntimeError(f"mumpy_hip: score_exceed needs a table of 1 .. {SWEEP_MAX_THRESHOLDS} thresholds, got {tuple(table.shape)}")
    k = table.shape[0]
    _chk_exact(table, "table", torch.float32, (k,), who)
    if gt.dim() != 2:
        raise RuntimeError("mumpy_hip: score_exceed needs gt of shape (nbank, npix)")
    nbank, npix = gt.shape
    _chk_exact(gt, "gt", torch.uint8, (nbank, npix), who)
    nclips = dest.shape[0] if dest.dim() == 1 else -1
    _chk_exact(dest, "dest", torch.int32, (nclips,), who)
    if not logits.is_cuda or logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() < 1 or \
            logits.shape[0] != nclips or logits.numel() != nclips * npix:
        raise RuntimeError(f"mumpy_hip: score_exceed needs logits as a contiguous float32 GPU tensor ({nclips}, ...) of {npix} elements "
                           f"per clip, got {logits.dtype} {tuple(logits.shape)} on {logits.device}")
    _chk_exact(exceed, "exceed", torch.int32, (nbank, 2, k + 1), who)
    _call("mumpy_score_exceed_fwd", _p(logits), _p(gt), _p(dest), _p(table), _p(exceed), nclips, npix, nbank, k, _stream(),
          work=float(5 * logits.numel()))
    return exceed


def sweep_metrics(exceed, nscored, npix, acc=None, pooled=None, accumulate=False):
    """Per-threshold [sum F1, sum IoU, n] float64 (K, 3) over frames 0 .. nscored - 1 of exceed (>= nscored, 2, K + 1) int32 as
    score_exceed writes it (mumpy_sweep_metrics_fwd): row k is what frame_metrics gives for video.exceed_counts(exceed, k).
    acc= (K, 3) float64 is written in place (allocated when not given).  pooled= (2, K + 1) int64, written in place, or True to have
    one allocated: the counts summed over the frames (the ROC points of the table); None: not computed.  accumulate=True adds into
    acc and pooled (both must then be the caller's).  Returns acc, or (acc, pooled) with pooled.  evaluate.finalize_sweep takes the
    two."""
    who = "sweep_metrics"
    rows, k = _chk_exceed(exceed, who)
    nscored, npix = int(nscored), int(npix)
    if not 0 <= nscored <= rows:
        raise RuntimeError(f"mumpy_hip: sweep_metrics needs exceed of shape (>= {nscored}, 2, K + 1), got {tuple(exceed.shape)}")
    if accumulate and (acc is None or pooled is True):
        raise RuntimeError("mumpy_hip: sweep_metrics: accumulate=True needs acc= (and pooled=, when given) as the caller's buffers")
    acc = torch.empty(k, 3, device=exceed.device, dtype=torch.float64) if acc is None else \
        _chk_exact(acc, "acc", torch.float64, (k, 3), who)
    if pooled is True:
        pooled = torch.empty(2, k + 1, device=exceed.device, dtype=torch.int64)
    elif pooled is not None:
        _chk_exact(pooled, "pooled", torch.int64, (2, k + 1), who)
    _call("mumpy_sweep_metrics_fwd", _p(exceed), nscored, npix, k, _p(acc), _p(pooled), int(bool(accumulate)), _stream())
    return acc if pooled is None else (acc, pooled)


_BILINEAR_TABLES = {}


def _bilinear_tables(hs: int, ws: int, ho: int, wo: int, device):
    """Pillow's BILINEAR taps of an (hs, ws) -> (ho, wo) resize (mumpy_hip.video.bilinear_taps), cached on the device:
    (ystart, ycount, ycoef, xstart, xcount, xcoef)."""
    key = (hs, ws, ho, wo, str(device))
    t = _BILINEAR_TABLES.get(key)
    if t is None:
        from .video import bilinear_taps
        t = _BILINEAR_TABLES[key] = tuple(torch.from_numpy(a).to(device) for a in bilinear_taps(hs, ho) + bilinear_taps(ws, wo))
    return t


def resize_bilinear_u8(src, size, out=None):
    """Image.resize((W, H), Image.BILINEAR) of single-channel 8-bit images on the GPU (mumpy_resize_bilinear_u8_fwd,
    include/mumpy_hip_ext6.h): src (n, Hs, Ws) uint8 -> (n, H, W) uint8, size = (H, W), Pillow's result bit for bit at any ratio
    (mumpy_hip.video.bilinear_resize is the numpy statement) -- the resize measure.py:21-40 applies to every annotation.  out= is
    written in place and must be contiguous uint8 of exactly that shape.  src is read where it is: never copied.  The first call for
    a pair of sizes uploads its six tap tables (cached per sizes and device): make that call outside a graph capture."""
    who = "resize_bilinear_u8"
    if not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 3 or not src.is_contiguous():
        raise RuntimeError(f"mumpy_hip: resize_bilinear_u8 needs a contiguous uint8 GPU tensor (n, H, W) (there is no CPU path), got "
                           f"{src.dtype} {tuple(src.shape)} on {src.device}")
    n, hs, ws = src.shape
    ho, wo = (int(v) for v in size)
    if hs < 1 or ws < 1 or ho < 1 or wo < 1:
        raise RuntimeError(f"mumpy_hip: resize_bilinear_u8: empty image, {hs}x{ws} -> {ho}x{wo}")
    out = torch.empty(n, ho, wo, device=src.device, dtype=torch.uint8) if out is None else \
        _chk_exact(out, "out", torch.uint8, (n, ho, wo), who)
    ys, yc, yk, xs, xc, xk = _bilinear_tables(hs, ws, ho, wo, src.device)
    _call("mumpy_resize_bilinear_u8_fwd", _p(src), _p(out), _p(ys), _p(yc), _p(yk), _p(xs), _p(xc), _p(xk), n, hs, ws, ho, wo,
          yk.shape[1], xk.shape[1], _stream(), work=float(src.numel() + out.numel()))
    return out


# ---------------------------------------------------------------------------------------------- perturbations (mumpy_perturb.h)
PERTURB_CHUNK_BYTES = 64 << 20       # workspace the perturbation wrappers allocate for themselves at the most: they chunk over images
_JPEG_TABLES = {}


def _frames_u8(frames, who, channels=3):
    """frames (..., H, W, channels) uint8, contiguous, on the GPU, read (or written) where it is -> (nimg, H, W)."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() < 3 \
            or frames.shape[-1] != channels or not frames.is_contiguous():
        raise RuntimeError(f"mumpy_hip: {who} needs a contiguous uint8 GPU tensor (..., H, W{', 3' if channels == 3 else ''}) (there is no CPU path), got "
                           f"{getattr(frames, 'dtype', type(frames))} {tuple(getattr(frames, 'shape', ()))}")
    h, w = frames.shape[-3:-1]
    if h < 1 or w < 1:
        raise RuntimeError(f"mumpy_hip: {who}: empty image {h}x{w}")
    return frames.numel() // (channels * h * w), h, w


def _perturb_out(frames, out, who):
    if out is None:
        return torch.empty_like(frames)
    _chk_exact(out, "out", torch.uint8, frames.shape, who)
    if out.data_ptr() != frames.data_ptr():
        lo, hi = sorted(((frames.data_ptr(), frames.numel()), (out.data_ptr(), out.numel())))
        if lo[0] + lo[1] > hi[0]:
            raise RuntimeError(f"mumpy_hip: {who}: out may be frames itself but must not overlap it partially")
    return out


def _perturb_chunks(entry, nimg, h, w, workspace, who, device):
    """-> (workspace, bytes per image, images per launch): the caller's workspace must hold all nimg images (one launch); without
    one the wrapper allocates at most PERTURB_CHUNK_BYTES and walks the images in chunks."""
    total = _ws_bytes((entry, nimg, h, w), entry, nimg, h, w)
    if total < 0:
        raise RuntimeError(f"mumpy_hip: {who}: {entry}({nimg}, {h}, {w}) refused (rc={total}): {_lib().mumpy_last_error().decode()}")
    if workspace is not None:
        if not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < total:
            raise RuntimeError(f"mumpy_hip: {who} needs workspace as a contiguous uint8 GPU tensor of at least {total} bytes, got "
                               f"{workspace.dtype} {tuple(workspace.shape)} on {workspace.device}")
        return workspace, max(nimg, 1)
    one = max(_ws_bytes((entry, 1, h, w), entry, 1, h, w), 16)
    step = max(1, min(nimg, PERTURB_CHUNK_BYTES // one))
    return torch.empty(max(_ws_bytes((entry, step, h, w), entry, step, h, w), 16), device=device, dtype=torch.uint8), step


def jpeg_tables_u16(tables, device=None):
    """(ntab, 2, 64) quantisation tables as the uint16 device tensor the kernel reads: from a numpy array / list of
    mumpy_hip.perturb.jpeg_tables rows (uploaded) or a device tensor of uint16 / int16 (the same bits) taken where it is."""
    if isinstance(tables, torch.Tensor):
        t = tables
    else:
        import numpy as np
        a = np.asarray(tables)
        if a.size == 0 or a.size % 128 or a.min() < 1 or a.max() > 65535:
            raise RuntimeError(f"mumpy_hip: jpeg tables must be (ntab, 2, 64) with entries in 1 .. 65535, got shape {a.shape}")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint16).reshape(-1, 2, 64))).to(device)
    if not t.is_cuda or t.dtype not in (torch.uint16, torch.int16) or t.dim() != 3 or tuple(t.shape[1:]) != (2, 64) or t.shape[0] < 1 \
            or not t.is_contiguous():
        raise RuntimeError(f"mumpy_hip: jpeg tables must be a contiguous uint16 GPU tensor (ntab, 2, 64) with ntab >= 1, got {t.dtype} "
                           f"{tuple(t.shape)} on {t.device}")
    return t


def jpeg_roundtrip_u8(frames, quality_or_tables, sel=None, out=None, workspace=None):
    """The JPEG round trip on the GPU (mumpy_jpeg_roundtrip_u8_fwd, include/mumpy_perturb.h): frames (..., H, W, 3) uint8 -> the
    same shape, every image what Pillow returns for save(format="JPEG", quality=q) + Image.open, bit for bit
    (mumpy_hip.perturb.jpeg_roundtrip is the numpy statement).  quality_or_tables: an integer quality 1 .. 100 for every image (its
    tables are uploaded once per quality and device: make the first call outside a graph capture), or a device tensor (ntab, 2, 64)
    uint16 of mumpy_hip.perturb.jpeg_tables rows with sel (nimg) int32 on the device choosing the table per image -- a negative
    (or too large) sel copies that image through; sel=None uses table 0 everywhere.  Tables and sel are read when the kernels run.
    out= (contiguous uint8 of the same shape) may be frames itself.  workspace= (uint8, at least
    mumpy_jpeg_roundtrip_workspace_bytes(nimg, H, W)) gives one pair of launches, as a capture wants; without it the wrapper
    allocates at most PERTURB_CHUNK_BYTES and walks the images in chunks."""
    who = "jpeg_roundtrip_u8"
    nimg, h, w = _frames_u8(frames, who)
    if isinstance(quality_or_tables, torch.Tensor):
        qtab = jpeg_tables_u16(quality_or_tables)
    else:
        from .perturb import jpeg_tables
        rows = jpeg_tables(quality_or_tables)                        # refuses a quality outside 1 .. 100
        key = (int(quality_or_tables), str(frames.device))
        qtab = _JPEG_TABLES.get(key)
        if qtab is None:
            qtab = _JPEG_TABLES[key] = jpeg_tables_u16(rows[None], frames.device)
    if sel is None:
        sel = torch.zeros(nimg, device=frames.device, dtype=torch.int32)
    _chk_exact(sel, "sel", torch.int32, (nimg,), who)
    out = _perturb_out(frames, out, who)
    ws, step = _perturb_chunks("mumpy_jpeg_roundtrip_workspace_bytes", nimg, h, w, workspace, who, frames.device)
    src, dst = frames.view(nimg, h, w, 3), out.view(nimg, h, w, 3)
    for i in range(0, nimg, step):
        m = min(step, nimg - i)
        _call("mumpy_jpeg_roundtrip_u8_fwd", _p(src[i:i + m]), _p(dst[i:i + m]), _p(qtab), _p(sel[i:i + m]), _p(ws), ws.numel(), m,
              qtab.shape[0], h, w, _stream(), work=float(6 * m * h * w))
    return out


def blur_params(radius_or_rows, nimg, device):
    """(nimg, 4) int32 on the device, {r, ww, fw, on} per image: one radius for every image, or one per image (a sequence of nimg
    radii; None means off) -- computed by mumpy_hip.perturb.box_params and uploaded."""
    import numpy as np
    from .perturb import box_params
    off = (0, 1 << 24, 0, 0)
    if np.ndim(radius_or_rows) == 0:
        rows = [box_params(radius_or_rows)] * nimg
    else:
        rows = [off if r is None else box_params(r) for r in radius_or_rows]
        if len(rows) != nimg:
            raise RuntimeError(f"mumpy_hip: blur_params: {len(rows)} radii for {nimg} images")
    return torch.from_numpy(np.asarray(rows, dtype=np.int64).astype(np.int32).reshape(nimg, 4)).to(device)


def gaussian_blur_u8(frames, radius_or_params, out=None, workspace=None):
    """ImageFilter.GaussianBlur(radius) of Pillow on the GPU (mumpy_gaussian_blur_u8_fwd, include/mumpy_perturb.h): frames
    (..., H, W, 3) uint8 -> the same shape, bit for bit (mumpy_hip.perturb.gaussian_blur is the numpy statement).
    radius_or_params: a radius for every image (its parameters are uploaded by this call: pass a tensor inside a graph capture), or
    a device tensor (nimg, 4) int32 of {r, ww, fw, on} rows (`blur_params`, mumpy_hip.perturb.box_params), read when the kernels
    run; on == 0 copies that image through.  out= and workspace= as in jpeg_roundtrip_u8 (mumpy_gaussian_blur_workspace_bytes)."""
    who = "gaussian_blur_u8"
    nimg, h, w = _frames_u8(frames, who)
    params = radius_or_params if isinstance(radius_or_params, torch.Tensor) else blur_params(radius_or_params, nimg, frames.device)
    _chk_exact(params, "params", torch.int32, (nimg, 4), who)
    out = _perturb_out(frames, out, who)
    ws, step = _perturb_chunks("mumpy_gaussian_blur_workspace_bytes", nimg, h, w, workspace, who, frames.device)
    src, dst = frames.view(nimg, h, w, 3), out.view(nimg, h, w, 3)
    for i in range(0, nimg, step):
        m = min(step, nimg - i)
        _call("mumpy_gaussian_blur_u8_fwd", _p(src[i:i + m]), _p(dst[i:i + m]), _p(params[i:i + m]), _p(ws), ws.numel(), m, h, w,
              _stream(), work=float(12 * m * h * w))
    return out


def photometric_params(spec_or_rows, nimg, device):
    """(nimg, 4) int32 on the device, {kind, value, 0, 0} per image: one (kind, value) for every image, or one per image (a sequence
    of nimg pairs; None means pass through) -- encoded by mumpy_hip.photometric.params_row and uploaded."""
    import numpy as np
    from .photometric import params_row
    if spec_or_rows is None or (isinstance(spec_or_rows, tuple) and len(spec_or_rows) == 2 and isinstance(spec_or_rows[0], str)):
        rows = [params_row(*(spec_or_rows or ("none", None)))] * nimg
    else:
        rows = [params_row(*(s or ("none", None))) for s in spec_or_rows]
        if len(rows) != nimg:
            raise RuntimeError(f"mumpy_hip: photometric_params: {len(rows)} settings for {nimg} images")
    return torch.from_numpy(np.asarray(rows, dtype=np.int32).reshape(nimg, 4)).to(device)


def photometric_u8(frames, spec_or_params, out=None, workspace=None):
    """One photometric operation of Pillow per image on the GPU (mumpy_photometric_u8_fwd, include/mumpy_photometric.h): frames
    (..., H, W, 3) uint8 -> the same shape, bit for bit ImageOps.autocontrast / invert / equalize / solarize / posterize or
    ImageEnhance.Contrast / Color / Brightness / Sharpness (mumpy_hip.photometric.apply is the numpy statement; statistics are per
    image).  spec_or_params: a (kind, value) for every image (its rows are uploaded by this call: pass a tensor inside a graph
    capture), or a device tensor (nimg, 4) int32 of mumpy_hip.photometric.params_row rows (`photometric_params`), read when the
    kernels run; kind 0 copies that image through.  out= and workspace= as in jpeg_roundtrip_u8
    (mumpy_photometric_workspace_bytes); out may be frames itself for every kind."""
    who = "photometric_u8"
    nimg, h, w = _frames_u8(frames, who)
    params = spec_or_params if isinstance(spec_or_params, torch.Tensor) else photometric_params(spec_or_params, nimg, frames.device)
    _chk_exact(params, "params", torch.int32, (nimg, 4), who)
    out = _perturb_out(frames, out, who)
    ws, step = _perturb_chunks("mumpy_photometric_workspace_bytes", nimg, h, w, workspace, who, frames.device)
    src, dst = frames.view(nimg, h, w, 3), out.view(nimg, h, w, 3)
    for i in range(0, nimg, step):
        m = min(step, nimg - i)
        _call("mumpy_photometric_u8_fwd", _p(src[i:i + m]), _p(dst[i:i + m]), _p(params[i:i + m]), _p(ws), ws.numel(), m, h, w,
              _stream(), work=float(6 * m * h * w))
    return out


def geometric_u8(src, params, out=None, channels=3):
    """One geometric operation per image on the GPU (mumpy_geometric_u8_fwd, include/mumpy_geometric.h): src (..., H, W, 3) uint8,
    or with channels=1 single-channel images (masks) (..., H, W), -> the same shape, bit for bit Pillow's Image.transform(size,
    AFFINE, m, NEAREST, fillcolor=0) / Image.rotate / ImageDraw.rectangle(xy, 0) (mumpy_hip.geometric.apply_row is the numpy
    statement).  params: a device tensor (nimg, 8) int32 of mumpy_hip.geometric.params_row rows, read when the kernel runs, or such
    rows on the host (a numpy array / list, uploaded by this call: pass a tensor inside a graph capture); mode 0 copies that image
    through.  One launch, no workspace.  out= is written in place and must be contiguous uint8 of src's shape; it must not overlap
    src, src itself included (a gather cannot run in place)."""
    who = "geometric_u8"
    if channels not in (1, 3):
        raise RuntimeError(f"mumpy_hip: geometric_u8: channels={channels} must be 1 or 3")
    if channels == 1 and isinstance(src, torch.Tensor) and src.dim() < 2:
        raise RuntimeError(f"mumpy_hip: geometric_u8 needs images (..., H, W) with channels=1, got {tuple(src.shape)}")
    img = src.unsqueeze(-1) if channels == 1 and isinstance(src, torch.Tensor) and src.is_contiguous() else src
    nimg, h, w = _frames_u8(img, who, channels)
    if not isinstance(params, torch.Tensor):
        import numpy as np
        rows = np.asarray(params)
        if rows.dtype != np.int32 or rows.shape != (nimg, 8):
            raise RuntimeError(f"mumpy_hip: geometric_u8 needs params as int32 rows of shape ({nimg}, 8), got {rows.dtype} {rows.shape}")
        params = torch.from_numpy(np.ascontiguousarray(rows)).to(src.device)
    _chk_exact(params, "params", torch.int32, (nimg, 8), who)
    out = torch.empty_like(src) if out is None else _chk_exact(out, "out", torch.uint8, src.shape, who)
    lo, hi = sorted(((src.data_ptr(), src.numel()), (out.data_ptr(), out.numel())))
    if nimg and lo[0] + lo[1] > hi[0]:
        raise RuntimeError(f"mumpy_hip: geometric_u8: out {tuple(out.shape)} overlaps src (a gather cannot run in place)")
    _call("mumpy_geometric_u8_fwd", _p(src), _p(out), _p(params), nimg, h, w, channels, _stream(), work=float(2 * out.numel()))
    return out


def mask_clean_params(spec, nimg, device):
    """(nimg, 4) int32 on the device, {min_area, max_hole, connectivity, 0} per image: one setting for every image (a dict as
    VideoPredictor(clean=...) takes it, or a (min_area, max_hole[, connectivity]) tuple), or one such setting per image (a list of
    nimg of them) -- encoded by mumpy_hip.postprocess.params_row and uploaded."""
    import numpy as np
    from .postprocess import params_row

    def row(s):
        if isinstance(s, dict):
            return params_row(s["min_area"], s["max_hole"], s.get("connectivity", 8))
        return params_row(*s)
    if isinstance(spec, dict) or (isinstance(spec, tuple) and len(spec) in (2, 3) and not isinstance(spec[0], (dict, tuple, list))):
        rows = [row(spec)] * nimg
    else:
        rows = [row(s) for s in spec]
        if len(rows) != nimg:
            raise RuntimeError(f"mumpy_hip: mask_clean_params: {len(rows)} settings for {nimg} images")
    return torch.from_numpy(np.asarray(rows, dtype=np.int32).reshape(nimg, 4)).to(device)


def mask_clean_workspace(nimg, h, w, device):
    """The workspace of one mask_clean_u8 call on nimg masks of h x w (mumpy_mask_clean_workspace_bytes); a refused shape raises."""
    need = int(_lib().mumpy_mask_clean_workspace_bytes(nimg, h, w))
    if need < 0:
        raise RuntimeError(f"mumpy_hip: mask_clean_u8 (rc={need}): {_lib().mumpy_last_error().decode()}")
    return torch.empty(max(need, 16), device=device, dtype=torch.uint8)


def mask_clean_u8(mask, params, out=None, gt=None, counts=None, stats=None, workspace=None, hw=None):
    """Small components out, small holes filled, per mask, on the GPU (mumpy_mask_clean_u8_fwd, include/mumpy_postprocess.h;
    mumpy_hip.postprocess.clean is the numpy statement): mask (nimg, H, W) uint8 -- or (nimg, H * W) with hw=(H, W), the layout of
    the predictor's bank --, non-zero is foreground -> out of the same shape, bytes 0 / 255.  params: a device tensor (nimg, 4) int32
    of mumpy_hip.postprocess.params_row rows {min_area, max_hole, connectivity, 0}, read when the kernel runs, or such rows on the
    host (a numpy array / list, uploaded by this call: pass a tensor inside a graph capture).  out= may be mask itself (in place) and
    must not overlap it otherwise.  gt (the shape of mask, > 0 is forged): also counts (nimg, 4) int32 = [sum p & g, sum p, sum g,
    sum p | g] of the cleaned masks, written, in the layout of mask_score_u8 (frame_metrics takes it).  stats (nimg, 8) int32:
    mumpy_hip.postprocess.STATS; allocated when not given.  workspace= a uint8 tensor of mumpy_mask_clean_workspace_bytes(nimg, H, W)
    bytes (`mask_clean_workspace`), allocated when not given.  One launch.  Returns (out, stats), or (out, counts, stats) with gt."""
    who = "mask_clean_u8"
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype != torch.uint8 or not mask.is_contiguous() or \
            mask.dim() != (3 if hw is None else 2):
        raise RuntimeError(f"mumpy_hip: {who} needs mask as a contiguous uint8 GPU tensor (nimg, H, W), or (nimg, H * W) with hw=, got "
                           f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    nimg = mask.shape[0]
    h, w = (int(v) for v in (mask.shape[1:] if hw is None else hw))
    if hw is not None and (h < 1 or w < 1 or h * w != mask.shape[1]):
        raise RuntimeError(f"mumpy_hip: {who}: hw={hw} does not give the {mask.shape[1]} pixels of a row of mask")
    if not isinstance(params, torch.Tensor):
        import numpy as np
        rows = np.asarray(params)
        if rows.dtype != np.int32 or rows.shape != (nimg, 4):
            raise RuntimeError(f"mumpy_hip: {who} needs params as int32 rows of shape ({nimg}, 4), got {rows.dtype} {rows.shape}")
        params = torch.from_numpy(np.ascontiguousarray(rows)).to(mask.device)
    _chk_exact(params, "params", torch.int32, (nimg, 4), who)
    out = torch.empty_like(mask) if out is None else _chk_exact(out, "out", torch.uint8, mask.shape, who)
    if counts is not None and gt is None:
        raise RuntimeError(f"mumpy_hip: {who}: counts= needs gt")
    if gt is not None:
        _chk_exact(gt, "gt", torch.uint8, mask.shape, who)
        counts = torch.empty(nimg, 4, device=mask.device, dtype=torch.int32) if counts is None else \
            _chk_exact(counts, "counts", torch.int32, (nimg, 4), who)
    stats = torch.empty(nimg, 8, device=mask.device, dtype=torch.int32) if stats is None else \
        _chk_exact(stats, "stats", torch.int32, (nimg, 8), who)
    lo, hi = sorted(((mask.data_ptr(), mask.numel()), (out.data_ptr(), out.numel())))
    if nimg and out.data_ptr() != mask.data_ptr() and lo[0] + lo[1] > hi[0]:
        raise RuntimeError(f"mumpy_hip: {who}: out {tuple(out.shape)} overlaps mask without being mask")
    need = int(_lib().mumpy_mask_clean_workspace_bytes(nimg, h, w))
    if need < 0:
        raise RuntimeError(f"mumpy_hip: {who} (rc={need}): {_lib().mumpy_last_error().decode()}")
    if workspace is None:
        workspace = torch.empty(max(need, 16), device=mask.device, dtype=torch.uint8)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise RuntimeError(f"mumpy_hip: {who} needs workspace as a contiguous uint8 GPU tensor of at least {need} bytes, got "
                           f"{workspace.dtype} {tuple(workspace.shape)} on {workspace.device}")
    _call("mumpy_mask_clean_u8_fwd", _p(mask), _p(out), _p(gt), _p(counts), _p(stats), _p(params), _p(workspace), workspace.numel(),
          nimg, h, w, _stream(), work=float(2 * mask.numel()))
    return (out, stats) if gt is None else (out, counts, stats)


def resize_nearest_u8(frames, size, out=None, channels=3):
    """Image.resize((W, H), Image.NEAREST) of RGB frames on the GPU (mumpy_resize_nearest_u8_fwd, include/mumpy_perturb.h): frames
    (..., Hs, Ws, 3) uint8 -> (..., H, W, 3) uint8, size = (H, W), through the tables of mumpy_resize_nearest_table (cached per
    sizes and device: make the first call for a pair of sizes outside a graph capture).  channels=1: single-channel images (masks)
    (..., Hs, Ws) -> (..., H, W).  out= is written in place and must be contiguous uint8 of exactly that shape, and must not
    overlap frames."""
    who = "resize_nearest_u8"
    if channels not in (1, 3):
        raise RuntimeError(f"mumpy_hip: resize_nearest_u8: channels={channels} must be 1 or 3")
    src = frames.unsqueeze(-1) if channels == 1 and isinstance(frames, torch.Tensor) and frames.is_contiguous() else frames
    nimg, hs, ws = _frames_u8(src, who, channels)
    ho, wo = (int(v) for v in size)
    if ho < 1 or wo < 1:
        raise RuntimeError(f"mumpy_hip: resize_nearest_u8: empty output {ho}x{wo}")
    shape = (*src.shape[:-3], ho, wo) + ((3,) if channels == 3 else ())
    out = torch.empty(shape, device=src.device, dtype=torch.uint8) if out is None else _chk_exact(out, "out", torch.uint8, shape, who)
    lo, hi = sorted(((src.data_ptr(), src.numel()), (out.data_ptr(), out.numel())))
    if nimg and lo[0] + lo[1] > hi[0]:
        raise RuntimeError("mumpy_hip: resize_nearest_u8: out overlaps frames")
    ytab, xtab = _nearest_table(hs, ho, src.device), _nearest_table(ws, wo, src.device)
    _call("mumpy_resize_nearest_u8_fwd", _p(src), _p(out), _p(ytab), _p(xtab), nimg, hs, ws, ho, wo, channels, _stream(),
          work=float(2 * out.numel()))
    return out


# ---------------------------------------------------------------------------------------------- training tail (8f-2)
def mask_loss(logits, target, need_grad=True, eps=0.0, loss_scale=1.0):
    """softIoULoss + WeightedFocalLoss as train.py:107-113 calls them (utils/loss.py:6-55).  logits (B,...) and 0/1 target of the
    same number of elements per sample -> (loss3 = [total*loss_scale, iou, focal] device tensor, dlogits or None)."""
    logits = _chk(logits, "logits")
    b = logits.shape[0]
    p = logits.numel() // b
    if target.numel() != b * p:
        raise RuntimeError(f"mask_loss: target has {target.numel()} elements, logits {b} x {p}")
    target = _chk(target.to(torch.float32).reshape(b, p), "target")
    loss3 = torch.empty(3, device=logits.device, dtype=torch.float32)
    dz = torch.empty_like(logits) if need_grad else None
    wsb = int(_lib().mumpy_mask_loss_workspace_bytes(b, p))
    ws = torch.empty(wsb // 4, device=logits.device, dtype=torch.float32)
    _call("mumpy_mask_loss_fwd_bwd", _p(logits), _p(target), _p(dz), _p(loss3), _p(ws), wsb, b, p, eps, loss_scale, _stream(),
          work=4.0 * logits.numel() * (5 if need_grad else 2))
    return loss3, dz


def adamw_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
    """In-place fused AdamW over flat fp32 buffers (torch.optim.AdamW defaults; step counts from 1)."""
    n = param.numel()
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _chk(t, name)
        if t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"adamw_step: {name} must be a contiguous buffer of {n} elements (in-place update)")
    _call("mumpy_adamw_step", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, lr, betas[0], betas[1], eps, weight_decay,
          int(step), grad_scale, _stream(), work=28.0 * n)
    return param


# ------------------------------------------------------------------------------------------ Swin block backward (8f-2)
def _ws(nbytes, device):
    return torch.empty(max(nbytes // 4, 4), device=device, dtype=torch.float32)


def layernorm_bwd(x, gamma, dy, eps=1e-5, dx_add=None, dg_out=None, db_out=None):
    """-> (dx like x, dgamma (C), dbeta (C)) of nn.LayerNorm over the last dim.  dx_add: a gradient to add to dx (the residual
    branch that bypasses the norm).  dg_out / db_out (both or neither): gradient buffers to ACCUMULATE into; the matching
    return values are then None."""
    x = _chk(x, "x")
    c = x.shape[-1]
    rows = x.numel() // c
    dy, gamma = _rd(dy, "dy", x.numel(), "layernorm_bwd"), _rd(gamma, "gamma", c, "layernorm_bwd")
    dx = torch.empty_like(x)
    if dx_add is not None:
        dx_add = _chk(dx_add, "dx_add")
        if dx_add.shape != x.shape:
            raise RuntimeError("layernorm_bwd: dx_add must have x's shape")
    if (dg_out is None) != (db_out is None):
        raise RuntimeError("layernorm_bwd: dg_out and db_out go together")
    acc = dg_out is not None
    dg = _wr(dg_out, "dg_out", c, "layernorm_bwd") if acc else torch.empty(c, device=x.device, dtype=torch.float32)
    db = _wr(db_out, "db_out", c, "layernorm_bwd") if acc else torch.empty(c, device=x.device, dtype=torch.float32)
    wsb = _ws_bytes(("lnbwd", rows, c), "mumpy_layernorm_bwd_workspace_bytes", rows, c)
    ws = _ws(wsb, x.device)
    _call("mumpy_layernorm_bwd", _p(x), _p(gamma), _p(dy), _p(dx_add), _p(dx), _p(dg), _p(db), _p(ws), wsb, rows, c, eps, int(acc),
          _stream(), work=12.0 * x.numel())
    return (dx, None, None) if acc else (dx, dg, db)


def gelu(x):
    x = _chk(x, "x")
    y = torch.empty_like(x)
    _call("mumpy_gelu_fwd", _p(x), _p(y), x.numel(), _stream(), work=8.0 * x.numel())
    return y


def gelu_bwd(x, dy):
    x = _chk(x, "x")
    dy = _rd(dy, "dy", x.numel(), "gelu_bwd")
    dx = torch.empty_like(x)
    _call("mumpy_gelu_bwd", _p(x), _p(dy), _p(dx), x.numel(), _stream(), work=12.0 * x.numel())
    return dx


def transpose(x2d, pad_rows_to=1):
    """(R,C) -> (C, Rp) with Rp = R rounded up to a multiple of `pad_rows_to` (extra columns zero): the K-contiguous
    operand layout of the weight-gradient GEMMs, whose reduction dim (the token count) must be a multiple of 32."""
    x2d = _chk(x2d, "x")
    r, c = x2d.shape
    rp = (r + pad_rows_to - 1) // pad_rows_to * pad_rows_to
    if rp != r:
        xp = torch.zeros(rp, c, device=x2d.device, dtype=torch.float32)
        xp[:r] = x2d
        x2d, r = xp, rp
    out = torch.empty(c, r, device=x2d.device, dtype=torch.float32)
    _call("mumpy_transpose_fwd", _p(x2d), _p(out), r, c, _stream(), work=8.0 * x2d.numel())
    return out


def linear_bwd(x2d, weight, dy2d, need_dx=True, dw_out=None, db_out=None, need_dw=True, need_db=False):
    """Backward of y = x W^T + b in ONE C-ABI call (mumpy_linear_bwd), no transposed copies: -> (dx, dW, db).
    dw_out / db_out: gradient buffers to ACCUMULATE into (e.g. views of FlatAdamW's flat gradient); the matching return
    value is then None (nothing left for autograd to add)."""
    dy2d = _chk(dy2d, "dy")
    if x2d is None and weight is None:                           # bias gradient only (column sums of dY, e.g. a convolution's bias)
        if need_dx or need_dw or not need_db:
            raise RuntimeError("linear_bwd: without x and weight only the bias gradient can be asked for")
        if dy2d.dim() != 2:
            raise RuntimeError(f"linear_bwd: dy must be (M, N), got {tuple(dy2d.shape)}")
        m, n = dy2d.shape
        k = 32
    else:
        x2d, weight = _chk(x2d, "x"), _chk(weight, "weight")
        m, k = x2d.shape
        n = weight.shape[0]
        if dy2d.shape != (m, n) or weight.shape[1] != k:
            raise RuntimeError(f"linear_bwd: x {tuple(x2d.shape)}, weight {tuple(weight.shape)}, dy {tuple(dy2d.shape)} do not match")
    dev = dy2d.device
    dx = torch.empty(m, k, device=dev, dtype=torch.float32) if need_dx else None
    acc = 0
    dw = db = None
    if need_dw:
        if dw_out is not None:
            dw, acc = _chk_exact(dw_out, "dw_out", torch.float32, (n, k), "linear_bwd"), acc | 1
        else:
            dw = torch.empty(n, k, device=dev, dtype=torch.float32)
    if need_db:
        if db_out is not None:
            db, acc = _wr(db_out, "db_out", n, "linear_bwd"), acc | 2
        else:
            db = torch.empty(n, device=dev, dtype=torch.float32)
    wsb = _ws_bytes(("lbwd", m, n, k), "mumpy_linear_bwd_workspace_bytes", m, n, k)
    ws = _ws(wsb, dev)
    if _MATH == MATH_BF16:
        acc |= MATH_BF16                                      # bf16 operands on the bf16 MFMA, fp32 accumulate (config 5's arithmetic)
    elif _MATH != MATH_FP32:
        raise RuntimeError("linear_bwd: the split-precision modes have no one-call backward (autograd routes them through linear)")
    _call("mumpy_linear_bwd", _p(x2d), _p(weight), _p(dy2d), _p(dx), _p(dw), _p(db), m, n, k, acc, _p(ws), wsb, _stream(),
          work=2.0 * m * n * k * (int(need_dx) + int(need_dw)))
    return dx, (None if dw_out is not None else dw), (None if db_out is not None else db)


def linear_gelu_dual(x, weight, bias=None):
    """fc1 of an MLP on the training tape: -> (z, a) with z = x @ weight.T + bias and a = gelu(z), both fp32, from ONE launch
    (mumpy_linear_gelu_dual_fwd) -- the plan and kernels of linear(x, weight, bias, act=ACT_GELU) with a second store in the
    epilogue.  Follows set_matrix_math for "fp32" / "bf16"; the split-precision modes have no such kernel (an error, no fallback)."""
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    n, k = weight.shape[0], weight.numel() // weight.shape[0]
    if x.shape[-1] != k:
        raise RuntimeError(f"linear_gelu_dual: x has {x.shape[-1]} features, weight expects {k}")
    if _MATH not in (MATH_FP32, MATH_BF16):
        raise RuntimeError("linear_gelu_dual: the split-precision modes have no dual-output kernel")
    m = x.numel() // k
    z = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float32)
    a = torch.empty_like(z)
    wsb = _ws_bytes((m, n, k), "mumpy_linear_workspace_bytes", m, n, k)
    ws = _kept_workspace(wsb, x.device) if wsb else None
    _call("mumpy_linear_gelu_dual_fwd", _p(x), _p(weight), _p(_rd_opt(bias, "bias", n, "linear_gelu_dual")), _p(z), _p(a), m, n, k, _MATH, _p(ws),
          0 if ws is None else ws.numel() * 4, _stream(), work=2.0 * m * n * k)
    return z, a


def linear_gelu_bwd(a2d, z2d, weight, dy2d, need_dz=True, need_dw=True, need_db=False, dw_out=None, db_out=None):
    """Backward of y = a W^T + b for a = gelu(z) in ONE C-ABI call (mumpy_linear_gelu_bwd): -> (dz, dW, db) with
    dz = (dy W) o gelu'(z); dW / db and the accumulate-into-slot contract (dw_out / db_out) are linear_bwd's."""
    dy2d, a2d, z2d, weight = _chk(dy2d, "dy"), _chk(a2d, "a"), _chk(z2d, "z"), _chk(weight, "weight")
    m, k = a2d.shape
    n = weight.shape[0]
    if dy2d.shape != (m, n) or weight.shape[1] != k or z2d.shape != a2d.shape:
        raise RuntimeError(f"linear_gelu_bwd: a {tuple(a2d.shape)}, z {tuple(z2d.shape)}, weight {tuple(weight.shape)}, "
                           f"dy {tuple(dy2d.shape)} do not match")
    dev = dy2d.device
    dz = torch.empty(m, k, device=dev, dtype=torch.float32) if need_dz else None
    acc = 0
    dw = db = None
    if need_dw:
        if dw_out is not None:
            dw, acc = _chk_exact(dw_out, "dw_out", torch.float32, (n, k), "linear_gelu_bwd"), acc | 1
        else:
            dw = torch.empty(n, k, device=dev, dtype=torch.float32)
    if need_db:
        if db_out is not None:
            db, acc = _wr(db_out, "db_out", n, "linear_gelu_bwd"), acc | 2
        else:
            db = torch.empty(n, device=dev, dtype=torch.float32)
    wsb = _ws_bytes(("lgbwd", m, n, k), "mumpy_linear_gelu_bwd_workspace_bytes", m, n, k)
    ws = _ws(wsb, dev)
    if _MATH == MATH_BF16:
        acc |= MATH_BF16
    elif _MATH != MATH_FP32:
        raise RuntimeError("linear_gelu_bwd: the split-precision modes have no one-call backward")
    _call("mumpy_linear_gelu_bwd", _p(a2d), _p(z2d), _p(weight), _p(dy2d), _p(dz), _p(dw), _p(db), m, n, k, acc, _p(ws), wsb,
          _stream(), work=2.0 * m * n * k * (int(need_dz) + int(need_dw)))
    return dz, (None if dw_out is not None else dw), (None if db_out is not None else db)


def final_conv_bwd(x, w_krsc, dy):
    """Backward of final_conv for C = 32: x logical (B,32,H,W) NHWC, w_krsc (1,3,3,32), dy (B,1,H,W) ->
    (dx like x, dw (1,3,3,32), db (1,)).  One streaming pass + a small fixed-tree reduce."""
    x = _nhwc(x, "x")
    b, c, h, w = x.shape
    dy = _rd(dy, "dy", b * h * w, "final_conv_bwd")
    if c != 32 or tuple(w_krsc.shape) != (1, 3, 3, 32):
        raise RuntimeError(f"final_conv_bwd is built for Conv2d(32, 1, 3, padding=1); got C={c}, weight {tuple(w_krsc.shape)}")
    dx = empty_nhwc(b, c, h, w, x.device)
    dw = torch.empty(1, 3, 3, 32, device=x.device, dtype=torch.float32)
    db = torch.empty(1, device=x.device, dtype=torch.float32)
    wsb = int(_lib().mumpy_final_conv_bwd_workspace_bytes(b, h, w))
    ws = _ws(wsb, x.device)
    _call("mumpy_final_conv_bwd", _p(x), _p(_chk(w_krsc, "weight")), _p(dy), _p(dx), _p(dw), _p(db), _p(ws), wsb, b, h, w, c, _stream(),
          work=4.0 * (2 * x.numel() + dy.numel()))
    return dx, dw, db


def patch_gather(x, b, h, w, c, inverse=False):
    """PatchMerging's 2x2 gather (swin:357-361): x (b,h,w,c) -> (b, h/2 * w/2, 4c); inverse=True maps a merged-layout tensor back to
    (b, h*w, c) (the gather's backward) -- one permutation launch either way."""
    x = _chk(x, "x")
    if x.numel() != b * h * w * c:
        raise RuntimeError(f"patch_gather: {tuple(x.shape)} is not {b} x {h} x {w} x {c}")
    out = torch.empty((b, h * w, c) if inverse else (b, (h // 2) * (w // 2), 4 * c), device=x.device, dtype=torch.float32)
    _call("mumpy_patch_gather_fwd", _p(x), _p(out), b, h, w, c, int(inverse), _stream(), work=8.0 * x.numel())
    return out


def conv_weight_dgrad(w_krsc):
    """(Cout,kh,kw,Cin) -> (Cin,kh,kw,Cout) with the taps flipped: the weight of the data-gradient convolution, one launch."""
    w_krsc = _chk(w_krsc, "weight")
    cout, kh, kw, cin = w_krsc.shape
    out = torch.empty(cin, kh, kw, cout, device=w_krsc.device, dtype=torch.float32)
    _call("mumpy_conv_weight_dgrad_fwd", _p(w_krsc), _p(out), cout, cin, kh, kw, _stream(), work=8.0 * out.numel())
    return out


def conv2d_wgrad(x, dy, kh, kw, dw_out=None):
    """Weight gradient of conv2d_nhwc in one launch over all taps: x logical (B,Cin,H,W), dy logical (B,Cout,H,W), both NHWC
    memory -> dW (Cout,kh,kw,Cin).  dw_out: a buffer to ACCUMULATE into (returns None then)."""
    x, dy = _nhwc(x, "x"), _nhwc(dy, "dy")
    b, cin, h, w = x.shape
    cout = dy.shape[1]
    if dy.shape != (b, cout, h, w):
        raise RuntimeError(f"conv2d_wgrad: x {tuple(x.shape)} and dy {tuple(dy.shape)} do not match")
    acc = dw_out is not None
    dw = _chk_exact(dw_out, "dw_out", torch.float32, (cout, kh, kw, cin), "conv2d_wgrad") if acc else \
        torch.empty(cout, kh, kw, cin, device=x.device, dtype=torch.float32)
    wsb = _ws_bytes(("cwgrad", b, h, w, cin, cout, kh, kw), "mumpy_conv2d_wgrad_workspace_bytes", b, h, w, cin, cout, kh, kw)
    ws = _ws(wsb, x.device) if wsb else None
    if _MATH not in (MATH_FP32, MATH_BF16):
        raise RuntimeError("conv2d_wgrad: the split-precision modes have no one-launch weight gradient")
    _call("mumpy_conv2d_wgrad_nhwc", _p(x), _p(dy), _p(dw), b, h, w, cin, cout, kh, kw, int(acc) | (MATH_BF16 if _MATH == MATH_BF16 else 0),
          _p(ws), wsb, _stream(),
          work=2.0 * b * h * w * cout * kh * kw * cin)
    return None if acc else dw


def col_sum(x2d):
    x2d = _chk(x2d, "x")
    r, c = x2d.shape
    out = torch.empty(c, device=x2d.device, dtype=torch.float32)
    wsb = int(_lib().mumpy_col_sum_workspace_bytes(r, c))
    ws = _ws(wsb, x2d.device)
    _call("mumpy_col_sum_fwd", _p(x2d), _p(out), _p(ws), wsb, r, c, _stream(), work=4.0 * x2d.numel())
    return out


def rel_index_csr(index: torch.Tensor) -> torch.Tensor:
    """Inverse of a `relative_position_index` buffer for the table-gradient kernel: int32 [ptr (170) | pairs (2401)], the pairs
    p = 49 i + j of one table entry contiguous and in increasing order.  Built once (host side, one synchronisation) and kept ON the
    buffer object like rel_index32's image: call it from the forward (eager warm-up), never for the first time under graph capture."""
    t = getattr(index, "_mumpy_csr", None)
    if t is None or t.device != index.device or getattr(index, "_mumpy_csr_version", -1) != index._version:
        idx = index.reshape(-1).to("cpu", torch.int64)
        if idx.numel() != 49 * 49 or int(idx.min()) < 0 or int(idx.max()) >= 169:
            raise RuntimeError("rel_index_csr: expected a (49,49) relative_position_index with values in [0, 169)")
        order = torch.sort(idx, stable=True).indices
        ptr = torch.zeros(170, dtype=torch.int64)
        ptr[1:] = torch.cumsum(torch.bincount(idx, minlength=169), 0)
        t = torch.cat([ptr, order]).to(torch.int32).to(index.device)
        index._mumpy_csr, index._mumpy_csr_version = t, index._version
    return t


def window_attention_bwd(qkv, dout, bias_pad, rel_index32, b, hs, w, c, shift, scale, mask_tab=None, mask_id=None, dtable_out=None,
                         rel_csr=None, math="fp32"):
    """-> (dqkv (B, hs*w, 3C), dtable (169, C/32)): gradients of the W-MSA core wrt qkv and the relative position bias table.
    dtable_out: a gradient buffer to ACCUMULATE into (the returned dtable is then None).  rel_csr = rel_index_csr(index): the table
    gradient reads its pairs through the inverse index instead of scanning the index.  math: "fp32" (default; it does NOT follow
    set_attention_math) or "bf16", the backward of window_attention_mm16 (mumpy_window_attention_mm16_bwd)."""
    _choice(math, _ATTN_MATHS, _ATTN_WHAT)
    qkv, dout = _chk(qkv, "qkv"), _chk(dout, "dout")
    if qkv.numel() != b * hs * w * 3 * c or dout.numel() != b * hs * w * c:
        raise RuntimeError("window_attention_bwd: shape mismatch")
    if rel_index32.dtype != torch.int32 or rel_index32.numel() != 49 * 49 or not rel_index32.is_cuda:
        raise RuntimeError("window_attention_bwd: rel_index32 must be the (49*49) int32 relative_position_index on the GPU")
    dqkv = torch.empty_like(qkv)
    acc = dtable_out is not None
    dtable = _chk_exact(dtable_out, "dtable_out", torch.float32, (169, c // 32), "window_attention_bwd") if acc else \
        torch.empty(169, c // 32, device=qkv.device, dtype=torch.float32)
    bias_pad = _rd(bias_pad, "bias", (c // 32) * 64 * 64, "window_attention_bwd")
    mask_tab, mask_id, n_mask = _chk_mask(mask_tab, mask_id, b * (hs // 7) * (w // 7), "window_attention_bwd")
    rel_index32 = rel_index32.contiguous()
    if rel_csr is not None:
        if rel_csr.dtype != torch.int32 or rel_csr.numel() != 170 + 49 * 49 or rel_csr.device != qkv.device:
            raise RuntimeError("window_attention_bwd: rel_csr must come from ops.rel_index_csr on this device")
        rel_csr = rel_csr.contiguous()
    if math == "bf16":
        wsb = _ws_bytes(("wabwd16", b, hs, w, c), "mumpy_window_attention_mm16_bwd_workspace_bytes", b, hs, w, c)
    else:
        wsb = _ws_bytes(("wabwd", b, hs, w, c), "mumpy_window_attention_bwd_workspace_bytes", b, hs, w, c)
    ws = _ws(wsb, qkv.device)
    if math == "bf16":
        name, csr_args = "mumpy_window_attention_mm16_bwd", (_p(rel_csr),)        # one entry: a null rel_csr selects the scanning kernel
    else:
        name, csr_args = "mumpy_window_attention_bwd" + ("" if rel_csr is None else "_csr"), (() if rel_csr is None else (_p(rel_csr),))
    _call(name, _p(qkv), _p(dout), _p(bias_pad), _p(mask_tab),
          _p(mask_id), n_mask, _p(rel_index32), *csr_args, _p(dqkv), _p(dtable), _p(ws), wsb, b, hs, w, c, shift, scale, int(acc), _stream(),
          work=5 * 153664.0 * b * (hs // 7) * (w // 7) * (c // 32))
    return dqkv, (None if acc else dtable)


GN_ACCUMULATE = 0x100     # mumpy_hip.h: MUMPY_GN_ACCUMULATE


def gn_bwd(z, stats, gamma, beta, dy, groups, eps=1e-5, act=ACT_RELU, dg_out=None, db_out=None):
    """GroupNorm(+activation) backward on NHWC: z, dy logical (B,C,H,W) with NHWC memory; stats = (partial, nsplit) from
    gn_stats(z); act = 0 / ACT_RELU / ACT_SIGMOID is the activation that followed the norm.  -> (dz like z, dgamma, dbeta);
    with dg_out AND db_out the parameter gradients are ACCUMULATED into those buffers (grad slots) and returned as None."""
    z, dy = _nhwc(z, "z"), _nhwc(dy, "dy")
    b, c, h, w = z.shape
    if dy.shape != z.shape:
        raise RuntimeError(f"gn_bwd: z {tuple(z.shape)} and dy {tuple(dy.shape)} do not match")
    partial, nsplit = stats
    partial = _rd(partial, "partial", b * nsplit * groups * 2, "gn_bwd")
    gamma, beta = _rd(gamma, "gamma", c, "gn_bwd"), _rd(beta, "beta", c, "gn_bwd")
    dz = empty_nhwc(b, c, h, w, z.device)
    acc = dg_out is not None and db_out is not None
    dg = _wr(dg_out, "dg_out", c, "gn_bwd") if acc else torch.empty(c, device=z.device, dtype=torch.float32)
    db = _wr(db_out, "db_out", c, "gn_bwd") if acc else torch.empty(c, device=z.device, dtype=torch.float32)
    wsb = int(_lib().mumpy_gn_bwd_workspace_bytes(b, h * w, c))
    ws = _ws(wsb, z.device)
    _call("mumpy_gn_bwd_nhwc", _p(z), _p(partial), nsplit, _p(gamma), _p(beta), _p(dy), _p(dz), _p(dg),
          _p(db), _p(ws), wsb, b, h * w, c, groups, eps, int(act) | (GN_ACCUMULATE if acc else 0), _stream(), work=20.0 * z.numel())
    return (dz, None, None) if acc else (dz, dg, db)


def upsample_bwd(dy, scale=2, align_corners=True):
    """dy logical (B,C,sH,sW) NHWC -> dx (B,C,H,W) NHWC: backward of the bilinear x2 / x4 upsample."""
    dy = _nhwc(dy, "dy")
    b, c, ho, wo = dy.shape
    dx = empty_nhwc(b, c, ho // scale, wo // scale, dy.device)
    _call("mumpy_upsample_bwd_nhwc", _p(dy), _p(dx), b, ho // scale, wo // scale, c, scale, 1 if align_corners else 0, _stream(),
          work=4.0 * (dy.numel() + dx.numel()))
    return dx


def upsample2x_bwd(dy, align_corners=True):
    return upsample_bwd(dy, 2, align_corners)


def scale_samples(x, scale):
    """out[b] = x[b] * scale[b] (stochastic depth); x (B, ...), scale (B,) on the GPU."""
    x, scale = _chk(x, "x"), _chk(scale, "scale")
    b = x.shape[0]
    if scale.numel() != b:
        raise RuntimeError("scale_samples: one scale per sample")
    out = torch.empty_like(x)
    _call("mumpy_scale_samples_fwd", _p(x), _p(scale), _p(out), b, x.numel() // b, _stream(), work=8.0 * x.numel())
    return out


def temporal_attention_bwd(qkv, dout, s_, t, c, heads, scale):
    qkv, dout = _rd(qkv, "qkv", s_ * t * 3 * c, "temporal_attention_bwd"), _rd(dout, "dout", s_ * t * c, "temporal_attention_bwd")
    dqkv = torch.empty_like(qkv)
    _call("mumpy_temporal_attention_bwd", _p(qkv), _p(dout), _p(dqkv), s_, t, c, heads, scale, _stream(), work=4.0 * (2 * qkv.numel() + dout.numel()))
    return dqkv


# ------------------------------------------------------------------------------- deformable attention, training (row 10)
def dwconv5_window(x, w25, b):
    """x (N,49,C) token-major windows, w25 (C,25), b (C) -> (N,49,C): depthwise 5x5 conv (padding 2) inside each 7x7 window."""
    x = _chk(x, "x")
    n, p49, c = x.shape
    if p49 != 49:
        raise RuntimeError(f"dwconv5_window: x must be (N, 49, C), got {tuple(x.shape)}")
    w25, b = _rd(w25, "w", c * 25, "dwconv5_window"), _rd(b, "b", c, "dwconv5_window")
    u = torch.empty_like(x)
    _call("mumpy_dwconv5_window_fwd", _p(x), _p(w25), _p(b), _p(u), n, c, _stream(), work=8.0 * x.numel())
    return u


def dwconv5_window_bwd(x, w25, du):
    """-> (dx (N,49,C), dw (C,25), db (C))."""
    x = _chk(x, "x")
    n, p49, c = x.shape
    if p49 != 49:
        raise RuntimeError(f"dwconv5_window_bwd: x must be (N, 49, C), got {tuple(x.shape)}")
    du, w25 = _rd(du, "du", x.numel(), "dwconv5_window_bwd"), _rd(w25, "w", c * 25, "dwconv5_window_bwd")
    dx = torch.empty_like(x)
    dw_t = torch.empty(26, c, device=x.device, dtype=torch.float32)       # rows 0..24 = taps; row 25 unused scratch
    db = torch.empty(c, device=x.device, dtype=torch.float32)
    wsb = int(_lib().mumpy_dwconv5_window_bwd_workspace_bytes(n, c))
    ws = _ws(wsb, x.device)
    _call("mumpy_dwconv5_window_bwd", _p(x), _p(w25), _p(du), _p(dx), _p(dw_t), _p(db), _p(ws), wsb, n, c, _stream(),
          work=16.0 * x.numel())
    return dx, transpose(dw_t[:25].contiguous()), db


def _grouped_bwd(entry, groups, nq, who):
    """_grouped() for the backward ops, which see window counts and no batch: -> (C-ABI entry, trailing arguments before the stream)
    for groups = 1 (the frozen entry, called exactly as before) or more (its _grouped form, include/mumpy_hip_ext9.h)."""
    if not isinstance(groups, int) or isinstance(groups, bool) or groups < 1 or not isinstance(nq, int) or nq < 1 or nq % groups:
        raise ValueError(f"{who}: groups={groups!r} must be a positive int that divides the {nq} q windows")
    return (entry, ()) if groups == 1 else (entry.replace("_bwd", "_grouped_bwd"), (groups,))


def deform_sample_bwd(x2w, pos, dsampled, groups=1):
    """window form: x2w, dsampled (B2,49,C), pos (nq,3,49,2) -> (dx2 (B2,49,C), dpos (nq,3,49,2)).  groups: the pairing rule of the
    forward this differentiates (cva_pairing): 1 is the reference's `i mod nq`."""
    entry, extra = _grouped_bwd("mumpy_deform_sample_bwd", groups, pos.shape[0] if pos.dim() else 0, "deform_sample_bwd")
    x2w, pos = _chk(x2w, "x2"), _chk(pos, "pos")
    b2, p49, c = x2w.shape
    nq = pos.shape[0]
    if p49 != 49 or nq < 1 or b2 % nq or pos.numel() != nq * 3 * 49 * 2:
        raise RuntimeError(f"deform_sample_bwd: x2 (B2, 49, C) and pos (nq, 3, 49, 2) with nq dividing B2, got {tuple(x2w.shape)} and {tuple(pos.shape)}")
    dsampled = _rd(dsampled, "dsampled", x2w.numel(), "deform_sample_bwd")
    dx2 = torch.empty_like(x2w)
    part = torch.empty(b2, 3, 49, 2, device=x2w.device, dtype=torch.float32)
    _call(entry, _p(x2w), _p(pos), _p(dsampled), _p(dx2), _p(part), b2, c, nq, *extra, _stream(), work=12.0 * x2w.numel())
    if groups == 1:
        # kv windows qw + m*nq share q window qw: a (r, nq, ...) view summed over r (a few KB: left to torch)
        return dx2, part.view(b2 // nq, nq, 3, 49, 2).sum(0)
    # per group the same: slots (g, m, j) share q window g*nqg + j (cva_pairing_members)
    return dx2, part.view(groups, b2 // nq, nq // groups, 3, 49, 2).sum(1).reshape(nq, 3, 49, 2)


def deform_attention_bwd(q, kv, dout, r, scale, math="fp32", groups=1):
    """window form: q (B1,49,C), kv (B1*r,49,2C), dout (B1,49,C) -> (dq (B1,49,C), dkv (B1*r,49,2C)).  math: "fp32" (default; it does
    NOT follow set_cva_math) or "bf16", the backward of deform_attention(..., math="bf16") (mumpy_deform_attention_mm16_bwd): the
    operands rounded to bf16 in registers, every product on the bf16 MFMA, softmax / D / dS and accumulation in fp32, and dq summed
    over its r kv windows on the device in a fixed order (no partial slices, no add launches).  groups: the pairing rule of the
    forward this differentiates (cva_pairing): 1 is the reference's `i mod B1`; G > 1 sums, per group, the same r contributions in
    the same order as groups = 1 does on that group alone."""
    _choice(math, _CVA_MATHS, _CVA_WHAT)
    entry, extra = _grouped_bwd("mumpy_deform_attention_mm16_bwd" if math == "bf16" else "mumpy_deform_attention_bwd", groups,
                                q.shape[0] if q.dim() else 0, "deform_attention_bwd")
    q = _chk(q, "q")
    b1, p49, c = q.shape
    b2 = b1 * r
    if p49 != 49:
        raise RuntimeError(f"deform_attention_bwd: q must be (B1, 49, C), got {tuple(q.shape)}")
    kv, dout = _rd(kv, "kv", b2 * 49 * 2 * c, "deform_attention_bwd"), _rd(dout, "dout", q.numel(), "deform_attention_bwd")
    if math == "bf16":
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        wsb = _ws_bytes(("cvabwd16", b1, r, c), "mumpy_deform_attention_mm16_bwd_workspace_bytes", b1, r, c)
        ws = _ws(wsb, q.device)
        _call(entry, _p(q), _p(kv), _p(dout), _p(dq), _p(dkv), _p(ws), wsb, b1, r, c, scale, *extra, _stream(),
              work=5 * 153664.0 * b2 * (c // 32))
        return dq, dkv
    part = torch.empty(b2, 49, c, device=q.device, dtype=torch.float32)
    dkv = torch.empty_like(kv)
    wsb = int(_lib().mumpy_deform_attention_bwd_workspace_bytes(b2, c))
    ws = _ws(wsb, q.device)
    _call(entry, _p(q), _p(kv), _p(dout), _p(part), _p(dkv), _p(ws), wsb, b1, r, c, scale, *extra, _stream(),
          work=5 * 153664.0 * b2 * (c // 32))
    if groups == 1:
        dq = part[:b1]
        for m in range(1, r):                                             # kv windows qw + m*B1 pair with q window qw: fixed order
            dq = add(dq.contiguous(), part[m * b1:(m + 1) * b1].contiguous())
        return dq.contiguous(), dkv
    slots = part.view(groups, r, b1 // groups, 49, c)                     # slots (g, m, j) pair with q window g*nqg + j: same order
    dq = slots[:, 0]
    for m in range(1, r):
        dq = add(dq.contiguous(), slots[:, m].contiguous())
    return dq.reshape(b1, 49, c).contiguous(), dkv


def adamw_hyper(step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
    """The 8 fp32 constants of one AdamW step as a pinned host tensor (for adamw_step_dev under hipGraph replay)."""
    return _hyper_out("mumpy_adamw_hyper", 8, lr, betas[0], betas[1], eps, weight_decay, int(step), grad_scale)


def adamw_step_dev(param, grad, exp_avg, exp_avg_sq, hyper_dev):
    """AdamW over flat buffers with the step constants in the device tensor `hyper_dev` (8 floats): capturable."""
    n = param.numel()
    _flat_bufs("adamw_step_dev", n, param=param, grad=grad, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq)
    _call("mumpy_adamw_step_dev", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(_chk_hyper("adamw_step_dev", hyper_dev, 8)), _stream(),
          work=28.0 * n)
    return param


def _chk_hyper(fn, hyper, count):
    """The staged device constants of a step: read where they are (grad_norm_finish scales them in place)."""
    if not hyper.is_cuda or hyper.dtype != torch.float32 or hyper.numel() < count or not hyper.is_contiguous():
        raise RuntimeError(f"{fn}: hyper must be a contiguous float32 GPU tensor of at least {count} constants")
    return hyper


def _flat_bufs(fn, n, **bufs):
    """The contiguity / size checks of adamw_step for the in-place optimizer buffers (None = buffer not used)."""
    for name, t in bufs.items():
        if t is None:
            continue
        _chk(t, name)
        if t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"{fn}: {name} must be a contiguous buffer of {n} elements (in-place update)")


def _hyper_out(fn, count, *args, dtype=torch.float32):
    """The `count` host constants that the C function `fn` derives from `args`, as a pinned tensor (float32, or float64)."""
    import ctypes
    out = torch.empty(count, dtype=dtype).pin_memory()
    ctype = ctypes.c_double if dtype == torch.float64 else ctypes.c_float
    rc = getattr(_lib(), fn)(ctypes.cast(out.data_ptr(), ctypes.POINTER(ctype)), *args)
    if rc != 0:
        raise RuntimeError(f"{fn} failed (rc={rc}): {_lib().mumpy_last_error().decode()}")
    return out


def sgd_step(param, grad, momentum_buf, lr, momentum=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0, dampening=0.0):
    """In-place fused SGD over flat fp32 buffers (torch.optim.SGD semantics; momentum_buf None when momentum == 0; a zero
    buffer reproduces torch's first step).  dampening must be 0."""
    n = param.numel()
    _flat_bufs("sgd_step", n, param=param, grad=grad, momentum_buf=momentum_buf)
    _call("mumpy_sgd_step", _p(param), _p(grad), _p(momentum_buf), n, lr, momentum, dampening, weight_decay, int(bool(nesterov)),
          grad_scale, _stream(), work=(20.0 if momentum_buf is not None else 12.0) * n)
    return param


def sgd_hyper(lr, momentum=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0, dampening=0.0):
    """The 4 fp32 constants of one SGD step as a pinned host tensor (for sgd_step_dev under hipGraph replay)."""
    return _hyper_out("mumpy_sgd_hyper", 4, lr, momentum, dampening, weight_decay, int(bool(nesterov)), grad_scale)


def sgd_step_dev(param, grad, momentum_buf, hyper_dev, nesterov=False):
    """SGD over flat buffers with the step constants in the device tensor `hyper_dev` (4 floats): capturable."""
    n = param.numel()
    _flat_bufs("sgd_step_dev", n, param=param, grad=grad, momentum_buf=momentum_buf)
    _call("mumpy_sgd_step_dev", _p(param), _p(grad), _p(momentum_buf), n, _p(_chk_hyper("sgd_step_dev", hyper_dev, 4)), int(bool(nesterov)),
          _stream(), work=(20.0 if momentum_buf is not None else 12.0) * n)
    return param


def rmsprop_step(param, grad, square_avg, momentum_buf, lr, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0,
                 grad_scale=1.0):
    """In-place fused RMSprop over flat fp32 buffers (torch.optim.RMSprop semantics, centered=False; momentum_buf None
    when momentum == 0)."""
    n = param.numel()
    _flat_bufs("rmsprop_step", n, param=param, grad=grad, square_avg=square_avg, momentum_buf=momentum_buf)
    _call("mumpy_rmsprop_step", _p(param), _p(grad), _p(square_avg), _p(momentum_buf), n, lr, alpha, eps, weight_decay, momentum,
          grad_scale, _stream(), work=(28.0 if momentum_buf is not None else 20.0) * n)
    return param


def rmsprop_hyper(lr, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, grad_scale=1.0):
    """The 8 fp32 constants of one RMSprop step as a pinned host tensor (for rmsprop_step_dev under hipGraph replay)."""
    return _hyper_out("mumpy_rmsprop_hyper", 8, lr, alpha, eps, weight_decay, momentum, grad_scale)


def rmsprop_step_dev(param, grad, square_avg, momentum_buf, hyper_dev):
    """RMSprop over flat buffers with the step constants in the device tensor `hyper_dev` (8 floats): capturable."""
    n = param.numel()
    _flat_bufs("rmsprop_step_dev", n, param=param, grad=grad, square_avg=square_avg, momentum_buf=momentum_buf)
    _call("mumpy_rmsprop_step_dev", _p(param), _p(grad), _p(square_avg), _p(momentum_buf), n, _p(_chk_hyper("rmsprop_step_dev", hyper_dev, 8)),
          _stream(), work=(28.0 if momentum_buf is not None else 20.0) * n)
    return param


GRAD_NORM_MAX_GROUPS = 8
_OPT_KINDS = {"AdamW": 0, "SGD": 1, "RMSprop": 2}        # MUMPY_OPT_* of include/mumpy_hip.h, keyed by _FlatOptimizer.KIND


def grad_norm_partials(n):
    """Partials that grad_norm_partial writes for a flat buffer of n floats (a pure host function of n); the partials buffer of a
    group holds twice as many 4-byte words: the fp32 sums of squares, then the uint32 counts of non-finite elements."""
    return int(_lib().mumpy_grad_norm_partials(int(n)))


def grad_norm_partial(grad, partials):
    """One streaming read of the flat gradient buffer `grad`: per-workgroup sums of squares and non-finite counts into `partials`
    (2 * grad_norm_partials(grad.numel()) floats; the second half holds integers).  `grad` is not written.  Capturable."""
    n = grad.numel()
    _flat_bufs("grad_norm_partial", n, grad=grad)
    need = 2 * grad_norm_partials(n)
    _chk(partials, "partials")
    if n < 1 or partials.numel() != need or not partials.is_contiguous():
        raise RuntimeError(f"grad_norm_partial: partials must be a contiguous buffer of {need} floats for a gradient of {n}")
    _call("mumpy_grad_norm_partial", _p(grad), n, _p(partials), _stream(), work=4.0 * n)
    return partials


def grad_norm_finish(partials, sizes, hypers, kinds, stats, max_norm=None):
    """Finish of up to 8 groups: `partials[g]` from grad_norm_partial over a buffer of `sizes[g]` floats, `hypers[g]` the staged
    device constants of that group's *_step_dev, `kinds[g]` its _FlatOptimizer.KIND.  Writes stats = [total_norm, coef, non-finite
    count, 0, norm_0 ... norm_{G-1}] (4 + G floats) and, when max_norm is given, multiplies every group's staged gradient scale by
    coef = min(1, max_norm / (total_norm + 1e-6)) in place.  max_norm None: measure only (coef = 1, `hypers` untouched).
    Capturable: the tables are packed into the launch on the host."""
    import ctypes
    groups = len(partials)
    if not (len(sizes) == len(hypers) == len(kinds) == groups):
        raise RuntimeError("grad_norm_finish: one partials buffer, size, hyper buffer and optimizer kind per group")
    if groups > GRAD_NORM_MAX_GROUPS:
        raise ValueError(f"grad_norm_finish: {groups} groups (at most {GRAD_NORM_MAX_GROUPS})")
    for g, (p, n, h, k) in enumerate(zip(partials, sizes, hypers, kinds)):
        if k not in _OPT_KINDS:
            raise ValueError(f"grad_norm_finish: unknown optimizer kind {k!r} (group {g})")
        _chk(p, "partials")
        if not p.is_contiguous() or p.numel() != 2 * grad_norm_partials(n):
            raise RuntimeError(f"grad_norm_finish: partials of group {g} must hold {2 * grad_norm_partials(n)} floats")
        _chk_hyper(f"grad_norm_finish (group {g})", h, 4 if k == "SGD" else 8)
    _chk(stats, "stats")
    if not stats.is_contiguous() or stats.numel() != 4 + groups:
        raise RuntimeError(f"grad_norm_finish: stats must be a contiguous buffer of {4 + groups} floats")
    if max_norm is not None and not float(max_norm) > 0.0:
        raise ValueError(f"grad_norm_finish: max_norm must be positive, got {max_norm}")
    ptrs = (ctypes.c_void_p * groups)(*[_p(p) for p in partials])
    hyps = (ctypes.c_void_p * groups)(*[_p(h) for h in hypers])
    ns = (ctypes.c_int64 * groups)(*[int(n) for n in sizes])
    ks = (ctypes.c_int * groups)(*[_OPT_KINDS[k] for k in kinds])
    _call("mumpy_grad_norm_finish", ptrs, ns, hyps, ks, groups, int(max_norm is not None), float(max_norm or 0.0), _p(stats),
          _stream(), work=8.0 * sum(grad_norm_partials(n) for n in sizes))
    return stats


# ---- skipping the update of a step whose gradient is non-finite (include/mumpy_hip_ext.h; train.UpdateGuard) ----
UPDATE_GATE_MAX = 8        # statistics buffers, and groups, behind one gate
GATE_WORDS = 8             # [skip, skipped, consecutive, updates, longest, 0, 0, 0] (uint32, kept in an int32 tensor)


def adamw_gate_hyper(step, lr, betas=(0.9, 0.999)):
    """The 4 doubles {lr, beta1, beta2, step} mumpy_update_gate re-derives AdamW's bias corrections from, as a pinned host tensor
    (staged beside adamw_hyper's 8 floats; `step` is the nominal count those were derived from)."""
    return _hyper_out("mumpy_adamw_gate_hyper", 4, lr, betas[0], betas[1], int(step), dtype=torch.float64)


def _chk_gate(fn, gate):
    if not gate.is_cuda or gate.dtype != torch.int32 or gate.numel() != GATE_WORDS or not gate.is_contiguous():
        raise RuntimeError(f"{fn}: gate must be a contiguous int32 GPU tensor of {GATE_WORDS} words")
    return gate


def update_gate(stats, gate, hypers, kinds, applied, adam_raw):
    """One launch at the head of an update, after every grad_norm_finish of the step: gate[0] = 1 if any of the `stats` buffers
    (1 ... 8) reports a non-finite gradient element or a NaN norm, else 0; the skip counters in gate[1 ... 4]; unless skipped,
    applied[g] += 1 for every group (1 ... 8: `kinds[g]` its _FlatOptimizer.KIND, `hypers[g]` its staged device constants, read
    for AdamW only), and an AdamW group whose applied count differs from the nominal count in adam_raw[4 g + 3] gets its two
    bias-correction constants recomputed from adam_raw[4 g : 4 g + 3] = (lr, beta1, beta2).  `applied`: int64, one per group;
    `adam_raw`: float64, 4 per group.  Capturable: the tables are packed into the launch on the host."""
    import ctypes
    groups = len(kinds)
    if not 1 <= len(stats) <= UPDATE_GATE_MAX:
        raise ValueError(f"update_gate: {len(stats)} statistics buffers (1 to {UPDATE_GATE_MAX})")
    if not 1 <= groups <= UPDATE_GATE_MAX:
        raise ValueError(f"update_gate: {groups} groups (1 to {UPDATE_GATE_MAX})")
    if len(hypers) != groups:
        raise RuntimeError("update_gate: one hyper buffer and optimizer kind per group")
    for s in stats:
        _chk(s, "stats")
        if not s.is_contiguous() or s.numel() < 4:
            raise RuntimeError("update_gate: a statistics buffer must be a contiguous buffer of at least 4 floats")
    for g, (h, k) in enumerate(zip(hypers, kinds)):
        if k not in _OPT_KINDS:
            raise ValueError(f"update_gate: unknown optimizer kind {k!r} (group {g})")
        _chk_hyper(f"update_gate (group {g})", h, 4 if k == "SGD" else 8)
    _chk_gate("update_gate", gate)
    if not applied.is_cuda or applied.dtype != torch.int64 or applied.numel() != groups or not applied.is_contiguous():
        raise RuntimeError(f"update_gate: applied must be a contiguous int64 GPU tensor of {groups} counts")
    if not adam_raw.is_cuda or adam_raw.dtype != torch.float64 or adam_raw.numel() != 4 * groups or not adam_raw.is_contiguous():
        raise RuntimeError(f"update_gate: adam_raw must be a contiguous float64 GPU tensor of {4 * groups} values")
    sts = (ctypes.c_void_p * len(stats))(*[_p(s) for s in stats])
    hyps = (ctypes.c_void_p * groups)(*[_p(h) for h in hypers])
    ks = (ctypes.c_int * groups)(*[_OPT_KINDS[k] for k in kinds])
    _call("mumpy_update_gate", sts, len(stats), _p(gate), hyps, ks, groups, _p(applied), _p(adam_raw), _stream())
    return gate


def adamw_step_gated_dev(param, grad, exp_avg, exp_avg_sq, hyper_dev, gate):
    """adamw_step_dev behind `gate` (update_gate): nothing is read or written when gate[0] != 0, the same bits otherwise."""
    n = param.numel()
    _flat_bufs("adamw_step_gated_dev", n, param=param, grad=grad, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq)
    _call("mumpy_adamw_step_gated_dev", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(_chk_hyper("adamw_step_gated_dev", hyper_dev, 8)),
          _p(_chk_gate("adamw_step_gated_dev", gate)), _stream(), work=28.0 * n)
    return param


def sgd_step_gated_dev(param, grad, momentum_buf, hyper_dev, gate, nesterov=False):
    """sgd_step_dev behind `gate` (as adamw_step_gated_dev)."""
    n = param.numel()
    _flat_bufs("sgd_step_gated_dev", n, param=param, grad=grad, momentum_buf=momentum_buf)
    _call("mumpy_sgd_step_gated_dev", _p(param), _p(grad), _p(momentum_buf), n, _p(_chk_hyper("sgd_step_gated_dev", hyper_dev, 4)), int(bool(nesterov)),
          _p(_chk_gate("sgd_step_gated_dev", gate)), _stream(), work=(20.0 if momentum_buf is not None else 12.0) * n)
    return param


def rmsprop_step_gated_dev(param, grad, square_avg, momentum_buf, hyper_dev, gate):
    """rmsprop_step_dev behind `gate` (as adamw_step_gated_dev)."""
    n = param.numel()
    _flat_bufs("rmsprop_step_gated_dev", n, param=param, grad=grad, square_avg=square_avg, momentum_buf=momentum_buf)
    _call("mumpy_rmsprop_step_gated_dev", _p(param), _p(grad), _p(square_avg), _p(momentum_buf), n, _p(_chk_hyper("rmsprop_step_gated_dev", hyper_dev, 8)),
          _p(_chk_gate("rmsprop_step_gated_dev", gate)), _stream(), work=(28.0 if momentum_buf is not None else 20.0) * n)
    return param
