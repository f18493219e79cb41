"""The opt-in bf16-MFMA window attention for bf16-stored qkv (mumpy_window_attention_bf16mm_fwd, ops.set_attention_math):
C ABI and switch on the CPU; layout, accuracy, determinism, the untouched fp32 paths, the whole model and graph replay on the GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT, rel_err, rms_err
from weight_fill import fill_module_, seeded_randn

gpu = pytest.mark.gpu
NAME = "mumpy_window_attention_bf16mm_fwd"
SCALE = 32 ** -0.5

if torch.cuda.is_available():
    from oracle import mumpy_oracle as O
    DEV = torch.device("cuda:0")


# ------------------------------------------------------------------ CPU: ABI and the switch
def _header_args(name):
    src = open(os.path.join(ROOT, "include", "mumpy_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    return None if m is None else [a.strip() for a in m.group(1).split(",")]


def test_c_abi_declares_exports_binds_and_validates():
    from mumpy_hip.lib import SIGNATURES, library_path, load_library, tuning_library_path
    args = _header_args(NAME)
    assert args is not None, f"{NAME} is not declared in include/mumpy_hip.h"
    assert args == _header_args("mumpy_window_attention_bf16_fwd")            # same arguments as the fp32-flow entry

    def kind(carg):
        if "*" in carg:
            return "ptr"
        return {"int": "int", "int64_t": "i64", "float": "f32", "double": "f64"}[carg.rsplit(None, 1)[0].replace("const ", "").strip()]

    def ckind(t):
        return "ptr" if t is ctypes.c_void_p else {ctypes.c_int: "int", ctypes.c_int64: "i64", ctypes.c_float: "f32", ctypes.c_double: "f64"}[t]

    assert NAME in SIGNATURES and [ckind(t) for t in SIGNATURES[NAME]] == [kind(a) for a in args]
    for path in (library_path(), tuning_library_path()):
        assert hasattr(ctypes.CDLL(path), NAME), f"{path} does not export {NAME}"
    lib = load_library()
    assert lib.mumpy_abi_version() == 2                                        # an added symbol changes no existing call
    fn = getattr(lib, NAME)
    # rejected before anything is launched: safe without a GPU
    assert fn(16, 16, 16, None, None, 0, 1, 10, 14, 96, 0, 0.1, None) == -1    # grid not divisible by 7
    assert fn(None, None, None, None, None, 0, 1, 14, 14, 96, 0, 0.1, None) == -3 and b"null" in lib.mumpy_last_error()


def _child(env_value):
    env = dict(os.environ)
    env.pop("MUMPY_ATTN_MATH", None)
    if env_value is not None:
        env["MUMPY_ATTN_MATH"] = env_value
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]; from mumpy_hip import ops; print('MODE=' + ops.attention_math())"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)


def test_attention_math_switch_and_environment():
    from mumpy_hip import ops
    if not os.environ.get("MUMPY_ATTN_MATH"):
        assert ops.attention_math() == "fp32"
    before = ops.attention_math()
    try:
        ops.set_attention_math("bf16")
        assert ops.attention_math() == "bf16"
        ops.set_attention_math("fp32")
        assert ops.attention_math() == "fp32"
        with pytest.raises(ValueError):
            ops.set_attention_math("fp16")
        assert ops.attention_math() == "fp32"
        ops.set_storage("bf16")                                                # set_storage does not touch the switch
        assert ops.attention_math() == "fp32"
    finally:
        ops.set_storage("fp32")
        ops.set_attention_math(before)
    # fresh processes (they import the package and never touch a GPU)
    r = _child(None)
    assert r.returncode == 0 and "MODE=fp32" in r.stdout, r.stderr[-2000:]
    r = _child("")
    assert r.returncode == 0 and "MODE=fp32" in r.stdout, r.stderr[-2000:]
    r = _child("bf16")
    assert r.returncode == 0 and "MODE=bf16" in r.stdout, r.stderr[-2000:]
    r = _child("nope")
    assert r.returncode != 0 and "ValueError" in r.stderr and "MODE=" not in r.stdout


# ------------------------------------------------------------------ GPU
def _bias_and_mask(c, hs, w, shift, seed=701):
    from models.modules.swinTransformer import build_shift_mask, relative_position_index
    from mumpy_hip import ops
    bias = ops.expand_relpos_bias(seeded_randn(seed, 169, c // 32).to(DEV) * 0.2, relative_position_index(7, 7).to(DEV))
    mask = build_shift_mask(hs, w, 7, shift) if shift else None
    tab, ids = ops.compact_attn_mask(mask.to(DEV)) if shift else (None, None)
    return bias, mask, tab, ids


@gpu
@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("hs,w", [(14, 14), (28, 14), (56, 56)])
def test_bf16mm_layout_bit_exact(hs, w, shift, c):
    """One-hot attention (bias 0 on (i, (i+1) % 49), -1e30 elsewhere, q = k = 0) copies V rows: P is exactly one-hot and V holds
    integers that bf16 represents exactly, so out == the rolled V rows bit for bit.  Pins the gather, the roll, the scatter and the
    permuted k order of the P V operand (a V fragment in natural key order fails)."""
    from mumpy_hip import ops
    b, nh, l = 2, c // 32, hs * w
    bi, ti, ci = torch.meshgrid(torch.arange(b), torch.arange(l), torch.arange(c), indexing="ij")
    v = ((bi * 101 + ti * 13 + ci * 5) % 257 - 128).float()                    # integers in [-128, 128]
    assert torch.equal(v.to(torch.bfloat16).float(), v)
    qkv = torch.zeros(b, l, 3 * c)
    qkv[:, :, 2 * c:] = v
    bias = torch.full((nh, 64, 64), -1e30)
    for i in range(49):
        bias[:, i, (i + 1) % 49] = 0.0
    bias[:, 49:, :] = 0.0
    bias[:, :, 49:] = -1e30
    tab = ids = None
    if shift:
        from models.modules.swinTransformer import build_shift_mask
        tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift).to(DEV))
    out = ops.window_attention_bf16(qkv.to(torch.bfloat16).to(DEV), bias.to(DEV), b, hs, w, c, shift, SCALE, tab, ids, math="bf16")
    assert out.dtype == torch.bfloat16
    idxw = O.window_token_index(hs, w, shift).view(-1, 49)
    expect = torch.empty_like(v)
    expect[:, idxw.reshape(-1)] = v[:, torch.roll(idxw, -1, dims=1).reshape(-1)]
    assert torch.equal(out.float().cpu(), expect)


def _fp64_reference(qkv16, bias, mask, b, hs, w, c, shift):
    """Per window and head, fp64 softmax(q k^T scale + bias + mask) v of the bf16 values; returns (out (B, L, C), vmax (B, L, C)):
    vmax = the largest |v| of the element's (window, head, channel) column over its 49 keys."""
    nh = c // 32
    idx = O.window_token_index(hs, w, shift)                                   # (nW * 49)
    nw = idx.numel() // 49
    x = qkv16.double().cpu()[:, idx].view(b, nw, 49, 3, nh, 32).permute(3, 0, 1, 4, 2, 5)   # (3, B, nW, nH, 49, 32)
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2) * float(torch.tensor(SCALE, dtype=torch.float32)) + bias.double().cpu()[None, None, :, :49, :49]
    if mask is not None:
        s = s + mask.double().cpu()[None, :, None]
    o = torch.softmax(s, dim=-1) @ v                                           # (B, nW, nH, 49, 32)
    vmax = v.abs().amax(dim=-2, keepdim=True).expand_as(o)
    out, vm = torch.empty(b, hs * w, c, dtype=torch.float64), torch.empty(b, hs * w, c, dtype=torch.float64)
    out[:, idx] = o.permute(0, 1, 3, 2, 4).reshape(b, nw * 49, c)
    vm[:, idx] = vmax.permute(0, 1, 3, 2, 4).reshape(b, nw * 49, c)
    return out, vm


@gpu
@pytest.mark.parametrize("amp", [1, 3])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("b,hs,w,c", [(2, 28, 14, 96), (2, 56, 56, 128)])
def test_bf16mm_accuracy_against_fp64_of_the_same_operands(b, hs, w, c, shift, amp):
    """Element-wise |out - ref| <= 2^-7 vmax (derived: one bf16 rounding of P moves an output by <= 2^-8 sum_j P_j |v_j| <= 2^-8 vmax, the
    output rounding by <= 2^-8 |O| <= 2^-8 vmax; bf16 x bf16 products are exact in fp32, fp32 accumulation and __expf terms are three
    orders smaller), and RMS error <= 2 x that of the fp32-flow kernel (existing code) on the same input."""
    from mumpy_hip import ops
    qkv16 = (seeded_randn(900 + 10 * shift + amp, b, hs * w, 3 * c) * amp).to(torch.bfloat16).to(DEV)
    bias, mask, tab, ids = _bias_and_mask(c, hs, w, shift)
    ref, vmax = _fp64_reference(qkv16, bias, mask, b, hs, w, c, shift)
    new = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids, math="bf16").double().cpu()
    old = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids, math="fp32").double().cpu()
    worst = float(((new - ref).abs() / (2.0 ** -7 * vmax)).max())
    worst_old = float(((old - ref).abs() / (2.0 ** -7 * vmax)).max())
    r_new, r_old = rms_err(new, ref), rms_err(old, ref)
    print(f"bf16mm accuracy {(b, hs, w, c)} shift {shift} amp {amp}: worst |err| / (2^-7 vmax) = {worst:.3f} (fp32 flow {worst_old:.3f}); "
          f"rms {r_new:.3e} vs fp32 flow {r_old:.3e}, ratio {r_new / r_old:.3f}")
    assert worst <= 1.0
    assert r_new <= 2.0 * r_old


@gpu
def test_bf16mm_two_launches_are_bitwise_equal():
    from mumpy_hip import ops
    b, hs, w, c, shift = 2, 56, 56, 128, 3
    qkv16 = seeded_randn(931, b, hs * w, 3 * c).to(torch.bfloat16).to(DEV)
    bias, _, tab, ids = _bias_and_mask(c, hs, w, shift)
    o1 = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids, math="bf16")
    o2 = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids, math="bf16")
    assert torch.equal(o1, o2)


@gpu
def test_switch_leaves_the_fp32_kernels_alone():
    """With the switch on, math="fp32" is still the fp32-flow kernel bit for bit, the default follows the switch, and fp32 qkv runs
    the fp32 kernel whatever the switch says."""
    from mumpy_hip import ops
    b, hs, w, c, shift = 2, 28, 14, 96, 3
    qkv16 = seeded_randn(941, b, hs * w, 3 * c).to(torch.bfloat16).to(DEV)
    bias, _, tab, ids = _bias_and_mask(c, hs, w, shift)
    off32 = ops.window_attention(qkv16.float(), bias, b, hs, w, c, shift, SCALE, tab, ids)
    off16 = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids)
    assert torch.equal(off16, off32.to(torch.bfloat16))
    before = ops.attention_math()
    try:
        ops.set_attention_math("bf16")
        on32 = ops.window_attention(qkv16.float(), bias, b, hs, w, c, shift, SCALE, tab, ids)
        forced = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids, math="fp32")
        follows = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids)
        mm = ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids, math="bf16")
    finally:
        ops.set_attention_math(before)
    assert torch.equal(on32, off32)
    assert torch.equal(forced, off32.to(torch.bfloat16))
    assert torch.equal(follows, mm) and not torch.equal(mm, forced)           # another arithmetic: some roundings differ
    with pytest.raises(ValueError):
        ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, SCALE, tab, ids, math="fp16")


def _load_filled(module):
    fill_module_(module)
    return module.to(DEV).eval()


@gpu
def test_full_model_bf16_storage_bf16_attention_b8_t5():
    """B=8, T=5 with bf16 storage + bf16-MFMA attention against the fp32 oracle, with the bars of test_full_model_bf16_storage_b8_t5:
    logits rel err < 2e-2, mask flips < 0.5 %, a pixel may flip only where the reference logit lies within the observed error of the
    threshold.  The parent's mode (attention math "fp32") runs beside it for comparison."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import ops
    enc = _load_filled(Encoder(num_frames=5))
    dec = _load_filled(Decoder(input_token_temporal_dims=[1, 1, 5]))
    x = seeded_randn(3535, 8, 5, 3, 224, 224)
    before = ops.attention_math()
    got = {}
    try:
        ops.set_storage("bf16")
        for mode in ("fp32", "bf16"):
            ops.set_attention_math(mode)
            with torch.no_grad():
                fx, vx, dx = enc(x.to(DEV))
                got[mode] = dec(fx, vx, dx)[0].cpu()
    finally:
        ops.set_storage("fp32")
        ops.set_attention_math(before)
    with torch.no_grad():
        ref = O.full_forward({k: v.detach().cpu() for k, v in enc.state_dict().items()},
                             {k: v.detach().cpu() for k, v in dec.state_dict().items()}, x)[0]
    fig = {}
    for mode, logits in got.items():
        flipped = O.mask_from_logits(logits) != O.mask_from_logits(ref)
        fig[mode] = (rel_err(logits, ref), float(flipped.float().mean()), flipped, logits)
        print(f"bf16 storage, attention math {mode}: logits rel err {fig[mode][0]:.3e}, mask flips {100 * fig[mode][1]:.4f} %")
    err, flips, flipped, logits = fig["bf16"]
    assert not torch.equal(got["bf16"], got["fp32"])                           # the switch reached the model
    assert err < 2e-2 and flips < 5e-3
    assert float(ref[flipped].abs().max()) <= float((logits - ref).abs().max())


@gpu
def test_graphed_forward_with_bf16_attention_replays_bitwise():
    """Both switches are read at launch time: set before the capture, the graph holds the bf16-MFMA kernels and replays bit for bit
    what the eager forward computes in that mode."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import ops
    from mumpy_hip.graph import GraphedForward
    enc, dec = _load_filled(Encoder()), _load_filled(Decoder())
    x = seeded_randn(78, 1, 3, 3, 224, 224).to(DEV)
    before = ops.attention_math()
    try:
        ops.set_storage("bf16")
        ops.set_attention_math("fp32")
        with torch.no_grad():
            other = dec(*enc(x))[0].clone()
        ops.set_attention_math("bf16")
        with torch.no_grad():
            eager = dec(*enc(x))[0].clone()
        g = GraphedForward(enc, dec, x)
        replay = g(x)[0].clone()
        replay2 = g(x)[0].clone()
    finally:
        ops.set_storage("fp32")
        ops.set_attention_math(before)
    assert torch.equal(replay, eager) and torch.equal(replay2, eager)
    assert not torch.equal(eager, other)
