"""bf16-MFMA window attention on the fp32-stored training tape (mumpy_window_attention_mm16_fwd / _mm16_bwd, reached through
ops.set_attention_math("bf16") and autograd.WindowAttentionFn): C ABI and validation on the CPU; accuracy against fp64 of the same
bf16-rounded operands, layout, determinism, the switch on the tape and graph capture on the GPU.

Arithmetic under test, r(x) = round-to-nearest-even to bf16:  S = scale (r(q) r(k)^T) + bias (+ mask), P = softmax(S), O = r(P) r(v),
dP = r(dO) r(v)^T, D = rowsum(P o dP), dS = P o (dP - D), dV = r(P)^T r(dO), dQ = scale r(dS) r(k), dK = scale r(dS)^T r(q), and the
bias-table gradient from the fp32 dS.  Each output therefore differs from the exact result of the rounded operands by ONE bf16 rounding
(unit roundoff 2^-8) of the accumulator operand, plus fp32 effects; the fp32 effects are measured on the existing fp32 kernels."""
import functools

import pytest
import torch

from conftest import rel_err
from weight_fill import seeded_randn

gpu = pytest.mark.gpu
FWD, BWD, WSQ = "mumpy_window_attention_mm16_fwd", "mumpy_window_attention_mm16_bwd", "mumpy_window_attention_mm16_bwd_workspace_bytes"
SCALE = 32 ** -0.5
SC = float(torch.tensor(SCALE, dtype=torch.float32))           # the fp32 value the kernels multiply by
U = 2.0 ** -8                                                   # unit roundoff of bf16 (8 significant bits, nearest even)
CASES = [(3, 7, 7, 32, 0),          # 3 windows, 1 head: a block with an idle fourth wave
         (1, 28, 14, 64, 3),        # non-square grid with the shift mask
         (2, 14, 14, 96, 0), (2, 14, 14, 96, 3),                # three heads
         (2, 280, 56, 128, 3)]      # 640 windows x 4 heads = 160 window quads per head on 128 persistent blocks per head: 32 blocks
#                                     walk two quads, 96 one -> the dBias running sum across units and the token-table reuse

if torch.cuda.is_available():
    from oracle import mumpy_oracle as O
    DEV = torch.device("cuda:0")


# ------------------------------------------------------------------ CPU: ABI and validation
def test_c_abi_declares_the_three_symbols_as_their_fp32_siblings():
    """Return type, argument types and argument names of the fp32 entries (tests/test_abi.py holds include/mumpy_hip.h, version 2,
    to its binding and to both libraries)."""
    from abi_surface import decls
    d = decls("mumpy_hip.h")
    assert d[FWD] == d["mumpy_window_attention_fwd"] and d[FWD].ret == "int"
    assert d[BWD] == d["mumpy_window_attention_bwd_csr"] and d[BWD].ret == "int"
    assert d[WSQ] == d["mumpy_window_attention_bwd_workspace_bytes"] and d[WSQ].ret == "int64_t"


def test_validation_needs_no_gpu():
    from mumpy_hip.lib import load_library
    lib = load_library()
    fwd, bwd, wsq = getattr(lib, FWD), getattr(lib, BWD), getattr(lib, WSQ)
    p = 16                                                                     # a non-null, 16-byte aligned stand-in: nothing is launched
    assert fwd(p, p, p, None, None, 0, 1, 10, 14, 96, 0, 0.1, None) == -1      # EINVAL: grid not divisible by 7
    assert fwd(None, None, None, None, None, 0, 1, 14, 14, 96, 0, 0.1, None) == -3 and b"null" in lib.mumpy_last_error()
    need = wsq(1, 14, 14, 96)
    assert need > 0 and wsq(1, 14, 14, 100) == 0 and wsq(1, 10, 14, 96) == 0 and wsq(0, 14, 14, 96) == 0   # C % 32, grid % 7, B
    ok = (p, p, p, None, None, 0, p, None, p, p, p, need, 1, 14, 14, 96, 0, 0.1, 0, None)                  # rel_csr may be null
    bad = lambda i, v: bwd(*(ok[:i] + (v,) + ok[i + 1:]))
    assert bad(13, 10) == -1 and b"divisible" in lib.mumpy_last_error()        # Hs = 10
    assert bad(0, None) == -3 and b"null" in lib.mumpy_last_error()            # qkv
    assert bad(10, None) == -3 and b"null" in lib.mumpy_last_error()           # workspace
    assert bad(11, need - 1) == -1 and b"workspace too small" in lib.mumpy_last_error()
    assert bad(18, 2) == -1 and b"accumulate" in lib.mumpy_last_error()
    assert bad(3, p) == -3                                                     # mask_tab without mask_id


def test_backward_rejects_an_unknown_math_mode_before_any_launch():
    from mumpy_hip import ops
    t = torch.zeros(1, 49, 96)
    with pytest.raises(ValueError):
        ops.window_attention_bwd(t, t[..., :32], t, t, 1, 7, 7, 32, 0, SCALE, math="fp16")
    import inspect
    assert inspect.signature(ops.window_attention_bwd).parameters["math"].default == "fp32"   # does not follow the switch


# ------------------------------------------------------------------ GPU
def _r(x):
    return x.to(torch.bfloat16).to(x.dtype)


@functools.lru_cache(maxsize=None)
def _setup(case, amp):
    """Inputs, the fp64 reference of the bf16-rounded operands with its bound tensors, and the existing fp32 kernels' results on the
    rounded-then-widened operands (the floor E32).  Computed once per (case, amplitude) and shared; nothing here is modified later."""
    from models.modules.swinTransformer import relative_position_index
    from mumpy_hip import ops
    b, hs, w, c, shift = case
    nh, l = c // 32, hs * w
    qkv = seeded_randn(1200 + 10 * shift + amp, b, l, 3 * c) * amp
    dout = seeded_randn(1300 + 10 * shift + amp, b, l, c)
    table = seeded_randn(701, 169, nh) * 0.2
    rel = relative_position_index(7, 7)
    mask = O.shift_attn_mask(hs, w, shift) if shift else None
    idx = O.window_token_index(hs, w, shift)
    nw = idx.numel() // 49
    x = _r(qkv).double()[:, idx].view(b, nw, 49, 3, nh, 32).permute(3, 0, 1, 4, 2, 5)       # (3, B, nW, nH, 49, 32)
    q, k, v = x[0], x[1], x[2]
    do = _r(dout).double()[:, idx].view(b, nw, 49, nh, 32).permute(0, 1, 3, 2, 4)
    s = q @ k.transpose(-1, -2) * SC + table.double()[rel.reshape(-1)].view(49, 49, nh).permute(2, 0, 1)
    if mask is not None:
        s = s + mask.double()[None, :, None]
    p = torch.softmax(s, dim=-1)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))

    def raster(t):                                                              # (B, nW, nH, 49, 32) -> (B, L, C)
        out = torch.empty(b, l, c, dtype=torch.float64)
        out[:, idx] = t.permute(0, 1, 3, 2, 4).reshape(b, nw * 49, c)
        return out

    ref = {"out": raster(p @ v), "dq": raster(SC * (ds @ k)), "dk": raster(SC * (ds.transpose(-1, -2) @ q)),
           "dv": raster(p.transpose(-1, -2) @ do)}
    bound = {"out": raster(U * (p @ v.abs())), "dq": raster(U * SC * (ds.abs() @ k.abs())),
             "dk": raster(U * SC * (ds.abs().transpose(-1, -2) @ q.abs())), "dv": raster(U * (p.transpose(-1, -2) @ do.abs()))}
    dbias = ds.sum(dim=(0, 1)).reshape(nh, 49 * 49)                             # (nH, 49*49)
    ref["dtable"] = torch.zeros(169, nh, dtype=torch.float64).index_add_(0, rel.reshape(-1), dbias.t().contiguous())
    relg = rel.to(DEV)
    g = {"qkv": qkv.to(DEV), "dout": dout.to(DEV), "idx32": ops.rel_index32(relg), "csr": ops.rel_index_csr(relg)}
    g["bias"] = ops.expand_relpos_bias(table.to(DEV), g["idx32"])
    g["tab"], g["ids"] = ops.compact_attn_mask(mask.to(DEV)) if shift else (None, None)
    # the parent's fp32 kernels on the rounded-then-widened operands: what fp32 accumulation, __expf and the summation order cost
    old_d, _ = ops.window_attention_bwd(_r(g["qkv"]), _r(g["dout"]), g["bias"], g["idx32"], b, hs, w, c, shift, SCALE, g["tab"], g["ids"],
                                        rel_csr=g["csr"], math="fp32")
    old_o = ops.window_attention(_r(g["qkv"]), g["bias"], b, hs, w, c, shift, SCALE, g["tab"], g["ids"])
    old = {"out": old_o, "dq": old_d[..., :c], "dk": old_d[..., c:2 * c], "dv": old_d[..., 2 * c:]}
    e32 = {n: float((t.double().cpu() - ref[n]).abs().max()) for n, t in old.items()}
    return g, ref, bound, e32


def _split(dqkv, c):
    return {"dq": dqkv[..., :c], "dk": dqkv[..., c:2 * c], "dv": dqkv[..., 2 * c:]}


def _check(tag, name, new, ref, bound, e32):
    err = (new.double().cpu() - ref).abs()
    worst = float((err / (bound + 2.0 * e32)).max())
    plain = float(((err - e32).clamp_min(0) / bound.clamp_min(1e-300)).max())
    print(f"{tag} {name}: worst |err| / (B + 2 E32) = {worst:.3f}; worst (|err| - E32) / B = {plain:.3f}; E32 = {e32:.3e}, "
          f"max |err| = {float(err.max()):.3e}, max |ref| = {float(ref.abs().max()):.3e}")
    return worst


@gpu
@pytest.mark.parametrize("amp", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_backward_accuracy_against_fp64_of_the_rounded_operands(case, amp):
    """Elementwise |new - ref| <= B + 2 E32 for dq, dk, dv: B = one bf16 rounding (2^-8) of dS resp. P pushed through the exact
    product, E32 = the largest error of the existing fp32 backward on the same rounded operands (a measured maximum, not a bound, and
    the new kernels add in another order: hence the factor 2).  The kernel is given the UNROUNDED fp32 input: rounding the operands is
    its job.  CPU emulation of the contract: worst (|err| - E32) / B of 0.57-0.80 at amplitude 1, 0.96-0.98 at amplitude 3 -- a
    truncating conversion (roundoff 2^-7) fails.  dtable < 2e-5 (the bar of test_hip_window_attention_bwd_vs_oracle: dBias is summed
    from the fp32 dS); the csr and scan forms agree as there."""
    from mumpy_hip import ops
    b, hs, w, c, shift = case
    g, ref, bound, e32 = _setup(case, amp)
    args = (g["qkv"], g["dout"], g["bias"], g["idx32"], b, hs, w, c, shift, SCALE, g["tab"], g["ids"])
    d_csr, t_csr = ops.window_attention_bwd(*args, rel_csr=g["csr"], math="bf16")
    d_scan, t_scan = ops.window_attention_bwd(*args, math="bf16")
    worst = {n: _check(f"bwd {case} amp {amp}", n, t, ref[n], bound[n], e32[n]) for n, t in _split(d_csr, c).items()}
    terr = rel_err(t_csr.cpu(), ref["dtable"])
    print(f"bwd {case} amp {amp} dtable: rel err {terr:.3e}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert terr < 2e-5
    assert torch.equal(d_scan, d_csr) and rel_err(t_csr.cpu(), t_scan.cpu()) < 1e-6


# the forward deals its window quads over up to 1024 / nH persistent blocks per head: on every shape above a wave owns at most one unit.
# 7 x 320 windows x 2 heads = 560 quads per head on 512 blocks -> 280 blocks of two quads: token tables rewritten by a wave's next unit
FWD_CASES = CASES + [(7, 280, 56, 64, 3)]


@gpu
@pytest.mark.parametrize("amp", [1, 3])
@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_accuracy_against_fp64_of_the_rounded_operands(case, amp):
    """|out - ref| <= 2^-8 (P |r(v)|) + 2 E32, E32 from ops.window_attention on the rounded-then-widened qkv."""
    from mumpy_hip import ops
    b, hs, w, c, shift = case
    g, ref, bound, e32 = _setup(case, amp)
    out = ops.window_attention_mm16(g["qkv"], g["bias"], b, hs, w, c, shift, SCALE, g["tab"], g["ids"])
    assert out.dtype == torch.float32 and out.shape == (b, hs * w, c)
    assert _check(f"fwd {case} amp {amp}", "out", out, ref["out"], bound["out"], e32["out"]) <= 1.0


@gpu
@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("hs,w", [(14, 14), (28, 14), (56, 56)])
def test_layout_bit_exact(hs, w, shift, c):
    """The one-hot construction of test_bf16mm_layout_bit_exact (bias 0 on (i, (i+1) % 49), -1e30 elsewhere, q = k = 0, integer v and dO
    that bf16 holds exactly): P is exactly one-hot, so out = the rolled V rows, dV = the inversely rolled dO rows, dQ = dK = 0, all bit
    for bit.  Pins the gathers, the roll, the scatters and the permuted k order of every accumulator-fed operand."""
    from models.modules.swinTransformer import build_shift_mask, relative_position_index
    from mumpy_hip import ops
    b, nh, l = 2, c // 32, hs * w
    bi, ti, ci = torch.meshgrid(torch.arange(b), torch.arange(l), torch.arange(c), indexing="ij")
    v = ((bi * 101 + ti * 13 + ci * 5) % 257 - 128).float()                    # integers in [-128, 128]
    do = ((bi * 37 + ti * 29 + ci * 11) % 257 - 128).float()
    assert torch.equal(_r(v), v) and torch.equal(_r(do), do)
    qkv = torch.zeros(b, l, 3 * c)
    qkv[:, :, 2 * c:] = v
    bias = torch.full((nh, 64, 64), -1e30)
    for i in range(49):
        bias[:, i, (i + 1) % 49] = 0.0
    bias[:, 49:, :] = 0.0
    bias[:, :, 49:] = -1e30
    tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift).to(DEV)) if shift else (None, None)
    idx32 = ops.rel_index32(relative_position_index(7, 7).to(DEV))
    out = ops.window_attention_mm16(qkv.to(DEV), bias.to(DEV), b, hs, w, c, shift, SCALE, tab, ids)
    dqkv, _ = ops.window_attention_bwd(qkv.to(DEV), do.to(DEV), bias.to(DEV), idx32, b, hs, w, c, shift, SCALE, tab, ids, math="bf16")
    idxw = O.window_token_index(hs, w, shift).view(-1, 49)
    expect_o, expect_dv = torch.empty_like(v), torch.empty_like(v)
    expect_o[:, idxw.reshape(-1)] = v[:, torch.roll(idxw, -1, dims=1).reshape(-1)]          # query i reads key i + 1
    expect_dv[:, idxw.reshape(-1)] = do[:, torch.roll(idxw, 1, dims=1).reshape(-1)]         # key j is read by query j - 1
    assert torch.equal(out.cpu(), expect_o)
    got = _split(dqkv.cpu(), c)
    assert torch.equal(got["dv"], expect_dv)
    assert not got["dq"].any() and not got["dk"].any()


@gpu
def test_backward_is_deterministic_and_accumulates():
    from mumpy_hip import ops
    case = (2, 280, 56, 128, 3)
    b, hs, w, c, shift = case
    g = _setup(case, 1)[0]
    args = (g["qkv"], g["dout"], g["bias"], g["idx32"], b, hs, w, c, shift, SCALE, g["tab"], g["ids"])
    d1, t1 = ops.window_attention_bwd(*args, rel_csr=g["csr"], math="bf16")
    d2, t2 = ops.window_attention_bwd(*args, rel_csr=g["csr"], math="bf16")
    assert torch.equal(d1, d2) and torch.equal(t1, t2)
    fill = seeded_randn(77, 169, c // 32).to(DEV)
    acc = fill.clone()
    d3, none = ops.window_attention_bwd(*args, dtable_out=acc, rel_csr=g["csr"], math="bf16")
    assert none is None and torch.equal(d3, d1)
    assert rel_err(acc.cpu(), (fill + t1).cpu()) < 1e-6


def _block_run(shift, flip_before_backward=None):
    """swin_block_train on the _block(shift) setup of tests/test_swin_backward.py -> (y, dx, {name: grad}) on the CPU."""
    from models.modules.swinTransformer import SwinTransformerBlock
    from mumpy_hip import ops
    from mumpy_hip.autograd import swin_block_train
    from weight_fill import fill_module_
    blk = fill_module_(SwinTransformerBlock(dim=96, input_resolution=(14, 14), num_heads=3, window_size=7, shift_size=shift)).eval().cuda()
    x = seeded_randn(700 + shift, 2, 196, 96).cuda().requires_grad_(True)
    gy = seeded_randn(710 + shift, 2, 196, 96).cuda()
    y = swin_block_train(blk, x)
    if flip_before_backward is not None:
        ops.set_attention_math(flip_before_backward)
    (y * gy).sum().backward()
    return y.detach().cpu(), x.grad.cpu(), {n: p.grad.cpu() for n, p in blk.named_parameters()}


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][n], b[2][n]) for n in a[2])


@gpu
@pytest.mark.parametrize("tag,shift", [("blk_s0", 0), ("blk_s3", 3)])
def test_switch_reaches_the_tape_and_leaves_fp32_alone(train_golden, tag, shift):
    """(a) never touched == set back to "fp32" after "bf16", bitwise.  (b) "bf16" differs, and stays inside the project's bars for bf16
    training arithmetic (test_hip_full_model_backward_bf16_vs_oracle's encoder group: relative L2 <= 5e-2, cosine >= 0.995; logits
    2e-2), also combined with set_matrix_math("bf16").  (c) a tape built under "bf16" runs its own backward after the switch went back."""
    from mumpy_hip import ops
    before, before_mm = ops.attention_math(), ops.matrix_math()
    try:
        if before != "fp32":                                                   # (a) "never touched" exists only in a process that started in
            ops.set_attention_math("fp32")                                     # the default mode; started with MUMPY_ATTN_MATH=bf16, set it
        untouched = _block_run(shift)
        ops.set_attention_math("bf16")
        on = _block_run(shift)
        carried = _block_run(shift, flip_before_backward="fp32")              # (c): forward under bf16, backward after the flip
        assert ops.attention_math() == "fp32"
        back = _block_run(shift)
        ops.set_attention_math("bf16")
        ops.set_matrix_math("bf16")
        both = _block_run(shift)
    finally:
        ops.set_matrix_math(before_mm)
        ops.set_attention_math(before)
    assert _same(untouched, back)
    assert not torch.equal(on[0], untouched[0]) and not torch.equal(on[1], untouched[1])
    assert not torch.equal(on[2]["attn.qkv.weight"], untouched[2]["attn.qkv.weight"])
    assert not torch.equal(on[2]["attn.relative_position_bias_table"], untouched[2]["attn.relative_position_bias_table"])
    assert _same(carried, on)
    for label, run in (("attention bf16", on), ("attention bf16 + matrix math bf16", both)):
        y, dx, grads = run
        names = sorted(grads)
        got = torch.cat([grads[n].double().reshape(-1) for n in names])
        ref = torch.cat([torch.as_tensor(train_golden[f"{tag}/grad/{n}"]).double().reshape(-1) for n in names])
        rdx = torch.as_tensor(train_golden[tag + "/dx"]).double().reshape(-1)
        gdx = dx.double().reshape(-1)
        fig = {"params": (float((got - ref).norm() / ref.norm()), float(torch.dot(got, ref) / (got.norm() * ref.norm()))),
               "dx": (float((gdx - rdx).norm() / rdx.norm()), float(torch.dot(gdx, rdx) / (gdx.norm() * rdx.norm())))}
        yerr = rel_err(y, train_golden[tag + "/y"])
        print(f"{tag}, {label}: y rel err {yerr:.3e}; parameter gradients rel L2 {fig['params'][0]:.3e} cos {fig['params'][1]:.6f}; "
              f"dx rel L2 {fig['dx'][0]:.3e} cos {fig['dx'][1]:.6f}")
        assert yerr < 2e-2
        assert all(l2 <= 5e-2 and cos >= 0.995 for l2, cos in fig.values()), fig


@gpu
def test_tape_under_bf16_captures_and_replays_bitwise():
    """WindowAttentionFn forward + backward under "bf16", captured the way GraphedForward._capture / GraphedTrainStep do it: every
    eager run (they are the warm-up) and the capture on ONE side stream, capture_error_mode="thread_local", .backward() into gradient
    buffers that exist before the capture.  No host synchronisation or allocation breaks the capture; two replays equal the eager
    result bitwise."""
    from models.modules.swinTransformer import relative_position_index
    from mumpy_hip import ops
    from mumpy_hip.autograd import WindowAttentionFn
    from mumpy_hip.streams import new_distinct_stream
    b, hs, w, c, shift = 2, 14, 14, 96, 3
    qkv = seeded_randn(1501, b, hs * w, 3 * c).to(DEV).requires_grad_(True)
    table = (seeded_randn(1502, 169, c // 32) * 0.2).to(DEV).requires_grad_(True)
    dout = seeded_randn(1503, b, hs * w, c).to(DEV)
    rel = relative_position_index(7, 7).to(DEV)
    tab, ids = ops.compact_attn_mask(O.shift_attn_mask(hs, w, shift).to(DEV))
    qkv.grad, table.grad = torch.zeros_like(qkv), torch.zeros_like(table)

    def fwd_bwd():
        qkv.grad.zero_()
        table.grad.zero_()
        y = WindowAttentionFn.apply(qkv, table, rel, (b, hs, w, c, shift, SCALE), tab, ids)
        y.backward(dout)
        return y.detach()

    def snapshot(y):
        return [y.clone(), qkv.grad.clone(), table.grad.clone()]

    before = ops.attention_math()
    try:
        side = new_distinct_stream(DEV, (torch.cuda.current_stream().cuda_stream,))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.set_attention_math("fp32")
            other = snapshot(fwd_bwd())
            ops.set_attention_math("bf16")
            for _ in range(2):
                eager = snapshot(fwd_bwd())
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            static_y = fwd_bwd()
        replays = []
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            replays.append(snapshot(static_y))
    finally:
        ops.set_attention_math(before)
    for rep in replays:
        assert all(torch.equal(a, e) for a, e in zip(rep, eager))
    assert not torch.equal(eager[0], other[0]) and not torch.equal(eager[1], other[1])
