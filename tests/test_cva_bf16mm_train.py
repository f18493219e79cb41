"""bf16-MFMA cross-view attention on the fp32-stored training tape (mumpy_deform_attention_mm16_fwd and, new here,
mumpy_deform_attention_mm16_bwd of include/mumpy_hip_ext2.h, reached through ops.set_cva_math("bf16") and autograd.DeformAttentionFn):
header, binding and validation on the CPU; accuracy against fp64 of the same bf16-rounded operands, layout, determinism and memory
discipline, the switch on the tape and graph capture on the GPU.

Arithmetic under test, r(x) = round-to-nearest-even to bf16, everything else fp32.  kv window b2 pairs with q window b2 % B1 and with
dO of output window b2 // r:
  S = scale (r(q) r(k)^T), P = softmax(S), dP = r(dO) r(v)^T, D = rowsum(P o dP), dS = P o (dP - D),
  dV = r(P)^T r(dO), dK = scale r(dS)^T r(q), dQ[qw] = sum over m = 0 .. r-1 of scale r(dS_b2) r(k_b2), b2 = qw + m B1.
Each output differs from the exact result of the rounded operands by ONE bf16 rounding (unit roundoff 2^-8) of the accumulator operand
(P resp. dS), plus fp32 effects; the fp32 effects are measured on the existing fp32 kernels."""
import functools
import inspect

import pytest
import torch

import guarded_alloc as GA
from conftest import rel_err
from weight_fill import fill_module_, seeded_randn

gpu = pytest.mark.gpu
BWD, WSQ = "mumpy_deform_attention_mm16_bwd", "mumpy_deform_attention_mm16_bwd_workspace_bytes"
SCALE = 32 ** -0.5
SC = float(torch.tensor(SCALE, dtype=torch.float32))           # the fp32 value the kernels multiply by
U = 2.0 ** -8                                                   # unit roundoff of bf16 (8 significant bits, nearest even)
# (b1, r, c), window form
CASES = [(3, 1, 32),        # one head; a block with an idle fourth wave
         (4, 1, 96),        # r = 1; three heads
         (2, 3, 192),       # six heads; r > 1 pairing
         (1, 5, 96),        # every member shares one q window
         (3, 5, 64)]        # b2 % 3 differs from b2 // 5; 30 units; a ragged last block

if torch.cuda.is_available():
    from oracle import mumpy_oracle as O
    DEV = torch.device("cuda:0")


# ------------------------------------------------------------------ CPU: header, binding and validation
def test_ext2_header_declares_the_backward_and_its_query():
    """(tests/test_abi.py holds mumpy_hip_ext2.h to its binding and to both libraries.)"""
    from abi_surface import decls
    assert {BWD, WSQ, "mumpy_ext2_version"} <= set(decls("mumpy_hip_ext2.h"))


def test_refusals_need_no_gpu():
    """Every refusal of mumpy_deform_attention_mm16_bwd returns its documented code with a message and launches nothing (every tuple
    below is refused, so the stand-in pointer is never dereferenced, with or without a device); the workspace query is 0 for each
    invalid shape."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    bwd, wsq = getattr(lib, BWD), getattr(lib, WSQ)
    p = 0x100000                                                               # non-null, 16-byte aligned, never dereferenced
    need = wsq(3, 5, 64)
    assert need == 3 * 5 * 2 * 192 * 4
    assert wsq(0, 5, 64) == 0 and wsq(3, 0, 64) == 0 and wsq(3, 5, 100) == 0 and wsq(-1, 5, 64) == 0 and wsq(3, 5, 0) == 0
    ok = (p, p, p, p, p, p, need, 3, 5, 64, 0.1, None)
    EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4

    def refused(i, v, code, word):
        assert lib.mumpy_deform_attention_bwd(None, p, p, p, p, p, 0, 1, 1, 32, 0.1, None) == ENULL   # the message is sticky per
        stale = lib.mumpy_last_error()                                                                # thread: leave a known one
        rc = bwd(*(ok[:i] + (v,) + ok[i + 1:]))
        err = lib.mumpy_last_error()
        assert rc == code and err != stale and b"deform_attention_mm16_bwd" in err and word in err, (i, v, rc, err)

    for i in range(6):                                                         # q, kv, dout, dq, dkv, workspace
        refused(i, None, ENULL, b"null")
        refused(i, p + 4, EALIGN, b"aligned")
    refused(7, 0, EINVAL, b"shape")                                            # B1w = 0
    refused(8, 0, EINVAL, b"shape")                                            # r = 0
    refused(9, 100, EINVAL, b"shape")                                          # C = 100
    refused(6, need - 1, EINVAL, b"workspace too small")
    big = 1 << 62                                                              # (a size no shape below needs more than)
    assert bwd(*(ok[:6] + (big, 1 << 31, 1, 32) + ok[10:])) == ERANGE and b"too many windows" in lib.mumpy_last_error()   # B1w
    assert bwd(*(ok[:6] + (big, 1 << 30, 2, 32) + ok[10:])) == ERANGE                                  # B1w * r = 2^31
    assert bwd(*(ok[:6] + (big, (1 << 31) - 1, 1, 32 * 8) + ok[10:])) == ERANGE                        # 2^34 kv units: the grid
    c_wide = (1 << 32) // (49 * 8) // 32 * 32 + 32                             # the first C % 32 == 0 with 49 * 2C * 4 >= 2^32
    assert 49 * 8 * c_wide >= 1 << 32 > 49 * 8 * (c_wide - 32)
    assert bwd(*(ok[:6] + (big, 1, 1, c_wide) + ok[10:])) == ERANGE and b"32-bit row offsets" in lib.mumpy_last_error()
    assert wsq(1 << 31, 1, 32) == 0 and wsq(1, 1, c_wide) == 0 and wsq(1, 1, c_wide - 32) == (c_wide - 32) // 32 * 192 * 4


def test_backward_rejects_an_unknown_math_mode_before_any_launch():
    from mumpy_hip import ops
    t = torch.zeros(1, 49, 32)
    with pytest.raises(ValueError):
        ops.deform_attention_bwd(t, torch.zeros(1, 49, 64), t, 1, SCALE, math="fp16")
    assert inspect.signature(ops.deform_attention_bwd).parameters["math"].default == "fp32"   # does not follow the switch
    assert inspect.signature(ops.deform_attention).parameters["math"].default == "fp32"


# ------------------------------------------------------------------ GPU
def _r(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _heads(t, nh):                                              # (N, 49, nh * 32) -> (N, nh, 49, 32)
    return t.reshape(t.shape[0], 49, nh, 32).transpose(1, 2)


def _rows(t):                                                   # (N, nh, 49, 32) -> (N, 49, nh * 32)
    return t.transpose(1, 2).reshape(t.shape[0], 49, -1)


def _reference(q, kv, do, r):
    """The formulas of the module docstring in float64 on r()-rounded CPU inputs -> (ref, bound, dS, q per kv window), each of ref /
    bound a dict of dq (B1,49,C), dk and dv (B2,49,C)."""
    b1, _, c = q.shape
    b2, nh = b1 * r, c // 32
    qh = _heads(_r(q).double()[torch.arange(b2) % b1], nh)
    k, v = _heads(_r(kv).double()[..., :c], nh), _heads(_r(kv).double()[..., c:], nh)
    doh = _heads(_r(do).double()[torch.arange(b2) // r], nh)
    p = torch.softmax(qh @ k.transpose(-1, -2) * SC, dim=-1)
    dp = doh @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))

    def members(t):                                              # kv windows qw + m B1 belong to q window qw
        return _rows(t).view(r, b1, 49, c).sum(0)

    ref = {"dq": members(SC * (ds @ k)), "dk": _rows(SC * (ds.transpose(-1, -2) @ qh)), "dv": _rows(p.transpose(-1, -2) @ doh)}
    bound = {"dq": members(U * SC * (ds.abs() @ k.abs())), "dk": _rows(U * SC * (ds.abs().transpose(-1, -2) @ qh.abs())),
             "dv": _rows(U * (p.transpose(-1, -2) @ doh.abs()))}
    return ref, bound, ds, qh


@functools.lru_cache(maxsize=None)
def _setup(case, amp):
    """Inputs, the fp64 reference of the bf16-rounded operands with its bound tensors, and the existing fp32 kernels' error on the
    rounded-then-widened operands (the floor E32).  Computed once per (case, amplitude) and shared; nothing here is modified later."""
    from mumpy_hip import ops
    b1, r, c = case
    q = seeded_randn(2200 + amp, b1, 49, c) * amp
    kv = seeded_randn(2300 + amp, b1 * r, 49, 2 * c) * amp
    do = seeded_randn(2400 + amp, b1, 49, c)
    ref, bound, _, _ = _reference(q, kv, do, r)
    g = {"q": q.to(DEV), "kv": kv.to(DEV), "dout": do.to(DEV)}
    # the parent's fp32 kernels on the rounded-then-widened operands: what fp32 accumulation, __expf and the summation order cost
    old_dq, old_dkv = ops.deform_attention_bwd(_r(g["q"]), _r(g["kv"]), _r(g["dout"]), r, SCALE, math="fp32")
    old = {"dq": old_dq, "dk": old_dkv[..., :c], "dv": old_dkv[..., c:]}
    e32 = {n: float((t.double().cpu() - ref[n]).abs().max()) for n, t in old.items()}
    return g, ref, bound, e32


def _split(dq, dkv, c):
    return {"dq": dq, "dk": dkv[..., :c], "dv": dkv[..., c:]}


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
    product (dv: 2^-8 P^T |r(dO)|; dk: 2^-8 scale |dS|^T |r(q)|; dq: 2^-8 scale sum_m |dS_m| |r(k_m)|), E32 = the largest error of
    the existing fp32 backward on the same rounded operands (a measured maximum, not a bound, and the new kernels add in another
    order: hence the factor 2).  The kernel is given the UNROUNDED fp32 input: rounding the operands is its job.  A wrong pairing
    (% against //), a missing scale or a dropped member misses the bound by orders of magnitude."""
    from mumpy_hip import ops
    b1, r, c = case
    g, ref, bound, e32 = _setup(case, amp)
    dq, dkv = ops.deform_attention_bwd(g["q"], g["kv"], g["dout"], r, SCALE, math="bf16")
    assert dq.shape == (b1, 49, c) and dkv.shape == (b1 * r, 49, 2 * c) and dq.dtype == dkv.dtype == torch.float32
    worst = {n: _check(f"bwd {case} amp {amp}", n, t, ref[n], bound[n], e32[n]) for n, t in _split(dq, dkv, c).items()}
    assert all(v <= 1.0 for v in worst.values()), worst


@gpu
@pytest.mark.parametrize("case", [(3, 5, 64), (2, 3, 192)])
def test_layout_bit_exact(case):
    """q = k = 0, integer v and dO in [-128, 128] that depend on (window, token, channel): P is fl32(1/49) everywhere, so
    dv[b2, j, ch] = bf16(fl32(1/49)) * sum_i dO[b2 // r, i, ch] exactly (8-bit x 13-bit products, every partial sum representable),
    for every key j; dq and dk are exactly zero.  Pins the dO window of every member, the gathers, the scatters and the permuted
    order of every accumulator-fed operand."""
    from mumpy_hip import ops
    b1, r, c = case
    b2 = b1 * r

    def ints(n, m0, m1, m2):
        wi, ti, ci = torch.meshgrid(torch.arange(n), torch.arange(49), torch.arange(c), indexing="ij")
        return ((wi * m0 + ti * m1 + ci * m2) % 257 - 128).float()

    v, do = ints(b2, 101, 13, 5), ints(b1, 37, 29, 11)
    assert torch.equal(_r(v), v) and torch.equal(_r(do), do)
    q, kv = torch.zeros(b1, 49, c), torch.zeros(b2, 49, 2 * c)
    kv[..., c:] = v
    dq, dkv = ops.deform_attention_bwd(q.to(DEV), kv.to(DEV), do.to(DEV), r, SCALE, math="bf16")
    p16 = _r(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(49.0, dtype=torch.float32)).double()
    colsum = do.double().sum(1)                                                # (b1, c): integers
    expect = (p16 * colsum[torch.arange(b2) // r]).float()[:, None, :].expand(b2, 49, c)
    assert torch.equal((p16 * colsum).float().double(), p16 * colsum)          # ... representable in fp32
    got = _split(dq.cpu(), dkv.cpu(), c)
    assert torch.equal(got["dv"], expect)
    assert not got["dq"].any() and not got["dk"].any()


@gpu
def test_backward_is_deterministic_writes_everything_and_stays_in_bounds(monkeypatch):
    """Two launches are bitwise equal.  Under the guard (tests/guarded_alloc.py, both fill patterns): the bands around dq, dkv and
    the workspace stay intact, every element of both outputs is written (prefilled with NaN, none is left), q, kv and dout are
    unchanged, and the results are bitwise those of the unguarded run."""
    from mumpy_hip import ops
    case = (3, 5, 64)
    b1, r, c = case
    g = _setup(case, 1)[0]
    first = ops.deform_attention_bwd(g["q"], g["kv"], g["dout"], r, SCALE, math="bf16")
    again = ops.deform_attention_bwd(g["q"], g["kv"], g["dout"], r, SCALE, math="bf16")
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    host = {k: t.cpu() for k, t in g.items()}
    blocks = []

    def body(guard):
        t = {k: guard.tensor(v) for k, v in host.items()}
        before = len(guard.log)
        dq, dkv = ops.deform_attention_bwd(t["q"], t["kv"], t["dout"], r, SCALE, math="bf16")
        blocks.append(len(guard.log) - before)
        return {"dq": dq, "dkv": dkv}, [], None

    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set() and blocks == [3] * len(GA.PASSES)               # dq, dkv and the workspace, all inside the guard
    for outs in runs:
        assert not torch.isnan(outs["dq"]).any() and not torch.isnan(outs["dkv"]).any()
        assert GA.same_bits(outs["dq"], first[0]) and GA.same_bits(outs["dkv"], first[1])


@gpu
def test_tape_runs_the_bf16_forward_and_its_own_backward():
    """DeformAttentionFn under set_cva_math("bf16"): the output is ops.deform_attention(math="bf16") and the gradients are
    ops.deform_attention_bwd(math="bf16"), bit for bit."""
    from mumpy_hip import ops
    from mumpy_hip.autograd import DeformAttentionFn
    case = (2, 3, 192)
    b1, r, c = case
    g = _setup(case, 1)[0]
    q, kv = g["q"].clone().requires_grad_(True), g["kv"].clone().requires_grad_(True)
    before = ops.cva_math()
    try:
        ops.set_cva_math("bf16")
        out = DeformAttentionFn.apply(q, kv, SCALE)
        out.backward(g["dout"])
    finally:
        ops.set_cva_math(before)
    direct = ops.deform_attention(g["q"], g["kv"], ops.pad_mask(DEV), b1, 7, 7, c, r, SCALE, math="bf16")
    dq, dkv = ops.deform_attention_bwd(g["q"], g["kv"], g["dout"], r, SCALE, math="bf16")
    assert torch.equal(out.detach(), direct) and torch.equal(q.grad, dq) and torch.equal(kv.grad, dkv)
    assert not torch.equal(direct, ops.deform_attention(g["q"], g["kv"], ops.pad_mask(DEV), b1, 7, 7, c, r, SCALE))


# ------------------------------------------------------------------ the switch on swin_dattention_train
def _module_inputs(b1, r, c=96):
    return seeded_randn(130, b1, 49, c), seeded_randn(131, b1 * r, 49, c), seeded_randn(132, b1, 49, c)


def _module_run(b1, r, flip_before_backward=None, record=None):
    """swin_dattention_train on SwinDAttention(96, 3, 0.0, 3) -> (y, dx1, dx2, {name: grad}) on the CPU.  record: a list that receives
    the (q, kv, dout) the attention core's backward was called with."""
    from models.modules.deformableAttention import SwinDAttention
    from mumpy_hip import ops
    from mumpy_hip.autograd import swin_dattention_train
    att = fill_module_(SwinDAttention(96, 3, 0.0, 3)).eval().cuda()
    x1, x2, gy = _module_inputs(b1, r)
    x1g, x2g = x1.cuda().requires_grad_(True), x2.cuda().requires_grad_(True)
    y = swin_dattention_train(att, x1g, x2g)
    if flip_before_backward is not None:
        ops.set_cva_math(flip_before_backward)
    inner = ops.deform_attention_bwd
    if record is not None:
        def spy(q, kv, dout, *a, **kw):
            record.append((q.detach().cpu(), kv.detach().cpu(), dout.detach().cpu()))
            return inner(q, kv, dout, *a, **kw)
        ops.deform_attention_bwd = spy
    try:
        (y * gy.cuda()).sum().backward()
    finally:
        ops.deform_attention_bwd = inner
    return y.detach().cpu(), x1g.grad.cpu(), x2g.grad.cpu(), {n: p.grad.cpu() for n, p in att.named_parameters()}


def _same(a, b):
    return all(torch.equal(a[i], b[i]) for i in range(3)) and set(a[3]) == set(b[3]) and all(torch.equal(a[3][n], b[3][n]) for n in a[3])


@functools.lru_cache(maxsize=None)
def _module_oracle(b1, r):
    """fp32 autograd on the oracle's swin_dattention (CPU), as test_hip_swin_dattention_backward_vs_oracle builds it."""
    from models.modules.deformableAttention import SwinDAttention
    att = fill_module_(SwinDAttention(96, 3, 0.0, 3)).eval()
    sd = {"a." + k: v.detach().clone().requires_grad_(True) for k, v in att.state_dict().items()}
    x1, x2, gy = _module_inputs(b1, r)
    x1o, x2o = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    yo = O.swin_dattention(x1o, x2o, sd, "a")
    (yo * gy).sum().backward()
    return yo.detach(), x1o.grad, x2o.grad, {n: sd["a." + n].grad for n, _ in att.named_parameters()}


def _l2_cos(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm() / ref.norm()), float(torch.dot(got, ref) / (got.norm() * ref.norm()))


def _figures(run, oracle):
    """(output rel_err, {what: (relative L2, cosine)}, max |proj_k.bias gradient|) of a run against the oracle.  proj_k.bias is
    treated as in test_hip_swin_dattention_backward_vs_oracle: it adds the same q.b_k to every key's score, the true gradient is 0
    and has no relative measure, so it is kept out of the concatenation and looked at on its own."""
    y, dx1, dx2, grads = run
    yo, dx1o, dx2o, go = oracle
    names = sorted(n for n in grads if n != "proj_k.bias")
    fig = {"params": _l2_cos(torch.cat([grads[n].reshape(-1) for n in names]), torch.cat([go[n].reshape(-1) for n in names])),
           "dx1": _l2_cos(dx1, dx1o), "dx2": _l2_cos(dx2, dx2o)}
    return rel_err(y, yo), fig, float(grads["proj_k.bias"].abs().max())


@gpu
@pytest.mark.parametrize("b1,r", [(2, 5), (4, 1)])
def test_switch_reaches_the_tape_and_leaves_fp32_alone(b1, r):
    """swin_dattention_train on SwinDAttention(96, 3, 0.0, 3).  (a) never touched == set back to "fp32" after "bf16", bitwise: output,
    both input gradients, every parameter gradient.  (b) "bf16" differs.  (c) a tape built under "bf16" runs its own backward after
    the switch went back.  (d) against fp32 autograd on the oracle, with the switch alone and combined with set_matrix_math("bf16"):
    output rel_err <= 2e-2; relative L2 <= 1e-1 and cosine >= 0.995 for the concatenated parameter gradients and for each input
    gradient (the cva-group bars of test_hip_full_model_backward_bf16_vs_oracle).  The matrix-bf16-only figures (the parent's
    arithmetic) are printed beside them.  proj_k.bias (true gradient 0): with dS rounded to bf16 its rows no longer sum to zero to
    fp32 accuracy, so sum_j dK_j keeps one bf16 rounding of every dS: per channel at most 2^-8 scale sum |dS_ij| |r(q_i)| over all
    (kv window, i, j), computed here in fp64 from the q / kv / dO the tape's backward received; matrix math bf16 also rounds dK before
    the bias sum (2^-8 sum |dK|, already the parent's); 1e-5 is the fp32 test's floor."""
    from mumpy_hip import ops
    before, before_mm = ops.cva_math(), ops.matrix_math()
    seen, seen_both = [], []
    try:
        if before != "fp32":                                                   # "never touched" exists only in a process that started in
            ops.set_cva_math("fp32")                                           # the default mode
        ops.set_matrix_math("fp32")
        untouched = _module_run(b1, r)
        ops.set_cva_math("bf16")
        on = _module_run(b1, r, record=seen)
        carried = _module_run(b1, r, flip_before_backward="fp32")             # (c): forward under bf16, backward after the flip
        assert ops.cva_math() == "fp32"
        back = _module_run(b1, r)
        ops.set_matrix_math("bf16")
        matrix_only = _module_run(b1, r)
        ops.set_cva_math("bf16")
        both = _module_run(b1, r, record=seen_both)
    finally:
        ops.set_matrix_math(before_mm)
        ops.set_cva_math(before)
    assert _same(untouched, back)                                                                      # (a)
    assert not any(torch.equal(on[i], untouched[i]) for i in range(3))                                 # (b)
    assert not torch.equal(on[3]["proj_q.weight"], untouched[3]["proj_q.weight"])
    assert not torch.equal(on[3]["proj_v.weight"], untouched[3]["proj_v.weight"])
    assert _same(carried, on)                                                                          # (c)
    oracle = _module_oracle(b1, r)                                                                     # (d)
    kb_bound = {}
    for label, rec in (("cva bf16", seen), ("cva bf16 + matrix math bf16", seen_both)):
        (q, kv, dout), = rec
        _, _, ds, qh = _reference(q, kv, dout, r)
        kb_bound[label] = 1e-5 + float((U * SC * (ds.abs().sum(-1).unsqueeze(-1) * qh.abs()).sum(dim=(0, 2))).max())   # worst channel
        if "matrix" in label:
            kb_bound[label] += U * float(_rows(SC * (ds.transpose(-1, -2) @ qh)).abs().sum(dim=(0, 1)).max())
    report = {label: _figures(run, oracle) for label, run in
              (("fp32", untouched), ("matrix math bf16 only", matrix_only), ("cva bf16", on), ("cva bf16 + matrix math bf16", both))}
    for label, (yerr, fig, kb) in report.items():
        print(f"({b1}, {r}) {label}: y rel err {yerr:.3e}; " + "; ".join(f"{k} rel L2 {v[0]:.3e} cos {v[1]:.6f}" for k, v in fig.items())
              + f"; max |d proj_k.bias| {kb:.3e}" + (f" (bound {kb_bound[label]:.3e})" if label in kb_bound else ""))
    for label in ("cva bf16", "cva bf16 + matrix math bf16"):
        yerr, fig, kb = report[label]
        assert yerr <= 2e-2, (label, yerr)
        assert all(l2 <= 1e-1 and cos >= 0.995 for l2, cos in fig.values()), (label, fig)
        assert all(bool(torch.isfinite(t).all()) for t in (on if label == "cva bf16" else both)[3].values())
        assert kb <= kb_bound[label], (label, kb, kb_bound[label])


@gpu
def test_tape_under_bf16_captures_and_replays_bitwise():
    """DeformAttentionFn forward + backward under "bf16" at (2, 3, 192), captured the way GraphedTrainStep does it: every eager run
    (they are the warm-up) and the capture on ONE side stream, capture_error_mode="thread_local", .backward() into gradient buffers
    that exist before the capture.  No host synchronisation or allocation breaks the capture; two replays equal the eager result
    bitwise."""
    from mumpy_hip import ops
    from mumpy_hip.autograd import DeformAttentionFn
    from mumpy_hip.streams import new_distinct_stream
    b1, r, c = 2, 3, 192
    q = seeded_randn(2501, b1, 49, c).to(DEV).requires_grad_(True)
    kv = seeded_randn(2502, b1 * r, 49, 2 * c).to(DEV).requires_grad_(True)
    dout = seeded_randn(2503, b1, 49, c).to(DEV)
    q.grad, kv.grad = torch.zeros_like(q), torch.zeros_like(kv)
    ops.pad_mask(DEV)                                                          # (a cached table: built before the capture)

    def fwd_bwd():
        q.grad.zero_()
        kv.grad.zero_()
        y = DeformAttentionFn.apply(q, kv, SCALE)
        y.backward(dout)
        return y.detach()

    def snapshot(y):
        return [y.clone(), q.grad.clone(), kv.grad.clone()]

    before = ops.cva_math()
    try:
        # (from the high-priority pool: torch deals pool streams round-robin per priority, and which normal-priority handle a later
        # capture of this process gets decides how many fork streams mumpy_hip.streams keeps per parent -- that deal is left alone)
        side = new_distinct_stream(DEV, (torch.cuda.current_stream().cuda_stream,), priority=-1)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.set_cva_math("fp32")
            other = snapshot(fwd_bwd())
            ops.set_cva_math("bf16")
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
        ops.set_cva_math(before)
    for rep in replays:
        assert all(torch.equal(a, e) for a, e in zip(rep, eager))
    assert not torch.equal(eager[0], other[0]) and not torch.equal(eager[1], other[1]) and not torch.equal(eager[2], other[2])
