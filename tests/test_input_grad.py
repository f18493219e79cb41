"""GPU: the gradient with respect to the input clip (include/mumpy_hip_ext10.h; ops.faf_bwd / tokenize_dx / pgd_step;
autograd.ClipInputFn behind encoder_train(input_grad=True); mumpy_hip.inputgrad.input_gradient and PGDAttack).

The kernels are held against the host restatements of mumpy_hip.inputgrad (themselves held against autograd in
tests/test_input_grad_host.py) and against autograd on the oracle; the whole model against autograd on the oracle with
x.requires_grad_(), per frame, at the project's per-parameter bar of 1e-2 (test_hip_full_model_backward_vs_oracle)."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from conftest import rel_err
from oracle import mumpy_oracle as O
from test_input_grad_host import TIGHT, tubelets_of
from weight_fill import fill_module_, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-2                                                                  # per frame; the bar of the tokenizer weights, at dx's depth


def _ops():
    from mumpy_hip import ops
    return ops


def _faf():
    from models.modules.dct import FAF
    faf = FAF()
    return faf, faf._mats(torch.device(DEV))


# ================================================================================================ ops.faf_bwd
def test_faf_bwd_vs_reference_oracle_and_adjoint(monkeypatch):
    from mumpy_hip.inputgrad import faf_bwd_reference
    ops = _ops()
    faf, (d, dt) = _faf()
    x = seeded_randn(31, 2, 3, 3, 224, 224)
    g = seeded_randn(32, 2, 9, 224, 224)
    lim = (faf.lo_hi, faf.mid_lo, faf.mid_hi)
    assert lim == (79, 79, 112)
    plain = ops.faf_bwd(g.to(DEV), d, dt, *lim)
    again = ops.faf_bwd(g.to(DEV), d, dt, *lim)
    assert GA.same_bits(plain, again)                                       # deterministic: no atomics, fixed summation order

    def body(guard):
        return {"dxf": ops.faf_bwd(guard.tensor(g), guard.tensor(d.cpu()), guard.tensor(dt.cpu()), *lim)}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:                                                       # bands intact, every element written, inputs unchanged
        assert GA.same_bits(outs["dxf"], plain)
    e_ref = rel_err(plain.cpu(), faf_bwd_reference(g))
    xr = x.clone().requires_grad_()
    (O.faf_frame1(xr) * g).sum().backward()
    e_orc = rel_err(plain.cpu(), xr.grad[:, 1])
    y = faf.forward_frame(x.to(DEV), 1)                                     # <faf(x), g> == <x_frame, faf_bwd(g)> on the device results
    lhs = float((y.double() * g.to(DEV).double()).sum())
    rhs = float((x[:, 1].to(DEV).double() * plain.double()).sum())
    e_adj = abs(lhs - rhs) / abs(lhs)
    print(f"faf_bwd: vs host restatement {e_ref:.3e}, vs oracle autograd {e_orc:.3e}, adjoint identity {e_adj:.3e}")
    assert e_ref < TIGHT and e_orc < TIGHT and e_adj < TIGHT


def test_faf_bwd_band_edges_with_impulse_spectra():
    """g_band = D^T E_ij D in all three bands gives count(i,j) D^T E_ij D: 2 on the anti-diagonal the low and mid bands share, 1
    inside a band and on its edges, 0 between the mid and the high band.  One clip per impulse, one call."""
    ops = _ops()
    faf, (d, dt) = _faf()
    cases = (((40, 39), 2), ((0, 0), 1), ((40, 38), 1), ((40, 40), 1), ((56, 56), 1), ((112, 112), 1), ((223, 223), 1), ((56, 57), 0),
             ((111, 112), 0))
    masks = O.band_masks(224)
    d64 = O.dct_matrix(224).double()
    basis = torch.stack([torch.outer(d64[i], d64[j]) for (i, j), _ in cases])                   # (9, 224, 224), asymmetric in (i, j)
    g = basis.float()[:, None].expand(-1, 9, -1, -1).contiguous()
    out = ops.faf_bwd(g.to(DEV), d, dt, faf.lo_hi, faf.mid_lo, faf.mid_hi).cpu().double()
    for k, ((i, j), count) in enumerate(cases):
        assert int(masks[:, i, j].sum()) == count, (i, j)
        for rgb in range(3):
            err = float((out[k, rgb] - count * basis[k]).abs().max() / basis[k].abs().max())
            assert err < TIGHT, ((i, j), rgb, err)


# ================================================================================================ ops.tokenize_dx
def _dcols(seed, b, t, h, w):
    """Random column gradients of the three views with NaN in the pad columns."""
    cols = []
    for v, tv in enumerate(tubelets_of(t)):
        rows, k = b * ((t - tv) // tv + 1) * (h // 4) * (w // 4), 48 * tv
        c = torch.full((rows, k + (-k) % 32), float("nan"))
        c[:, :k] = seeded_randn(seed + v, rows, k)
        cols.append(c)
    return cols


@pytest.mark.parametrize("with_dxf", [False, True])
@pytest.mark.parametrize("b,t,h,w", [(2, 3, 8, 12), (2, 5, 8, 12), (2, 9, 8, 12), (1, 3, 224, 224)])
def test_tokenize_dx_vs_reference(monkeypatch, b, t, h, w, with_dxf):
    from mumpy_hip.inputgrad import tokenize_dx_reference
    ops = _ops()
    tub = tubelets_of(t)
    cols = _dcols(200 + t, b, t, h, w)
    if t == 3:
        assert [c.shape[1] for c in cols] == [160, 96, 64]                   # 144, 96, 48 padded: every view has pad columns but one
    dxf = seeded_randn(210, b, 3, h, w) if with_dxf else None
    ref = tokenize_dx_reference(cols, tub, b, t, h, w, dxf=dxf, frame=1)

    def body(guard):                                                        # the output arrives filled with NaN (then 3.39e38) and guard-banded
        return {"dx": ops.tokenize_dx([guard.tensor(c) for c in cols], tub, b, t, h, w,
                                      dxf=None if dxf is None else guard.tensor(dxf), frame=1)}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        dx = outs["dx"].cpu()
        assert bool(torch.isfinite(dx).all())                               # nothing unwritten, no pad column leaked
        assert rel_err(dx, ref) < TIGHT
    assert len(runs) == len(GA.PASSES) and all(GA.same_bits(runs[0]["dx"], outs["dx"]) for outs in runs[1:])
    # view 2 (project2, tubelet T-1) alone: frame T-1 gets exact zeros
    zero = [torch.zeros_like(cols[0]), cols[1], torch.zeros_like(cols[2])]
    only2 = ops.tokenize_dx([c.to(DEV) for c in zero], tub, b, t, h, w).cpu()
    assert float(only2[:, t - 1].abs().max()) == 0.0 and float(only2[:, :t - 1].abs().max()) > 0.0


def test_tokenize_dx_writes_into_a_given_buffer_and_other_frames():
    from mumpy_hip.inputgrad import tokenize_dx_reference
    ops = _ops()
    b, t, h, w = 2, 5, 8, 12
    cols, dxf = _dcols(220, b, t, h, w), seeded_randn(221, b, 3, h, w)
    out = torch.full((b, t, 3, h, w), float("nan"), device=DEV)
    for frame in (0, 4):
        got = ops.tokenize_dx([c.to(DEV) for c in cols], tubelets_of(t), b, t, h, w, dxf=dxf.to(DEV), frame=frame, out=out)
        assert got is out
        assert rel_err(out.cpu(), tokenize_dx_reference(cols, tubelets_of(t), b, t, h, w, dxf=dxf, frame=frame)) < TIGHT


# ================================================================================================ ops.pgd_step
def _pgd_torch(x, g, x0, alpha, eps3, lo3, hi3):
    """The expression of include/mumpy_hip_ext10.h in torch, fp32, in its order."""
    sh = (1,) * (x.dim() - 3) + (3, 1, 1)
    eps, lo, hi = (torch.tensor(a, dtype=torch.float32, device=x.device).reshape(sh) for a in (eps3, lo3, hi3))
    sgn = torch.where(g > 0, 1.0, torch.where(g < 0, -1.0, 0.0)).to(torch.float32)      # sgn(0) = sgn(NaN) = 0, sgn(+-inf) = +-1
    v = x + torch.tensor(alpha, dtype=torch.float32, device=x.device) * sgn
    v = torch.minimum(torch.maximum(v, x0 - eps), x0 + eps)
    return torch.minimum(torch.maximum(v, lo), hi)


@pytest.mark.parametrize("shape", [(1, 1, 3, 5, 5), (2, 3, 3, 8, 12)])
@pytest.mark.parametrize("alpha", [1.0 / 255 / 0.2085, -0.013, 0.5])
def test_pgd_step_bit_for_bit(shape, alpha):
    from mumpy_hip.inputgrad import pgd_bounds
    ops = _ops()
    eps3, lo3, hi3 = pgd_bounds(4 / 255)
    x0 = (seeded_randn(300, *shape) * 1.5).to(DEV)                          # some pixels outside [lo3, hi3]: the range clamp works
    x = x0 + (seeded_randn(301, *shape) * 0.05).to(DEV)                     # some of them outside the eps ball as well
    g = seeded_randn(302, *shape).to(DEV)
    flat = g.view(-1)
    special = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e-45, -1e-45]
    flat[:len(special)] = torch.tensor(special, device=DEV)
    flat[-len(special):] = torch.tensor(special, device=DEV)               # ... in the tail as well
    sh = (1,) * (len(shape) - 3) + (3, 1, 1)
    e = torch.tensor(eps3, device=DEV).reshape(sh)
    xv = x.view(-1)
    xv[10:14] = (x0 + e).reshape(-1)[10:14]                                  # elements at both bounds of the ball
    xv[20:24] = (x0 - e).reshape(-1)[20:24]
    want = _pgd_torch(x, g, x0, alpha, eps3, lo3, hi3)
    x0_before, g_before = x0.clone(), g.clone()
    got = ops.pgd_step(x, g, x0, alpha, eps3, lo3, hi3)
    assert got is x and GA.same_bits(x, want)
    assert GA.same_bits(x0, x0_before) and GA.same_bits(g, g_before)
    lo, hi = (torch.tensor(a, device=DEV).reshape(sh) for a in (lo3, hi3))
    assert bool(((x >= lo) & (x <= hi)).all())
    # a NaN or zero gradient only re-projects
    idx = torch.tensor([0, 1, 2], device=DEV)
    keep = _pgd_torch(x0 + 0, torch.zeros_like(g), x0, alpha, eps3, lo3, hi3)
    x2 = x0.clone()
    ops.pgd_step(x2, g, x0, alpha, eps3, lo3, hi3)
    assert GA.same_bits(x2.view(-1)[idx], keep.view(-1)[idx])


def test_pgd_step_eps_zero_returns_the_clamped_clip():
    from mumpy_hip.inputgrad import pgd_bounds
    ops = _ops()
    _, lo3, hi3 = pgd_bounds(0.0)
    x0 = (seeded_randn(310, 2, 3, 3, 8, 12) * 1.5).to(DEV)
    x = x0 + 0.3
    ops.pgd_step(x, seeded_randn(311, 2, 3, 3, 8, 12).to(DEV), x0, 0.1, (0.0, 0.0, 0.0), lo3, hi3)
    lo, hi = (torch.tensor(a, device=DEV).reshape(1, 1, 3, 1, 1) for a in (lo3, hi3))
    assert GA.same_bits(x, torch.minimum(torch.maximum(x0, lo), hi))


# ================================================================================================ refusals
def test_ops_refuse_bad_calls_on_the_device():
    ops = _ops()
    faf, (d, dt) = _faf()
    g = torch.zeros(1, 9, 224, 224, device=DEV)
    for bad in (dict(dout=g[:, :8]), dict(d=d[:100]), dict(dt=dt.double()), dict(out=torch.zeros(1, 3, 224, 223, device=DEV))):
        kw = dict(dout=g, d=d, dt=dt)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="faf_bwd"):
            ops.faf_bwd(kw.pop("dout"), kw.pop("d"), kw.pop("dt"), 79, 79, 112, **kw)
    with pytest.raises(RuntimeError, match="band"):
        ops.faf_bwd(g, d, dt, 79, 120, 112)                                  # the library's refusal: mid_hi < mid_lo
    odd = torch.zeros(224 * 224 + 1, device=DEV)[1:].view(224, 224)         # contiguous, 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="aligned"):
        ops.faf_bwd(g, odd, dt, 79, 79, 112)
    b, t, h, w = 2, 3, 8, 12
    cols = [c.to(DEV).nan_to_num(0.0) for c in _dcols(230, b, t, h, w)]
    dxf = torch.zeros(b, 3, h, w, device=DEV)
    for kw in (dict(frame=3, dxf=dxf), dict(frame=-1, dxf=dxf), dict(dxf=dxf[:1]), dict(out=torch.zeros(b, t, 3, h, w + 4, device=DEV)),
               dict(out=torch.zeros(b, t, 3, w, h, device=DEV).transpose(3, 4)), dict(h=12), dict(t=4)):
        args = dict(b=b, t=t, h=h, w=w)
        args.update(kw)
        with pytest.raises(RuntimeError, match="tokenize_dx"):
            ops.tokenize_dx(cols, tubelets_of(3), **args)
    with pytest.raises(RuntimeError, match="tokenize_dx"):
        ops.tokenize_dx([cols[0], cols[1], cols[2].double()], tubelets_of(3), b, t, h, w)
    off = torch.zeros(cols[2].numel() + 1, device=DEV)[1:].view(cols[2].shape)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.tokenize_dx([cols[0], cols[1], off], tubelets_of(3), b, t, h, w)
    x = torch.zeros(2, 3, 3, 8, 12, device=DEV)
    bounds = ((0.1,) * 3, (-2.0,) * 3, (2.0,) * 3)
    for bad in (dict(g=x[:1]), dict(x0=x.double()), dict(x_adv=x.transpose(3, 4)), dict(x_adv=torch.zeros(2, 3, 4, 8, 12, device=DEV))):
        kw = dict(x_adv=x, g=x, x0=x)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="pgd_step"):
            ops.pgd_step(kw["x_adv"], kw["g"], kw["x0"], 0.1, *bounds)
    for bad in (((-0.1, 0.1, 0.1), bounds[1], bounds[2]), (bounds[0], (3.0, -2.0, -2.0), bounds[2]), ((0.1, 0.1), bounds[1], bounds[2])):
        with pytest.raises(RuntimeError, match="pgd_step"):
            ops.pgd_step(x, x, x, 0.1, *bad)
    with pytest.raises(RuntimeError, match="alpha"):
        ops.pgd_step(x, x, x, float("nan"), *bounds)
    assert float(x.abs().max()) == 0.0                                       # nothing was launched on it


# ================================================================================================ the whole model
_MODELS, _ORACLE = {}, {}


def _model(t):
    """The three-view model with the test weights on the GPU, eval mode, built once per temporal length."""
    if t not in _MODELS:
        from models.decoder.decoder import Decoder
        from models.encoder.encoder import Encoder
        enc = fill_module_(Encoder(num_frames=t)).eval()
        dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, t])).eval()
        sd = ({k: v.detach().clone() for k, v in enc.state_dict().items()}, {k: v.detach().clone() for k, v in dec.state_dict().items()})
        _MODELS[t] = (enc.to(DEV), dec.to(DEV), sd)
    return _MODELS[t]


def _inputs(b, t):
    return seeded_randn(990, b, t, 3, 224, 224), seeded_randn(991, b, 1, 224, 224)


def _oracle_dx(b, t, clip=None):
    """dL/dx of loss = sum(logits * g) from autograd on the oracle (CPU, fp32) with x.requires_grad_(); clip = c: clip c of the batch
    alone, at B = 1.  Computed once per configuration and never modified."""
    key = (b, t, clip)
    if key not in _ORACLE:
        _, _, (sde, sdd) = _model(t)
        x, g = _inputs(b, t)
        if clip is not None:
            x, g = x[clip:clip + 1], g[clip:clip + 1]
        xr = x.clone().requires_grad_()
        lo = O.full_forward(sde, sdd, xr)[0]
        (lo * g).sum().backward()
        _ORACLE[key] = (lo.detach(), xr.grad.detach())
    return _ORACLE[key]


def _tape(b, t, input_grad, coupling=None):
    """One taped forward + backward of loss = sum(logits * g) -> (logits, {name: grad}, dx or None); the grads are taken off the
    parameters, which are left without one."""
    from mumpy_hip.autograd import decoder_train, encoder_train
    enc, dec, _ = _model(t)
    x, g = _inputs(b, t)
    xg = x.to(DEV)
    if input_grad:
        xg.requires_grad_()
    lg, _ = decoder_train(dec, *encoder_train(enc, xg, coupling=coupling, input_grad=input_grad))
    (lg * g.to(DEV)).sum().backward()
    grads = {}
    for which, mod in (("enc", enc), ("dec", dec)):
        for n, p in mod.named_parameters():
            grads[f"{which}.{n}"] = p.grad
            p.grad = None
    return lg.detach(), grads, xg.grad


def _per_frame(dx, ref):
    return [rel_err(dx[:, f], ref[:, f]) for f in range(ref.shape[1])]


@pytest.mark.parametrize("b,t", [(1, 3), (2, 5)])
def test_input_grad_on_the_tape_vs_oracle(b, t):
    """(B,T) = (1,3) and (2,5), loss sum(logits * g): every frame of dx on its own against autograd on the oracle, below 1e-2.
    Measured on an MI355X: see profiles/input_gradient.md.  Same run: logits and every parameter gradient are the same bits with the
    node in (input_grad=True) and out."""
    lo, ref = _oracle_dx(b, t)
    lg, grads, dx = _tape(b, t, True)
    errs = _per_frame(dx.cpu(), ref)
    print(f"input gradient B={b} T={t}: logits {rel_err(lg.cpu(), lo):.3e}, per-frame rel_err of dx {['%.3e' % e for e in errs]}, "
          f"per-frame max|dx| {['%.3e' % float(ref[:, f].abs().max()) for f in range(t)]}")
    assert rel_err(lg.cpu(), lo) < 1e-3
    assert all(e < BAR for e in errs), errs
    lg0, grads0, none = _tape(b, t, False)
    assert none is None
    assert GA.same_bits(lg, lg0)
    assert set(grads) == set(grads0) and all(v is not None for v in grads.values())
    differ = [n for n in grads if not GA.same_bits(grads[n], grads0[n])]
    assert not differ, differ[:10]


def test_input_grad_without_the_faf_branch_is_the_wrong_gradient():
    """What the refusal of encoder_train(x.requires_grad_(), input_grad=False) protects from: without the FAF branch frame 1 of dx is
    off by most of its size, frames 0 and 2 are untouched (tokenize_dx alone, from the tape's own column gradients)."""
    from mumpy_hip.autograd import decoder_train, encoder_train
    enc, dec, _ = _model(3)
    x, g = _inputs(1, 3)
    _, ref = _oracle_dx(1, 3)
    with pytest.raises(RuntimeError, match="input_grad=True"):
        encoder_train(enc, x.to(DEV).requires_grad_())
    xg = x.to(DEV).requires_grad_()
    fx, vx, dct = encoder_train(enc, xg, input_grad=True)
    lg, _ = decoder_train(dec, fx, vx, dct.detach())                         # the FAF branch cut
    (lg * g.to(DEV)).sum().backward()
    for mod in (enc, dec):
        for p in mod.parameters():
            p.grad = None
    errs = _per_frame(xg.grad.cpu(), ref)
    assert errs[0] < BAR and errs[2] < BAR and errs[1] > 0.5, errs


def test_input_gradient_leaves_parameters_alone_and_launches_no_weight_gradient(monkeypatch):
    from mumpy_hip import autograd as A, ops
    from mumpy_hip.inputgrad import input_gradient
    enc, dec, _ = _model(3)
    x, _ = _inputs(1, 3)
    target = (torch.rand(1, 1, 224, 224, generator=torch.Generator().manual_seed(7)) < 0.1).float().to(DEV)
    xg = x.to(DEV)
    params = [p for m in (enc, dec) for p in m.parameters()]
    params[3].requires_grad_(False)                                          # a flag the caller had set survives
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, 0.25 + i)                                # a pattern in every .grad
    before = [p.grad.clone() for p in params]
    flags = [p.requires_grad for p in params]
    seen = []
    real_lb, real_lgb, real_wg, real_cs = ops.linear_bwd, ops.linear_gelu_bwd, ops.conv2d_wgrad, ops.col_sum

    def linear_bwd(*a, **kw):
        seen.append(("linear_bwd", kw.get("need_dw", True), kw.get("need_db", False)))
        return real_lb(*a, **kw)

    def linear_gelu_bwd(*a, **kw):
        seen.append(("linear_gelu_bwd", kw.get("need_dw", True), kw.get("need_db", False)))
        return real_lgb(*a, **kw)

    def conv2d_wgrad(*a, **kw):
        seen.append(("conv2d_wgrad", True, False))
        return real_wg(*a, **kw)

    def col_sum(*a, **kw):
        seen.append(("col_sum", False, True))
        return real_cs(*a, **kw)
    for name, fn in (("linear_bwd", linear_bwd), ("linear_gelu_bwd", linear_gelu_bwd), ("conv2d_wgrad", conv2d_wgrad), ("col_sum", col_sum)):
        monkeypatch.setattr(ops, name, fn)
    loss3, dx = input_gradient(enc, dec, xg, target)
    monkeypatch.undo()
    assert seen and not [s for s in seen if s[1] or s[2]], [s for s in seen if s[1] or s[2]][:5]
    assert [p.requires_grad for p in params] == flags
    assert all(GA.same_bits(p.grad, b) for p, b in zip(params, before))
    assert not xg.requires_grad and xg.grad is None
    # loss3 is ops.mask_loss of the taped logits; dx is the tape's gradient of that loss
    for p in params:
        p.grad = None
    xr = x.to(DEV).requires_grad_()
    lg, _ = A.decoder_train(dec, *A.encoder_train(enc, xr, input_grad=True))
    want3, dlg = ops.mask_loss(lg.detach(), target)
    lg.backward(dlg)
    assert GA.same_bits(loss3, want3)
    assert rel_err(dx, xr.grad) < TIGHT
    # the flags come back after an exception raised inside as well
    params[3].requires_grad_(False)
    flags = [p.requires_grad for p in params]
    with pytest.raises(RuntimeError):
        input_gradient(enc, dec, xg, target[:, :, :100])                    # mask_loss refuses the target, after the taped forward
    assert [p.requires_grad for p in params] == flags
    for p in params:
        p.requires_grad_(True)
        p.grad = None


def test_input_grad_with_per_clip_coupling_vs_per_clip_oracle():
    """coupling="clip" at (2,3): each clip's dx against the oracle run on that clip alone at B = 1."""
    lg, _, dx = _tape(2, 3, True, coupling="clip")
    for c in range(2):
        lo, ref = _oracle_dx(2, 3, clip=c)
        errs = _per_frame(dx[c:c + 1].cpu(), ref)
        print(f"input gradient, coupling='clip', clip {c} of 2, T=3: logits {rel_err(lg[c:c + 1].cpu(), lo):.3e}, "
              f"per-frame rel_err of dx {['%.3e' % e for e in errs]}")
        assert all(e < BAR for e in errs), (c, errs)


def test_pgd_attack_graphed_and_eager():
    from mumpy_hip import ops
    from mumpy_hip.inputgrad import PGDAttack, input_gradient, pgd_bounds
    enc, dec, _ = _model(3)
    x, _ = _inputs(1, 3)
    x0 = (x * 0.5).to(DEV)                                                   # most pixels inside the valid range
    target = (torch.rand(1, 1, 224, 224, generator=torch.Generator().manual_seed(7)) < 0.1).float().to(DEV)
    eps, alpha = 4 / 255, 1 / 255
    eps3, lo3, hi3 = pgd_bounds(eps)
    e, lo, hi = (torch.tensor(a, device=DEV).reshape(1, 1, 3, 1, 1) for a in (eps3, lo3, hi3))
    x0c = torch.minimum(torch.maximum(x0, lo), hi)                           # a clip of valid pixels, as a loader produces
    graphed = PGDAttack(enc, dec, x0c, target, eps, alpha, graph=True)
    eager = PGDAttack(enc, dec, x0c, target, eps, alpha, graph=False)
    xa_g, xa_e = graphed.run(3), eager.run(3)
    assert rel_err(xa_g, xa_e) < TIGHT
    for xa in (xa_g, xa_e):
        assert bool(((xa - x0c).abs() <= e).all()) and bool(((xa >= lo) & (xa <= hi)).all())
    loss_clean = float(input_gradient(enc, dec, x0c, target)[0][0])
    loss_adv = float(input_gradient(enc, dec, xa_g, target)[0][0])
    print(f"PGD eps=4/255 alpha=1/255 3 steps: mask loss {loss_clean:.6f} -> {loss_adv:.6f}")
    assert loss_adv > loss_clean
    # FGSM: one step with alpha = eps from an independently computed dx
    _, dx = input_gradient(enc, dec, x0c, target)
    want = torch.minimum(torch.maximum(torch.minimum(torch.maximum(x0c + e * torch.sign(dx), x0c - e), x0c + e), lo), hi)
    fgsm = PGDAttack(enc, dec, x0c, target, eps, eps, graph=False).run(1)
    assert rel_err(fgsm, want) < TIGHT
    # a second run with a new clip replays the same capture
    graph_before = graphed.graph
    x1 = torch.minimum(torch.maximum((seeded_randn(995, 1, 3, 3, 224, 224) * 0.5).to(DEV), lo), hi)
    xb_g = graphed.run(3, x=x1)
    assert graphed.graph is graph_before
    xb_e = eager.run(3, x=x1)
    assert rel_err(xb_g, xb_e) < TIGHT and bool(((xb_g - x1).abs() <= e).all())
    assert not GA.same_bits(xb_g, xa_g)
    assert all(p.requires_grad and p.grad is None for m in (enc, dec) for p in m.parameters())
