"""CPU only: the host half of the input-clip gradient (include/mumpy_hip_ext10.h, mumpy_hip.inputgrad, encoder_train(input_grad=)).

  * the header declares exactly the pinned names; the error codes are the frozen header's;
  * every new entry refuses null, misaligned and out-of-range arguments with its code, nothing launched (the calls made here are
    refusals only, so the test is safe with or without a device);
  * faf_bwd_reference against autograd of the oracle's faf_frame1; tokenize_dx_reference against autograd of F.conv3d with the three
    strides; pgd_bounds; the new refusal of encoder_train and the unchanged old ones."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from abi_surface import define, names_of
from oracle import mumpy_oracle as O
from weight_fill import seeded_randn

TIGHT = 5e-5
EINVAL, EALIGN, ENULL = -1, -2, -3
ARGS = {
    "mumpy_faf_bwd": ["dout", "D", "Dt", "scratch", "dxf", "B", "lo_hi", "mid_lo", "mid_hi", "stream"],
    "mumpy_tokenize_dx": ["dcols0", "dcols1", "dcols2", "dxf", "dx", "B", "T", "H", "W", "t0", "t1", "t2", "ld0", "ld1", "ld2", "frame",
                          "stream"],
    "mumpy_pgd_step": ["x_adv", "g", "x0", "n", "hw", "alpha", "eps3", "lo3", "hi3", "stream"],
}


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def tubelets_of(t):
    """The three views' tubelet lengths (project1, project2, project3) for a clip of t frames: (T, T-1, 1)."""
    return [t, t - 1, 1]


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_error_codes_are_the_headers():
    for name, code in (("MUMPY_EINVAL", EINVAL), ("MUMPY_EALIGN", EALIGN), ("MUMPY_ENULL", ENULL)):
        assert define("mumpy_hip.h", name) == code, name


def test_ext10_header_declares_exactly_the_pinned_names():
    """(tests/test_abi.py holds the header to its binding and to both libraries.)"""
    assert names_of("mumpy_hip_ext10.h") == dict(ARGS, mumpy_ext10_version=[])


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
P = 4096                                                                   # a fake, 16-byte aligned, never dereferenced address
F3 = ctypes.c_float * 3


def _valid(entry):
    if entry == "mumpy_faf_bwd":
        return dict(dout=P, D=P, Dt=P, scratch=P, dxf=P, B=2, lo_hi=79, mid_lo=79, mid_hi=112, stream=None)
    if entry == "mumpy_tokenize_dx":
        return dict(dcols0=P, dcols1=P, dcols2=P, dxf=P, dx=P, B=2, T=3, H=8, W=12, t0=3, t1=2, t2=1, ld0=160, ld1=96, ld2=64, frame=1,
                    stream=None)
    return dict(x_adv=P, g=P, x0=P, n=3 * 25 * 2, hw=25, alpha=0.1, eps3=F3(0.1, 0.1, 0.1), lo3=F3(-2, -2, -2), hi3=F3(2, 2, 2),
                stream=None)


def _call(lib, entry, **over):
    v = _valid(entry)
    v.update(over)
    return getattr(lib, entry)(*[v[n] for n in ARGS[entry]])


def test_new_entries_refuse_before_launch():
    """Every call here is a refusal: a negative code and a message, nothing launched."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    for ptr in ("dout", "D", "Dt", "scratch", "dxf"):
        assert _call(lib, "mumpy_faf_bwd", **{ptr: None}) == ENULL and b"null" in lib.mumpy_last_error(), ptr
        assert _call(lib, "mumpy_faf_bwd", **{ptr: P + 4}) == EALIGN, ptr
    for bad in (dict(B=0), dict(B=-1), dict(lo_hi=-1), dict(mid_lo=-1), dict(mid_lo=113), dict(mid_hi=448)):
        assert _call(lib, "mumpy_faf_bwd", **bad) == EINVAL and b"faf_bwd" in lib.mumpy_last_error(), bad
    for ptr in ("dcols0", "dcols1", "dcols2", "dx"):
        assert _call(lib, "mumpy_tokenize_dx", **{ptr: None}) == ENULL and b"null" in lib.mumpy_last_error(), ptr
    for ptr in ("dcols0", "dcols1", "dcols2", "dxf", "dx"):
        assert _call(lib, "mumpy_tokenize_dx", **{ptr: P + 8}) == EALIGN, ptr
    for bad in (dict(B=0), dict(T=0), dict(H=10), dict(W=6), dict(H=0), dict(W=-4), dict(t0=0), dict(t0=4), dict(t1=-1), dict(ld2=44),
                dict(ld1=95), dict(ld2=66), dict(frame=3), dict(frame=-1), dict(frame=7)):
        assert _call(lib, "mumpy_tokenize_dx", **bad) == EINVAL and b"tokenize_dx" in lib.mumpy_last_error(), bad
    for ptr in ("x_adv", "g", "x0", "eps3", "lo3", "hi3"):
        assert _call(lib, "mumpy_pgd_step", **{ptr: None}) == ENULL and b"null" in lib.mumpy_last_error(), ptr
    for ptr in ("x_adv", "g", "x0"):
        assert _call(lib, "mumpy_pgd_step", **{ptr: P + 4}) == EALIGN, ptr
    for bad in (dict(n=-75), dict(hw=0), dict(n=76), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(eps3=F3(0.1, -0.1, 0.1)),
                dict(eps3=F3(float("nan"), 0.1, 0.1)), dict(lo3=F3(-2, 3, -2))):
        assert _call(lib, "mumpy_pgd_step", **bad) == EINVAL and b"pgd_step" in lib.mumpy_last_error(), bad


def test_ops_refuse_without_a_device():
    """The wrappers compare sizes, dtypes and devices before the call: CPU tensors and wrong shapes never reach the library."""
    from mumpy_hip import ops
    d = torch.zeros(224, 224)
    with pytest.raises(RuntimeError, match="faf_bwd"):
        ops.faf_bwd(torch.zeros(1, 9, 224, 224), d, d, 79, 79, 112)       # on the CPU
    with pytest.raises(RuntimeError, match="faf_bwd"):
        ops.faf_bwd(torch.zeros(1, 3, 224, 224), d, d, 79, 79, 112)
    cols = [torch.zeros(2 * 1 * 6, 160), torch.zeros(2 * 1 * 6, 96), torch.zeros(2 * 3 * 6, 64)]
    with pytest.raises(RuntimeError, match="tokenize_dx"):
        ops.tokenize_dx(cols, [3, 2, 1], 2, 3, 8, 12)                     # on the CPU
    for bad in (dict(h=10), dict(w=6), dict(frame=3, dxf=torch.zeros(2, 3, 8, 12)), dict(t=2)):
        kw = dict(b=2, t=3, h=8, w=12)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="tokenize_dx"):
            ops.tokenize_dx(cols, [3, 2, 1], **kw)
    with pytest.raises(RuntimeError, match="tokenize_dx"):
        ops.tokenize_dx(cols[:2], [3, 2], 2, 3, 8, 12)
    with pytest.raises(RuntimeError, match="tokenize_dx"):
        ops.tokenize_dx([cols[0], cols[1][:, :92], cols[2]], [3, 2, 1], 2, 3, 8, 12)
    x = torch.zeros(1, 1, 3, 5, 5)
    with pytest.raises(RuntimeError, match="pgd_step"):
        ops.pgd_step(x, x, x, 0.1, (0.1,) * 3, (-2.0,) * 3, (2.0,) * 3)   # on the CPU
    with pytest.raises(RuntimeError, match="pgd_step"):
        ops.pgd_step(torch.zeros(1, 4, 5, 5), x, x, 0.1, (0.1,) * 3, (-2.0,) * 3, (2.0,) * 3)


# ------------------------------------------------------------------------------------------------ host restatements
def test_faf_bwd_reference_vs_oracle_autograd():
    from mumpy_hip.inputgrad import faf_bwd_reference
    x = seeded_randn(31, 2, 3, 3, 224, 224).requires_grad_()
    g = seeded_randn(32, 2, 9, 224, 224)
    (O.faf_frame1(x) * g).sum().backward()
    assert float(x.grad[:, 0].abs().max()) == 0.0 and float(x.grad[:, 2].abs().max()) == 0.0      # only frame 1 is read
    e = rel_err(faf_bwd_reference(g), x.grad[:, 1])
    print(f"faf_bwd_reference vs autograd of O.faf_frame1: {e:.3e}")
    assert e < TIGHT


def test_faf_bwd_reference_counts_band_overlap():
    """An impulse spectrum in all three bands comes back multiplied by the number of bands its coefficient lies in."""
    from mumpy_hip.inputgrad import faf_bwd_reference
    d = O.dct_matrix(224).double()
    masks = O.band_masks(224)
    for (i, j), count in (((40, 39), 2), ((0, 0), 1), ((40, 38), 1), ((40, 40), 1), ((56, 56), 1), ((112, 112), 1), ((223, 223), 1),
                          ((56, 57), 0), ((111, 112), 0)):
        assert int(masks[:, i, j].sum()) == count, (i, j)
        basis = torch.outer(d[i], d[j]).float()                            # D^T E_ij D
        out = faf_bwd_reference(basis.expand(1, 9, 224, 224).contiguous())
        assert float((out[0, 0].double() - count * basis.double()).abs().max()) < TIGHT * float(basis.abs().max()), (i, j)


@pytest.mark.parametrize("t", [3, 5, 9])
def test_tokenize_dx_reference_vs_conv3d_autograd(t):
    from mumpy_hip.inputgrad import tokenize_dx_reference
    b, h, w = 2, 8, 12
    tub = tubelets_of(t)
    assert tub[1] == t - 1
    x = seeded_randn(40 + t, b, t, 3, h, w).requires_grad_()
    ws = [seeded_randn(50 + v, 8, 3, tv, 4, 4) for v, tv in enumerate(tub)]
    gs, dcols, loss = [], [], 0
    for v, tv in enumerate(tub):
        y = F.conv3d(x.permute(0, 2, 1, 3, 4), ws[v], stride=(tv, 4, 4))                  # (B, C, tt, H/4, W/4)
        g = seeded_randn(60 + v, *y.shape)
        loss = loss + (y * g).sum()
        # dcols_v = dY W_v with rows (b, tt, py, px) and columns (ch, t, y%4, x%4), padded to a multiple of 32 with NaN
        dy = g.permute(0, 2, 3, 4, 1).reshape(-1, 8)
        dc = dy @ ws[v].reshape(8, -1)
        dcols.append(F.pad(dc, (0, (-dc.shape[1]) % 32), value=float("nan")))
    loss.backward()
    dx = tokenize_dx_reference(dcols, tub, b, t, h, w)
    assert bool(torch.isfinite(dx).all())                                 # the NaN pad columns are not read
    assert rel_err(dx, x.grad) < TIGHT
    only2 = tokenize_dx_reference([torch.zeros_like(dcols[0]), dcols[1], torch.zeros_like(dcols[2])], tub, b, t, h, w)
    assert float(only2[:, t - 1].abs().max()) == 0.0                      # view 2 (project2, tubelet T-1) never reaches frame T-1
    assert float(only2[:, :t - 1].abs().max()) > 0.0
    dxf = seeded_randn(70, b, 3, h, w)
    with_f = tokenize_dx_reference(dcols, tub, b, t, h, w, dxf=dxf, frame=1)
    assert torch.equal(with_f[:, 1], dx[:, 1] + dxf) and torch.equal(with_f[:, 0], dx[:, 0]) and torch.equal(with_f[:, 2:], dx[:, 2:])


def test_pgd_bounds_values():
    from mumpy_hip.inputgrad import pgd_bounds
    from mumpy_hip.ops import EVAL_MEAN, EVAL_STD
    eps3, lo3, hi3 = pgd_bounds(4 / 255)
    m, s = np.asarray(EVAL_MEAN, np.float32), np.asarray(EVAL_STD, np.float32)
    assert np.array_equal(np.asarray(eps3, np.float32), np.float32(4 / 255) / s)
    assert np.array_equal(np.asarray(lo3, np.float32), (np.float32(0) - m) / s)
    assert np.array_equal(np.asarray(hi3, np.float32), (np.float32(1) - m) / s)
    assert all(isinstance(v, float) for a in (eps3, lo3, hi3) for v in a) and len(eps3) == len(lo3) == len(hi3) == 3
    assert all(l < 0 < h for l, h in zip(lo3, hi3))
    assert pgd_bounds(0.0)[0] == (0.0, 0.0, 0.0)
    assert pgd_bounds(0.5, mean=(0.5, 0.5, 0.5), std=(0.25, 0.5, 1.0)) == ((2.0, 1.0, 0.5), (-2.0, -1.0, -0.5), (2.0, 1.0, 0.5))
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            pgd_bounds(bad)
    with pytest.raises(ValueError):
        pgd_bounds(0.1, std=(0.2, 0.0, 0.2))


# ------------------------------------------------------------------------------------------------ the tape's argument
def test_encoder_train_refuses_a_clip_that_requires_grad_without_input_grad():
    from mumpy_hip import autograd
    x = torch.zeros(1, 3, 3, 224, 224, requires_grad=True)
    with pytest.raises(RuntimeError, match="input_grad=True"):
        autograd.encoder_train(None, x)
    with pytest.raises(RuntimeError, match="input_grad=True"):
        autograd.encoder_train(None, x, coupling="clip")
    for bad in (x.detach(), x.detach().double().requires_grad_(), None):   # input_grad=True needs a float32 clip that requires grad
        with pytest.raises(RuntimeError, match="requires_grad"):
            autograd.encoder_train(None, bad, input_grad=True)


def test_encoder_train_old_refusals_are_unchanged():
    from mumpy_hip import autograd, ops
    x = torch.zeros(1, 3, 3, 224, 224, requires_grad=True)
    for bad in ("bogus", "", 1, "CLIP", True):
        with pytest.raises(ValueError, match="coupling"):                  # ... ahead of the new checks
            autograd.encoder_train(None, x, coupling=bad)
        with pytest.raises(ValueError, match="coupling"):
            autograd.encoder_train(None, None, coupling=bad)
    before = ops.clip_coupling()
    with ops.clip_coupling_as("clip"):
        with pytest.raises(RuntimeError, match="per-clip"):
            autograd.encoder_train(None, None)
        with pytest.raises(RuntimeError, match="per-clip"):
            autograd.encoder_train(None, x, input_grad=True)
    assert ops.clip_coupling() == before
