"""The launch forms of the fp32 attention cores (csrc/window_attention.hip, csrc/deform_attention.hip): a small grid runs each
(window, head) unit on two waves, one per 32-query tile ("split"); a large one runs the persistent / one-wave-per-unit form.  Which
form a launch takes is a pure host function of the shape (mumpy_window_attention_plan / mumpy_deform_attention_plan: bit 0 = split,
bit 1 = K/V ring, which no launch takes), and every form computes bitwise the same output.

CPU: the plan functions.  GPU: the same windows through both forms are torch.equal, and each form agrees with the oracle and with
the one-hot construction of test_hip_parity.test_window_indexing_bit_exact."""
import pytest
import torch

from conftest import rel_err
from weight_fill import seeded_randn

gpu = pytest.mark.gpu
TIGHT = 5e-5        # the single-operator bar of tests/test_hip_parity.py (fp32 MFMA = exact fma chain)
SCALE = 32 ** -0.5

# (B, Hs, W, C) of the eight self-attention launches and (B, H, W, C) of the four cross-view launches (each with r = 1 and r = 5)
# of the B=8, T=5 forward, with the plan the file headers document
SELF_FORWARD = {(8, 280, 56, 128): 0, (8, 140, 28, 256): 0, (8, 70, 14, 512): 1, (8, 35, 7, 1024): 1,
                (8, 56, 56, 96): 1, (8, 28, 28, 192): 1, (8, 14, 14, 384): 1, (8, 7, 7, 768): 1}
CROSS_FORWARD = {(8, 56, 56, 96): 0, (8, 28, 28, 192): 1, (8, 14, 14, 384): 1, (8, 7, 7, 768): 1}


def _lib():
    from mumpy_hip.lib import load_library
    return load_library()


# ------------------------------------------------------------------ CPU: the planners
def test_plans_of_the_forward_are_the_documented_ones():
    lib = _lib()
    for shape, plan in SELF_FORWARD.items():
        assert lib.mumpy_window_attention_plan(*shape) == plan, shape
    for shape, plan in CROSS_FORWARD.items():
        for r in (1, 5):
            assert lib.mumpy_deform_attention_plan(*shape, r) == plan, (shape, r)


@pytest.mark.parametrize("hs,w,c", [(7, 7, 32), (7, 7, 768), (14, 14, 384), (28, 28, 192), (35, 7, 96), (56, 56, 96), (280, 56, 128)])
def test_plans_are_monotone_in_the_unit_count(hs, w, c):
    """Growing the batch only ever moves a launch from the split form to the persistent one, never back, and bit 1 is never set."""
    lib = _lib()
    per_image = (hs // 7) * (w // 7) * (c // 32)
    batches = sorted({b for u in (1, 100, 500, 768, 769, 1000, 1024, 1025, 1536, 2000, 2560, 2561, 3072, 3073, 5000, 20000)
                      for b in (u // per_image, u // per_image + 1) if b >= 1})
    for plan in (lib.mumpy_window_attention_plan, lambda *s: lib.mumpy_deform_attention_plan(*s, 3)):
        seen = [plan(b, hs, w, c) for b in batches]
        assert all(p in (0, 1) for p in seen), seen
        assert seen == sorted(seen, reverse=True), (batches, seen)
    assert lib.mumpy_window_attention_plan(1, 7, 7, 32) == 1 and lib.mumpy_deform_attention_plan(1, 7, 7, 32, 1) == 1
    assert lib.mumpy_window_attention_plan(64, 56, 56, 128) == 0 and lib.mumpy_deform_attention_plan(64, 56, 56, 128, 1) == 0


def test_bf16_storage_entry_points_take_neither_form():
    lib = _lib()
    for shape in list(SELF_FORWARD) + [(1, 7, 7, 32), (1, 14, 14, 64)]:
        assert lib.mumpy_window_attention_bf16_plan(*shape) == 0, shape


def test_plans_reject_what_the_entry_points_reject():
    lib = _lib()
    assert lib.mumpy_window_attention_plan(1, 10, 14, 96) == -1 and b"window_attention_plan" in lib.mumpy_last_error()
    assert lib.mumpy_window_attention_plan(1, 14, 14, 100) == -1
    assert lib.mumpy_deform_attention_plan(1, 14, 14, 96, 0) == -1 and b"deform_attention_plan" in lib.mumpy_last_error()


# ------------------------------------------------------------------ GPU: self-attention
def _self_inputs(seed, b, hs, w, c, shift):
    from models.modules.swinTransformer import relative_position_index
    from oracle import mumpy_oracle as O
    qkv = seeded_randn(seed, b, hs * w, 3 * c)
    table = seeded_randn(seed + 1, 169, c // 32) * 0.2
    idx = relative_position_index(7, 7)
    mask = O.shift_attn_mask(hs, w, shift) if shift else None
    return qkv, table, idx, mask


def _self_run(qkv, table, idx, mask, b, hs, w, c, shift):
    from mumpy_hip import ops
    dev = torch.device("cuda:0")
    bias = ops.expand_relpos_bias(table.to(dev), idx.to(dev))
    tab, ids = ops.compact_attn_mask(mask.to(dev)) if mask is not None else (None, None)
    return ops.window_attention(qkv.to(dev), bias, b, hs, w, c, shift, SCALE, tab, ids)


def _batch_that_flips(plan, b, limit=4096):
    """The smallest multiple of the batch whose plan differs from the batch's own."""
    small = plan(b)
    for k in range(2, limit):
        if plan(b * k) != small:
            return k
    raise AssertionError("the plan never flips")


@gpu
@pytest.mark.parametrize("hs,w,c,shift,b", [(7, 7, 32, 0, 1), (7, 21, 96, 0, 1), (14, 14, 64, 3, 1), (35, 7, 96, 0, 2)])
def test_self_split_and_whole_forms_agree_bitwise(hs, w, c, shift, b):
    """A single unit; 3 windows (the last block of the split form is half empty); masked and unmasked windows in one launch; frames
    stacked on rows.  The same images once in a launch the planner splits and once at the head of a batch it does not."""
    from oracle import mumpy_oracle as O
    lib = _lib()
    plan = lambda bb: lib.mumpy_window_attention_plan(bb, hs, w, c)
    k = _batch_that_flips(plan, b)
    assert plan(b) & 1 and not plan(b * k) & 1
    qkv, table, idx, mask = _self_inputs(900 + hs + w + c, b, hs, w, c, shift)
    small = _self_run(qkv, table, idx, mask, b, hs, w, c, shift)
    big_in = torch.cat([qkv, seeded_randn(7, b * (k - 1), hs * w, 3 * c)])
    big = _self_run(big_in, table, idx, mask, b * k, hs, w, c, shift)
    assert torch.equal(small, big[:b])
    assert not torch.isnan(big).any()
    ref = O.window_attention_core(qkv.double(), table.double(), idx, hs, w, shift, None if mask is None else mask.double())
    err = rel_err(small.cpu(), ref)
    print(f"split self ({b}, {hs}, {w}, {c}) shift {shift}: rel err vs oracle {err:.2e}; whole form at batch {b * k}")
    assert err < TIGHT


@gpu
@pytest.mark.parametrize("b,hs,w,c,shift", [(13, 28, 28, 512, 0), (13, 28, 28, 512, 3), (13, 35, 21, 512, 3)])
def test_self_persistent_walk_of_several_units(b, hs, w, c, shift):
    """More than 3,072 units, so waves of the persistent form walk several units, some an odd number of them; (35, 21) leaves 195
    windows, a partial last quad.  Against the oracle, and image by image against the split form."""
    from oracle import mumpy_oracle as O
    lib = _lib()
    assert b * (hs // 7) * (w // 7) * (c // 32) > 3072
    assert not lib.mumpy_window_attention_plan(b, hs, w, c) & 1 and lib.mumpy_window_attention_plan(1, hs, w, c) & 1
    qkv, table, idx, mask = _self_inputs(950 + hs + shift, b, hs, w, c, shift)
    big = _self_run(qkv, table, idx, mask, b, hs, w, c, shift)
    ref = O.window_attention_core(qkv, table, idx, hs, w, shift, mask)          # fp32 oracle: the bar is far above its own error
    err = rel_err(big.cpu(), ref)
    print(f"persistent self ({b}, {hs}, {w}, {c}) shift {shift}: rel err vs oracle {err:.2e}")
    assert err < TIGHT
    for i in (0, b // 2, b - 1):
        assert torch.equal(big[i:i + 1], _self_run(qkv[i:i + 1], table, idx, mask, 1, hs, w, c, shift)), i


@gpu
@pytest.mark.parametrize("b,hs,w,shift", [(1, 14, 14, 3), (1, 7, 21, 0), (13, 28, 28, 3), (13, 35, 21, 0)])
def test_window_indexing_is_bit_exact_in_both_forms(b, hs, w, shift):
    """The one-hot 'attention' of test_hip_parity.test_window_indexing_bit_exact (bias 0 on (i, (i+1) % 49), -1e30 elsewhere) makes
    the kernel copy V rows exactly: pins gather, roll and scatter of the split form (B = 1) and of the persistent walk (B = 13)."""
    from mumpy_hip import ops
    from oracle import mumpy_oracle as O
    dev = torch.device("cuda:0")
    c = 512 if b > 1 else 64
    nh, l = c // 32, hs * w
    assert bool(_lib().mumpy_window_attention_plan(b, hs, w, c) & 1) == (b == 1)
    qkv = torch.zeros(b, l, 3 * c)
    v = torch.arange(b * l * c, dtype=torch.float32).reshape(b, l, c) % 4093     # exactly representable
    qkv[:, :, 2 * c:] = v
    bias = torch.full((nh, 64, 64), -1e30)
    for i in range(49):
        bias[:, i, (i + 1) % 49] = 0.0
    bias[:, 49:, :] = 0.0
    bias[:, :, 49:] = -1e30
    out = ops.window_attention(qkv.to(dev), bias.to(dev), b, hs, w, c, shift, SCALE).cpu()
    idxw = O.window_token_index(hs, w, shift).view(-1, 49)
    expect = torch.empty_like(v)
    expect[:, idxw.reshape(-1)] = v[:, torch.roll(idxw, -1, dims=1).reshape(-1)]
    assert torch.equal(out, expect)


# ------------------------------------------------------------------ GPU: cross-view attention
def _cross_reference(q, kv, b, h, w, c, r):
    """softmax(q k^T * scale) v per (kv window, head) in fp64, q window = kv window mod B1, summed over adjacent r-tuples."""
    from oracle import mumpy_oracle as O
    b1w, nh = b * (h // 7) * (w // 7), c // 32
    qw = q.double()[:, O.window_token_index(h, w, 0)].reshape(b1w, 49, c)
    sel = torch.arange(b1w * r) % b1w
    qh = qw[sel].reshape(b1w * r, 49, nh, 32).transpose(1, 2)
    k = kv.double()[..., :c].reshape(b1w * r, 49, nh, 32).transpose(1, 2)
    v = kv.double()[..., c:].reshape(b1w * r, 49, nh, 32).transpose(1, 2)
    o = ((qh @ k.transpose(-2, -1)) * SCALE).softmax(-1) @ v
    return o.transpose(1, 2).reshape(b1w, r, 49, c).sum(1)


@gpu
@pytest.mark.parametrize("r", [1, 3, 5])
@pytest.mark.parametrize("b,h,w,c", [(1, 7, 7, 32), (1, 21, 7, 96), (2, 14, 14, 192)])
def test_cross_split_and_whole_forms_agree_bitwise(b, h, w, c, r):
    """1, 3 and 8 output windows.  The whole form comes from repeating the q batch k >= r times: q window j of the repeated batch is q
    window j mod B1 of the small one, so with the small launch's kv windows first its first B1 output windows see the same q and kv."""
    from mumpy_hip import ops
    lib = _lib()
    dev = torch.device("cuda:0")
    plan = lambda bb: lib.mumpy_deform_attention_plan(bb, h, w, c, r)
    k = max(_batch_that_flips(plan, b), r)
    assert plan(b) & 1 and not plan(b * k) & 1
    b1w = b * (h // 7) * (w // 7)
    q, kv = seeded_randn(600 + c + r, b, h * w, c), seeded_randn(601 + c + r, b1w * r, 49, 2 * c)
    pad = ops.pad_mask(dev)
    small = ops.deform_attention(q.to(dev), kv.to(dev), pad, b, h, w, c, r, SCALE)
    kv_big = torch.cat([kv, seeded_randn(9, b1w * r * (k - 1), 49, 2 * c)])
    big = ops.deform_attention(q.repeat(k, 1, 1).to(dev), kv_big.to(dev), pad, b * k, h, w, c, r, SCALE)
    assert torch.equal(small, big[:b1w])
    assert not torch.isnan(big).any()
    err = rel_err(small.cpu(), _cross_reference(q, kv, b, h, w, c, r))
    err_big = rel_err(big.cpu(), _cross_reference(q.repeat(k, 1, 1), kv_big, b * k, h, w, c, r))
    print(f"cross ({b}, {h}, {w}, {c}) r {r}: rel err vs fp64 split {err:.2e}, whole (batch {b * k}) {err_big:.2e}")
    assert err < TIGHT and err_big < TIGHT
