"""Derived weights and captured graphs follow weight changes.

Many kernels do not read a parameter: they read a tensor derived from it and cached by models.modules.layers.Derived (bf16 copies,
LayerNorm-folded GEMM operands, the expanded relative-position bias, concatenated k|v weights, transposed tokenizer weights, KRSC
convolution images), and mumpy_hip.graph.GraphedForward bakes the addresses of those tensors into a hipGraph.  A stale one makes the
model compute with a mix of old and new weights, which no kernel test can see.  Three parts:

  1. (CPU) the contract of Derived itself, mutator by mutator, over one source and over several;
  2. (GPU) every derived site of the models, one source tensor of its key at a time, under every mutator;
  3. (GPU) GraphedForward at B = 1, T = 3, per changed parameter and mutator, plus its steady state.

Every mutator moves ONE parameter to the same new value (`Change`): a draw of nn.init.normal_ from a seeded generator at the old
value's mean and 1.25 x its spread, so that the nn.init mutator lands on it too.  torch.optim.SGD (lr = 1, grad = old - new) lands
within one rounding of it, fl(old - fl(old - new)): five orders below the tightest bar here, so the oracle of the new value serves
that case as well, while the bitwise comparison always uses a fresh module holding the weights the mutated module actually has.
"""
import collections
import contextlib
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN, rel_err, rms_err
from weight_fill import fill_module_, seeded_randn

gpu = pytest.mark.gpu
TOL = 1e-3          # the whole-model bar (tests/test_hip_parity.py)
TIGHT = 5e-5        # the single-operator fp32 bar (tests/test_hip_parity.py)
BF16 = 2e-2         # the project's bar for bf16 operands against the fp32/fp64 oracle (test_full_model_bf16_storage_b8_t5); bf16 rounds
#                     to 2^-9 = 2e-3 per operand, and a stale matrix (every element redrawn) is wrong by the order of the output itself

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")


# ====================================================================================================== the change and the mutators
class Change:
    """The new value of one parameter (see the module docstring)."""

    def __init__(self, p: torch.Tensor, seed: int):
        self.seed, self.mean, self.std = seed, float(p.detach().mean()), 1.25 * max(float(p.detach().std()), 0.02)
        self.value = self.draw_(torch.empty_like(p.detach()))

    def draw_(self, t):
        return nn.init.normal_(t, self.mean, self.std, generator=torch.Generator(device=t.device).manual_seed(self.seed))


def _split(root: nn.Module, dotted: str):
    """-> (the submodule that owns the parameter, its leaf name)."""
    path, _, leaf = dotted.rpartition(".")
    return (root.get_submodule(path) if path else root), leaf


def _bump():
    from mumpy_hip.state import bump_weights_epoch
    bump_weights_epoch()


# each mutator: (root module, dotted parameter name, Change) -> the module that now holds the new weights
def mut_load_state_dict(root, name, ch):
    """load_state_dict on the OWNING SUBMODULE (a root-level load goes through the same per-module copy)."""
    sub, leaf = _split(root, name)
    sub.load_state_dict({leaf: ch.value.clone()}, strict=False)
    return root


def mut_sgd_step(root, name, ch):
    p = root.get_parameter(name)
    p.grad = p.detach() - ch.value
    torch.optim.SGD([p], lr=1.0).step()
    p.grad = None
    return root


def mut_no_grad_inplace(root, name, ch):
    with torch.no_grad():
        root.get_parameter(name).mul_(0.0).add_(ch.value)
    return root


def mut_nn_init(root, name, ch):
    ch.draw_(root.get_parameter(name))
    return root


def mut_data_assign(root, name, ch):
    root.get_parameter(name).data = ch.value.clone()
    return root


def mut_to_round_trip(root, name, ch):
    """Away and back (GPU module: through the host; CPU module: through float64), edited while away."""
    p = root.get_parameter(name)
    if p.is_cuda:
        dev = p.device
        root.cpu()
        with torch.no_grad():
            root.get_parameter(name).copy_(ch.value)
        return root.to(dev)
    root.double()
    with torch.no_grad():
        root.get_parameter(name).copy_(ch.value)
    return root.float()


def mut_deepcopy(root, name, ch):
    """The copy's weights change; the copy must not serve what the original cached."""
    twin = copy.deepcopy(root)
    with torch.no_grad():
        twin.get_parameter(name).copy_(ch.value)
    return twin


def mut_data_inplace_then_bump(root, name, ch):
    """`.data` has a version counter of its own: torch cannot see this edit, so the documented call follows it."""
    root.get_parameter(name).data.copy_(ch.value)
    _bump()
    return root


# (id, mutator, freeze every parameter of the module before its first use)
MUTATORS = [("load_state_dict", mut_load_state_dict, False),
            ("sgd_step", mut_sgd_step, False),
            ("no_grad_inplace", mut_no_grad_inplace, False),
            ("nn_init", mut_nn_init, False),
            ("data_assign", mut_data_assign, False),
            ("to_round_trip", mut_to_round_trip, False),
            ("deepcopy", mut_deepcopy, False),
            ("data_inplace_bump", mut_data_inplace_then_bump, False),
            ("data_inplace_bump_frozen", mut_data_inplace_then_bump, True)]
MUT = {m[0]: m for m in MUTATORS}
mutators = pytest.mark.parametrize("mutator", [m[0] for m in MUTATORS])


# ====================================================================================================== 1. the Derived contract (CPU)
class _Owner(nn.Module):
    """The smallest module with the models' caching idiom: a Derived over one source (the tokenizers' transposed weight), one over
    four (the LayerNorm fold's key) and one over a buffer alone (attn_mask).  `calls` counts how often each fn ran."""

    def __init__(self):
        from models.modules.layers import Derived
        super().__init__()
        self.lin, self.norm = nn.Linear(8, 6), nn.LayerNorm(8)
        self.register_buffer("mask", torch.arange(12.0).reshape(3, 4))
        self._wt, self._fold, self._mask = Derived(), Derived(), Derived()
        self.calls = collections.Counter()

    def wt_now(self):
        return self.lin.weight.detach().t().contiguous()

    def fold_now(self):
        w, b, g, beta = (t.detach().double() for t in (self.lin.weight, self.lin.bias, self.norm.weight, self.norm.bias))
        return torch.cat([(w * g).flatten(), w @ beta + b]).float()

    def _counted(self, tag, fn):
        def run():
            self.calls[tag] += 1
            return fn()
        return run

    def wt(self):
        return self._wt.get((self.lin.weight,), self._counted("wt", self.wt_now))

    def fold(self):
        return self._fold.get((self.lin.weight, self.lin.bias, self.norm.weight, self.norm.bias), self._counted("fold", self.fold_now))

    def packed_mask(self):
        return self._mask.get((self.mask,), self._counted("mask", lambda: self.mask * 2))


def _owner(frozen=False):
    o = fill_module_(_Owner(), "owner/")
    return o.requires_grad_(False) if frozen else o


FOLD_SOURCES = ["lin.weight", "lin.bias", "norm.weight", "norm.bias"]


@mutators
@pytest.mark.parametrize("source", FOLD_SOURCES)
def test_derived_is_rebuilt_after_every_kind_of_weight_change(mutator, source):
    """Each mutator on each source of a four-source key and on the source of a one-source key: the cached value is rebuilt and
    equals a recomputation from the current sources; a key that does not list the changed source keeps its value and is not
    recomputed.  (Before this file's fix, data_inplace_bump_frozen served the stale value: the epoch entered a key only for sources
    with requires_grad.)"""
    _, fn, frozen = MUT[mutator]
    o = _owner(frozen)
    wt0, fold0 = o.wt().clone(), o.fold().clone()
    assert torch.equal(wt0, o.wt_now()) and torch.equal(fold0, o.fold_now()) and o.calls == {"wt": 1, "fold": 1}
    m = fn(o, source, Change(o.get_parameter(source), 11))
    fold1, wt1 = m.fold(), m.wt()
    assert torch.equal(fold1, m.fold_now()) and not torch.equal(fold1, fold0)
    assert torch.equal(wt1, m.wt_now())
    assert not torch.equal(wt1, wt0) if source == "lin.weight" else torch.equal(wt1, wt0)
    assert fold1.dtype == torch.float32 and wt1.dtype == torch.float32
    if m is not o:                                                   # deepcopy: the original is untouched and still cached
        assert torch.equal(o.fold(), fold0) and torch.equal(o.wt(), wt0) and o.calls == {"wt": 1, "fold": 1}
        assert m._fold is not o._fold and m._wt is not o._wt
    m.fold(), m.wt()                                                 # and once rebuilt it is cached again
    assert m.calls["fold"] == 2
    if mutator in ("load_state_dict", "sgd_step", "no_grad_inplace", "nn_init") and source != "lin.weight":
        assert m.calls["wt"] == 1        # torch-visible change of ANOTHER tensor: the one-source cache did not even recompute


def test_derived_does_not_call_fn_again_when_nothing_changed():
    o = _owner()
    a, b, c = o.wt(), o.fold(), o.packed_mask()
    for _ in range(3):
        assert o.wt() is a and o.fold() is b and o.packed_mask() is c
    assert o.calls == {"wt": 1, "fold": 1, "mask": 1}
    assert o._wt.current() and o._fold.current() and o._mask.current()


@pytest.mark.parametrize("frozen", [False, True])
def test_buffer_only_keys_ignore_the_weights_epoch(frozen):
    """attn_mask / relative_position_index keys: no optimizer writes a buffer, and rebuilding the compacted mask synchronises with
    the host (ops.compact_attn_mask), which a captured training step must not do.  Parameter keys in the same module do follow."""
    o = _owner(frozen)
    o.packed_mask(), o.wt()
    _bump()
    assert o._mask.current() and not o._wt.current()
    o.packed_mask(), o.wt()
    assert o.calls == {"mask": 1, "wt": 2}
    with torch.no_grad():
        o.mask.add_(1.0)                                             # a buffer that IS written in place is still followed
    assert torch.equal(o.packed_mask(), o.mask * 2) and o.calls["mask"] == 2


def test_current_reports_every_followed_change_without_calling_fn():
    """Derived.current(): what GraphedForward asks before a replay."""
    for mutator, fn, frozen in MUTATORS:
        if mutator == "deepcopy":
            continue
        o = _owner(frozen)
        o.fold()
        assert o._fold.current()
        fn(o, "norm.bias", Change(o.norm.bias, 12))
        assert not o._fold.current(), mutator
        assert o.calls == {"fold": 1}, mutator
    from models.modules.layers import Derived
    assert not Derived().current()                                   # never built: nothing to replay against


def test_a_replaced_storage_cannot_come_back_at_the_same_address():
    """`p.data = new` twice with no use in between: the allocator may hand the second tensor the address the cache was keyed on,
    with the version unchanged.  The cache holds an alias of what it was built from, so that address stays taken."""
    for size in (6, 4096, 1 << 16):
        o = _owner()
        o.lin = nn.Linear(size, 6)
        o.wt()
        ptr0 = o.lin.weight.data_ptr()
        for k in range(4):
            o.lin.weight.data = torch.full_like(o.lin.weight.data, float(k))
            assert o.lin.weight.data_ptr() != ptr0
        assert torch.equal(o.wt(), o.wt_now()) and float(o.wt()[0, 0]) == 3.0


def test_a_copied_or_pickled_module_starts_with_empty_caches(tmp_path):
    o = _owner()
    o.wt(), o.fold()
    twin = copy.deepcopy(o)
    assert twin._wt._val is None and twin._fold._key is None and twin._wt is not o._wt
    torch.save(o, tmp_path / "m.pt")
    back = torch.load(tmp_path / "m.pt", weights_only=False)
    assert back._wt._val is None and torch.equal(back.wt(), o.wt())


def test_derived_seen_lists_every_cache_consulted_while_it_is_set():
    """The bookkeeping GraphedForward._capture relies on, without a GPU: while mumpy_hip.state.derived_seen holds a list, every
    Derived consulted is appended to it; outside, nothing is recorded."""
    from mumpy_hip import state
    o = _owner()
    o.wt()
    assert state.derived_seen[0] is None
    state.derived_seen[0] = []
    try:
        o.wt(), o.fold(), o.wt()
        seen = state.derived_seen[0]
    finally:
        state.derived_seen[0] = None
    assert [d is o._wt for d in seen] == [True, False, True] and seen[1] is o._fold
    o.packed_mask()
    assert len(seen) == 3


# ====================================================================================================== 2. every derived site (GPU)
@contextlib.contextmanager
def _storage_bf16():
    from mumpy_hip import ops
    try:
        ops.set_storage("bf16")
        yield
    finally:
        ops.set_storage("fp32")


@contextlib.contextmanager
def _cva_bf16():
    from mumpy_hip import ops
    was = ops.cva_math()
    try:
        ops.set_cva_math("bf16")
        yield
    finally:
        ops.set_cva_math(was)


@contextlib.contextmanager
def _cva_unfused():
    from models.modules import deformableAttention as da
    was = dict(da.FUSED)
    try:
        da.FUSED["sample_kv"] = False
        yield
    finally:
        da.FUSED.update(was)


def _golden(name):
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "full_model.npz"))[name])


class Site:
    """One derived site: how to build the module, what to feed it, its float64 reference, the sources of its cache keys that are
    parameters, the bar of its existing parity test, the C-ABI entries that prove the derived path ran, and the mode it runs in."""

    def __init__(self, build, inputs, oracle, sources, tol, ran, mode=contextlib.nullcontext, call=None):
        self.build, self.inputs, self.oracle, self.sources = build, inputs, oracle, sources
        self.tol, self.ran, self.mode, self.call = tol, set(ran), mode, call or (lambda m, *xs: m(*xs))


def _sd64(m, prefix=""):
    return {prefix + k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}


def _swin_block_96():
    from models.modules.swinTransformer import SwinTransformerBlock
    return SwinTransformerBlock(96, (14, 14), 3, shift_size=3)


def _swin_blocks_512():
    from models.modules.swinTransformer import SwinTransformerBlock
    return nn.Sequential(*[SwinTransformerBlock(512, (14, 14), 16, window_size=7, shift_size=s, temporal_dim=5) for s in (0, 3)])


def _global_blocks():
    from models.modules.blocks import Block
    return nn.Sequential(Block(768, 12, 3072, 0.0, 0.0), Block(768, 12, 3072, 0.0, 0.0))


GLOBAL_ROWS = (599, 3)     # S x T = 1797 rows: ops.linear_ln_tiles(m, 2304, 768) and (m, 768, 3072) admit m >= 1793 (asserted below)


def _sda():
    from models.modules.deformableAttention import SwinDAttention
    return SwinDAttention(96, 3, 0.0, n_groups=3)


def _tok3():
    from models.encoder.multiTemporalViewEncoder import CrossThreeViewTokenize
    from models.factory.modelFactory import multiswin_view_configs
    return CrossThreeViewTokenize(multiswin_view_configs(3))


def _tok_base():
    from models.factory.modelFactory import RESOLUTIONS, create_view_config
    from models.modules.swinTransformer import BaselineTokenize
    return BaselineTokenize(create_view_config([128, 256, 512, 1024], (4, 4, 3), [2, 2, 18, 2], [4, 8, 16, 32], 3072, 3, RESOLUTIONS, 3))


def _decoder():
    from models.decoder.decoder import Decoder
    return Decoder()


def _baseline_decoder():
    from models.decoder.decoder import BaselineDecoder
    return BaselineDecoder(in_channels=1024)


def _o():
    from oracle import mumpy_oracle as O
    return O


def _oracle_swin_512(sd, x):
    y = _o().swin_block(x, sd, "0", 70, 14, 0)
    return _o().swin_block(y, sd, "1", 70, 14, 3)


def _oracle_tok_base(sd, x):
    """BaselineTokenize in plain float64 torch: Conv3d(k = s = (3,4,4)) squeezing T, tokens row-major, LayerNorm (swin:11-32)."""
    y = F.conv3d(x.permute(0, 2, 1, 3, 4), sd["proj.weight"], sd["proj.bias"], stride=(3, 4, 4))
    y = y.squeeze(2).flatten(2).transpose(1, 2)
    return F.layer_norm(y, y.shape[-1:], sd["norm.weight"], sd["norm.bias"], 1e-5)


@functools.lru_cache(maxsize=None)
def _encoder_outputs():
    """(final tokens, per-stage view tokens, frequency input) of the filled Encoder at B = 1, T = 3 on CPU: what feeds the Decoder
    in the whole-model tests.  One encoder forward for the whole file."""
    from models.encoder.encoder import Encoder
    enc = fill_module_(Encoder()).eval().to(DEV)
    with torch.no_grad():
        fx, vx, dx = enc(seeded_randn(4321, 1, 3, 3, 224, 224).to(DEV))
    return fx.cpu(), [[v.cpu() for v in stage] for stage in vx], dx.cpu()


def _to(x, f):
    return [_to(v, f) for v in x] if isinstance(x, (list, tuple)) else f(x)


LNX = "mumpy_linear_lnx_fwd"
SDA_SOURCES = ["proj_k.weight", "proj_v.weight", "proj_k.bias", "proj_v.bias"]
SITES = {
    # swinTransformer.py: expanded relative-position bias (the compacted shift mask rides along: its key is a buffer)
    "relpos_bias": Site(_swin_block_96, lambda: (seeded_randn(301, 1, 196, 96),),
                        lambda sd, x: _o().swin_block(x, sd, "", 14, 14, 3), ["attn.relative_position_bias_table"], TIGHT,
                        {"mumpy_window_attention_fwd"}),
    # swinTransformer.py::_w16: bf16 copies of qkv / proj / fc1 / fc2
    "w16": Site(_swin_block_96, lambda: (seeded_randn(301, 1, 196, 96),), lambda sd, x: _o().swin_block(x, sd, "", 14, 14, 3),
                ["attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"], BF16, {"mumpy_linear_bf16s_fwd"},
                mode=_storage_bf16),
    # swinTransformer.py: LayerNorm folds of Mlp.forward_ln (block 0) and WindowAttention.attend_ln (block 1)
    "ln_fold_swin": Site(_swin_blocks_512, lambda: (seeded_randn(77, 8, 980, 512),), _oracle_swin_512,
                         ["0.mlp.fc1.weight", "0.mlp.fc1.bias", "0.norm2.weight", "0.norm2.bias",
                          "1.attn.qkv.weight", "1.attn.qkv.bias", "1.norm1.weight", "1.norm1.bias"], TIGHT, {LNX}),
    # blocks.py: LayerNorm fold of the second global block's qkv GEMM
    "ln_fold_global": Site(_global_blocks, lambda: (seeded_randn(78, *GLOBAL_ROWS, 768),),
                           lambda sd, x: _o().global_block(_o().global_block(x, sd, "0", 12), sd, "1", 12),
                           ["1.attn.qkv.weight", "1.attn.qkv.bias", "1.norm1.weight", "1.norm1.bias"], TIGHT, {LNX}),
    # deformableAttention.py: concatenated k|v weight and bias, on the module's three routes
    "sda_fused": Site(_sda, lambda: (seeded_randn(302, 2, 49, 96), seeded_randn(303, 6, 49, 96)),
                      lambda sd, a, b: _o().swin_dattention(a, b, sd, ""), SDA_SOURCES, TIGHT, {"mumpy_deform_sample_kv_fwd"},
                      call=lambda m, a, b: m(a, b)[0]),
    "sda_bf16": Site(_sda, lambda: (seeded_randn(302, 2, 49, 96), seeded_randn(303, 6, 49, 96)),
                     lambda sd, a, b: _o().swin_dattention(a, b, sd, ""), SDA_SOURCES, BF16, {"mumpy_deform_sample_kv_mm16_fwd"},
                     mode=_cva_bf16, call=lambda m, a, b: m(a, b)[0]),
    "sda_unfused": Site(_sda, lambda: (seeded_randn(302, 2, 49, 96), seeded_randn(303, 6, 49, 96)),
                        lambda sd, a, b: _o().swin_dattention(a, b, sd, ""), SDA_SOURCES, TIGHT,
                        {"mumpy_deform_sample_fwd"}, mode=_cva_unfused, call=lambda m, a, b: m(a, b)[0]),
    # transposed tokenizer weights
    "tokenize3": Site(_tok3, lambda: (seeded_randn(304, 1, 3, 3, 224, 224),),
                      lambda sd, x: _o().tokenize(x, sd, _o().MumpyConfig(frames=3), ""),
                      ["project1.weight", "project2.weight", "project3.weight"], TIGHT, {"mumpy_patch_embed_fwd"}),
    "tokenize_baseline": Site(_tok_base, lambda: (seeded_randn(305, 1, 3, 3, 224, 224),), _oracle_tok_base, ["proj.weight"], TIGHT,
                              {"mumpy_patch_embed_fwd"}),
    # decoder.py: a KRSC convolution image, the per-view head-weight sums / time-slice images of one temporal head, the final conv
    "decoder": Site(_decoder, _encoder_outputs, lambda sd, fx, vx, dx: _o().decoder_forward(sd, fx, vx, dx, [1, 1, 3])[0],
                    ["gcm1.conv_l1.weight", "rgb_decoder_1.0.weight", "final_out.weight"], TOL,
                    {"mumpy_conv2d_nhwc_fwd", "mumpy_final_conv_fwd"}, call=lambda m, fx, vx, dx: m(fx, vx, dx)[0]),
    "baseline_decoder": Site(_baseline_decoder, lambda: (_golden("base_b1t3/y"),), lambda sd, x: _o().baseline_decoder_forward(sd, x),
                             ["decoder_1.0.weight", "final_out.weight"], TOL, {"mumpy_conv2d_nhwc_fwd", "mumpy_final_conv_fwd"}),
}
# (oracle.tokenize / swin_block / swin_dattention build their keys as prefix + "." + name: an empty prefix needs the dot)
_DOTTED = {"relpos_bias", "w16", "sda_fused", "sda_bf16", "sda_unfused", "tokenize3"}
SITE_SOURCES = [(s, src) for s, site in SITES.items() for src in site.sources]


@functools.lru_cache(maxsize=None)
def _pristine(site):
    """The filled module of a site on the CPU, never run: every test deep-copies it (no cache to inherit) instead of rebuilding."""
    return fill_module_(SITES[site].build(), site + "/").eval()


@functools.lru_cache(maxsize=None)
def _inputs(site):
    return tuple(SITES[site].inputs())


@functools.lru_cache(maxsize=None)
def _inputs_gpu(site):
    return tuple(_to(list(_inputs(site)), lambda t: t.to(DEV)))


def _outputs(y):
    return list(y) if isinstance(y, (list, tuple)) else [y]


def _run(site, module):
    """-> (outputs, names of the C-ABI entries launched)."""
    from mumpy_hip import ops
    s = SITES[site]
    was, ops.PROFILE = ops.PROFILE, {}
    try:
        with s.mode(), torch.no_grad():
            y = _outputs(s.call(module, *_inputs_gpu(site)))
        names = {k for k, v in ops.PROFILE.items() if len(v) > 0}
    finally:
        ops.PROFILE = was
    torch.cuda.synchronize()
    return y, names


@functools.lru_cache(maxsize=None)
def _change(site, source):
    """The new value of one source of one site, on the GPU (nn.init draws it with the device's generator)."""
    return Change(_pristine(site).get_parameter(source).to(DEV), 1000 + SITE_SOURCES.index((site, source)))


_FRESH = {}


def _fresh_outputs(site, source, weight):
    """Outputs of a freshly built module that holds `weight` in `source` and has never computed anything else.  Cached per (site,
    source, whether the weight is the Change's value to the bit); the cached entry is checked against the weight it is asked for."""
    exact = torch.equal(weight, _change(site, source).value)
    hit = _FRESH.get((site, source, exact))
    if hit is None:
        m = copy.deepcopy(_pristine(site))
        m.load_state_dict({source: weight.detach().cpu()}, strict=False)
        hit = _FRESH[(site, source, exact)] = (weight.detach().clone(), _run(site, m.to(DEV))[0])
    assert torch.equal(hit[0], weight), "two mutators left different weights where one fresh reference was expected"
    return hit[1]


@functools.lru_cache(maxsize=None)
def _oracle_outputs(site, source):
    """float64 oracle of the site with the Change's value in `source`: one evaluation per (site, source)."""
    m = copy.deepcopy(_pristine(site))
    sd = _sd64(m, "." if site in _DOTTED else "")
    key = ("." if site in _DOTTED else "") + source
    assert key in sd
    sd[key] = _change(site, source).value.cpu().double()
    with torch.no_grad():
        return _outputs(SITES[site].oracle(sd, *_to(list(_inputs(site)), lambda t: t.double())))


@gpu
def test_the_global_block_fold_shape_is_the_smallest_the_planner_admits():
    from mumpy_hip import ops
    m = GLOBAL_ROWS[0] * GLOBAL_ROWS[1]
    admits = lambda rows: ops.linear_ln_tiles(rows, 2304, 768) > 0 and ops.linear_ln_tiles(rows, 768, 3072) > 0      # noqa: E731
    first = next(r for r in range(1, 4096) if admits(r))
    assert admits(m) and first <= m < first + GLOBAL_ROWS[1] + 2, (first, m)


@gpu
@mutators
@pytest.mark.parametrize("site,source", SITE_SOURCES, ids=[f"{s}-{src}" for s, src in SITE_SOURCES])
def test_every_derived_site_follows_every_source(site, source, mutator):
    """One source of one site's cache key, one mutator.  The module has already run with the old weights (its caches are warm); after
    the change its output (a) equals, bit for bit, that of a freshly built module holding the same weights, (b) differs from the
    output before, (c) meets the site's parity bar against the float64 oracle of the new weights, and (d) the launch that reads the
    derived tensor really ran."""
    _, fn, frozen = MUT[mutator]
    s = SITES[site]
    module = copy.deepcopy(_pristine(site)).to(DEV)
    if frozen:
        module.requires_grad_(False)
    before, _ = _run(site, module)
    after_module = fn(module, source, _change(site, source))
    after, names = _run(site, after_module)
    weight = after_module.get_parameter(source).detach()
    fresh = _fresh_outputs(site, source, weight)
    assert s.ran <= names, (s.ran - names)                                                      # (d)
    assert all(torch.equal(a, f) for a, f in zip(after, fresh)) and len(after) == len(fresh)    # (a)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))                            # (b)
    ref = _oracle_outputs(site, source)
    errs = [max(rel_err(a.cpu(), r), rms_err(a.cpu(), r)) for a, r in zip(after, ref)]
    print(f"{site} {source} {mutator}: err vs float64 oracle {max(errs):.3e} (bar {s.tol:g})")
    assert len(ref) == len(after) and max(errs) < s.tol, errs                                   # (c)
    if after_module is not module:                                   # deepcopy: the original still computes with the old weights
        again, _ = _run(site, module)
        assert all(torch.equal(a, b) for a, b in zip(again, before))


# ====================================================================================================== 3. captured graphs (GPU)
GRAPH_PARAMS = {"relpos_table": ("enc", "base.layers.layers.0.blocks.1.block1.attn.relative_position_bias_table"),
                "tokenizer_proj": ("enc", "base.tokenize.project1.weight"),
                "decoder_conv": ("dec", "gcm2.conv_l1.weight"),
                "layernorm_weight": ("enc", "base.layers.layers.2.blocks.3.block3.norm1.weight")}


def mut_flat_sgd_step(root, name, ch):
    """The project's own flat optimizer over this one parameter: a HIP kernel rewrites it (p <- p - lr * grad)."""
    from mumpy_hip.train import FlatSGD
    p = root.get_parameter(name)
    old = p.detach().clone()
    opt = FlatSGD([p], lr=1.0)
    p.grad.copy_(old - ch.value)
    opt.step()
    return root


GRAPH_MUTATORS = {"torch_sgd_step": mut_sgd_step, "no_grad_inplace": mut_no_grad_inplace, "submodule_load_state_dict": mut_load_state_dict,
                  "flat_sgd_step": mut_flat_sgd_step, "data_inplace_bump": mut_data_inplace_then_bump, "data_assign": mut_data_assign}
# frozen: the whole model has requires_grad False, the usual deployment (an optimizer steps trainable parameters only)
GRAPH_CASES = [(m, False) for m in GRAPH_MUTATORS] + [("no_grad_inplace", True), ("data_inplace_bump", True)]


@pytest.fixture(scope="module")
def graph_model():
    """Encoder + Decoder of this file alone (weights are changed here; every test restores the one it touched)."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import streams
    from mumpy_hip.graph import GraphedForward
    enc, dec = fill_module_(Encoder()).eval().to(DEV), fill_module_(Decoder()).eval().to(DEV)
    x = seeded_randn(92, 1, 3, 3, 224, 224).to(DEV)
    # ONE GraphedForward for the file: each owns a capture stream and the fork/join side streams under it, which come from torch's
    # pool of 32 and are never handed back, so one per test would exhaust the pool.  Tests start from g._capture() instead.
    g = GraphedForward(enc, dec, x)
    print(f"graph_model: {len(streams._SIDE)} fork/join side streams in use after the capture")
    return {"enc": enc, "dec": dec, "x": x, "g": g}


def _eager(gm):
    with torch.no_grad():
        out = gm["dec"](*gm["enc"](gm["x"]))[0].clone()
    torch.cuda.synchronize()
    return out


def _restore(p, old, requires_grad):
    """Back to the old value in a storage of its own (a flat optimizer re-points the parameter into its buffer)."""
    p.data = old.clone()
    p.grad = None
    if hasattr(p, "_mumpy_flat_grad"):
        del p._mumpy_flat_grad
    p.requires_grad_(requires_grad)
    _bump()


@gpu
@pytest.mark.parametrize("mutator,frozen", GRAPH_CASES, ids=[m + ("-frozen" if f else "") for m, f in GRAPH_CASES])
@pytest.mark.parametrize("param", list(GRAPH_PARAMS))
def test_graphed_forward_follows_the_weight_change(graph_model, param, mutator, frozen):
    """A GraphedForward captured before one parameter changes: its next call equals, bit for bit, the eager forward of the new
    weights and differs from its output before -- with no call from the user, except the documented one after a `.data` edit.
    frozen: the whole model has requires_grad False."""
    which, name = GRAPH_PARAMS[param]
    root, x, g = graph_model[which], graph_model["x"], graph_model["g"]
    p = root.get_parameter(name)
    old, was_trainable = p.detach().clone(), p.requires_grad
    for m in (graph_model["enc"], graph_model["dec"]):
        m.requires_grad_(not frozen)
    try:
        g._capture()                                                 # whatever the test before left: a capture of the weights as they are
        before = g(x)[0].clone()
        assert torch.equal(before, _eager(graph_model))
        GRAPH_MUTATORS[mutator](root, name, Change(p, 2000 + list(GRAPH_PARAMS).index(param)))
        assert not torch.equal(p.detach(), old)
        after = g(x)[0].clone()
        eager = _eager(graph_model)
        assert torch.equal(after, eager)
        assert not torch.equal(after, before)
        graph = g.graph
        for _ in range(3):                                           # and the new capture is then simply replayed
            assert torch.equal(g(x)[0], eager) and g.graph is graph
    finally:
        _restore(p, old, was_trainable)
        for m in (graph_model["enc"], graph_model["dec"]):
            m.requires_grad_(True)


@gpu
@pytest.mark.parametrize("param", list(GRAPH_PARAMS))
def test_graphed_forward_follows_when_an_eager_call_came_first(graph_model, param):
    """The order validation code uses: change, EAGER forward (which rebuilds the caches, so every cache is current again), then
    the graph.  The graph still points at the tensors built before the change and must notice."""
    which, name = GRAPH_PARAMS[param]
    root, x, g = graph_model[which], graph_model["x"], graph_model["g"]
    p = root.get_parameter(name)
    old, was_trainable = p.detach().clone(), p.requires_grad
    try:
        g._capture()
        before = g(x)[0].clone()
        mut_no_grad_inplace(root, name, Change(p, 2100 + list(GRAPH_PARAMS).index(param)))
        eager = _eager(graph_model)
        after = g(x)[0].clone()
        assert torch.equal(after, eager) and not torch.equal(after, before)
    finally:
        _restore(p, old, was_trainable)


@gpu
def test_graphed_forward_steady_state_replays_one_graph(graph_model):
    """Detection must not turn into a capture per call: with nothing changed, three calls replay the same CUDAGraph object."""
    x, g = graph_model["x"], graph_model["g"]
    g._capture()
    graph, first = g.graph, g(x)[0].clone()
    for _ in range(3):
        assert torch.equal(g(x)[0], first) and g.graph is graph


@gpu
def test_graphed_forward_checks_the_caches_its_warm_up_consulted(graph_model):
    """What the check before a replay looks at: every Derived the forward consults, once each (bias tables, tokenizer weights and
    every decoder cache are among them), and nothing is stale right after a capture."""
    g, enc, dec = graph_model["g"], graph_model["enc"], graph_model["dec"]
    g._capture()
    assert not g._stale()
    listed = [d for d, _ in g._derived]
    assert len(listed) > 100 and len({id(d) for d in listed}) == len(listed)
    assert all(d.current() and d.key == key for d, key in g._derived)
    blk = enc.get_submodule("base.layers.layers.0.blocks.1.block1")
    assert any(d is blk.attn._bias for d in listed)
    assert all(any(d is w for d in listed) for w in enc.base.tokenize._wt)
    assert all(any(d is w for d in listed) for w in dec._derived.values())
