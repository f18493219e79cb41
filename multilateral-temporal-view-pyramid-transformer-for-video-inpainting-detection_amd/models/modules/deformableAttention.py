"""Window-based deformable cross-view attention (SwinDAttention) on the MI355X HIP kernels.

State_dict keys and constructor follow the reference's models/modules/deformableAttention.py:218-309.  Every route starts
with the proj_q GEMM and the offsets kernel (depthwise 5x5 + LN + GELU + 1x1 + tanh) on raster-ordered tokens and then takes
one of three forms, chosen at launch time:
  * fused fp32 (default; fp32 matrix math and storage): sample -> [proj_k|proj_v] as ONE kernel whose A-operand loader is the
    bilinear sampling (mumpy_deform_sample_kv_fwd) -> attention + r-tuple aggregation kernel -> proj_out, which in the cross
    block is ONE kernel with the scrambled reshape and both residual terms (mumpy_deform_out_combine_fwd): 5 launches;
  * unfused (set_matrix_math / set_storage other than fp32, or MUMPY_CVA_FUSED=0): bilinear sampling kernel -> [proj_k|proj_v]
    as one generic GEMM with concatenated weights -> the same fp32 attention kernel -> proj_out generic GEMM -> combine kernel:
    7 launches, the GEMMs in the generic GEMM's operand mode;
  * fused bf16-MFMA (ops.set_cva_math("bf16"), opt-in): the fused route with the _mm16 form of all three kernels -- fp32
    tensors in memory, operands rounded to bf16 on the way to v_mfma_f32_32x32x16_bf16, fp32 accumulation, softmax, bias and
    residual terms.  The switch takes PRECEDENCE: when it is "bf16" these kernels run whatever matrix_math(), storage() and
    MUMPY_CVA_FUSED say; proj_q and the offsets kernel keep following matrix_math().
The reference's index behaviour is specification and is reproduced exactly:
kv window i pairs with q window (i mod B1) (`x1.repeat`, deform:330), the "(b t)" sum adds ADJACENT kv windows
(deform:394-395), and the output is the flat (C,49) image re-read as (49,C) (deform:403).  The (B, r*nH, 49, 49)
attention tensor the reference also returns is discarded by its only caller (mTVE:284) and is not materialised.
Because B1 counts the q windows of every clip of the batch, that rule couples the clips of a batch.  Under
ops.set_clip_coupling("clip") the block entries (attend_combine, attend_raster) apply it inside each clip instead (groups = b
on the grouped kernels, include/mumpy_hip_ext8.h; ops.cva_pairing is the host statement): every clip pairs as a batch of one.
"""
import torch
import torch.nn as nn

from models.modules.layers import Derived
from mumpy_hip import ops


# Round 3: the index work around two of the module's GEMMs rides inside them (csrc/cva_fused.hip).  Switchable per kernel for
# A/B runs (MUMPY_CVA_FUSED=0 / "kv" / "out" / 1); the split-precision and bf16 modes keep the unfused route (their operand
# modes live in the generic GEMM).
import os as _os
_f = _os.environ.get("MUMPY_CVA_FUSED", "1")
FUSED = {"sample_kv": _f in ("1", "kv"), "out_combine": _f in ("1", "out")}


class LayerNormProxy(nn.Module):
    """LayerNorm over channels of a (B,C,H,W) map; inside the HIP offsets kernel this is fused, the module only
    holds the parameters (key `...conv_offset.1.norm.*`)."""

    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):                       # (B,C,H,W), API parity only
        b, c, h, w = x.shape
        y = ops.layernorm(x.permute(0, 2, 3, 1).contiguous(), self.norm.weight, self.norm.bias, self.norm.eps)
        return y.permute(0, 3, 1, 2)


class SwinDAttention(nn.Module):
    def __init__(self, dim1, n_heads, attn_drop, n_groups, ws=7, stride=1, offset_range_factor=2, no_off=False,
                 height_scale=[1, 1], dwc_pe=False, use_pe=False, fixed_pe=False):
        super().__init__()
        if ws != 7 or stride != 1 or offset_range_factor != 2 or no_off or use_pe or dwc_pe or fixed_pe or n_groups != 3:
            raise NotImplementedError("only the configuration the encoder instantiates (mTVE:131) is built: "
                                      "ws=7, n_groups=3, offset_range_factor=2, no positional-encoding branches")
        self.n_heads, self.ws, self.n_groups = n_heads, ws, n_groups
        self.n_head_channels = dim1 // n_heads
        if self.n_head_channels != 32:
            raise NotImplementedError("HIP deformable attention is built for 32-wide heads")
        self.scale = self.n_head_channels ** -0.5
        self.nc = dim1
        self.n_group_channels = cg = dim1 // n_groups
        self.conv_offset = nn.Sequential(
            nn.Conv2d(cg, cg, 5, 1, 2, groups=cg),
            LayerNormProxy(cg),
            nn.GELU(),
            nn.Conv2d(cg, 2, 1, 1, 0, bias=False))
        self.proj_q = nn.Conv2d(dim1, dim1, 1)
        self.proj_k = nn.Conv2d(dim1, dim1, 1)
        self.proj_v = nn.Conv2d(dim1, dim1, 1)
        self.proj_out = nn.Conv2d(dim1, dim1, 1)
        self.proj_drop = nn.Dropout(attn_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.rpe_table = None
        for m in (self.proj_q, self.proj_k, self.proj_v):       # deform:302-309
            nn.init.trunc_normal_(m.weight)
            nn.init.zeros_(m.bias)
        nn.init.zeros_(self.proj_out.weight)
        nn.init.zeros_(self.proj_out.bias)
        self._wkv, self._bkv, self._pad = Derived(), Derived(), Derived()

    def _prep(self, x1, q_grid):
        """The q side, which needs nothing from the other view: q = proj_q(x1) and the sampling positions of the offset
        network (deform:332-349).  The cross block runs this BEFORE it waits for the other view's tokens."""
        b, h, w = q_grid
        q = ops.linear(x1, self.proj_q.weight, self.proj_q.bias)
        off = self.conv_offset
        pos = ops.deform_offsets(q, off[0].weight, off[0].bias, off[1].norm.weight, off[1].norm.bias, off[3].weight,
                                 b, h, w, self.nc)
        return q, pos

    def _run(self, x1, x2, q_grid, kv_grid, prep=None, groups=None):
        """q_grid = (b, h, w): x1 is (b, h*w, C) raster;  kv_grid = (b2, hs2, w2): x2 is (b2, hs2*w2, C) raster.
        Returns proj_out output Yt (nq, 49, C): window-major, token-major, i.e. BEFORE the deform:403 reshape."""
        o = self._attend(x1, x2, q_grid, kv_grid, prep, groups=groups)
        return ops.linear(o, self.proj_out.weight, self.proj_out.bias)

    def _attend(self, x1, x2, q_grid, kv_grid, prep=None, want_maps=False, groups=None):
        """Everything up to (not including) proj_out: -> o (nq,49,C), the attention output summed over the r-tuples.
        want_maps: also return the attention maps (nq, r*nH, 49, 49) the reference hands back (deform:396) -- a visualisation path
        (the fast kernel keeps the probabilities in registers; a small separate kernel recomputes them from q and k).
        groups: the pairing rule (ops.cva_pairing).  None follows ops.clip_coupling(), read here, at launch time: b (every clip of
        the grid pairs as a batch of one) under "clip", 1 (the reference's batch-wide `i mod B1`) under "batch"."""
        c = self.nc
        b, h, w = q_grid
        b2, hs2, w2 = kv_grid
        nq = b * (h // 7) * (w // 7)
        nkv = b2 * (hs2 // 7) * (w2 // 7)
        if nkv % nq:
            raise RuntimeError(f"SwinDAttention: {nkv} kv windows is not a multiple of {nq} q windows")
        if groups is None:
            groups = b if ops.clip_coupling() == "clip" else 1
        if groups > 1 and b2 % groups:
            raise RuntimeError(f"SwinDAttention: groups={groups} does not divide the kv side's batch {b2}")
        q, pos = prep if prep is not None else self._prep(x1, q_grid)
        wkv = self._wkv.get((self.proj_k.weight, self.proj_v.weight),
                            lambda: torch.cat([self.proj_k.weight.reshape(c, c), self.proj_v.weight.reshape(c, c)], 0))
        bkv = self._bkv.get((self.proj_k.bias, self.proj_v.bias), lambda: torch.cat([self.proj_k.bias, self.proj_v.bias]))
        math = ops.cva_math()                                                     # "bf16": the _mm16 kernels, before any other mode
        if math == "bf16" or (FUSED["sample_kv"] and ops.matrix_math() == "fp32" and ops.storage() == "fp32"):
            kv = ops.deform_sample_kv(x2, pos, wkv, bkv, b2, hs2, w2, c, nq, math=math, groups=groups)   # sampling = the projection's A loader
        else:
            sampled = ops.deform_sample(x2, pos, b2, hs2, w2, c, nq, groups=groups)
            kv = ops.linear(sampled, wkv, bkv)                                    # (nkv,49,2C)
        pad = self._pad.get((self.proj_q.weight,), lambda: ops.pad_mask().to(x1.device))
        o = ops.deform_attention(q, kv, pad, b, h, w, c, nkv // nq, self.scale, math=math, groups=groups)      # (nq,49,C)
        if not want_maps:
            return o
        # kv window i pairs with q window i mod nq; q is raster (b, h*w, C): gather its windows first (49 x C each)
        qw = q.view(b, h // 7, 7, w // 7, 7, c).permute(0, 1, 3, 2, 4, 5).reshape(nq, 49, c).contiguous()
        if groups > 1:      # the same rule inside each group: one launch per group on host slices (not a hot path)
            nqg, nkg = nq // groups, nkv // groups
            maps = torch.cat([ops.attention_probs(qw[g * nqg:(g + 1) * nqg], kv[g * nkg:(g + 1) * nkg], nkg, self.n_heads, 49, 49, 32,
                                                  (49 * c, c), (49 * 2 * c, 2 * c), self.scale, q_mod=nqg) for g in range(groups)])
            return o, maps.reshape(nq, (nkv // nq) * self.n_heads, 49, 49)
        maps = ops.attention_probs(qw, kv, nkv, self.n_heads, 49, 49, 32, (49 * c, c), (49 * 2 * c, 2 * c), self.scale, q_mod=nq)
        return o, maps.reshape(nq, (nkv // nq) * self.n_heads, 49, 49)                # '(B nH) n m -> B (r nH) n m' (deform:396)

    def attend_combine(self, x1, x2, b, h, w, hs2, prep=None):
        """The cross block's use of the module (mTVE:283-286): x1 + x1[window order] + the scrambled attention output, i.e.
        CVAModule's `x1w + D` laid out window-major and added to raster x1.  Fused form: proj_out, the un-permuted (C,49)->(49,C)
        reshape and both residual terms are ONE launch (mumpy_deform_out_combine_fwd; under set_cva_math("bf16") its _mm16 form,
        whatever the other modes say)."""
        math = ops.cva_math()
        if math == "bf16" or (FUSED["out_combine"] and ops.matrix_math() == "fp32" and ops.storage() == "fp32"):
            o = self._attend(x1, x2, (b, h, w), (b, hs2, w), prep)
            return ops.deform_out_combine(o, self.proj_out.weight.reshape(self.nc, self.nc), self.proj_out.bias, x1, b, h, w, self.nc,
                                          math=math)
        yt = self._run(x1, x2, (b, h, w), (b, hs2, w), prep)
        return ops.deform_combine(x1, yt, b, h, w, self.nc)

    def attend_raster(self, x1, x2, b, h, w, hs2, prep=None):
        """Fused-block entry: x1 (B, h*w, C) q-side tokens, x2 (B, hs2*w, C) kv-side tokens (already through
        `pre`), both raster with frames stacked on rows.  prep: the result of `_prep(x1, (b, h, w))` if already computed."""
        return self._run(x1, x2, (b, h, w), (b, hs2, w), prep)

    def forward(self, x1, x2, return_attention=False, groups=None):
        """Reference signature (deform:324): x1 (B1,49,C) q windows, x2 (B2,49,C) kv windows, B2 = r*B1.
        Every window is its own 7x7 image for the kernels.  Returns (y (B1,49,C), None).
        groups: window lists carry no clip boundaries, so this entry does NOT follow ops.clip_coupling(): None means 1, the
        reference's pairing over all B1 windows; a caller that knows its clips passes their number (it must divide B1 and B2)."""
        b1, b2, c = x1.shape[0], x2.shape[0], x1.shape[2]
        groups = 1 if groups is None else groups
        if return_attention:      # the reference returns (x, attn) always (deform:405); here the maps cost a launch, so on request
            o, maps = self._attend(x1, x2, (b1, 7, 7), (b2, 7, 7), want_maps=True, groups=groups)
            yt = ops.linear(o, self.proj_out.weight, self.proj_out.bias)
            return yt.transpose(1, 2).reshape(b1, 49, c), maps
        yt = self._run(x1, x2, (b1, 7, 7), (b2, 7, 7), groups=groups)
        return yt.transpose(1, 2).reshape(b1, 49, c), None       # flat (C,49) re-read as (49,C) (deform:403)
