"""CPU only: the host checks of every C-ABI entry point that launches (a `void* stream` parameter), swept without a GPU.

Without a device the sign of an entry point's return code says how far a call got: rc < 0, refused by the host checks (a MUMPY_E*
code); rc > 0, every check passed and the launch reached the runtime, which has no device (hipErrorNoDevice); rc == 0, accepted as an
empty no-op.  So a VALID call -- fake, 16-byte aligned, never dereferenced addresses and a small shape the header allows -- must give
rc > 0, and the same call with one argument made invalid must give rc < 0: the mutation is then the only reason for the refusal.

Per entry of TABLE (the header's comments are the specification):
  * the valid tuple gives rc > 0;
  * each required pointer set to NULL gives rc < 0 with a message of this call's own (the thread's message is sticky, so a known
    message of another entry is left there first; pointers the header calls optional are marked and exempt);
  * each integer that is not a mode or a hyper-parameter set to -1 gives rc < 0; each dimension set to 0 gives rc <= 0 (offsets,
    strides, counts and byte sizes may be 0) -- and no host crash (a division by a zero dimension);
  * each divisibility / membership / range / aliasing rule the header states is violated once and gives rc < 0.
Pointer alignment is out of scope.  The few arguments the host itself reads are real host arrays (mean3 / std3, the index tables of
the uint8 entries, the pointer tables of mumpy_grad_norm_finish).

The sweep runs in ONE fresh child process (`python tests/test_abi_refusals.py`), which prints one JSON line per probe BEFORE the
call, so a host crash is reported as "died at entry X, mutation Y".  It must never run where a GPU is visible -- there a valid tuple
of fake addresses would really launch: the tests skip when conftest.have_gpu(), and the child checks torch.cuda.is_available() itself
before its first call and exits without calling anything."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

from abi_surface import arg_names, decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd")

# ------------------------------------------------------------------------------------------------------------ the table
# entry -> dict(v=scalar arguments by header name (valid), opt=pointers the header calls optional, null=pointers that are NULL in the
# valid tuple, flags=scalars that are MODES or hyper-parameters (act, shift, scale, eps, accumulate, the optimizer constants: no -1 / 0
# probe), neg=offsets, strides, counts and byte sizes (probed with -1; 0 is a valid value of theirs), every other scalar is a
# dimension (probed with -1 and 0), rules=[{name: value}] each violating one stated rule (a pointer name with None makes it NULL;
# "WS-1" is one byte less than the workspace query), ws=(query function, its arguments: names, or tuples of names to multiply)
# filling workspace_bytes, host={pointer: host array factory}, alias=[(a, b)] pointer pairs the header forbids to alias,
# also=[spec overrides] further valid tuples of the same entry (probed as valid + their rules))
MASKED = dict(v=dict(n_mask=1), null=set(), rules=[{"n_mask": 0}, {"n_mask": -1}])                    # a mask needs n_mask >= 1
WA = dict(v=dict(n_mask=0, B=1, Hs=7, W=7, C=32, shift=0, scale=0.125), opt={"mask_tab", "mask_id"}, null={"mask_tab", "mask_id"},
          flags={"shift", "scale"}, neg={"n_mask"}, also=[MASKED],
          rules=[{"Hs": 8}, {"W": 8}, {"C": 33}, {"shift": 7}, {"shift": -1}])          # grid a multiple of 7, heads of 32, shift in [0, 7)
WA_BWD = dict(v=dict(n_mask=0, workspace_bytes=0, B=1, Hs=7, W=7, C=32, shift=0, scale=0.125, accumulate=0), opt={"mask_tab", "mask_id"},
              null={"mask_tab", "mask_id"}, flags={"shift", "scale", "accumulate"}, neg={"n_mask", "workspace_bytes"}, also=[MASKED],
              rules=[{"Hs": 8}, {"W": 8}, {"C": 33}, {"shift": 7}, {"shift": -1}, {"workspace_bytes": "WS-1"}], ws=("mumpy_window_attention_bwd_workspace_bytes", ("B", "Hs", "W", "C")))
LIN = dict(v=dict(M=4, N=32, K=32, act=0), opt={"bias", "residual"}, flags={"act"}, rules=[{"N": 33}, {"K": 33}])
LIN_WS = dict(LIN, v=dict(LIN["v"], workspace_bytes=0), opt={"bias", "residual", "workspace"}, flags={"act"}, neg={"workspace_bytes"})
CVA_KV = dict(v=dict(B=1, Hs2=7, W=7, C=96, nq=1), rules=[{"C": 128}, {"Hs2": 8}, {"W": 8}])           # C in {96,192,384,768}
CVA_OUT = dict(v=dict(B=1, H=7, W=7, C=96), rules=[{"C": 128}, {"H": 8}, {"W": 8}], alias=[("out", "x1")])
CVA_CORE = dict(v=dict(B=1, H=7, W=7, C=96, r=1, scale=0.17), flags={"scale"}, rules=[{"H": 8}, {"W": 8}, {"C": 97}])
LN = dict(v=dict(rows=4, C=96, eps=1e-5), flags={"eps"}, rules=[{"C": 97}, {"C": 4100}])               # C % 4, C <= 4096
OPT_FLAGS = {"lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale", "momentum", "dampening", "nesterov", "alpha"}
F3 = lambda: (ctypes.c_float * 3)(0.5, 0.5, 0.5)
I8 = lambda: (ctypes.c_int32 * 8)(*range(8))

TABLE = {
    "mumpy_linear_rd_fwd": dict(LIN, v=dict(M=64, N=64, K=64, act=0), rules=[{"N": 65}, {"K": 65}]),
    "mumpy_window_attention_bg_fwd": WA, "mumpy_window_attention_fwd": WA, "mumpy_window_attention_bf16_fwd": WA,
    "mumpy_window_attention_bf16mm_fwd": WA, "mumpy_window_attention_mm16_fwd": WA,
    # the producer form (stats_out given, no ln_stats); M x N x K is filled in by _lnx_shape(): the first shape the planner folds
    "mumpy_linear_lnx_fwd": dict(v=dict(M=0, N=0, K=0, act=0, workspace_bytes=1 << 26, ln_gn=0, ln_eps=0.0),
                                 opt={"bias", "residual", "stats_out", "ln_stats", "ln_colsum"}, null={"ln_stats", "ln_colsum", "residual"},
                                 flags={"act", "ln_eps"}, neg={"workspace_bytes", "ln_gn"},
                                 rules=[{"M": 64, "N": 64, "K": 64}, {"workspace_bytes": 0}]),    # a shape the planner does not fold; no workspace
    "mumpy_deform_sample_kv_fwd": CVA_KV, "mumpy_deform_sample_kv_mm16_fwd": CVA_KV,
    "mumpy_deform_out_combine_fwd": CVA_OUT, "mumpy_deform_out_combine_mm16_fwd": CVA_OUT,
    "mumpy_avgpool2_pad_nhwc_fwd": dict(v=dict(B=1, H=4, W=4, C=4, Cpad=8, nchw_in=0), flags={"nchw_in"},
                                        rules=[{"H": 5}, {"W": 5}, {"Cpad": 9}, {"C": 5}]),
    "mumpy_copy_rows_fwd": dict(v=dict(src_stride=8, dst_stride=8, rows=2, cols=4), rules=[{"cols": 5}, {"src_stride": 9}, {"dst_stride": 9}]),
    "mumpy_merge_views_fwd": dict(v=dict(B=1, T=5, n=49, C1=32, C2=32, C3=32, t1=1, t2=1, t3=5), rules=[{"t1": 2}, {"t2": 2}, {"t3": 4}]),   # t_k in {1, T}
    "mumpy_trunk_head_fwd": dict(v=dict(B=1, h=2, w=2, C=4)),
    "mumpy_layernorm_fwd": LN, "mumpy_layernorm_bf16_fwd": LN,
    "mumpy_linear_fwd": LIN, "mumpy_linear_ws_fwd": LIN_WS, "mumpy_linear_wsz_fwd": LIN_WS,
    "mumpy_linear_bf16s_fwd": dict(LIN, v=dict(M=4, N=32, K=32, act=0, out_bf16=1), flags={"act", "out_bf16"}, null={"residual"}),   # (a bf16 y takes no residual)
    "mumpy_linear_rows_fwd": dict(LIN_WS, v=dict(rows_per_block=2, block_stride=64, M=4, N=32, K=32, act=0, workspace_bytes=0),
                                  flags={"act"}, neg={"workspace_bytes", "block_stride"}),
    "mumpy_linear_rows_kseg_fwd": dict(LIN_WS, v=dict(rows_per_block=2, block_stride=128, kseg=32, kstride=64, M=4, N=32, K=64, act=0,
                                                       workspace_bytes=0), flags={"act"}, neg={"workspace_bytes", "block_stride", "kstride"},
                                       rules=[{"N": 33}, {"kseg": 33}, {"kseg": 64, "K": 96}]),        # kseg % 32, K % kseg
    "mumpy_conv2d_nhwc_fwd": dict(v=dict(B=1, H=4, W=4, Cin=32, Cout=32, kh=3, kw=3, act=0, workspace_bytes=0),
                                  opt={"bias", "residual", "workspace"}, flags={"act"}, neg={"workspace_bytes"},
                                  rules=[{"Cin": 33}, {"Cout": 33}, {"kh": 2}, {"kw": 2}]),           # odd kernel
    "mumpy_deform_offsets_fwd": dict(v=dict(B=1, H=7, W=7, C=96), rules=[{"H": 8}, {"W": 8}, {"C": 780}]),    # Cg = C/3 <= 256
    "mumpy_deform_sample_fwd": dict(v=dict(B=1, Hs2=7, W=7, C=96, nq=1), rules=[{"Hs2": 8}, {"W": 8}]),
    "mumpy_deform_attention_fwd": CVA_CORE,
    "mumpy_deform_attention_mm16_fwd": dict(CVA_CORE, rules=CVA_CORE["rules"] + [{"H": 3584, "W": 3584}]),      # H * W * C * 4 < 2^32
    "mumpy_deform_combine_fwd": dict(v=dict(B=1, H=7, W=7, C=96), rules=[{"H": 8}, {"W": 8}], alias=[("out", "x1")]),
    "mumpy_faf_fwd": dict(v=dict(B=1, T=3, frame=1, lo_hi=74, mid_lo=75, mid_hi=149), neg={"frame", "lo_hi", "mid_lo", "mid_hi"},
                          rules=[{"frame": 3}, {"mid_lo": 150}]),
    "mumpy_patch_embed_fwd": dict(v=dict(B=1, T=3, H=8, W=8, t=1, C=96, eps=1e-5), flags={"eps"},
                                  rules=[{"T": 3, "t": 4}, {"H": 10}, {"W": 10}, {"C": 160}, {"C": 48}]),     # t <= T, H / W % 4, C in 32..128 by 32
    "mumpy_patch_merge_ln_fwd": dict(v=dict(B=1, Hs=2, W=2, C=96, eps=1e-5), flags={"eps"}, rules=[{"Hs": 3}, {"W": 3}]),
    "mumpy_temporal_attention_fwd": dict(v=dict(S=4, T=3, C=768, heads=12, scale=0.125), flags={"scale"},
                                         rules=[{"T": 17}, {"heads": 11}]),                        # T <= 16, heads of width 64
    "mumpy_temporal_attention_q_fwd": dict(v=dict(S=4, T=3, Tq=1, C=768, heads=12, scale=0.125), flags={"scale"},
                                           rules=[{"T": 17}, {"Tq": 4}, {"heads": 11}]),           # Tq <= T
    "mumpy_attention_probs_fwd": dict(v=dict(outer=2, heads=2, nq=3, nk=3, d=32, q_outer_stride=192, q_row_stride=64, k_outer_stride=192,
                                             k_row_stride=64, q_mod=2, scale=0.17),
                                      flags={"scale"}, neg={"q_outer_stride", "q_row_stride", "k_outer_stride", "k_row_stride"},
                                      rules=[{"nq": 65}, {"nk": 65}, {"d": 65}]),
    "mumpy_gn_stats_nhwc_fwd": dict(v=dict(B=1, HW=16, C=32, G=8, nsplit=1), rules=[{"G": 5}, {"C": 260}]),
    "mumpy_gn_apply_resample_nhwc_fwd": dict(v=dict(nsplit=1, G=8, eps=1e-5, act=1, mean4=0, scale=1, align_corners=0, ep_mode=0, out_ctot=32,
                                                    out_coff=0, B=1, H=4, W=4, C=32), opt={"partial", "gamma", "beta", "ep_a", "ep_b"},
                                             null={"ep_a", "ep_b"}, flags={"eps", "act", "mean4", "scale", "align_corners", "ep_mode"}, neg={"out_coff"},
                                             rules=[{"C": 260}, {"scale": 3}, {"out_ctot": 16}, {"ep_mode": 1}, {"act": 3}, {"G": 5},
                                                    {"out_coff": -4}, {"gamma": None}, {"beta": None}]),      # gamma / beta go with partial
    "mumpy_final_conv_fwd": dict(v=dict(B=1, H=4, W=4, C=32, thr=0.5), opt={"mask"}, flags={"thr"}, rules=[{"C": 33}]),
    "mumpy_final_conv_bwd": dict(v=dict(workspace_bytes=0, B=1, H=4, W=4, C=32), neg={"workspace_bytes"},
                                 rules=[{"C": 64}, {"workspace_bytes": "WS-1"}],
                                 ws=("mumpy_final_conv_bwd_workspace_bytes", ("B", "H", "W"))),
    "mumpy_sigmoid_threshold_fwd": dict(v=dict(n=16, thr=0.5), flags={"thr"}),
    "mumpy_normalize_u8_fwd": dict(v=dict(nframes=1, H=4, W=4), host={"mean3": F3, "std3": F3}),
    "mumpy_resize_normalize_u8_fwd": dict(v=dict(nframes=1, Hs=8, Ws=8, H=4, W=4), host={"mean3": F3, "std3": F3, "ytab": I8, "xtab": I8},
                                          rules=[{"W": 5}]),
    "mumpy_add_fwd": dict(v=dict(n=16), rules=[{"n": 17}]),
    "mumpy_mask_loss_fwd_bwd": dict(v=dict(workspace_bytes=0, B=2, P=16, eps=0.0, loss_scale=1.0), opt={"dlogits"},
                                    flags={"eps", "loss_scale"}, neg={"workspace_bytes"}, rules=[{"workspace_bytes": "WS-1"}],
                                    ws=("mumpy_mask_loss_workspace_bytes", ("B", "P"))),
    "mumpy_adamw_step": dict(v=dict(n=16, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=1, grad_scale=1.0),
                             flags=OPT_FLAGS, neg={"step"}, rules=[{"step": 0}]),
    "mumpy_adamw_step_dev": dict(v=dict(n=16)),
    "mumpy_sgd_step": dict(v=dict(n=16, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=0, grad_scale=1.0),
                           opt={"momentum_buf"}, null={"momentum_buf"}, flags=OPT_FLAGS,
                           rules=[{"dampening": 0.1}, {"nesterov": 1}, {"momentum": 0.9}]),        # nesterov / momentum need momentum > 0 / a buffer
    "mumpy_sgd_step_dev": dict(v=dict(n=16, nesterov=0), opt={"momentum_buf"}, flags=OPT_FLAGS),
    "mumpy_rmsprop_step": dict(v=dict(n=16, lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, grad_scale=1.0),
                               opt={"momentum_buf"}, null={"momentum_buf"}, flags=OPT_FLAGS, rules=[{"momentum": 0.9}]),
    "mumpy_rmsprop_step_dev": dict(v=dict(n=16), opt={"momentum_buf"}),
    "mumpy_grad_norm_partial": dict(v=dict(n=16)),
    "mumpy_grad_norm_finish": dict(v=dict(groups=1, clip=0, max_norm=0.0), flags={"clip", "max_norm"},
                                   host={"partials": lambda: (ctypes.c_void_p * 8)(*[4096] * 8), "n": lambda: (ctypes.c_int64 * 8)(*[16] * 8),
                                         "hyper_dev": lambda: (ctypes.c_void_p * 8)(*[8192] * 8), "optimizer_kind": lambda: (ctypes.c_int * 8)()},
                                   rules=[{"groups": 9}, {"clip": 1}]),                             # 1 ... 8 groups; clip needs max_norm > 0
    "mumpy_layernorm_bwd": dict(v=dict(workspace_bytes=0, rows=4, C=96, eps=1e-5, accumulate=0), opt={"dx_add"},
                                flags={"eps", "accumulate"}, neg={"workspace_bytes"},
                                rules=[{"C": 97}, {"C": 2052}, {"workspace_bytes": "WS-1"}],
                                ws=("mumpy_layernorm_bwd_workspace_bytes", ("rows", "C"))),
    "mumpy_gelu_fwd": dict(v=dict(n=16), rules=[{"n": 17}]), "mumpy_gelu_bwd": dict(v=dict(n=16), rules=[{"n": 17}]),
    "mumpy_transpose_fwd": dict(v=dict(R=4, C=4)),
    "mumpy_col_sum_fwd": dict(v=dict(workspace_bytes=0, R=4, C=32), neg={"workspace_bytes"}, rules=[{"workspace_bytes": "WS-1"}], ws=("mumpy_col_sum_workspace_bytes", ("R", "C"))),
    "mumpy_linear_bwd": dict(v=dict(M=4, N=32, K=32, accumulate=0, workspace_bytes=0), opt={"dx", "dW", "db", "workspace", "x", "W"},
                             flags={"accumulate"}, neg={"workspace_bytes"},
                             rules=[{"N": 33}, {"K": 33}, {"x": None, "W": None, "dx": None, "dW": None, "workspace": None}],    # db alone needs the workspace
                             ws=("mumpy_linear_bwd_workspace_bytes", ("M", "N", "K"))),
    "mumpy_patch_gather_fwd": dict(v=dict(B=1, H=2, W=2, C=4, inverse=0), flags={"inverse"}, rules=[{"H": 3}, {"W": 3}, {"C": 5}]),
    "mumpy_conv_weight_dgrad_fwd": dict(v=dict(Cout=4, Cin=4, kh=3, kw=3)),
    "mumpy_conv2d_wgrad_nhwc": dict(v=dict(B=1, H=4, W=4, Cin=32, Cout=32, kh=3, kw=3, accumulate=0, workspace_bytes=0), opt={"workspace"},
                                    flags={"accumulate"}, neg={"workspace_bytes"}, rules=[{"Cin": 33}, {"Cout": 33}, {"kh": 2}, {"kw": 2}]),
    "mumpy_window_attention_bwd": WA_BWD, "mumpy_window_attention_bwd_csr": WA_BWD,
    "mumpy_window_attention_mm16_bwd": dict(WA_BWD, opt={"mask_tab", "mask_id", "rel_csr"},
                                            ws=("mumpy_window_attention_mm16_bwd_workspace_bytes", ("B", "Hs", "W", "C"))),
    "mumpy_relpos_bias_expand_fwd": dict(v=dict(nH=3)),
    "mumpy_gn_bwd_nhwc": dict(v=dict(nsplit_stats=1, workspace_bytes=0, B=1, HW=16, C=32, G=8, eps=1e-5, relu=1), flags={"eps", "relu"}, neg={"workspace_bytes"},
                              rules=[{"G": 5}, {"C": 260}, {"relu": 3}, {"workspace_bytes": "WS-1"}], ws=("mumpy_gn_bwd_workspace_bytes", ("B", "HW", "C"))),
    "mumpy_temporal_attention_bwd": dict(v=dict(S=4, T=3, C=768, heads=12, scale=0.125), flags={"scale"}, rules=[{"T": 17}, {"heads": 11}]),
    "mumpy_scale_samples_fwd": dict(v=dict(B=2, per_sample=16), rules=[{"per_sample": 17}]),
    "mumpy_upsample_bwd_nhwc": dict(v=dict(B=1, H=4, W=4, C=32, scale=2, align_corners=0), flags={"scale", "align_corners"}, rules=[{"scale": 3}]),
    "mumpy_dwconv5_window_fwd": dict(v=dict(N=2, C=32), rules=[{"C": 388}]),                      # C <= 384
    "mumpy_dwconv5_window_bwd": dict(v=dict(workspace_bytes=0, N=2, C=32), neg={"workspace_bytes"}, rules=[{"C": 388}, {"workspace_bytes": "WS-1"}],
                                     ws=("mumpy_dwconv5_window_bwd_workspace_bytes", ("N", "C"))),
    "mumpy_deform_attention_bwd": dict(v=dict(workspace_bytes=0, B1w=1, r=2, C=96, scale=0.17), flags={"scale"}, neg={"workspace_bytes"},
                                       rules=[{"C": 97}, {"workspace_bytes": "WS-1"}],
                                       ws=("mumpy_deform_attention_bwd_workspace_bytes", (("B1w", "r"), "C"))),
    "mumpy_deform_sample_bwd": dict(v=dict(B2=2, C=96, nq=1)),
}
EXCLUDED = {}            # entry -> reason; at most 8
LNX_SHAPES = [(1960, 768, 768), (2000, 1024, 1024), (7840, 512, 512), (7840, 512, 2048)]


def _params():
    """-> {entry of include/mumpy_hip.h: [(argument name, is pointer)]}"""
    return {n: [(name, "*" in a) for name, a in zip(arg_names(d.args), d.args)] for n, d in decls("mumpy_hip.h").items()}


def stream_entries():
    return sorted(n for n, a in _params().items() if a and a[-1] == ("stream", True))


# ------------------------------------------------------------------------------------------------------------ the child
def _probes(lib):
    """-> [(entry, mutation, expectation, argument list)] for every table entry; expectation in {"pos", "neg", "nonpos"}."""
    declared = _params()
    keep, probes = [], []
    for entry, spec in TABLE.items():
        params = declared[entry][:-1]                                     # (the stream stays NULL)
        v = dict(spec["v"])
        if entry == "mumpy_linear_lnx_fwd":
            m, n, k = next(s for s in LNX_SHAPES if lib.mumpy_linear_ln_tiles(*s) > 0)
            v.update(M=m, N=n, K=k)
        if "ws" in spec:
            fn, names = spec["ws"]
            vals = [v[nm] if isinstance(nm, str) else math.prod(v[f] for f in nm) for nm in names]
            v["workspace_bytes"] = int(getattr(lib, fn)(*vals))
            assert v["workspace_bytes"] > 0, entry
        missing = [p for p, is_ptr in params if not is_ptr and p not in v]
        assert not missing and not set(v) - {p for p, _ in params}, (entry, missing, set(v) - {p for p, _ in params})
        host = {p: f() for p, f in spec.get("host", {}).items()}
        keep.append(host)
        ptrs = {p: host.get(p, 0x100000 * (i + 1)) for i, (p, is_ptr) in enumerate(params) if is_ptr}
        for p in spec.get("null", ()):
            ptrs[p] = None

        def args(over=None, base=None, params=params, v=v, ptrs=ptrs):
            a = dict(ptrs, **v)
            a.update(base or {})
            a.update(over or {})
            if a.get("workspace_bytes") == "WS-1":
                a["workspace_bytes"] = v["workspace_bytes"] - 1
            return [a[p] for p, _ in params] + [None]

        def label(rule):
            return ",".join(f"{k}={'NULL' if val is None else val}" for k, val in rule.items())
        assert not set(spec.get("neg", ())) - set(v), entry
        probes.append((entry, "valid", "pos", args()))
        for p, is_ptr in params:
            if is_ptr and p not in spec.get("opt", ()):
                probes.append((entry, f"{p}=NULL", "neg-msg", args({p: None})))
            if not is_ptr and p not in spec.get("flags", ()):
                probes.append((entry, f"{p}=-1", "neg", args({p: -1})))
                if p not in spec.get("neg", ()):
                    probes.append((entry, f"{p}=0", "nonpos", args({p: 0})))
        for rule in spec.get("rules", ()):
            probes.append((entry, "rule " + label(rule), "neg", args(rule)))
        for a, b in spec.get("alias", ()):
            probes.append((entry, f"alias {a}={b}", "neg", args({a: ptrs[b]})))
        for n, more in enumerate(spec.get("also", ())):
            base = dict(more["v"], **{p: (None if p in more["null"] else host.get(p, 0x100000 * (i + 1)))
                                      for i, (p, is_ptr) in enumerate(params) if is_ptr})
            probes.append((entry, f"valid#{n + 2} {label(more['v'])}", "pos", args(None, base)))
            for rule in more["rules"]:
                probes.append((entry, f"#{n + 2} rule " + label(rule), "neg", args(rule, base)))
    return probes, keep


def child():
    import torch
    if torch.cuda.is_available():                                         # a valid tuple of fake addresses would really launch
        print(json.dumps({"refused": "a GPU is visible"}), flush=True)
        return 3
    sys.path.insert(0, PKG)
    from mumpy_hip.lib import SIGNATURES, load_library
    lib = load_library()
    probes, keep = _probes(lib)
    for entry, mutation, expect, args in probes:
        print(json.dumps({"entry": entry, "mutation": mutation, "expect": expect}), flush=True)      # BEFORE the call
        if expect == "neg-msg":          # the message is sticky per thread: leave a known one of ANOTHER entry there first
            other = "mumpy_gelu_fwd" if entry == "mumpy_add_fwd" else "mumpy_add_fwd"
            assert getattr(lib, other)(*([None] * (len(SIGNATURES[other]) - 2)), 16, None) < 0
            stale = lib.mumpy_last_error()
        rc = int(getattr(lib, entry)(*args))
        if expect == "neg-msg" and rc and lib.mumpy_last_error() == stale:
            print(json.dumps({"rc": rc, "err": ""}), flush=True)                                      # refused without a message of its own
            continue
        print(json.dumps({"rc": rc, "err": lib.mumpy_last_error().decode(errors="replace") if rc else ""}), flush=True)
    print(json.dumps({"done": len(probes)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(child())


# ------------------------------------------------------------------------------------------------------------ the tests
import pytest  # noqa: E402

from conftest import have_gpu  # noqa: E402

needs_no_gpu = pytest.mark.skipif(have_gpu(), reason="with a device present a valid tuple of fake addresses would really launch")


@functools.lru_cache(maxsize=None)
def _sweep():
    """-> ({entry: [(mutation, expectation, rc, err)]}, how the child ended)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    results, pending, done = {}, None, False
    for ln in lines:
        if "entry" in ln:
            pending = ln
        elif "rc" in ln:
            results.setdefault(pending["entry"], []).append((pending["mutation"], pending["expect"], ln["rc"], ln["err"]))
            pending = None
        elif "done" in ln:
            done = True
    end = "finished" if done and r.returncode == 0 else (
        f"died (exit {r.returncode}) at entry {pending['entry']}, mutation {pending['mutation']}" if pending else
        f"ended early (exit {r.returncode}): {r.stdout[-300:]} {r.stderr[-600:]}")
    return results, end


def test_every_entry_point_with_a_stream_is_swept_or_excluded_with_a_reason():
    entries = stream_entries()
    assert len(entries) >= 73
    assert len(EXCLUDED) <= 8 and all(isinstance(r, str) and len(r) > 20 for r in EXCLUDED.values())
    assert not set(TABLE) & set(EXCLUDED)
    assert set(entries) == set(TABLE) | set(EXCLUDED), (sorted(set(entries) - set(TABLE) - set(EXCLUDED)), sorted((set(TABLE) | set(EXCLUDED)) - set(entries)))


@needs_no_gpu
def test_the_sweep_ran_to_its_end_without_a_host_crash():
    results, end = _sweep()
    assert end == "finished", end
    assert set(results) == set(TABLE)


@needs_no_gpu
@pytest.mark.parametrize("entry", sorted(TABLE))
def test_entry_point_refuses_what_its_header_forbids(entry):
    results, end = _sweep()
    assert entry in results, end
    bad = []
    for mutation, expect, rc, err in results[entry]:
        ok = {"pos": rc > 0, "neg": rc < 0, "neg-msg": rc < 0 and bool(err), "nonpos": rc <= 0}[expect]
        if not ok:
            bad.append(f"{mutation}: rc = {rc} ({err!r}), expected {expect}")
    assert results[entry][0][0] == "valid" and not bad, "\n".join(bad)
