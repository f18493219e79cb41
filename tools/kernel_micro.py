#!/usr/bin/env python3
"""Launch one kernel shape repeatedly (for rocprofv3 --pmc / timing).
  kernel_micro.py linear M N K [act]      | kernel_micro.py winattn B Hs W C shift | kernel_micro.py sample B Hs2 W C
  | kernel_micro.py winattn_bwd B Hs W C shift | kernel_micro.py ln_bwd rows C
  | kernel_micro.py adamw N | kernel_micro.py maskloss B P | kernel_micro.py ln rows C
  | kernel_micro.py winattn16 B Hs W C shift    bf16-stored qkv: the fp32-flow kernel and the bf16-MFMA kernel on the same input,
                                                alternating in one process (ROUNDS rounds of REPS launches each, default 12 x 20)
  | kernel_micro.py winattn_mm16 B Hs W C shift   fp32-stored qkv: mumpy_window_attention_fwd and the bf16-MFMA forward of the training
                                                tape (window_attention_mm16) on the same input, same alternating protocol
  | kernel_micro.py winattn_bwd16 B Hs W C shift  the fp32 backward pair and the bf16-MFMA pair (window_attention_bwd math="fp32" /
                                                "bf16", each with its reduce and table kernels) on the same input, same protocol
  | kernel_micro.py winattn_ab B Hs W C shift     mumpy_window_attention_fwd of several LIBRARIES / launch forms on the same input
  | kernel_micro.py cva_attn B H W C r            mumpy_deform_attention_fwd, likewise.  MUMPY_AB_LIBS="name=path[@VAR=VALUE],..." names
                                                the variants (e.g. parent=<old>/libmumpy_hip.so, new=<lib>/libmumpy_hip.so, and the tuning
                                                build twice with @MUMPY_WA_SPLIT_UNITS=0 / =1000000 to force a form; VAR is set while that
                                                variant's launches are issued).  Each variant's REPS launches are captured in one graph (an
                                                eager loop of ~10 us kernels measures the launch rate, not the kernel); the graphs replay
                                                alternately for ROUNDS rounds; prints median [min..max] us per launch and whether every
                                                variant's output is bitwise the first one's
  | kernel_micro.py cva_attn_bwd16 B1w r C        window form: the fp32 cross-view attention backward (deform_attention_bwd math="fp32",
                                                its r - 1 add launches included) against the bf16-MFMA pair (math="bf16"), and the two
                                                forwards, on the same input; each one's REPS calls captured in one graph, the four graphs
                                                replayed alternately for ROUNDS rounds
  | kernel_micro.py cva_bwd_grouped G B1w r C     window form: the cross-view backward ops with groups=G (the _grouped entries of
                                                include/mumpy_hip_ext9.h; their dpos / dq reductions included) against the frozen ones --
                                                deform_attention_bwd fp32 and bf16, deform_sample_bwd when C is a multiple of 96 -- on the
                                                same input, same protocol; the frozen call is captured twice, so its own spread shows
  | kernel_micro.py mlp M C hidden                the launches of one MLP on the training tape, fused (ops.set_mlp_fusion) against the ones
                                                they replace, MUMPY_MATH=fp32|bf16: fc1 as linear + gelu / linear_gelu_dual; fc2's
                                                backward (dz, dW2, db2) as linear_bwd + gelu_bwd / the big-M pair (dX on the forward
                                                GEMM against W^T, linear_bwd for dW2 and db2, gelu_bwd) / linear_gelu_bwd; same protocol"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd")]
from mumpy_hip import ops
dev = torch.device("cuda:0")
ops.set_matrix_math(os.environ.get("MUMPY_MATH", "fp32"))      # fp32 | bf16 | bf16x3 for the linear micro
op, a = sys.argv[1], [int(v) for v in sys.argv[2:]]
reps = int(os.environ.get("REPS", "20"))
if op == "winattn16":
    b, hs, w, c, shift = a
    from models.modules.swinTransformer import build_shift_mask, relative_position_index
    qkv16 = torch.randn(b, hs * w, 3 * c, device=dev).to(torch.bfloat16)
    bias = ops.expand_relpos_bias(torch.randn(169, c // 32, device=dev) * 0.2, relative_position_index(7, 7).to(dev))
    tab = ids = None
    if shift:
        tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift).to(dev))
    rounds = int(os.environ.get("ROUNDS", "12"))
    times = {"fp32": [], "bf16": []}
    for math in ("fp32", "bf16"):
        for _ in range(5):
            ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, 32 ** -0.5, tab, ids, math=math)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for math in ("fp32", "bf16"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.window_attention_bf16(qkv16, bias, b, hs, w, c, shift, 32 ** -0.5, tab, ids, math=math)
            e1.record(); torch.cuda.synchronize()
            times[math].append(e0.elapsed_time(e1) * 1e3 / reps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    gb = 2.0 * 4 * b * hs * w * c / 1e3            # bf16 q, k, v read + out written, per us -> GB/s
    print(f"winattn16 {a}: fp32-flow {med['fp32']:.1f} us [{min(times['fp32']):.1f}..{max(times['fp32']):.1f}], "
          f"bf16-MFMA {med['bf16']:.1f} us [{min(times['bf16']):.1f}..{max(times['bf16']):.1f}] ({gb / med['bf16']:.0f} GB/s), "
          f"fp32/bf16 = {med['fp32'] / med['bf16']:.2f}  (median of {rounds} rounds x {reps} launches, alternating)")
    sys.exit(0)
if op in ("winattn_ab", "cva_attn"):
    import ctypes
    from mumpy_hip.lib import SIGNATURES
    entry = "mumpy_window_attention_fwd" if op == "winattn_ab" else "mumpy_deform_attention_fwd"
    variants = []                                   # (name, function, (VAR, VALUE) or None)
    for spec in os.environ["MUMPY_AB_LIBS"].split(","):
        name, path = spec.split("=", 1)
        path, _, setting = path.partition("@")
        fn = getattr(ctypes.CDLL(os.path.abspath(path)), entry)
        fn.argtypes, fn.restype = SIGNATURES[entry], ctypes.c_int
        variants.append((name, fn, tuple(setting.split("=", 1)) if setting else None))
    torch.manual_seed(0)
    if op == "winattn_ab":
        b, hs, w, c, shift = a
        from models.modules.swinTransformer import build_shift_mask, relative_position_index
        qkv = torch.randn(b, hs * w, 3 * c, device=dev)
        bias = ops.expand_relpos_bias(torch.randn(169, c // 32, device=dev) * 0.2, relative_position_index(7, 7).to(dev))
        tab = ids = None
        if shift:
            tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift).to(dev))
        ptr = lambda t: None if t is None else t.data_ptr()
        shape = (b, hs * w, c)
        args = lambda out, st: (qkv.data_ptr(), out.data_ptr(), bias.data_ptr(), ptr(tab), ptr(ids), 0 if ids is None else ids.numel(),
                                b, hs, w, c, shift, 32 ** -0.5, st)
    else:
        b, h, w, c, r = a
        b1w = b * (h // 7) * (w // 7)
        q = torch.randn(b, h * w, c, device=dev); kv = torch.randn(b1w * r, 49, 2 * c, device=dev); pad = ops.pad_mask(dev)
        shape = (b1w, 49, c)
        args = lambda out, st: (q.data_ptr(), kv.data_ptr(), pad.data_ptr(), out.data_ptr(), b, h, w, c, r, 32 ** -0.5, st)
    rounds = int(os.environ.get("ROUNDS", "12"))
    outs, graphs = {}, {}
    for name, fn, setting in variants:
        if setting:
            os.environ[setting[0]] = setting[1]
        outs[name] = torch.full(shape, float("nan"), device=dev)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                assert fn(*args(outs[name], side.cuda_stream)) == 0
        side.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=side):
            for _ in range(reps):
                assert fn(*args(outs[name], torch.cuda.current_stream().cuda_stream)) == 0
        if setting:
            del os.environ[setting[0]]
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, _, _ in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graphs[name].replay(); e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    first = variants[0][0]
    print(f"{op} {a}: " + ", ".join(f"{n} {sorted(t)[len(t) // 2]:.2f} us [{min(t):.2f}..{max(t):.2f}]" for n, t in times.items())
          + f"  (median of {rounds} alternating replays of {reps} captured launches); bitwise equal to {first}: "
          + ", ".join(f"{n} {bool(torch.equal(outs[n], outs[first]))}" for n in outs if n != first))
    sys.exit(0)
if op == "cva_attn_bwd16":
    b1w, r, c = a
    torch.manual_seed(0)
    q = torch.randn(b1w, 49, c, device=dev); kv = torch.randn(b1w * r, 49, 2 * c, device=dev); dout = torch.randn(b1w, 49, c, device=dev)
    pad = ops.pad_mask(dev)
    run = {}
    for m in ("fp32", "bf16"):
        run["bwd " + m] = lambda m=m: ops.deform_attention_bwd(q, kv, dout, r, 32 ** -0.5, math=m)      # fp32: with its r - 1 adds
        run["fwd " + m] = lambda m=m: ops.deform_attention(q, kv, pad, b1w, 7, 7, c, r, 32 ** -0.5, math=m)
    rounds = int(os.environ.get("ROUNDS", "12"))
    graphs = {}
    for name, fn in run.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        side.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=side):
            for _ in range(reps):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {name: [] for name in run}
    for _ in range(rounds):
        for name in run:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graphs[name].replay(); e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(f"{op} {a}: " + ", ".join(f"{n} {med[n]:.2f} us [{min(t):.2f}..{max(t):.2f}]" for n, t in times.items())
          + f"; bwd fp32/bf16 = {med['bwd fp32'] / med['bwd bf16']:.2f}, fwd fp32/bf16 = {med['fwd fp32'] / med['fwd bf16']:.2f}"
          + f"  (median of {rounds} alternating replays of {reps} captured launches)")
    sys.exit(0)
if op == "cva_bwd_grouped":
    groups, b1w, r, c = a
    torch.manual_seed(0)
    q = torch.randn(b1w, 49, c, device=dev); kv = torch.randn(b1w * r, 49, 2 * c, device=dev); dout = torch.randn(b1w, 49, c, device=dev)
    x2 = torch.randn(b1w * r, 49, c, device=dev); pos = torch.rand(b1w, 3, 49, 2, device=dev) * 2.6 - 1.3
    ds = torch.randn(b1w * r, 49, c, device=dev)
    run = {}
    for label, g in (("frozen", 1), ("frozen again", 1), ("grouped", groups)):       # frozen twice: the spread of one and the same call
        kw = {} if g == 1 else {"groups": g}
        for m in ("fp32", "bf16"):
            run[f"attn {m} {label}"] = lambda m=m, kw=kw: ops.deform_attention_bwd(q, kv, dout, r, 32 ** -0.5, math=m, **kw)
        if c % 96 == 0:
            run[f"sample {label}"] = lambda kw=kw: ops.deform_sample_bwd(x2, pos, ds, **kw)
    rounds = int(os.environ.get("ROUNDS", "12"))
    graphs = {}
    for name, fn in run.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        side.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=side):
            for _ in range(reps):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {name: [] for name in run}
    for _ in range(rounds):
        for name in run:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graphs[name].replay(); e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    parts = []
    for kind in sorted({n.rsplit(" frozen", 1)[0] for n in run if " frozen" in n}):
        f1, f2, g = med[kind + " frozen"], med[kind + " frozen again"], med[kind + " grouped"]
        lo = min(times[kind + " frozen"] + times[kind + " frozen again"]); hi = max(times[kind + " frozen"] + times[kind + " frozen again"])
        parts.append(f"{kind}: frozen {f1:.2f} / {f2:.2f} us [{lo:.2f}..{hi:.2f}], grouped {g:.2f} us "
                     f"[{min(times[kind + ' grouped']):.2f}..{max(times[kind + ' grouped']):.2f}], grouped/frozen = {g / f1:.3f}"
                     + ("" if lo <= g <= hi else "  OUTSIDE the frozen spread"))
    print(f"{op} groups={groups} {a[1:]}: " + "; ".join(parts) + f"  (medians of {rounds} alternating replays of {reps} captured calls)")
    sys.exit(0)
if op == "mlp":
    m, c, hid = a
    torch.manual_seed(0)
    x = torch.randn(m, c, device=dev); w1 = torch.randn(hid, c, device=dev) / c ** 0.5; b1 = torch.randn(hid, device=dev)
    w2 = torch.randn(c, hid, device=dev) / hid ** 0.5; dy = torch.randn(m, c, device=dev)
    z, act = ops.linear_gelu_dual(x, w1, b1)

    def big_pair():
        ops.linear_bwd(act, w2, dy, need_dx=False, need_dw=True, need_db=True)
        return ops.gelu_bwd(z, ops.linear(dy, ops.transpose(w2)))
    run = {"fwd linear + gelu": lambda: ops.gelu(ops.linear(x, w1, b1)), "fwd dual": lambda: ops.linear_gelu_dual(x, w1, b1),
           "bwd linear_bwd + gelu_bwd": lambda: ops.gelu_bwd(z, ops.linear_bwd(act, w2, dy, need_dx=True, need_dw=True, need_db=True)[0]),
           "bwd big pair": big_pair,
           "bwd gated": lambda: ops.linear_gelu_bwd(act, z, w2, dy, need_dz=True, need_dw=True, need_db=True)}
    rounds = int(os.environ.get("ROUNDS", "12"))
    graphs = {}
    for name, fn in run.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        side.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=side):
            for _ in range(reps):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {name: [] for name in run}
    for _ in range(rounds):
        for name in run:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graphs[name].replay(); e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    print(f"{op} {a} {ops.matrix_math()}: " + ", ".join(f"{n} {sorted(t)[len(t) // 2]:.2f} us [{min(t):.2f}..{max(t):.2f}]" for n, t in times.items())
          + f"  (median of {rounds} alternating replays of {reps} captured calls)")
    sys.exit(0)
if op in ("winattn_mm16", "winattn_bwd16"):
    b, hs, w, c, shift = a
    from models.modules.swinTransformer import build_shift_mask, relative_position_index
    qkv = torch.randn(b, hs * w, 3 * c, device=dev); dout = torch.randn(b, hs * w, c, device=dev)
    idx = relative_position_index(7, 7).to(dev)
    bias = ops.expand_relpos_bias(torch.randn(169, c // 32, device=dev) * 0.2, idx)
    idx32, csr = ops.rel_index32(idx), ops.rel_index_csr(idx)
    tab = ids = None
    if shift:
        tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift).to(dev))
    if op == "winattn_mm16":
        run = {"fp32": lambda: ops.window_attention(qkv, bias, b, hs, w, c, shift, 32 ** -0.5, tab, ids),
               "bf16": lambda: ops.window_attention_mm16(qkv, bias, b, hs, w, c, shift, 32 ** -0.5, tab, ids)}
    else:
        run = {m: (lambda m=m: ops.window_attention_bwd(qkv, dout, bias, idx32, b, hs, w, c, shift, 32 ** -0.5, tab, ids, rel_csr=csr, math=m))
               for m in ("fp32", "bf16")}
    rounds = int(os.environ.get("ROUNDS", "12"))
    times = {"fp32": [], "bf16": []}
    for math in ("fp32", "bf16"):
        for _ in range(5):
            run[math]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for math in ("fp32", "bf16"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run[math]()
            e1.record(); torch.cuda.synchronize()
            times[math].append(e0.elapsed_time(e1) * 1e3 / reps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(f"{op} {a}: fp32 {med['fp32']:.1f} us [{min(times['fp32']):.1f}..{max(times['fp32']):.1f}], "
          f"bf16-MFMA {med['bf16']:.1f} us [{min(times['bf16']):.1f}..{max(times['bf16']):.1f}], "
          f"fp32/bf16 = {med['fp32'] / med['bf16']:.2f}  (median of {rounds} rounds x {reps} launches, alternating)")
    sys.exit(0)
if op == "linear":
    m, n, k = a[:3]; act = a[3] if len(a) > 3 else 0
    x = torch.randn(m, k, device=dev); w = torch.randn(n, k, device=dev) / k ** 0.5; b = torch.randn(n, device=dev)
    fn = lambda: ops.linear(x, w, b, act=act)
    work, unit = 2.0 * m * n * k, "TFLOP/s"
elif op == "winattn":
    b, hs, w, c, shift = a
    qkv = torch.randn(b, hs * w, 3 * c, device=dev)
    bias = ops.expand_relpos_bias(torch.randn(169, c // 32, device=dev) * 0.2,
                                  __import__("models.modules.swinTransformer", fromlist=["x"]).relative_position_index(7, 7).to(dev))
    tab = ids = None
    if shift:
        from models.modules.swinTransformer import build_shift_mask
        tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift).to(dev))
    fn = lambda: ops.window_attention(qkv, bias, b, hs, w, c, shift, 32 ** -0.5, tab, ids)
    work, unit = 307328.0 * b * (hs // 7) * (w // 7) * (c // 32), "TFLOP/s"
elif op == "sample":
    b, hs2, w, c = a
    nw = b * (hs2 // 7) * (w // 7)
    x2 = torch.randn(b, hs2 * w, c, device=dev); pos = torch.rand(nw, 3, 49, 2, device=dev) * 2 - 1
    fn = lambda: ops.deform_sample(x2, pos, b, hs2, w, c, nw)
    work, unit = 4.0 * (2 * nw * 49 * c + nw * 3 * 49 * 2), "GB/s"
if op == "winattn_bwd":
    b, hs, w, c, shift = a
    from models.modules.swinTransformer import build_shift_mask, relative_position_index
    qkv = torch.randn(b, hs * w, 3 * c, device=dev); dout = torch.randn(b, hs * w, c, device=dev)
    idx = relative_position_index(7, 7).to(dev)
    bias = ops.expand_relpos_bias(torch.randn(169, c // 32, device=dev) * 0.2, idx)
    idx32 = idx.to(torch.int32).reshape(-1).contiguous()
    tab = ids = None
    if shift:
        tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift).to(dev))
    fn = lambda: ops.window_attention_bwd(qkv, dout, bias, idx32, b, hs, w, c, shift, 32 ** -0.5, tab, ids)
    work, unit = 5 * 153664.0 * b * (hs // 7) * (w // 7) * (c // 32), "TFLOP/s"      # 5 products of 2*49*49*32 FLOP per unit
if op == "ln_bwd":
    rows, c = a
    x = torch.randn(rows, c, device=dev); g = torch.ones(c, device=dev); dy = torch.randn(rows, c, device=dev)
    fn = lambda: ops.layernorm_bwd(x, g, dy)
    work, unit = 12.0 * rows * c, "GB/s"
if op == "adamw":
    n, = a
    bufs = [torch.randn(n, device=dev) for _ in range(2)] + [torch.zeros(n, device=dev) for _ in range(2)]
    fn = lambda: ops.adamw_step(bufs[0], bufs[1], bufs[2], bufs[3], 3, lr=1e-3)
    work, unit = 28.0 * n, "GB/s"
if op == "maskloss":
    b, p_ = a
    z = torch.randn(b, p_, device=dev); t = (torch.rand(b, p_, device=dev) < 0.1).float()
    fn = lambda: ops.mask_loss(z, t)
    work, unit = 20.0 * b * p_, "GB/s"
if op == "ln":
    rows, c = a
    x = torch.randn(rows, c, device=dev); g = torch.ones(c, device=dev); b = torch.zeros(c, device=dev)
    fn = lambda: ops.layernorm(x, g, b)
    work, unit = 8.0 * rows * c, "GB/s"
for _ in range(3):
    fn()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    fn()
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1e3 / reps
print(f"{op} {a}: {us:.1f} us/launch, {work / us / (1e6 if unit == 'TFLOP/s' else 1e3):.1f} {unit}")
