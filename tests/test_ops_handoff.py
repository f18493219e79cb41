"""What mumpy_hip.ops hands to the kernels when a caller's tensor is NOT right by construction.

The C ABI sees addresses and integers; the ops layer is the one place that holds both the tensors and the dimensions.  This file
sweeps the table of valid calls (CASES of tests/test_memory_discipline.py, plus EXTRA below for parameters that table does not reach)
and mutates ONE input tensor at a time:
  dtype    the same values at another width (float32 <-> float64, bfloat16 -> float32, int32 <-> int64, uint8 -> int32);
  host     the tensor left on the CPU;
  strided  same shape and values, every second element of a buffer twice as long in the last dimension;
  nchw     (4-D NHWC inputs only) the NCHW-dense layout of the same logical tensor;
  short    an allocation of its own with the first dimension of size > 1 reduced by one (tensors of one element: skipped, counted).
Phase 1 runs every mutated call in RECORD mode (tests/handoff_audit.py: nothing is launched) and judges it against the hand-off of
the valid call: refused before any launch / re-dimensioned (short only) / same launch with every pointer a contiguous GPU tensor of
the valid dtype and at least the valid byte size; in-place inputs must be handed in the caller's storage.  Phase 2 launches, for
real, only the triples phase 1 judged "same launch" on inputs that are not in-place, and compares every output bit for bit with the
valid call's, and the caller's tensor with its own earlier bits: a wrapper's conversion or copy must be faithful.  A triple that
phase 1 failed is never launched.

CPU tests: the recorder's own self-tests on a fake ops module (no GPU, no library), the facts of the table, and the coverage
conditions (every mutation kind reaches every (op, argument) pair; at most 10 % of the short mutations skipped).
GPU tests: the sweep, and two numeric regressions -- LayerNorm-fold statistics do not survive an overwrite, and accumulate-into
buffers are used where they are (a slice of a flat buffer) or refused (a strided view)."""
import types
from collections import Counter

import pytest
import torch

import handoff_audit as HA
from test_memory_discipline import CASES, Case, _T, _bias_pad, _nhwc, _outside, _shift_mask
from weight_fill import seeded_randn

gpu = pytest.mark.gpu
KINDS = ("dtype", "host", "strided", "nchw", "short")
WIDER = {torch.float32: torch.float64, torch.float64: torch.float32, torch.bfloat16: torch.float32, torch.int32: torch.int64,
         torch.int64: torch.int32, torch.uint8: torch.int32}
LIBRARY_CASE = "linear_ln/2000x1024x3072-emit_stats"             # the one case of the parent's table whose build() asks the library
# arguments that never hold more than one element anywhere in the table: `short` and `strided` cannot be formed for them
ONE_ELEMENT_ONLY = {("final_conv", "bias"): "Conv2d(32k, 1, 3): the bias of the single output channel"}


# What no check on the host can decide.  How many (64, 64) patterns a mask_id tensor refers to is device data (the largest id in
# it): ops checks that mask_tab holds whole patterns, at least one, and that the int32 mask_id divides the windows, but a table one
# pattern short can only be told by reading the ids back -- a synchronisation per launch, which the ops layer does not pay.  The
# pair comes from ops.compact_attn_mask, which builds both from one mask.  Such a triple is judged, reported and never launched.
UNCHECKABLE = {("window_attention", "tab", "short"), ("window_attention_bf16", "tab", "short"), ("window_attention_bf16mm", "tab", "short"),
               ("window_attention_mm16", "tab", "short"), ("window_attention_bwd", "tab", "short")}


# ================================================================================================ the extra cases
EXTRA = []


def case(id_, inplace=()):
    def deco(build):
        EXTRA.append(Case(id_, build, tuple(inplace), {}))
        return build
    return deco


@case("layernorm/out=", inplace=("out",))
def _():
    i = {"x": seeded_randn(1, 5, 96) * 3 + 1, "g": seeded_randn(2, 96), "b": seeded_randn(3, 96), "out": torch.zeros(5, 96)}
    return i, lambda ops, t: {"y": ops.layernorm(t.x, t.g, t.b, out=t.out)}


@case("linear/out=", inplace=("out",))
def _():
    i = {"x": seeded_randn(1, 5, 32), "w": seeded_randn(2, 64, 32) / 32 ** 0.5, "b": seeded_randn(3, 64), "r": seeded_randn(4, 5, 64),
         "out": torch.zeros(5, 64)}
    return i, lambda ops, t: {"y": ops.linear(t.x, t.w, t.b, residual=t.r, out=t.out)}


@case("linear_rows/out=", inplace=("out",))
def _():
    i = {"x": seeded_randn(1, 2, 2, 7, 32), "w": seeded_randn(2, 64, 32) / 32 ** 0.5, "bias": seeded_randn(3, 64), "r": seeded_randn(4, 14, 64),
         "out": torch.zeros(14, 64)}
    return i, lambda ops, t: {"y": ops.linear_rows(t.x[:, 0], t.w, t.bias, residual=t.r, out=t.out)}


@case("add/out=", inplace=("out",))
def _():
    return ({"a": seeded_randn(1, 3, 5, 8), "b": seeded_randn(2, 3, 5, 8), "out": torch.zeros(3, 5, 8)},          # (n % 4 == 0: the header)
            lambda ops, t: {"y": ops.add(t.a, t.b, out=t.out)})


for _op in ("window_attention", "window_attention_mm16"):
    @case(f"{_op}/out=", inplace=("out",))
    def _(op=_op):
        b, hs, w, c, s = 1, 14, 14, 32, 3
        i = {"qkv": seeded_randn(5, b, hs * w, 3 * c), "bias": _bias_pad(seeded_randn(6, 169, c // 32) * 0.2), **_shift_mask(hs, w, s),
             "out": torch.zeros(b, hs * w, c)}
        return i, lambda ops, t: {"y": getattr(ops, op)(t.qkv, t.bias, b, hs, w, c, s, 32 ** -0.5, t.tab, t.ids, out=t.out)}


@case("linear_gelu_bwd/50x96x64-accumulate", inplace=("gw", "gb"))
def _():
    m, n, k = 50, 96, 64
    z = seeded_randn(1, m, k)
    i = {"a": torch.nn.functional.gelu(z), "z": z, "w": seeded_randn(2, n, k) / k ** 0.5, "dy": seeded_randn(3, m, n),
         "gw": seeded_randn(4, n, k), "gb": seeded_randn(5, n)}

    def call(ops, t):
        dz, r1, r2 = ops.linear_gelu_bwd(t.a, t.z, t.w, t.dy, need_dz=True, need_dw=True, need_db=True, dw_out=t.gw, db_out=t.gb)
        assert r1 is None and r2 is None
        return {"dz": dz, "gw": t.gw, "gb": t.gb}
    return i, call


def _stage_inputs(warp):
    """nclips 2, T 2, 5 x 6 source, L = 4: in-range tables (the kernels clamp them anyway), two masks."""
    g = torch.Generator().manual_seed(11)
    nclips, t, hs, ws, L = 2, 2, 5, 6, 4
    i = {"frames": torch.randint(0, 256, (nclips, t, hs, ws, 3), generator=g, dtype=torch.uint8),
         "tab_a": torch.randint(0, hs, (nclips, L), generator=g, dtype=torch.int32),
         "tab_b": torch.randint(0, ws, (nclips, L), generator=g, dtype=torch.int32), "swap": torch.tensor([0, 1], dtype=torch.int32)}
    if warp:
        coef = torch.tensor([0, 1 << 21, 1 << 21, 0], dtype=torch.int32).repeat(nclips, L, 1)
        i.update(mode=torch.tensor([1, 2], dtype=torch.int32), pos_y=torch.randint(0, hs - 3, (nclips, L), generator=g, dtype=torch.int32),
                 pos_x=torch.randint(0, ws - 3, (nclips, L), generator=g, dtype=torch.int32), coef_y=coef, coef_x=coef.clone(),
                 affine=torch.tensor([[1.0, 0.0, 0.5, 0.0, 1.0, 0.5, 0.0, 0.0]] * nclips))
    i.update(masks=torch.randint(0, 2, (2, hs, ws), generator=g, dtype=torch.uint8), out=torch.zeros(nclips, t, 3, L, L),
             target=torch.zeros(nclips, L * L))
    return i


@case("augment_stage_u8/out=+target=", inplace=("out", "target"))
def _():
    def call(ops, t):
        out, target = ops.augment_stage_u8(t.frames, t.tab_a, t.tab_b, t.swap, masks=t.masks, out=t.out, target=t.target)
        return {"out": out, "target": target}
    return _stage_inputs(False), call


@case("augment_warp_u8/out=+target=", inplace=("out", "target"))
def _():
    def call(ops, t):
        out, target = ops.augment_warp_u8(t.frames, t.tab_a, t.tab_b, t.swap, t.mode, t.pos_y, t.pos_x, t.coef_y, t.coef_x, t.affine,
                                          masks=t.masks, out=t.out, target=t.target)
        return {"out": out, "target": target}
    return _stage_inputs(True), call


@case("clip_window_u8/out=", inplace=("out",))
def _():
    g = torch.Generator().manual_seed(12)
    i = {"frames": torch.randint(0, 256, (4, 5, 6, 3), generator=g, dtype=torch.uint8),
         "idx": torch.tensor([[0, 1, 2], [2, 3, 7]], dtype=torch.int32), "out": torch.zeros(2, 3, 3, 4, 8)}
    return i, lambda ops, t: {"out": ops.clip_window_u8(t.frames, t.idx, (4, 8), out=t.out)}


@case("mask_score_u8/gt+counts", inplace=("bank", "counts"))
def _():
    g = torch.Generator().manual_seed(13)
    nclips, npix, nbank = 3, 32, 4
    i = {"mask": torch.randint(0, 2, (nclips, 1, npix), generator=g, dtype=torch.uint8), "dest": torch.tensor([2, 0, 9], dtype=torch.int32),
         "bank": torch.zeros(nbank, npix, dtype=torch.uint8), "gt": torch.randint(0, 2, (nbank, npix), generator=g, dtype=torch.uint8) * 255,
         "counts": torch.zeros(nbank, 4, dtype=torch.int32)}

    def call(ops, t):
        bank, counts = ops.mask_score_u8(t.mask, t.dest, t.bank, gt=t.gt, counts=t.counts)
        return {"bank": bank, "counts": counts}
    return i, call


@case("frame_metrics/acc=", inplace=("acc",))
def _():
    i = {"counts": torch.tensor([[3, 5, 4, 6], [0, 0, 0, 0], [7, 7, 7, 7]], dtype=torch.int32), "acc": torch.ones(3, dtype=torch.float64)}
    return i, lambda ops, t: {"acc": ops.frame_metrics(t.counts, 3, 32, acc=t.acc, accumulate=True)}


@case("resize_bilinear_u8/out=", inplace=("out",))
def _():
    i = {"src": torch.randint(0, 256, (2, 5, 7), generator=torch.Generator().manual_seed(14), dtype=torch.uint8),
         "out": torch.zeros(2, 3, 4, dtype=torch.uint8)}
    return i, lambda ops, t: {"out": ops.resize_bilinear_u8(t.src, (3, 4), out=t.out)}


@case("copy_rows/pitched-rows", inplace=("dst",))
def _():
    """copy_rows called directly: 6 rows of 8 floats from a pitch of 16 into a pitch of 12.  One row less in either tensor and the last
    row runs past its storage; a strided tensor has no dense rows."""
    return ({"src": seeded_randn(61, 6, 16), "dst": torch.zeros(6, 12)},
            lambda ops, t: {"dst": ops.copy_rows(t.src, 16, t.dst, 12, 6, 8)})


# the staged device constants of one step, laid out as csrc/train.hip reads them (AdamHyper / SgdHyper / RmsHyper)
_ADAM_HYPER = [1.0 - 3e-5, 0.1, 0.999, 0.001, 1e-8, 3e-3, 0.0316, 0.5]
_SGD_HYPER = [0.5, 1e-2, 0.9, 3e-2]
_RMS_HYPER = [0.5, 1e-2, 0.99, 0.01, 1e-8, 0.9, 3e-3, 0.0]
_GATE = [0, 0, 0, 0, 0, 0, 0, 0]


def _flat(n=37):
    return {"p": seeded_randn(21, n), "g": seeded_randn(101, n)}


for _gated in (False, True):
    _sfx = "_gated_dev" if _gated else "_dev"

    @case(f"adamw_step{_sfx}/n37", inplace=("p", "m", "v"))
    def _(gated=_gated):
        i = dict(_flat(), m=torch.zeros(37), v=torch.zeros(37), hyper=torch.tensor(_ADAM_HYPER))
        if gated:
            i["gate"] = torch.tensor(_GATE, dtype=torch.int32)

        def call(ops, t):
            if gated:
                ops.adamw_step_gated_dev(t.p, t.g, t.m, t.v, t.hyper, t.gate)
            else:
                ops.adamw_step_dev(t.p, t.g, t.m, t.v, t.hyper)
            return {"p": t.p, "m": t.m, "v": t.v}
        return i, call

    @case(f"sgd_step{_sfx}/n37", inplace=("p", "buf"))
    def _(gated=_gated):
        i = dict(_flat(), buf=torch.zeros(37), hyper=torch.tensor(_SGD_HYPER))
        if gated:
            i["gate"] = torch.tensor(_GATE, dtype=torch.int32)

        def call(ops, t):
            if gated:
                ops.sgd_step_gated_dev(t.p, t.g, t.buf, t.hyper, t.gate, nesterov=True)
            else:
                ops.sgd_step_dev(t.p, t.g, t.buf, t.hyper, nesterov=True)
            return {"p": t.p, "buf": t.buf}
        return i, call

    @case(f"rmsprop_step{_sfx}/n37", inplace=("p", "sq", "buf"))
    def _(gated=_gated):
        i = dict(_flat(), sq=torch.zeros(37), buf=torch.zeros(37), hyper=torch.tensor(_RMS_HYPER))
        if gated:
            i["gate"] = torch.tensor(_GATE, dtype=torch.int32)

        def call(ops, t):
            if gated:
                ops.rmsprop_step_gated_dev(t.p, t.g, t.sq, t.buf, t.hyper, t.gate)
            else:
                ops.rmsprop_step_dev(t.p, t.g, t.sq, t.buf, t.hyper)
            return {"p": t.p, "sq": t.sq, "buf": t.buf}
        return i, call


@case("update_gate/adamw+sgd", inplace=("gate", "h_adam", "applied"))
def _():
    i = {"stats": torch.tensor([1.5, 1.0, 0.0, 0.0]), "gate": torch.tensor(_GATE, dtype=torch.int32),
         "h_adam": torch.tensor(_ADAM_HYPER), "h_sgd": torch.tensor(_SGD_HYPER), "applied": torch.tensor([4, 4], dtype=torch.int64),
         "adam_raw": torch.tensor([3e-3, 0.9, 0.999, 5.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)}

    def call(ops, t):
        ops.update_gate([t.stats], t.gate, [t.h_adam, t.h_sgd], ["AdamW", "SGD"], t.applied, t.adam_raw)
        return {"gate": t.gate, "h_adam": t.h_adam, "applied": t.applied}
    return i, call


@case("grad_norm/partial+finish-n10000", inplace=("partials", "stats", "hyper"))
def _():
    n = 10000
    npart = min(2048, -(-n // 4096))             # csrc/train.hip, grad_norm_grid: one partial per 4096 elements, at most 2048
    i = {"g": seeded_randn(31, n), "partials": torch.zeros(2 * npart), "hyper": torch.tensor(_ADAM_HYPER), "stats": torch.zeros(5)}

    def call(ops, t):
        if ops.grad_norm_partials(n) != npart:
            raise AssertionError(f"the case counts {npart} partials for {n} elements, the library {ops.grad_norm_partials(n)}")
        ops.grad_norm_partial(t.g, t.partials)
        ops.grad_norm_finish([t.partials], [n], [t.hyper], ["AdamW"], t.stats, max_norm=1.0)
        return {"partials": t.partials, "stats": t.stats, "hyper": t.hyper}
    return i, call


ALL_CASES = list(CASES) + EXTRA


# ================================================================================================ the mutations
def _is_nhwc(v):
    if v.dim() != 4 or v.is_contiguous():
        return False
    b, c, h, w = v.shape
    return v.stride() == (h * w * c, 1, w * c, c)


def mutate(v, kind, to_dev=lambda t: t):
    """The mutated twin of the CPU input v, placed with to_dev, or None where the mutation cannot be formed (counted by the callers)."""
    if kind == "dtype":
        return to_dev(v.to(WIDER[v.dtype]))
    if kind == "host":
        return v.clone(memory_format=torch.preserve_format)
    if kind == "strided":
        if v.dim() == 0:
            return None
        m = to_dev(torch.zeros(*v.shape[:-1], 2 * v.shape[-1], dtype=v.dtype))[..., ::2]      # sliced on the device: a copy would be dense
        m.copy_(v)
        return None if m.is_contiguous() else m                     # (a tensor of one element is contiguous whatever its strides)
    if kind == "nchw":
        return to_dev(v.contiguous()) if _is_nhwc(v) else None
    if kind == "short":
        d = next((d for d, s in enumerate(v.shape) if s > 1), None)
        if d is None:
            return None
        m = v.narrow(d, 0, v.shape[d] - 1)
        return to_dev(_nhwc(m) if _is_nhwc(v) else m.contiguous().clone())
    raise ValueError(kind)


def _op(case_):
    return case_.id.split("/")[0]


def _build_all(cases):
    """[(case, inputs)]; the one case whose build() needs the built library is left out where there is no library."""
    out = []
    for c in cases:
        try:
            out.append((c, c.build()[0]))
        except (OSError, RuntimeError):
            if c.id != LIBRARY_CASE:
                raise
    return out


# ================================================================================================ CPU: the recorder itself
def _fake_ops():
    """A stand-in for mumpy_hip.ops whose wrappers accept CPU tensors: one clean op, and one wrapper per way of going wrong."""
    fake = types.SimpleNamespace()
    fake._p = lambda t: None if t is None else t.data_ptr()

    def _call(name, *args, work=0.0):
        raise AssertionError("the recorder must never reach the library")
    fake._call = _call

    def _read(t, n):
        if t.dtype != torch.float32 or t.numel() != n:
            raise RuntimeError("operand")
        return t if t.is_contiguous() else t.contiguous()

    def scale(x, s, acc):                                    # clean: x read (copied when strided), s measured, acc taken in place
        x = _read(x, x.numel())
        s = _read(s, x.shape[-1])
        if acc.dtype != torch.float32 or acc.shape != x.shape or not acc.is_contiguous():
            raise RuntimeError("acc")
        fake._call("fake_scale", fake._p(x), fake._p(s), fake._p(acc), x.numel() // x.shape[-1], x.shape[-1], 0.5)
        return acc

    def hands_short(x, s, acc):                              # s is never measured against the row length
        fake._call("fake_scale", fake._p(_read(x, x.numel())), fake._p(s.contiguous()), fake._p(acc), x.numel() // x.shape[-1], x.shape[-1], 0.5)
        return acc

    def hands_dtype(x, s, acc):                              # s is handed at whatever width it has
        if s.numel() != x.shape[-1]:
            raise RuntimeError("operand")
        fake._call("fake_scale", fake._p(_read(x, x.numel())), fake._p(s.contiguous()), fake._p(acc), x.numel() // x.shape[-1], x.shape[-1], 0.5)
        return acc

    def copies_inplace(x, s, acc):                           # the accumulate buffer goes through a copying check
        x = _read(x, x.numel())
        fake._call("fake_scale", fake._p(x), fake._p(_read(s, x.shape[-1])), fake._p(_read(acc, x.numel())), x.numel() // x.shape[-1], x.shape[-1], 0.5)
        return None

    def raises_late(x, s, acc):                              # the second launch's operand is checked after the first launch
        x = _read(x, x.numel())
        if acc.dtype != torch.float32 or acc.shape != x.shape or not acc.is_contiguous():
            raise RuntimeError("acc")
        fake._call("fake_first", fake._p(x), fake._p(acc), x.numel())
        fake._call("fake_scale", fake._p(x), fake._p(_read(s, x.shape[-1])), fake._p(acc), x.numel() // x.shape[-1], x.shape[-1], 0.5)
        return acc

    fake.scale, fake.hands_short, fake.hands_dtype, fake.copies_inplace, fake.raises_late = scale, hands_short, hands_dtype, copies_inplace, raises_late
    return fake


def _audit(monkeypatch, ops, call, inputs, inplace, to_dev, on_gpu, launch=None, report=None, op=None, partial=None, trace=None):
    """Phase 1 (and phase 2 when `launch` is given) of one case -> the list of failures."""
    failures, tally = [], Counter()

    def place(name=None, kind=None):
        t = _T({k: to_dev(v.clone(memory_format=torch.preserve_format)) for k, v in inputs.items()})
        if name is not None:
            t[name] = mutate(inputs[name], kind, to_dev)
        return t

    t0 = place()
    valid, _, error, _ = HA.record(monkeypatch, ops, lambda: call(ops, t0), on_gpu)
    assert error is None and valid, f"the valid call was refused or launched nothing: {error}"
    verdict, problems = HA.judge(valid, valid, None, "valid")
    failures += [f"valid call: {p}" for p in problems + HA.inplace_problems(valid, {k: t0[k] for k in inplace})]
    cleared = []
    for name, v in inputs.items():
        for kind in KINDS:
            if mutate(v, kind) is None:
                tally[kind, "skipped"] += 1
                continue
            t = place(name, kind)
            got, _, error, launched = HA.record(monkeypatch, ops, lambda: call(ops, t), on_gpu)
            verdict, problems = HA.judge(valid, got, error, kind, launched)
            if error is None:
                problems = problems + HA.inplace_problems(got, {k: t[k] for k in inplace})
            if trace is not None:
                trace.append((name, kind, verdict, "" if error is None else str(error), list(problems)))
            if (op, name, kind) in UNCHECKABLE:
                if verdict == "same launch" and problems and all("bytes, the launch addresses" in p for p in problems):
                    tally[kind, "uncheckable"] += 1
                    continue
                problems = [f"listed in UNCHECKABLE, but judged {verdict!r} with {problems}: take it off the list"]
            tally[kind, verdict] += 1
            failures += [f"{name} / {kind}: {p}" for p in problems]
            if verdict == "same launch" and not problems and name not in inplace:
                cleared.append((name, kind))
    if report is not None:
        report.update(tally)
    if launch is None or failures:
        return failures
    want = launch(call, place())                                                      # phase 2: real launches of cleared triples only
    for name, kind in cleared:
        t = place(name, kind)
        before = _bits(t[name])
        got = launch(call, t)
        if not torch.equal(_bits(t[name]), before):
            failures.append(f"{name} / {kind}: the caller's tensor was modified")
        for out in want:
            keep = slice(None) if out not in (partial or {}) else _outside(want[out].shape, partial[out][0])     # (a region the op leaves unwritten)
            if got[out].shape != want[out].shape or got[out].dtype != want[out].dtype or \
                    not torch.equal(_bits(got[out][keep]), _bits(want[out][keep])):
                failures.append(f"{name} / {kind}: output {out} differs from the valid call's (the wrapper's conversion is not faithful)")
    return failures


def _bits(t):
    """The elements of t as bytes on the CPU (torch.equal on floats calls NaN != NaN and -0.0 == 0.0)."""
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


_FAKE_INPUTS = {"x": seeded_randn(1, 6, 5), "s": seeded_randn(2, 5), "acc": seeded_randn(3, 6, 5)}


def _fake_audit(monkeypatch, op):
    fake = _fake_ops()
    return _audit(monkeypatch, fake, lambda ops, t: {"y": getattr(ops, op)(t.x, t.s, t.acc)}, _FAKE_INPUTS, ("acc",), lambda t: t, lambda t: True)


def test_recorder_passes_a_clean_op_and_launches_nothing(monkeypatch):
    assert _fake_audit(monkeypatch, "scale") == []
    fake = _fake_ops()
    log, result, error, _ = HA.record(monkeypatch, fake, lambda: fake.scale(*(_FAKE_INPUTS[k].clone() for k in "x s acc".split())), lambda t: True)
    assert error is None and [launch.name for launch in log] == ["fake_scale"] and log[0].scalars == ("ptr", "ptr", "ptr", 6, 5, 0.5)
    assert [(p.pos, p.dtype, p.contiguous, p.nbytes) for p in log[0].ptrs] == [(0, torch.float32, True, 120), (1, torch.float32, True, 20),
                                                                               (2, torch.float32, True, 120)]
    assert fake._call.__name__ == "_call" and fake.scale.__name__ == "scale"           # the module has its own functions back
    with pytest.raises(AssertionError, match="never reach the library"):
        fake.scale(*(_FAKE_INPUTS[k].clone() for k in "x s acc".split()))


def test_a_shorter_buffer_fails_rule_3(monkeypatch):
    failures = _fake_audit(monkeypatch, "hands_short")
    assert any(f.startswith("s / short: fake_scale argument 1: handed 16 bytes, the launch addresses 20") for f in failures), failures


def test_another_dtype_fails_rule_3(monkeypatch):
    failures = _fake_audit(monkeypatch, "hands_dtype")
    assert any(f.startswith("s / dtype: fake_scale argument 1: handed torch.float64, the launch reads / writes torch.float32") for f in failures), failures


def test_a_copied_inplace_buffer_fails_rule_4(monkeypatch):
    failures = _fake_audit(monkeypatch, "copies_inplace")
    assert failures == ["acc / strided: in-place input acc: no launch was handed the caller's storage (a copy: the result is lost)"]


def test_a_refusal_after_the_first_launch_fails_rule_1(monkeypatch):
    failures = _fake_audit(monkeypatch, "raises_late")
    assert failures and all("refused only after 1 recorded launch(es) (first fake_first)" in f for f in failures), failures
    assert {f.split(":")[0] for f in failures} == {"s / dtype", "s / short"}


def test_a_pointer_table_is_resolved_through_the_addresses_handed_out(monkeypatch):
    import ctypes
    fake = _fake_ops()
    a, b = torch.zeros(4), torch.zeros(6, dtype=torch.float64)

    def packed():
        table = (ctypes.c_void_p * 2)(fake._p(a), fake._p(b))
        fake._call("fake_table", table, (ctypes.c_int64 * 2)(4, 6), 2, None)
    log, _, error, _ = HA.record(monkeypatch, fake, packed, lambda t: True)
    assert error is None and log[0].scalars == (("ptrs", 2), (4, 6), 2, None)
    assert [(p.pos, p.dtype, p.nbytes) for p in log[0].ptrs] == [((0, 0), torch.float32, 16), ((0, 1), torch.float64, 48)]
    with pytest.raises(AssertionError, match="did not pass through ops._p"):
        HA.record(monkeypatch, fake, lambda: fake._call("fake", a), lambda t: True)


# ================================================================================================ CPU: the table and its coverage
def test_only_the_listed_arguments_never_hold_more_than_one_element():
    most = Counter()
    for c, inputs in _build_all(ALL_CASES):
        for k, v in inputs.items():
            most[_op(c), k] = max(most[_op(c), k], v.numel())
    assert {pair for pair, n in most.items() if n == 1} == set(ONE_ELEMENT_ONLY)


def test_the_list_of_undecidable_triples_does_not_grow():
    """Five ops, one argument, one mutation: the window-attention family's mask_tab one pattern short.  Anything else is a check that
    is missing in ops.py, not an entry for this list."""
    assert UNCHECKABLE == {(op, "tab", "short") for op in ("window_attention", "window_attention_bf16", "window_attention_bf16mm",
                                                           "window_attention_mm16", "window_attention_bwd")}
    carriers = [c.id for c, inputs in _build_all(ALL_CASES) if "tab" in inputs and (_op(c), "tab", "short") in UNCHECKABLE]
    assert len(carriers) == 8, carriers                      # the eight triples the sweep reports as "uncheckable"


def test_every_mutation_reaches_every_argument():
    built = _build_all(ALL_CASES)
    reach, short = {}, Counter()
    for c, inputs in built:
        assert set(c.inplace) <= set(inputs), c.id
        for k, v in inputs.items():
            assert v.dtype in WIDER, (c.id, k, v.dtype)
            reach.setdefault((_op(c), k), set())
            for kind in KINDS:
                m = mutate(v, kind)
                if m is not None:
                    reach[_op(c), k].add(kind)
                    assert m.shape == v.shape or kind == "short", (c.id, k, kind)
                    assert kind != "strided" or not m.is_contiguous()
                    assert kind != "short" or m.numel() < v.numel()
            short["skipped" if mutate(v, "short") is None else "formed"] += 1
    nhwc_pairs = {(_op(c), k) for c, inputs in built for k, v in inputs.items() if _is_nhwc(v)}
    for pair, kinds in reach.items():
        want = set(KINDS) - ({"nchw"} if pair not in nhwc_pairs else set())
        if pair in ONE_ELEMENT_ONLY:
            want -= {"short", "strided"}
        assert kinds >= want, f"{pair}: no case carries a {sorted(want - kinds)} mutation of this argument"
    share = short["skipped"] / (short["skipped"] + short["formed"])
    print(f"short mutations skipped (tensors of one element): {short['skipped']} of {short['skipped'] + short['formed']} = {100 * share:.1f} %")
    assert share <= 0.10


def test_case_ids_are_unique():
    ids = [c.id for c in ALL_CASES]
    assert len(set(ids)) == len(ids)


# ================================================================================================ GPU: the sweep
_REPORT = Counter()


@gpu
@pytest.mark.parametrize("case_", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_handoff(case_, monkeypatch):
    from mumpy_hip import ops
    dev = torch.device("cuda:0")
    inputs, call = case_.build()

    def launch(call, t):
        out = call(ops, t)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}
    failures = _audit(monkeypatch, ops, call, inputs, case_.inplace, lambda t: t.to(dev), lambda t: t.is_cuda, launch, _REPORT, _op(case_), case_.partial)
    assert not failures, f"{case_.id}: {len(failures)} hand-off failure(s):\n  " + "\n  ".join(failures)


@gpu
def test_zz_report_the_share_of_redimensioned_verdicts():
    """Printed, not capped: how many `short` mutations moved a dimension instead of being refused (runs after the sweep)."""
    short = {v: n for (k, v), n in _REPORT.items() if k == "short" and v != "skipped"}
    total = sum(short.values())
    print(f"short mutations: {short}; re-dimensioned {short.get('re-dimensioned', 0)} of {total}"
          + (f" = {100 * short.get('re-dimensioned', 0) / total:.1f} %" if total else ""))
    print("all verdicts:", dict(sorted(_REPORT.items())))


# ================================================================================================ GPU: two numeric regressions
def _smallest_folding_block(ops):
    """(s, c, kp) of the smallest global Block input (s, 3, c), c a multiple of the 64-wide heads, for which the host query says
    that both the producer linear(..., emit_stats=True) at (3 s, c, kp) and the block's folded qkv GEMM at (3 s, 3 c, c) run on the
    statistics kernel: the smallest (m, n, k) at which Block.forward would fold."""
    kp = ops.LN_FOLD_MIN_K                                                # emit_stats asks for K >= LN_FOLD_MIN_K
    found = []
    for c in (256, 384, 512, 768, 1024, 1536, 2048):
        s = next((s for s in range(64, 8192, 64) if ops.linear_ln_tiles(3 * s, c, kp) > 0 and ops.linear_ln_tiles(3 * s, 3 * c, c) > 0), None)
        if s is not None:
            found.append((s * c, s, c, kp))
    assert found, "no shape runs on the persistent kernel: is LayerNorm folding off?"
    return min(found)[1:]


@gpu
def test_ln_fold_statistics_do_not_survive_an_overwrite(monkeypatch):
    """x = linear(..., emit_stats=True) carries {mean, M2} of its rows; ops.add(a, b, out=x) rewrites x.  The statistics must be gone,
    and the block-level path that would have folded -- models.modules.blocks.Block.forward, which folds norm1 into its qkv GEMM when
    ln_stats_of(x) is there -- must compute LayerNorm + Linear of the NEW x: its qkv against float64 from the same fp32 values at
    test_layernorm_folded_into_its_gemms' bar of 5e-5, and the whole block bit for bit what it gives for a plain copy of x.  The
    folded GEMM fed the OLD statistics misses that bar by orders of magnitude: that is what used to happen."""
    import torch.nn.functional as F
    from conftest import rel_err
    from models.modules.blocks import Block
    from mumpy_hip import ops
    from weight_fill import fill_module_
    dev = torch.device("cuda:0")
    s_, c, kp = _smallest_folding_block(ops)
    print(f"smallest folding block input: ({s_}, 3, {c}) from a producer with K = {kp}")
    g = torch.Generator().manual_seed(s_ + c)
    h, wp, bp = torch.randn(s_, 3, kp, generator=g), torch.randn(c, kp, generator=g) / kp ** 0.5, torch.randn(c, generator=g)
    a, b = torch.randn(s_, 3, c, generator=g) * 3.0 + 2.0, torch.randn(s_, 3, c, generator=g)
    blk = fill_module_(Block(c, c // 64, 4 * c, 0.0, 0.0).eval(), "handoff_blk/").to(dev)
    calls = []
    for name in ("linear", "linear_ln"):                                  # what the block's first GEMM is, and what it returns
        def spy(*args, _fn=getattr(ops, name), _name=name, **kw):
            out = _fn(*args, **kw)
            calls.append((_name, out))
            return out
        monkeypatch.setattr(ops, name, spy)

    def block(x):
        del calls[:]
        with torch.no_grad():
            y = blk(x)
        return y, calls[0]

    hd, wpd, bpd = h.to(dev), wp.to(dev), bp.to(dev)
    x = ops.linear(hd, wpd, bpd, emit_stats=True)
    old = ops.ln_stats_of(x)
    assert old is not None and block(x)[1][0] == "linear_ln", "the block must fold this shape for the test to mean anything"
    assert ops.add(a.to(dev), b.to(dev), out=x) is x
    assert ops.ln_stats_of(x) is None and torch.equal(x.cpu(), a + b)
    y, (first, qkv) = block(x)
    y_plain, (first_plain, _) = block((a + b).to(dev))
    assert first == first_plain == "linear" and torch.equal(y, y_plain)
    n1, lin = blk.norm1, blk.attn.qkv
    ref = F.layer_norm((a + b).double(), (c,), n1.weight.detach().cpu().double(), n1.bias.detach().cpu().double(), n1.eps) @ lin.weight.detach().cpu().double().t() \
        + lin.bias.detach().cpu().double()
    wg, cs, bpr = ops.fold_ln_weights(lin.weight, lin.bias, n1.weight, n1.bias)
    e_new, e_stale = rel_err(qkv.cpu(), ref), rel_err(ops.linear_ln(x, old, wg, cs, bpr, n1.eps).cpu(), ref)
    print(f"the block's qkv of the new x: {e_new:.2e}; the fold with the stale statistics: {e_stale:.2e}")
    assert e_new < 5e-5 and e_stale > 1e-2
    monkeypatch.undo()
    # every op that writes into a caller's tensor drops them; linear(..., out=, emit_stats=True) leaves the fresh ones
    m = 3 * s_
    for rewrite in (lambda t: ops.linear(hd, wpd, bpd, out=t), lambda t: ops.layernorm(a.to(dev), n1.weight, n1.bias, out=t),
                    lambda t: ops.copy_rows(a.to(dev), c, t, c, m, c)):
        t = ops.linear(hd, wpd, bpd, emit_stats=True)
        assert ops.ln_stats_of(t) is not None
        rewrite(t)
        assert ops.ln_stats_of(t) is None
    t = ops.linear(hd, wpd, bpd, emit_stats=True)
    stale = ops.ln_stats_of(t)
    ops.linear(hd * 2.0, wpd, bpd, out=t, emit_stats=True)
    assert ops.ln_stats_of(t) is not None and ops.ln_stats_of(t) is not stale


def _acc_layernorm_bwd():
    import torch.nn.functional as F
    rows, c = 37, 128
    x, g, dy = seeded_randn(1, rows, c) * 2 + 0.5, 1 + 0.1 * seeded_randn(2, c), seeded_randn(4, rows, c)
    gr, br = g.double().requires_grad_(True), torch.zeros(c, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x.double(), (c,), gr, br, 1e-5).backward(dy.double())

    def run(ops, dev, s):
        assert ops.layernorm_bwd(x.to(dev), g.to(dev), dy.to(dev), 1e-5, dg_out=s["dg_out"], db_out=s["db_out"])[1:] == (None, None)
    return {"dg_out": (c,), "db_out": (c,)}, run, {"dg_out": gr.grad, "db_out": br.grad}, 2e-5      # test_hip_layernorm_bwd


def _acc_gn_bwd():
    import torch.nn.functional as F
    b, c, h, w, groups = 1, 64, 7, 9, 8
    z, g, bt = seeded_randn(30, b, c, h, w) * 2 + 0.3, 1 + 0.1 * seeded_randn(31, c), 0.1 * seeded_randn(32, c)
    dy = seeded_randn(33, b, c, h, w)
    gr, br = g.double().requires_grad_(True), bt.double().requires_grad_(True)
    F.relu(F.group_norm(z.double(), groups, gr, br, 1e-5)).backward(dy.double())

    def run(ops, dev, s):
        zd, partial, nsplit = ops.gn_stats(_nhwc(z).to(dev), groups)
        r = ops.gn_bwd(zd, (partial, nsplit), g.to(dev), bt.to(dev), _nhwc(dy).to(dev), groups, 1e-5, ops.ACT_RELU, dg_out=s["dg_out"], db_out=s["db_out"])
        assert r[1] is None and r[2] is None
    return {"dg_out": (c,), "db_out": (c,)}, run, {"dg_out": gr.grad, "db_out": br.grad}, 5e-5      # test_hip_groupnorm_relu_bwd


def _acc_linear_bwd():
    m, n, k = 50, 96, 96
    x, w, dy = seeded_randn(1, m, k), seeded_randn(2, n, k) / k ** 0.5, seeded_randn(3, m, n)

    def run(ops, dev, s):
        assert ops.linear_bwd(x.to(dev), w.to(dev), dy.to(dev), need_dx=False, need_dw=True, need_db=True, dw_out=s["dw_out"],
                              db_out=s["db_out"]) == (None, None, None)
    return {"dw_out": (n, k), "db_out": (n,)}, run, {"dw_out": dy.double().t() @ x.double(), "db_out": dy.double().sum(0)}, 1e-5


def _acc_linear_gelu_bwd():
    m, n, k = 50, 96, 64
    z, w, dy = seeded_randn(1, m, k), seeded_randn(2, n, k) / k ** 0.5, seeded_randn(3, m, n)
    a = torch.nn.functional.gelu(z)

    def run(ops, dev, s):
        r = ops.linear_gelu_bwd(a.to(dev), z.to(dev), w.to(dev), dy.to(dev), need_dz=False, need_dw=True, need_db=True, dw_out=s["dw_out"],
                                db_out=s["db_out"])
        assert r == (None, None, None)
    return {"dw_out": (n, k), "db_out": (n,)}, run, {"dw_out": dy.double().t() @ a.double(), "db_out": dy.double().sum(0)}, 2e-5


def _acc_conv2d_wgrad():
    import torch.nn.functional as F
    b, cin, cout, h, w = 2, 64, 32, 9, 11
    x, dy = seeded_randn(1, b, cin, h, w), seeded_randn(2, b, cout, h, w)
    wr = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, padding=1).backward(dy.double())

    def run(ops, dev, s):
        assert ops.conv2d_wgrad(_nhwc(x).to(dev), _nhwc(dy).to(dev), 3, 3, dw_out=s["dw_out"]) is None
    return {"dw_out": (cout, 3, 3, cin)}, run, {"dw_out": wr.grad.permute(0, 2, 3, 1)}, 1e-5        # test_hip_conv2d_wgrad_one_launch


def _acc_window_attention_bwd():
    from models.modules.swinTransformer import build_shift_mask, relative_position_index
    from oracle import mumpy_oracle as O
    b, hs, w, c, shift = 2, 14, 14, 64, 3
    qkv, table, dout = seeded_randn(20, b, hs * w, 3 * c), seeded_randn(21, 169, c // 32) * 0.2, seeded_randn(22, b, hs * w, c)
    idx = relative_position_index(7, 7)
    mask = build_shift_mask(hs, w, 7, shift)
    tr = table.double().requires_grad_(True)
    O.window_attention_core(qkv.double(), tr, idx, hs, w, shift, mask.double()).backward(dout.double())

    def run(ops, dev, s):
        tab, ids = ops.compact_attn_mask(mask.to(dev))
        idx_d = idx.to(dev)
        d, none = ops.window_attention_bwd(qkv.to(dev), dout.to(dev), ops.expand_relpos_bias(table.to(dev), ops.rel_index32(idx_d)),
                                           ops.rel_index32(idx_d), b, hs, w, c, shift, 32 ** -0.5, tab, ids, dtable_out=s["dtable_out"],
                                           rel_csr=ops.rel_index_csr(idx_d))
        assert none is None
    return {"dtable_out": (169, c // 32)}, run, {"dtable_out": tr.grad}, 2e-5                       # test_hip_window_attention_bwd_vs_oracle


ACCUMULATORS = {"layernorm_bwd": _acc_layernorm_bwd, "gn_bwd": _acc_gn_bwd, "linear_bwd": _acc_linear_bwd,
                "linear_gelu_bwd": _acc_linear_gelu_bwd, "conv2d_wgrad": _acc_conv2d_wgrad, "window_attention_bwd": _acc_window_attention_bwd}


@gpu
@pytest.mark.parametrize("op", list(ACCUMULATORS))
def test_accumulate_buffers_are_used_where_they_are_or_refused(op):
    """FlatAdamW's layout: each gradient slot is a contiguous slice of one flat buffer.  The slice receives old + gradient (float64
    reference from the same fp32 inputs, at the bar of the op's own test), the rest of the flat buffer keeps its bits, and the same
    call with a strided view of the buffer raises before anything is launched: the flat buffer keeps ALL its bits."""
    from conftest import rel_err
    from mumpy_hip import ops
    dev = torch.device("cuda:0")
    shapes, run, refs, bar = ACCUMULATORS[op]()
    sizes = {k: int(torch.Size(s).numel()) for k, s in shapes.items()}
    offsets, end = {}, 64
    for k, n in sizes.items():                                            # 256-byte aligned slots with room for the strided twin, gaps between them
        offsets[k], end = end, end + (2 * n + 127) // 64 * 64
    flat0 = seeded_randn(77, end + 64)
    flat = flat0.to(dev)
    run(ops, dev, {k: flat[offsets[k]:offsets[k] + n].view(shapes[k]) for k, n in sizes.items()})
    torch.cuda.synchronize()
    got, rest = flat.cpu(), torch.ones(flat0.numel(), dtype=torch.bool)
    for k, n in sizes.items():
        sl = slice(offsets[k], offsets[k] + n)
        rest[sl] = False
        err = rel_err(got[sl].view(shapes[k]), flat0[sl].view(shapes[k]).double() + refs[k])
        print(f"{op} {k}: old + gradient within {err:.2e} (bar {bar:.0e})")
        assert err < bar, (k, err)
        assert rel_err(got[sl].view(shapes[k]).double() - flat0[sl].view(shapes[k]).double(), refs[k]) < 10 * bar      # (a gradient, not mostly `old`)
    assert torch.equal(_bits(got[rest]), _bits(flat0[rest])), "the call wrote outside its slots"
    for bad in sizes:                                                     # one strided slot at a time
        flat = flat0.to(dev)
        slots = {k: flat[offsets[k]:offsets[k] + n].view(shapes[k]) for k, n in sizes.items()}
        slots[bad] = flat[offsets[bad]:offsets[bad] + 2 * sizes[bad]].view(*shapes[bad][:-1], 2 * shapes[bad][-1])[..., ::2]
        assert slots[bad].shape == torch.Size(shapes[bad]) and not slots[bad].is_contiguous()
        with pytest.raises(RuntimeError, match="contiguous"):
            run(ops, dev, slots)
        torch.cuda.synchronize()
        assert torch.equal(_bits(flat.cpu()), _bits(flat0)), f"a refused call ({bad} strided) touched the flat buffer"
