"""GPU: training with per-clip cross-view pairing (include/mumpy_hip_ext9.h, groups= on ops.deform_sample_bwd /
ops.deform_attention_bwd, the Grouped autograd functions, encoder_train(coupling="clip")).

The oracle of every grouped backward kernel is the FROZEN entry run on each group's slice of the batch, as in
tests/test_clip_coupling.py for the forward: a grouped launch with G groups must give, bit for bit, the concatenation of the frozen
op's results on the G slices, G = 1 must be the frozen op on the whole batch, and so must any G when r = 1.  (dpos is the exception:
its r slots are summed by torch, which promises no order: the project's single-operator bar, 5e-5, holds there.)  Module and whole
model are held to autograd on the CPU oracle run clip by clip with the gradients summed -- and the batch-coupled tape of the same
library must MISS that reference, or the input could not tell the two pairings apart.

Kernel shapes, window form (B clips, q windows per clip, r, C): (2,1,3,96), (3,2,3,192), (2,4,5,96), (4,2,1,96); the attention
backwards also (3,1,3,32) -- one head, three idle waves in every block -- and (3,1,5,64) -- 30 kv units, a ragged last block."""
import pytest
import torch

import guarded_alloc as GA
from conftest import rel_err
from weight_fill import fill_module_, seeded_randn

pytestmark = pytest.mark.gpu
TIGHT = 5e-5        # single operators in fp32 (tests/test_hip_parity.py; the bar of test_hip_deform_sample_bwd on dpos)
SCALE = 32 ** -0.5

if torch.cuda.is_available():
    from oracle import mumpy_oracle as O
    DEV = torch.device("cuda:0")

SAMPLE_CASES = [(2, 1, 3, 96), (3, 2, 3, 192), (2, 4, 5, 96), (4, 2, 1, 96)]
ATTN_CASES = SAMPLE_CASES + [(3, 1, 3, 32), (3, 1, 5, 64)]
ENTRY_CASES = ([("sample", *s) for s in SAMPLE_CASES] + [("attention", *s) for s in ATTN_CASES]
               + [("attention_mm16", *s) for s in ATTN_CASES])
OUTPUTS = {"sample": ("dx2", "dpos"), "attention": ("dq", "dkv"), "attention_mm16": ("dq", "dkv")}


def _ops():
    from mumpy_hip import ops
    return ops


# ------------------------------------------------------------------------------------------------ the three entries
def _inputs(entry, b, nqc, r, c):
    """CPU inputs of one launch in window form: b nqc q windows, b nqc r kv windows, clip-major.  The sampling positions reach
    outside the window."""
    nq, nkv = b * nqc, b * nqc * r
    seed = 7000 + 1000 * b + 100 * nqc + 10 * r + c
    if entry == "sample":
        return {"x2": seeded_randn(seed + 1, nkv, 49, c), "pos": (seeded_randn(seed + 2, nq, 3, 49, 2) * 0.7).clamp(-1.3, 1.3),
                "ds": seeded_randn(seed + 3, nkv, 49, c)}
    return {"q": seeded_randn(seed + 4, nq, 49, c), "kv": seeded_randn(seed + 5, nkv, 49, 2 * c), "dout": seeded_randn(seed + 6, nq, 49, c)}


def _launch(entry, t, r, groups):
    """The op on tensors t (a dict of device tensors) -> {name: output}; groups=None calls it without the keyword, as before it
    existed."""
    ops = _ops()
    kw = {} if groups is None else {"groups": groups}
    if entry == "sample":
        out = ops.deform_sample_bwd(t["x2"], t["pos"], t["ds"], **kw)
    else:
        out = ops.deform_attention_bwd(t["q"], t["kv"], t["dout"], r, SCALE, math="bf16" if entry.endswith("mm16") else "fp32", **kw)
    return dict(zip(OUTPUTS[entry], out))


def _slice(t, g, groups):
    """Group g's share of the inputs: its clips' windows (copies: fresh, aligned buffers)."""
    out = {}
    for k, v in t.items():
        n = v.shape[0] // groups
        out[k] = v[g * n:(g + 1) * n].clone()
    return out


def _frozen_by_slices(entry, t, r, groups):
    parts = [_launch(entry, _slice(t, g, groups), r, None) for g in range(groups)]
    return {k: torch.cat([p[k] for p in parts]) for k in OUTPUTS[entry]}


def _guarded(monkeypatch, entry, cpu, r, groups):
    """The grouped launch under tests/guarded_alloc.py: bands intact, every element of the outputs written, inputs unchanged.
    dpos comes out of a torch reduction of the guarded slot buffer, which the proxy cannot see: the only output allowed to live
    outside a guarded block (an unwritten slot would reach it as NaN under the first pattern).  -> the outputs of each guarded run (one per pass of GA.PASSES)."""
    def body(guard):
        return _launch(entry, {k: guard.tensor(v) for k, v in cpu.items()}, r, groups), (), None
    runs, unguarded = GA.run_both(monkeypatch, [_ops()], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded <= {"dpos"}
    return runs


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b) and bool(torch.isfinite(a).all())


def _assert_is(entry, got, want):
    """Bit for bit, except dpos (torch's reduction over r): within the single-operator bar."""
    for k in OUTPUTS[entry]:
        if k == "dpos":
            e = rel_err(got[k].cpu(), want[k].cpu())
            print(f"{entry} dpos rel_err {e:.3e}")
            assert got[k].shape == want[k].shape and bool(torch.isfinite(got[k]).all()) and e <= TIGHT
        else:
            assert _same(got[k], want[k]), k


@pytest.mark.parametrize("entry,b,nqc,r,c", ENTRY_CASES, ids=lambda v: str(v))
def test_grouped_backward_is_the_frozen_op_clip_by_clip(monkeypatch, entry, b, nqc, r, c):
    cpu = _inputs(entry, b, nqc, r, c)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    per_clip = _frozen_by_slices(entry, dev, r, b)                         # the frozen op, one call per clip
    whole = _launch(entry, dev, r, None)                                   # the frozen op on the batch: coupled
    for out in _guarded(monkeypatch, entry, cpu, r, b):                    # G = B
        _assert_is(entry, out, per_clip)
    one = _launch(entry, dev, r, 1)                                        # G = 1
    assert all(_same(one[k], whole[k]) for k in OUTPUTS[entry])
    grouped = _launch(entry, dev, r, b)
    for k in OUTPUTS[entry]:
        if r == 1:                                                         # the two rules coincide
            assert _same(per_clip[k], whole[k]) and _same(grouped[k], whole[k]), k
        else:                                                              # ... and otherwise the case tells them apart
            assert not torch.equal(grouped[k], whole[k]), k


@pytest.mark.parametrize("c", [96, 192])
@pytest.mark.parametrize("entry", sorted(OUTPUTS))
def test_backward_two_groups_of_two_clips(monkeypatch, entry, c):
    """B = 4, G = 2 (r = 3, two q windows per clip): the frozen op on the two halves -- neither per-clip nor batch-wide."""
    b, nqc, r = 4, 2, 3
    cpu = _inputs(entry, b, nqc, r, c)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    halves = _frozen_by_slices(entry, dev, r, 2)
    for out in _guarded(monkeypatch, entry, cpu, r, 2):
        _assert_is(entry, out, halves)
    whole, per_clip = _launch(entry, dev, r, 1), _launch(entry, dev, r, 4)
    for k in OUTPUTS[entry]:
        assert not torch.equal(halves[k], whole[k]) and not torch.equal(halves[k], per_clip[k]), k
    members = _ops().cva_pairing_members(b * nqc * r, b * nqc, 2)           # the host statement agrees on which halves pair
    assert members[:4].max() == 11 and members[4:].min() == 12


def test_backward_ops_refuse_a_bad_grouping_on_real_buffers():
    """... before any launch: nothing is recorded for a refused call, and the next valid call is unaffected."""
    ops = _ops()
    b, nqc, r, c = 3, 2, 3, 96
    for entry in sorted(OUTPUTS):
        dev = {k: v.to(DEV) for k, v in _inputs(entry, b, nqc, r, c).items()}
        was, ops.PROFILE = ops.PROFILE, {}
        try:
            for groups in (0, 4, 5, 12, -3):
                with pytest.raises(ValueError, match="groups"):
                    _launch(entry, dev, r, groups)
            launched = set(ops.PROFILE)
        finally:
            ops.PROFILE = was
        assert launched == set()
        out, want = _launch(entry, dev, r, 3), _frozen_by_slices(entry, dev, r, 3)
        _assert_is(entry, out, want)


# ------------------------------------------------------------------------------------------------ the module
MODULE_CASES = [(2, 1, 3, 96), (3, 2, 3, 192), (2, 4, 5, 96)]


def _module_inputs(b, nqc, r, c):
    nq = b * nqc
    return seeded_randn(8130 + c + r, nq, 49, c), seeded_randn(8131 + c + r, nq * r, 49, c), seeded_randn(8132 + c + r, nq, 49, c)


_MODULE_ORACLE = {}


def _module_oracle(b, nqc, r, c):
    """fp32 autograd on the oracle's swin_dattention (CPU), run on each clip alone: outputs and input gradients concatenated, the
    parameter gradients summed over the clips (one loss, sum(y * g), over the concatenation).  Computed once per case."""
    key = (b, nqc, r, c)
    if key not in _MODULE_ORACLE:
        from models.modules.deformableAttention import SwinDAttention
        att = fill_module_(SwinDAttention(c, c // 32, 0.0, 3)).eval()
        sd = {"a." + k: v.detach().clone().requires_grad_(True) for k, v in att.state_dict().items()}
        x1, x2, gy = _module_inputs(b, nqc, r, c)
        x1o, x2o = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        yo = torch.cat([O.swin_dattention(x1o[i * nqc:(i + 1) * nqc], x2o[i * nqc * r:(i + 1) * nqc * r], sd, "a") for i in range(b)])
        (yo * gy).sum().backward()
        _MODULE_ORACLE[key] = (yo.detach(), x1o.grad, x2o.grad, {n: sd["a." + n].grad for n, _ in att.named_parameters()})
    return _MODULE_ORACLE[key]


def _module_run(b, nqc, r, c, groups, spy=None, flip_before_backward=None):
    """swin_dattention_train(groups=) on SwinDAttention(c, c / 32, 0.0, 3) -> (y, dx1, dx2, {name: grad}) on the CPU.  spy: a list
    that receives (q, kv, dout, keywords, (dq, dkv)) of the attention core's backward call."""
    from models.modules.deformableAttention import SwinDAttention
    from mumpy_hip.autograd import swin_dattention_train
    ops = _ops()
    att = fill_module_(SwinDAttention(c, c // 32, 0.0, 3)).eval().cuda()
    x1, x2, gy = _module_inputs(b, nqc, r, c)
    x1g, x2g = x1.cuda().requires_grad_(True), x2.cuda().requires_grad_(True)
    y = swin_dattention_train(att, x1g, x2g, groups=groups)
    if flip_before_backward is not None:
        ops.set_cva_math(flip_before_backward)
    inner = ops.deform_attention_bwd
    if spy is not None:
        def wrapped(q, kv, dout, *a, **kw):
            res = inner(q, kv, dout, *a, **kw)
            spy.append((q.detach().clone(), kv.detach().clone(), dout.detach().clone(), (a, kw), tuple(t.clone() for t in res)))
            return res
        ops.deform_attention_bwd = wrapped
    try:
        (y * gy.cuda()).sum().backward()
    finally:
        ops.deform_attention_bwd = inner
    return y.detach().cpu(), x1g.grad.cpu(), x2g.grad.cpu(), {n: p.grad.cpu() for n, p in att.named_parameters()}


@pytest.mark.parametrize("b,nqc,r,c", MODULE_CASES, ids=lambda v: str(v))
def test_module_tape_matches_the_per_clip_oracle(b, nqc, r, c):
    """The bars of test_hip_swin_dattention_backward_vs_oracle: output 2e-5, input and parameter gradients 2e-4, proj_k.bias (true
    gradient 0) by magnitude.  The batch-coupled tape misses the per-clip reference by more than 0.1 on y, dx1 and dx2 (the oracle's
    own two pairings differ by 0.48 to 1.03 there); the biases are not asked to miss (proj_v.bias and proj_out.bias have
    pairing-invariant gradients)."""
    ops = _ops()
    assert (ops.cva_math(), ops.matrix_math(), ops.clip_coupling()) == ("fp32", "fp32", "batch")
    yo, dx1o, dx2o, go = _module_oracle(b, nqc, r, c)
    was, ops.PROFILE = ops.PROFILE, {}
    try:
        y, dx1, dx2, grads = _module_run(b, nqc, r, c, b)
        names = set(ops.PROFILE)
    finally:
        ops.PROFILE = was
    torch.cuda.synchronize()
    assert {"mumpy_deform_sample_grouped_fwd", "mumpy_deform_attention_grouped_fwd", "mumpy_deform_sample_grouped_bwd",
            "mumpy_deform_attention_grouped_bwd"} <= names
    assert not names & {"mumpy_deform_sample_fwd", "mumpy_deform_attention_fwd", "mumpy_deform_sample_bwd", "mumpy_deform_attention_bwd"}
    fig = {"y": rel_err(y, yo), "dx1": rel_err(dx1, dx1o), "dx2": rel_err(dx2, dx2o)}
    fig.update({n: rel_err(grads[n], go[n]) for n in grads if n != "proj_k.bias"})
    print(f"swin_dattention_train(groups={b}) at {(b, nqc, r, c)} vs per-clip oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["y"] < 2e-5
    assert all(v < 2e-4 for k, v in fig.items() if k != "y"), fig
    assert float(grads["proj_k.bias"].abs().max()) < 1e-5 and float(go["proj_k.bias"].abs().max()) < 1e-5
    yb, dx1b, dx2b, _ = _module_run(b, nqc, r, c, 1)
    miss = {"y": rel_err(yb, yo), "dx1": rel_err(dx1b, dx1o), "dx2": rel_err(dx2b, dx2o)}
    print(f"... the batch-coupled tape vs the same reference: " + ", ".join(f"{k} {v:.2e}" for k, v in miss.items()))
    assert all(v > 0.1 for v in miss.values()), miss


def test_module_tape_at_one_group_launches_the_frozen_entries_and_keeps_its_refusal():
    """The other half of the launch-name assertion above: swin_dattention_train(groups=1) runs the four frozen entries and none of
    the grouped ones.  Under ops.set_clip_coupling("clip") the same call is refused when it reaches the first of the two Functions
    (proj_q and the offset network, which pair nothing, have run by then): no cross-view entry, frozen or grouped, is launched, and
    each Function called directly with groups = 1 is refused before anything at all is recorded."""
    from mumpy_hip.autograd import DeformAttentionFn, DeformSampleFn
    ops = _ops()
    b, nqc, r, c = 2, 1, 3, 96
    frozen = {"mumpy_deform_sample_fwd", "mumpy_deform_attention_fwd", "mumpy_deform_sample_bwd", "mumpy_deform_attention_bwd"}
    s, a = ({k: v.to(DEV) for k, v in _inputs(e, b, nqc, r, c).items()} for e in ("sample", "attention"))
    assert (ops.cva_math(), ops.clip_coupling()) == ("fp32", "batch")
    was, ops.PROFILE = ops.PROFILE, {}
    try:
        _module_run(b, nqc, r, c, 1)
        names = set(ops.PROFILE)
        ops.PROFILE = {}
        with ops.clip_coupling_as("clip"):
            for call in (lambda: DeformSampleFn.apply(s["x2"], s["pos"], 1), lambda: DeformAttentionFn.apply(a["q"], a["kv"], SCALE, 1)):
                with pytest.raises(RuntimeError, match="set_clip_coupling"):
                    call()
                assert ops.PROFILE == {}
            with pytest.raises(RuntimeError, match="set_clip_coupling"):
                _module_run(b, nqc, r, c, 1)
        refused = set(ops.PROFILE)
    finally:
        ops.PROFILE = was
    torch.cuda.synchronize()
    assert frozen <= names and not names & {n.replace("_fwd", "_grouped_fwd").replace("_bwd", "_grouped_bwd") for n in frozen}
    assert not any("deform_sample" in n or "deform_attention" in n for n in refused), sorted(refused)
    assert ops.clip_coupling() == "batch"


def test_module_tape_carries_bf16_to_the_grouped_backward():
    """Forward under ops.set_cva_math("bf16"), the switch set back BEFORE the backward: ctx.math and ctx.groups reach
    ops.deform_attention_bwd, and what it returns for the batch is, bit for bit, the frozen bf16 op on each clip's slice of the very
    tensors it was given.  (The arithmetic's accuracy: tests/test_cva_bf16mm_train.py.)"""
    ops = _ops()
    b, nqc, r, c = 3, 2, 3, 192
    before = ops.cva_math()
    seen = []
    try:
        ops.set_cva_math("fp32")
        plain = _module_run(b, nqc, r, c, b)
        ops.set_cva_math("bf16")
        run = _module_run(b, nqc, r, c, b, spy=seen, flip_before_backward="fp32")
    finally:
        ops.set_cva_math(before)
    (q, kv, dout, (args, kw), (dq, dkv)), = seen
    assert kw.get("math") == "bf16" and kw.get("groups") == b
    want = _frozen_by_slices("attention_mm16", {"q": q, "kv": kv, "dout": dout}, r, b)
    assert _same(dq, want["dq"]) and _same(dkv, want["dkv"])
    fp32 = _frozen_by_slices("attention", {"q": q, "kv": kv, "dout": dout}, r, b)
    assert not torch.equal(dq, fp32["dq"]) and not torch.equal(dkv, fp32["dkv"])
    assert not torch.equal(run[0], plain[0]) and not torch.equal(run[1], plain[1]) and not torch.equal(run[2], plain[2])


# ------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("math", ["fp32", "bf16"])
@pytest.mark.parametrize("b,nqc,r,c", [(2, 1, 3, 96), (2, 4, 5, 96)], ids=lambda v: str(v))
def test_grouped_tape_captures_and_replays_bitwise(b, nqc, r, c, math):
    """swin_dattention_train(groups=B) forward + backward captured the way GraphedTrainStep does it (modelled on
    test_tape_under_bf16_captures_and_replays_bitwise): every eager run (they are the warm-up) and the capture on ONE side stream,
    capture_error_mode="thread_local", .backward() into gradient buffers that exist before the capture.  No host synchronisation or
    allocation inside the ops breaks the capture; two replays equal the eager result bitwise, output and every gradient."""
    from models.modules.deformableAttention import SwinDAttention
    from mumpy_hip.autograd import swin_dattention_train
    from mumpy_hip.streams import new_distinct_stream
    ops = _ops()
    att = fill_module_(SwinDAttention(c, c // 32, 0.0, 3)).eval().to(DEV)
    x1, x2, gy = (t.to(DEV) for t in _module_inputs(b, nqc, r, c))
    x1.requires_grad_(True)
    x2.requires_grad_(True)
    leaves = [x1, x2] + [p for _, p in sorted(att.named_parameters())]
    for t in leaves:
        t.grad = torch.zeros_like(t)
    ops.pad_mask(DEV)                                                      # (a cached table: built before the capture)

    def fwd_bwd(groups):
        for t in leaves:
            t.grad.zero_()
        y = swin_dattention_train(att, x1, x2, groups=groups)
        y.backward(gy)
        return y.detach()

    def snapshot(y):
        return [y.clone()] + [t.grad.clone() for t in leaves]

    before = ops.cva_math()
    try:
        ops.set_cva_math(math)
        # (from the high-priority pool, as the test this one is modelled on: the deal of torch's normal-priority pool is left alone)
        side = new_distinct_stream(DEV, (torch.cuda.current_stream().cuda_stream,), priority=-1)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = snapshot(fwd_bwd(1))
            for _ in range(2):
                eager = snapshot(fwd_bwd(b))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            static_y = fwd_bwd(b)
        replays = []
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            replays.append(snapshot(static_y))
    finally:
        ops.set_cva_math(before)
    assert all(bool(torch.isfinite(e).all()) for e in eager)
    for rep in replays:
        assert len(rep) == len(eager) and all(torch.equal(a, e) for a, e in zip(rep, eager))
    assert not any(torch.equal(eager[i], other[i]) for i in range(3))      # y, dx1, dx2: per-clip is not the batch-coupled tape


# ------------------------------------------------------------------------------------------------ the whole model
WB, WT_ = 2, 3


@pytest.fixture(scope="module")
def whole_model_oracle():
    """B = 2, T = 3: autograd on the reference-pinned oracle (CPU, fp32), each clip run ALONE, loss sum(logits * g): the logits
    concatenated, every parameter gradient summed over the clips.  Computed once, never modified."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    enc, dec = fill_module_(Encoder(num_frames=WT_)).eval(), fill_module_(Decoder(input_token_temporal_dims=[1, 1, WT_])).eval()

    def leaf_sd(mod):
        return {k: (v.detach().clone().requires_grad_(True) if v.dtype.is_floating_point and "attn_mask" not in k else v)
                for k, v in mod.state_dict().items()}
    sde, sdd = leaf_sd(enc), leaf_sd(dec)
    x, g = seeded_randn(990, WB, WT_, 3, 224, 224), seeded_randn(991, WB, 1, 224, 224)
    logits = []
    for i in range(WB):
        lo = O.full_forward(sde, sdd, x[i:i + 1])[0]
        (lo * g[i:i + 1]).sum().backward()                                 # .grad accumulates: the sum over clips
        logits.append(lo.detach())
    return {"x": x, "g": g, "logits": torch.cat(logits),
            "enc": {k: v.grad for k, v in sde.items() if getattr(v, "grad", None) is not None},
            "dec": {k: v.grad for k, v in sdd.items() if getattr(v, "grad", None) is not None}}


def _hip_whole(ref, coupling):
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip.autograd import decoder_train, encoder_train
    enc = fill_module_(Encoder(num_frames=WT_)).eval().cuda()
    dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, WT_])).eval().cuda()
    fx, vx, dx = encoder_train(enc, ref["x"].cuda(), coupling=coupling)
    lg, _ = decoder_train(dec, fx, vx, dx)
    (lg * ref["g"].cuda()).sum().backward()
    return enc, dec, lg.detach().cpu()


def _cva_l2(enc, dec, ref):
    """Relative L2 of the "cva" optimizer group's gradients (train.py:202-213) against the reference."""
    from mumpy_hip.train import split_param_groups
    names = {id(p): ("enc", n) for n, p in enc.named_parameters()}
    names.update({id(p): ("dec", n) for n, p in dec.named_parameters()})
    got, want = [], []
    for prm in split_param_groups(enc, dec)["cva"]:
        which, n = names[id(prm)]
        got.append(prm.grad.detach().cpu().double().reshape(-1))
        want.append(ref[which][n].double().reshape(-1))
    got, want = torch.cat(got), torch.cat(want)
    return float((got - want).norm() / want.norm())


def test_whole_model_tape_under_clip_coupling_vs_the_per_clip_oracle(whole_model_oracle):
    """The bars of test_hip_full_model_backward_vs_oracle: logits 1e-3, EVERY parameter gradient 1e-2 (proj_k.bias of the cross
    attention by magnitude, as there).  The batch-coupled tape (coupling=None) must miss: logits by more than 1e-3 and the cva group
    by more than 3e-2 in relative L2 (the oracle's own two pairings differ by 7.4e-3 and 9.0e-2; a margin of three for fp32 route
    noise).  With the global switch at "clip" the explicit argument runs without a refusal and gives the same bits."""
    ops = _ops()
    ref = whole_model_oracle
    assert ops.clip_coupling() == "batch"
    enc, dec, lg = _hip_whole(ref, "clip")
    e_logits = rel_err(lg, ref["logits"])
    bad, worst = [], 0.0
    for mod, which in ((enc, "enc"), (dec, "dec")):
        for name, prm in mod.named_parameters():
            assert prm.grad is not None, name
            want = ref[which][name]
            if name.endswith("crossattn.proj_k.bias"):          # softmax-invariant: true gradient 0
                assert float(prm.grad.abs().max()) < 1e-4 * max(1.0, float(want.abs().max()) * 1e4), name
                continue
            e = rel_err(prm.grad.cpu(), want)
            worst = max(worst, e)
            if e > 1e-2:
                bad.append((name, e))
    cva = _cva_l2(enc, dec, ref)
    print(f"encoder_train(coupling='clip') B={WB} T={WT_} vs per-clip oracle: logits {e_logits:.3e}, worst parameter gradient "
          f"{worst:.3e}, cva group relative L2 {cva:.3e}")
    assert e_logits < 1e-3
    assert not bad, bad[:10]
    enc_b, dec_b, lg_b = _hip_whole(ref, None)
    e_logits_b, cva_b = rel_err(lg_b, ref["logits"]), _cva_l2(enc_b, dec_b, ref)
    print(f"... the batch-coupled tape vs the same reference: logits {e_logits_b:.3e}, cva group relative L2 {cva_b:.3e}")
    assert e_logits_b > 1e-3 and cva_b > 3e-2
    del enc_b, dec_b
    with ops.clip_coupling_as("clip"):
        enc_s, dec_s, lg_s = _hip_whole(ref, "clip")
    assert ops.clip_coupling() == "batch"
    assert torch.equal(lg_s, lg)
    for mod, mod_s in ((enc, enc_s), (dec, dec_s)):
        for (name, prm), (_, prm_s) in zip(mod.named_parameters(), mod_s.named_parameters()):
            assert torch.equal(prm.grad, prm_s.grad), name
